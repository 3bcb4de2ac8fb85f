"""[SPECTRUM] on the CPU: the config section, ``bin_index`` against a rational comparison, ``level_spectra_reference``
against a plain-numpy double loop and analytic identities (Parseval, a plane wave, SR = +-HR), ``spectrum_from_sums`` on
a hand-made table, the evaluation loop with the section on a CPU device, and the names the C ABI carries.

Shared with test_spectra_gpu.py: ``ref_spectra`` - the five sums in float64 with this file's own numpy code (DFT matrices
with integer-reduced angles, bins from an integer loop; nothing of spectra.py) - and the bound of every (sample, level,
bin, sum).  Per mode of one (sample, field a, component, level) plane

    delta_a = LAMBDA * 2^-24 * sqrt(X Y) * || w (|f_a| + |m_a|) ||_2

(each term of the transform carries one rounding of its twiddle, of its product and of the detrend; the sums behave as a
random walk - kernel_bounds.py's argument with the l2 norm in place of A, because the terms' signs are the twiddles'),
and per bin

    e_a:  1/2 sum_comp sum_modes h (2 |F_a| delta_a + delta_a^2) / (X Y W2)                      + 2^-100
    c_b:  1/2 sum_comp sum_modes h (|F_HR| delta_b + |F_b| delta_HR + delta_HR delta_b) / (X Y W2) + 2^-100

``spectrum_bounds`` carries bounds of the sums through the formulas of ``spectrum_from_sums``.
"""
import cmath
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import REPO
from kernel_bounds import LAMBDA, TINY, U_FP32
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained

NS = 5
BIN_CASES = [(7, 6), (16, 16), (1, 8), (5, 1), (33, 20)]


# ------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def np_bins(X, Y):
    """(bins (X, Y // 2 + 1) int64, NK) from Python integers: the smallest k with 4 N^2 q < (2k + 1)^2 (XY)^2"""
    N = max(X, Y)
    out = np.zeros((X, Y // 2 + 1), dtype=np.int64)
    for kx in range(X):
        ks = kx if kx <= X // 2 else kx - X
        for ky in range(Y // 2 + 1):
            lhs, k = 4 * N * N * ((ks * Y) ** 2 + (ky * X) ** 2), 0
            while lhs >= (2 * k + 1) ** 2 * (X * Y) ** 2:
                k += 1
            out[kx, ky] = k
    nk = 0
    while (2 * nk + 1) ** 2 <= 2 * N * N:  # floor(N / sqrt(2) + 1/2): the largest k with (2k - 1)^2 <= 2 N^2
        nk += 1
    return out, nk + 1


def np_window(X, Y, window):
    def axis(n):
        if window == "none" or n == 1:
            return np.ones(n)
        return np.sin(np.pi * (np.arange(n) + 0.5) / n) ** 2

    return axis(X)[:, None] * axis(Y)[None, :]


def np_hermitian(Y):
    h = np.full(Y // 2 + 1, 2.0)
    h[0] = 1.0
    if Y % 2 == 0:
        h[-1] = 1.0
    return h


def _dft_matrix(n, nk):
    """exp(-2 pi i k j / n), (nk, n), the angle reduced in integers"""
    kj = (np.arange(nk)[:, None] * np.arange(n)[None, :]) % n
    return np.exp(-2j * np.pi * kj / n)


def ref_spectra(HR, SR, TL, window):
    """(sums, bound), both float64 numpy (B, NZ, NK, 5), from the fp32 (or any) values given - see the module docstring"""
    f = np.stack([t[:, :3].detach().cpu().double().numpy() for t in (HR, SR, TL)], axis=1)  # (B, 3, 3, X, Y, NZ)
    f = np.moveaxis(f, -1, 3)  # (B, a, comp, NZ, X, Y)
    B, _, _, NZ, X, Y = f.shape
    w = np_window(X, Y, window)
    W2 = float((w ** 2).sum())
    m = f.mean(axis=(-2, -1), keepdims=True)
    g = (f - m) * w
    F = _dft_matrix(X, X) @ g @ _dft_matrix(Y, Y // 2 + 1).T  # (B, a, comp, NZ, X, KY)
    delta = LAMBDA * U_FP32 * math.sqrt(X * Y) * np.sqrt(((w * (np.abs(f) + np.abs(m))) ** 2).sum(axis=(-2, -1), keepdims=True))
    h = np_hermitian(Y)
    absF = np.abs(F)
    terms = [(absF[:, a] ** 2 * h).sum(axis=1) for a in range(3)]
    terms += [((F[:, 0] * np.conj(F[:, b])).real * h).sum(axis=1) for b in (1, 2)]
    bnds = [((2 * absF[:, a] * delta[:, a] + delta[:, a] ** 2) * h).sum(axis=1) for a in range(3)]
    bnds += [((absF[:, 0] * delta[:, b] + absF[:, b] * delta[:, 0] + delta[:, 0] * delta[:, b]) * h).sum(axis=1) for b in (1, 2)]
    bins, NK = np_bins(X, Y)
    onehot = np.zeros((X * (Y // 2 + 1), NK))
    onehot[np.arange(onehot.shape[0]), bins.ravel()] = 1.0
    scale = 0.5 / (X * Y * W2)

    def binned(ts):  # each (B, NZ, X, KY) -> (B, NZ, NK, 5)
        return np.stack([t.reshape(B, NZ, -1) @ onehot for t in ts], axis=-1) * scale

    return binned(terms), binned(bnds) + TINY


def spectrum_bounds(sums, bnd, nplanes, uvw):
    """allowed |difference| of the ``SPECTRUM_COLUMNS`` made of ``sums`` (NK, 5) when sum k moved by at most ``bnd[:, k]``
    (numpy): the linear columns by b / n U^2; a ratio e_b / e_hr by (b_b + ratio b_hr) / (e_hr - b_hr); a coherence
    c / D, D = sqrt(e_hr e_b), by (b_c + |c / D| dev) / Dmin with Dmin, Dmax the extremes of D and dev its largest move."""
    s, b, n, U2 = np.asarray(sums, dtype=float), np.asarray(bnd, dtype=float), float(nplanes), float(uvw) ** 2
    out = {"E_HR": b[:, 0] / n * U2, "E_SR": b[:, 1] / n * U2, "E_trilinear": b[:, 2] / n * U2,
           "err_SR": (b[:, 0] + b[:, 1] + 2 * b[:, 3]) / n * U2, "err_trilinear": (b[:, 0] + b[:, 2] + 2 * b[:, 4]) / n * U2}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, e, c in (("SR", 1, 3), ("trilinear", 2, 4)):
            den = np.clip(s[:, 0] - b[:, 0], 0, None)
            out["ratio_" + name] = np.where(den > 0, (b[:, e] + s[:, e] / s[:, 0] * b[:, 0]) / den, np.inf)
            D = np.sqrt(s[:, 0] * s[:, e])
            Dmin = np.sqrt(np.clip(s[:, 0] - b[:, 0], 0, None) * np.clip(s[:, e] - b[:, e], 0, None))
            Dmax = np.sqrt((s[:, 0] + b[:, 0]) * (s[:, e] + b[:, e]))
            dev = np.maximum(Dmax - D, D - Dmin)
            out["coherence_" + name] = np.where(Dmin > 0, (b[:, c] + np.abs(s[:, c]) / D * dev) / Dmin, np.inf)
    return out


def random_fields(B, X, Y, NZ, seed, noise=None, mean=0.0, c=3):
    """fp32 HR, SR, TL (B, c, X, Y, NZ); ``noise``: SR = HR + noise * N(0, 1), None: independent; ``mean`` added to all"""
    g = torch.Generator().manual_seed(seed)
    HR = torch.randn((B, c, X, Y, NZ), generator=g) + mean
    SR = (torch.randn((B, c, X, Y, NZ), generator=g) + mean) if noise is None else HR + noise * torch.randn((B, c, X, Y, NZ), generator=g)
    TL = HR + 0.3 * torch.randn((B, c, X, Y, NZ), generator=g)
    return HR.contiguous(), SR.contiguous(), TL.contiguous()


def plane_wave(X, Y, NZ, p, q, a=0.75, comp=1, dtype=torch.float32):
    """(1, 3, X, Y, NZ) in ``dtype``: a cos(2 pi (p i / X + q j / Y)) in component ``comp`` (the angle reduced in integers), 0 elsewhere"""
    i, j = np.arange(X)[:, None], np.arange(Y)[None, :]
    ang = 2 * np.pi * (((p * i * Y + q * j * X) % (X * Y)) / (X * Y))
    f = np.zeros((1, 3, X, Y, NZ))
    f[0, comp] = (a * np.cos(ang))[:, :, None]
    return torch.from_numpy(f).to(dtype).contiguous()


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    plain = Config(LOCAL_INI).asINI()
    assert Config(LOCAL_INI).spectrum.present is False and Config(LOCAL_INI).spectrum.on is False
    assert "SPECTRUM" not in plain
    cfg = Config(_ini_with(tmp_path, "[SPECTRUM]\n"))
    s = cfg.spectrum
    assert s.present and s.on and (s.energy_spectrum, s.per_level, s.window) == (True, False, "hann")
    assert cfg.asINI() == plain + "\n[SPECTRUM]\nenergy_spectrum = True\nper_level = False\nwindow = hann\n"
    both = Config(_ini_with(tmp_path, "[DIAGNOSTICS]\n[SPECTRUM]\nper_level = True\nwindow = None\n"))
    text = both.asINI()
    assert text.index("[DIAGNOSTICS]") < text.index("[SPECTRUM]") and text.endswith("per_level = True\nwindow = none\n")
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.spectrum) == vars(both.spectrum) and again.asINI() == text and again.spectrum.window == "none"
    off = Config(_ini_with(tmp_path, "[SPECTRUM]\nenergy_spectrum = False\n"))
    assert off.spectrum.present and not off.spectrum.on
    for key in ("energy_spectrum", "per_level"):
        with pytest.raises(ValueError, match=rf"\[SPECTRUM\] {key}"):
            Config(_ini_with(tmp_path, f"[SPECTRUM]\n{key} = maybe\n"))
    with pytest.raises(ValueError, match=r"\[SPECTRUM\] per_level"):
        Config(_ini_with(tmp_path, "[SPECTRUM]\nenergy_spectrum = False\nper_level = True\n"))
    with pytest.raises(ValueError, match=r"\[SPECTRUM\] window.*hamming"):
        Config(_ini_with(tmp_path, "[SPECTRUM]\nwindow = hamming\n"))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.spectrum.present is False and back.spectrum.window == "hann" and back.asINI() == plain


# ---------------------------------------------------------------------------------------------------- 2. the bins
@pytest.mark.parametrize("dims", BIN_CASES, ids=lambda d: "x".join(map(str, d)))
def test_bin_index_against_a_rational_comparison(dims):
    from gan_sr_wind_field_amd.spectra import bin_index, mode_counts, n_bins

    X, Y = dims
    N = max(X, Y)
    got = bin_index(X, Y)
    assert got.dtype == torch.int64 and tuple(got.shape) == (X, Y // 2 + 1)
    NK = n_bins(X, Y)
    assert NK == math.floor(N / math.sqrt(2) + 0.5) + 1  # (no N <= 1024 sits near enough an edge for double to err)
    for kx in range(X):
        ks = kx if kx <= X // 2 else kx - X
        for ky in range(Y // 2 + 1):
            kappa2 = N * N * (Fraction(ks * ks, X * X) + Fraction(ky * ky, Y * Y))  # kappa^2, exact
            k = int(got[kx, ky])
            assert 0 <= k < NK
            # floor(kappa + 1/2) = k  <=>  k - 1/2 <= kappa < k + 1/2, compared in squares (k = 0: the right half alone)
            assert kappa2 < Fraction(2 * k + 1, 2) ** 2, (kx, ky, k)
            assert k == 0 or kappa2 >= Fraction(2 * k - 1, 2) ** 2, (kx, ky, k)
    mine, nk = np_bins(X, Y)
    assert nk == NK and np.array_equal(mine, got.numpy())
    counts = mode_counts(X, Y)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (NK,) and int(counts.sum()) == X * Y and int(counts[0]) == 1


def test_bin_index_and_n_bins_at_the_limits():
    from gan_sr_wind_field_amd.spectra import bin_index, n_bins

    for N in range(1, 1025):
        k = n_bins(N, 1) - 1
        assert (2 * k - 1) ** 2 <= 2 * N * N < (2 * k + 1) ** 2
    assert int(bin_index(1024, 1024).max()) == n_bins(1024, 1024) - 1 == 724  # (the integer test at its widest)
    for bad in ((0, 4), (4, 1025)):
        with pytest.raises(ValueError, match=r"\d"):
            bin_index(*bad)


# ---------------------------------------------------------------------------------------------------- 3. the reference
def test_reference_against_a_plain_numpy_double_loop():
    from gan_sr_wind_field_amd.spectra import SPECTRUM_SUMS, level_spectra_reference

    assert SPECTRUM_SUMS == ("e_hr", "e_sr", "e_tl", "c_sr", "c_tl")
    X, Y, NZ = 5, 4, 3
    HR, SR, TL = random_fields(1, X, Y, NZ, seed=9, mean=2.0, c=4)
    bins, NK = np_bins(X, Y)
    for window in ("hann", "none"):
        got = level_spectra_reference(HR, SR, TL, window)
        assert tuple(got.shape) == (1, NZ, NK, NS) and got.dtype == torch.float64
        w = np_window(X, Y, window)
        W2 = sum(w[i, j] ** 2 for i in range(X) for j in range(Y))
        want = np.zeros((NZ, NK, NS))
        for z in range(NZ):
            for comp in range(3):
                F = []
                for t in (HR, SR, TL):
                    f = t[0, comp, :, :, z].double().numpy()
                    m = sum(f[i, j] for i in range(X) for j in range(Y)) / (X * Y)
                    F.append({(kx, ky): sum((f[i, j] - m) * w[i, j] * cmath.exp(-2j * math.pi * (kx * i / X + ky * j / Y))
                                            for i in range(X) for j in range(Y)) for kx in range(X) for ky in range(Y // 2 + 1)})
                for (kx, ky), fh in F[0].items():
                    h = 1.0 if ky == 0 or 2 * ky == Y else 2.0
                    fs, ft = F[1][(kx, ky)], F[2][(kx, ky)]
                    want[z, bins[kx, ky]] += 0.5 * h / (X * Y * W2) * np.array(
                        [abs(fh) ** 2, abs(fs) ** 2, abs(ft) ** 2, (fh * fs.conjugate()).real, (fh * ft.conjugate()).real])
        assert np.allclose(got[0].numpy(), want, rtol=1e-11, atol=1e-13), window
        mine, bnd = ref_spectra(HR, SR, TL, window)
        assert np.allclose(mine[0], want, rtol=1e-11, atol=1e-13) and bool((bnd > 0).all())
        # the fp32 evaluation of the same composition sits inside the bound of the GPU tests
        f32 = level_spectra_reference(HR, SR, TL, window, dtype=torch.float32)
        assert f32.dtype == torch.float32 and float((np.abs(f32.double().numpy() - mine) / bnd).max()) <= 1.0


@pytest.mark.parametrize("window", ["hann", "none"])
def test_parseval_on_every_level(window):
    from gan_sr_wind_field_amd.spectra import level_spectra_reference

    for (B, X, Y, NZ) in ((2, 7, 6, 5), (1, 16, 16, 3), (1, 1, 8, 3), (1, 5, 1, 4)):
        fields = random_fields(B, X, Y, NZ, seed=X + NZ, mean=3.0)
        got = level_spectra_reference(*fields, window).numpy()
        w = np_window(X, Y, window)[None, None, :, :, None]
        for a, f in enumerate(fields):
            f = f.double().numpy()
            d = (f - f.mean(axis=(2, 3), keepdims=True)) * w
            want = 0.5 * (d ** 2).sum(axis=(1, 2, 3)) / (w ** 2).sum()  # half the window-weighted variance, (B, NZ)
            assert np.allclose(got[..., a].sum(axis=-1), want, rtol=1e-12, atol=1e-15), (X, Y, NZ, a)


@pytest.mark.parametrize("dims,pq", [((16, 16), (3, 2)), ((12, 10), (2, 3)), ((7, 6), (3, 1))], ids=str)
def test_a_plane_wave_lands_in_its_bin(dims, pq):
    from gan_sr_wind_field_amd.spectra import bin_index, level_spectra_reference

    (X, Y), (p, q), a = dims, pq, 0.75
    HR = plane_wave(X, Y, 2, p, q, a, dtype=torch.float64)
    got = level_spectra_reference(HR, HR, torch.zeros_like(HR), "none")[0].numpy()
    k = int(bin_index(X, Y)[p, q])
    want = np.zeros_like(got)
    want[:, k, [0, 1, 3]] = a * a / 4
    assert np.allclose(got, want, rtol=0, atol=1e-15)


def test_identical_and_negated_fields():
    from gan_sr_wind_field_amd.spectra import level_spectra_reference

    HR, _, TL = random_fields(2, 7, 6, 5, seed=3, mean=1.0)
    s = level_spectra_reference(HR, HR.clone(), TL)
    assert torch.equal(s[..., 1], s[..., 0]) and torch.equal(s[..., 3], s[..., 0]) and bool((s[..., 0].sum(-1) > 0).all())
    n = level_spectra_reference(HR, -HR, TL)
    assert torch.equal(n[..., 1], s[..., 0]) and torch.equal(n[..., 3], -s[..., 0]) and torch.equal(n[..., 4], s[..., 4])


# ---------------------------------------------------------------------------------------------------- 4. the columns
def test_spectrum_from_sums_on_a_hand_made_table():
    from gan_sr_wind_field_amd.spectra import SPECTRUM_COLUMNS, mode_counts, n_bins, spectrum_from_sums

    assert SPECTRUM_COLUMNS == ("wavelength_m", "n_modes", "E_HR", "E_SR", "E_trilinear", "ratio_SR", "ratio_trilinear",
                                "coherence_SR", "coherence_trilinear", "err_SR", "err_trilinear")
    rows = [[8.0, 2.0, 0.0, 4.0, 0.0], [0.0, 4.0, 1.0, 0.0, 0.0], [4.0, 16.0, 1.0, -8.0, 1.0]]
    counts = [1, 8, 12]
    for table in (rows, torch.tensor(rows, dtype=torch.float64)):
        p = spectrum_from_sums(table, 4, 10.0, 8, 50.0, counts)
        assert tuple(p) == SPECTRUM_COLUMNS and all(len(v) == 3 and all(isinstance(e, float) for e in v) for v in p.values())
        assert p["wavelength_m"] == [math.inf, 400.0, 200.0] and p["n_modes"] == [1.0, 8.0, 12.0]
        assert p["E_HR"] == [200.0, 0.0, 100.0] and p["E_SR"] == [50.0, 100.0, 400.0] and p["E_trilinear"] == [0.0, 25.0, 25.0]
        assert p["ratio_SR"][0] == 0.25 and math.isnan(p["ratio_SR"][1]) and p["ratio_SR"][2] == 4.0
        assert p["ratio_trilinear"][0] == 0.0 and math.isnan(p["ratio_trilinear"][1]) and p["ratio_trilinear"][2] == 0.25
        assert p["coherence_SR"][0] == 1.0 and math.isnan(p["coherence_SR"][1]) and p["coherence_SR"][2] == -1.0
        assert math.isnan(p["coherence_trilinear"][0]) and math.isnan(p["coherence_trilinear"][1])
        assert p["coherence_trilinear"][2] == 0.5
        assert p["err_SR"] == [50.0, 100.0, 900.0] and p["err_trilinear"] == [200.0, 25.0, 75.0]
    square = spectrum_from_sums(torch.zeros((n_bins(6, 6), 5), dtype=torch.float64), 1, 1.0, 6, 1.0)  # (counts of the square domain)
    assert square["n_modes"] == [float(v) for v in mode_counts(6, 6)] and all(math.isnan(v) for v in square["ratio_SR"])


# ---------------------------------------------------------------------------------------------------- 5. the loop
def _spectrum(name, suffix=""):
    with open(os.path.join("test_output", f"{name}____energy_spectrum{suffix}.csv")) as f:
        return [r.split(",") for r in f.read().strip().splitlines()]


def test_section_on_a_cpu_device_writes_the_spectrum(data_root, tmp_path, monkeypatch):  # noqa: F811
    from gan_sr_wind_field_amd.config.config import SpectrumConfig
    from gan_sr_wind_field_amd.spectra import SPECTRUM_COLUMNS, grid_spacing, level_spectra_reference, mode_counts, n_bins
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "spectrum", SpectrumConfig())
    cfg.spectrum.setSpectrumConfig(None)
    cfg.name = "plain"
    avg_a = evaluate(cfg, ds)
    assert not any("energy_spectrum" in f for f in os.listdir("test_output"))
    cfg.spectrum.present, cfg.spectrum.per_level = True, True
    cfg.name = "spec"
    avg_b = evaluate(cfg, ds)
    metrics = [open(os.path.join("test_output", f"{n}____metrics.csv")).read() for n in ("plain", "spec")]
    assert metrics[0] == metrics[1] and avg_a == avg_b  # the existing files: byte for byte
    HR = ds[0][1]
    X, Y, NZ = HR.shape[1:]
    NK = n_bins(X, Y)
    rows = _spectrum("spec")
    assert rows[0] == ["bin"] + list(SPECTRUM_COLUMNS) and [r[0] for r in rows[1:]] == [str(k) for k in range(NK)]
    vals = {k: [float(r[1 + i]) for r in rows[1:]] for i, k in enumerate(SPECTRUM_COLUMNS)}
    assert vals["n_modes"] == [float(v) for v in mode_counts(X, Y)]
    d = grid_spacing(np.asarray(ds.x), np.asarray(ds.y))
    assert vals["wavelength_m"][0] == math.inf and vals["wavelength_m"][1] == pytest.approx(max(X, Y) * d)
    occupied = [k for k in range(NK) if vals["n_modes"][k] > 0]
    assert all(vals["E_HR"][k] > 0 and -1 - 1e-12 <= vals["coherence_SR"][k] <= 1 + 1e-12 for k in occupied[1:])
    # Parseval: the bins' energies add up to half the window-weighted variance of the truth, averaged over the planes
    uvw = float(ds.UVW_MAX)
    total = sum(float(level_spectra_reference(ds[i][1][None], ds[i][1][None], ds[i][1][None])[..., 0].sum()) for i in range(len(ds)))
    assert sum(vals["E_HR"]) == pytest.approx(total / (len(ds) * NZ) * uvw ** 2, rel=1e-12)
    per = _spectrum("spec", "_levels")
    assert per[0] == ["level", "bin"] + list(SPECTRUM_COLUMNS) and len(per) == 1 + NZ * NK
    assert [r[0] for r in per[1::NK]] == [str(k) for k in range(NZ)] and [r[1] for r in per[1:1 + NK]] == [str(k) for k in range(NK)]
    i = 2 + SPECTRUM_COLUMNS.index("E_SR")
    for k in occupied:  # the mean over the levels of a level's energy is the summed file's
        col = [float(r[i]) for r in per[1:] if int(r[1]) == k]
        assert vals["E_SR"][k] == pytest.approx(sum(col) / NZ, rel=1e-12, abs=1e-300)


def gan_stub(scale=4):
    """what ``wind_field_GAN_3D.level_spectra`` uses of its object: the scale"""
    from types import SimpleNamespace

    return SimpleNamespace(cfg=SimpleNamespace(scale=scale))


def test_gan_level_spectra_on_a_cpu_device():
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.spectra import level_spectra_reference, n_bins

    HR, SR, _ = random_fields(2, 12, 8, 5, seed=4)
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
    for window in ("hann", "none"):
        got = wind_field_GAN_3D.level_spectra(gan_stub(), HR, SR, LR, window)
        assert got.shape == (2, 5, n_bins(12, 8), NS) and got.dtype == torch.float64
        assert torch.equal(got, level_spectra_reference(HR, SR, TL, window))
    with pytest.raises(ValueError, match="window"):
        wind_field_GAN_3D.level_spectra(gan_stub(), HR, SR, LR, "hamming")


# ---------------------------------------------------------------------------------------------------- 6. the ABI
def test_exports_header_and_wrapper_limits_agree():
    from gan_sr_wind_field_amd import _lib, hip_ops, spectra

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_spectra", "wsr_level_spectra_bins", "wsr_level_spectra_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define WSR_SPECTRUM_SUMS {hip_ops.SPECTRUM_SUMS}" in header and hip_ops.SPECTRUM_SUMS == len(spectra.SPECTRUM_SUMS)
    assert f"#define WSR_SPECTRUM_MAX_XY {hip_ops.SPECTRUM_MAX_XY}" in header and hip_ops.SPECTRUM_MAX_XY == spectra.MAX_XY
    for name, code in hip_ops.SPECTRUM_WINDOWS.items():
        assert f"#define WSR_SPECTRUM_WINDOW_{name.upper()} {code}" in header and spectra.WINDOWS[code] == name
    assert "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        assert "spectra.hip" in f.read()
