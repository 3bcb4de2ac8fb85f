"""[SPECTRAL_LOSS] on the CPU: the config section, ``bin_set`` against a Python-integer loop, ``spectral_energy_reference``
against a plain double loop, ``gradcheck`` of the reference and of the whole loss, this file's numpy vector-Jacobian product
against autograd of the reference (the truth test_spectral_loss_gpu.py leans on), the three analytic properties of the loss,
a generator iteration with the section on a CPU device, and the names the C ABI carries.

Shared with test_spectral_loss_gpu.py - float64 numpy from the definitions (explicit DFT matrices with integer-reduced
angles, ``np_bins`` of tests/test_spectra.py; nothing of spectral_loss.py or of the kernels):

``ref_vjp(SR, gbin, window)``: with G = gbin[bin], T = h G F_sr,  u = Re(conj(Dx) T conj(Dy)),  v = 2 scale w u,
``dsr = v - mean_plane(v)``, and per element the bound (kernel_bounds.py's convention, LAMBDA = 16 untouched)

    b  =  2 scale w delta_sr sum_modes h |G|                     the forward's error in the saved F_sr, propagated
                                                                (delta_sr: tests/test_spectra.py's per-mode bound)
       +  LAMBDA 2^-24 sqrt(X KY) 2 scale w || h G F_sr ||_2     the inverse transform's own rounding
       +  2^-24 2 scale w sum_modes h |G| |F_sr|                 gbin rounded to fp32 once
    bound = b + mean_plane(b) + 2^-100                          the mean term carries the same three, averaged

``truth_loss`` / ``loss_bounds``: L_spec from a float64 table e and what a move of e by at most ``be`` can do to the value
and to dL/de_sr (first derivatives times ``be``, widened by the relative size of the second-order term).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from kernel_bounds import LAMBDA, TINY, U_FP32
from test_eval import LOCAL_INI, _ini_with
from test_spectra import _dft_matrix, np_bins, np_hermitian, np_window, random_fields

ABS_FLOOR = 1e-20


# ------------------------------------------------------------------------------------------------- shared references
def np_counts(X, Y):
    """modes of the full X x Y spectrum per bin, from ``np_bins`` and the Hermitian weight -> int64 (NK,)"""
    bins, NK = np_bins(X, Y)
    c = np.zeros(NK, dtype=np.int64)
    np.add.at(c, bins.ravel(), np.broadcast_to(np_hermitian(Y).astype(np.int64), bins.shape).ravel())
    return c


def np_bin_set(X, Y, k_min=1, k_max=0):
    c = np_counts(X, Y)
    last = len(c) - 1 if k_max == 0 else k_max
    return np.array([k for k in range(len(c)) if k_min <= k <= last and c[k] > 0], dtype=np.int64)


def _transform(f, window):
    """f (B, >= 3, X, Y, NZ) -> (F (B, 3, NZ, X, KY), delta (B, 3, NZ, 1, 1), w (X, Y), scale)"""
    f = np.moveaxis(f[:, :3].detach().cpu().double().numpy(), -1, 2)  # (B, 3, NZ, X, Y)
    X, Y = f.shape[-2:]
    w = np_window(X, Y, window)
    m = f.mean(axis=(-2, -1), keepdims=True)
    F = _dft_matrix(X, X) @ ((f - m) * w) @ _dft_matrix(Y, Y // 2 + 1).T
    delta = LAMBDA * U_FP32 * math.sqrt(X * Y) * np.sqrt(((w * (np.abs(f) + np.abs(m))) ** 2).sum(axis=(-2, -1), keepdims=True))
    return F, delta, w, 0.5 / (X * Y * float((w ** 2).sum()))


def ref_energy(HR, SR, window):
    """(e (B, NZ, NK, 2), bound) float64 numpy: tests/test_spectra.py's formulas for the two fields"""
    out, bnd = [], []
    for f in (HR, SR):
        F, delta, _, scale = _transform(f, window)
        B, _, NZ, X, KY = F.shape
        bins, NK = np_bins(X, f.shape[3])
        h = np_hermitian(f.shape[3])
        onehot = np.zeros((X * KY, NK))
        onehot[np.arange(X * KY), bins.ravel()] = 1.0
        a = np.abs(F)
        out.append(((a ** 2 * h).sum(axis=1).reshape(B, NZ, -1) @ onehot) * scale)
        bnd.append((((2 * a * delta + delta ** 2) * h).sum(axis=1).reshape(B, NZ, -1) @ onehot) * scale + TINY)
    return np.stack(out, axis=-1), np.stack(bnd, axis=-1)


def ref_vjp(SR, gbin, window, dgbin=None):
    """(dsr (B, 3, X, Y, NZ), bound) float64 numpy - see the module docstring; ``gbin`` (B, NZ, NK) numpy.  ``dgbin``
    (optional, >= 0): gbin itself is only known to within it - its image 2 scale w sum h dG |F| joins b."""
    F, delta, w, scale = _transform(SR, window)
    B, _, NZ, X, KY = F.shape
    Y = SR.shape[3]
    bins, _ = np_bins(X, Y)
    h = np_hermitian(Y)
    G = np.asarray(gbin, dtype=np.float64)[:, :, bins][:, None]  # (B, 1, NZ, X, KY)
    T = h * G * F
    u = (np.conj(_dft_matrix(X, X)) @ T @ np.conj(_dft_matrix(Y, KY))).real  # (B, 3, NZ, X, Y)
    v = 2 * scale * w * u
    dsr = v - v.mean(axis=(-2, -1), keepdims=True)
    hG = (h * np.abs(G))
    b = 2 * scale * w * delta * hG.sum(axis=(-2, -1), keepdims=True)
    b = b + LAMBDA * U_FP32 * math.sqrt(X * KY) * 2 * scale * w * np.sqrt((np.abs(T) ** 2).sum(axis=(-2, -1), keepdims=True))
    b = b + U_FP32 * 2 * scale * w * (hG * np.abs(F)).sum(axis=(-2, -1), keepdims=True)
    if dgbin is not None:
        dG = np.asarray(dgbin, dtype=np.float64)[:, :, bins][:, None]
        b = b + 2 * scale * w * (h * dG * np.abs(F)).sum(axis=(-2, -1), keepdims=True)
    bound = b + b.mean(axis=(-2, -1), keepdims=True) + TINY
    return np.moveaxis(dsr, 2, -1), np.moveaxis(bound, 2, -1)


def truth_loss(e, X, Y, k_min=1, k_max=0, rel_floor=1e-6):
    """L_spec from e (B, NZ, NK, 2) (a float64 torch tensor; differentiable) - this file's own statement of the formula"""
    K = torch.from_numpy(np_bin_set(X, Y, k_min, k_max))
    e_hr, e_sr = e[..., 0], e[..., 1]
    fl = rel_floor * e_hr.sum(dim=-1, keepdim=True) + ABS_FLOOR
    r = torch.log((e_sr[..., K] + fl) / (e_hr[..., K] + fl))
    return (r ** 2).sum() / r.numel()


def loss_bounds(e, be, X, Y, k_min=1, k_max=0, rel_floor=1e-6):
    """(L, bound of L, gbin = dL/de_sr (B, NZ, NK), bound of gbin) in float64 numpy when every entry of ``e`` may move by
    ``be``: first derivatives times ``be``, times 1 + 4 max(be / (e + floor)) over the bins in K for the higher orders
    (the derivatives are products of log, 1 / (e + floor) and 1 / (e + floor)^2: a relative move t of an argument moves
    each by less than a factor 1 + 4 t for t < 0.1, which is asserted)."""
    e64 = torch.from_numpy(np.asarray(e, dtype=np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(np.asarray(be, dtype=np.float64))
    L = truth_loss(e64, X, Y, k_min, k_max, rel_floor)
    (g,) = torch.autograd.grad(L, e64, create_graph=True)
    K = torch.from_numpy(np_bin_set(X, Y, k_min, k_max))
    fl = rel_floor * e64[..., 0].sum(dim=-1, keepdim=True) + ABS_FLOOR
    t = float((b64[:, :, K] / (e64[:, :, K].detach() + fl.detach().unsqueeze(-1))).max())
    assert t < 0.1, f"the energies are not known well enough for a first-order bound: {t}"
    widen = 1 + 4 * t
    dL = float((g.detach().abs() * b64).sum()) * widen
    gs = g[..., 1]
    dg = torch.zeros_like(gs)
    # |d gbin(b, z, k) / d e| be, summed over the entries gbin(b, z, k) depends on: e_sr(k), e_hr(k), and every e_hr(k') of
    # the level through the floor.  gbin(b, z, k) depends on nothing outside its (b, z): one backward pass per bin
    for k in K.tolist():
        (row,) = torch.autograd.grad(gs[:, :, k].sum(), e64, retain_graph=True)
        dg[:, :, k] = (row.abs() * b64).sum(dim=(-2, -1))
    return float(L.detach()), dL, gs.detach().numpy(), (dg * widen).detach().numpy()


SL = dict(weight=0.05, window="hann", k_min=1, k_max=0, rel_floor=1e-6)


class Section:
    """the attributes ``spectral_loss`` reads from a config section"""

    def __init__(self, **kw):
        self.__dict__.update(dict(SL, **kw))


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.spectral_loss import SPECTRAL_LOSS

    plain = Config(LOCAL_INI).asINI()
    off = Config(LOCAL_INI).spectral_loss
    assert off.present is False and off.on is False and "SPECTRAL_LOSS" not in plain
    cfg = Config(_ini_with(tmp_path, "[SPECTRAL_LOSS]\nweight = 0.05\n"))
    s = cfg.spectral_loss
    assert s.present and s.on and {k: getattr(s, k) for k in SPECTRAL_LOSS} == dict(SPECTRAL_LOSS, weight=0.05)
    assert (s.window, s.k_min, s.k_max, s.rel_floor) == ("hann", 1, 0, 1e-6)
    assert cfg.asINI() == plain + "\n[SPECTRAL_LOSS]\nweight = 0.05\nwindow = hann\nk_min = 1\nk_max = 0\nrel_floor = 1e-06\n"
    # comments on their own lines, every key, after another optional section
    both = Config(_ini_with(tmp_path, "[SPECTRUM]\n[SPECTRAL_LOSS]\n; the weight\nweight = 2\nwindow = None\nk_min = 2\n"
                                      "k_max = 5\nrel_floor = 0\n"))
    text = both.asINI()
    assert text.index("[SPECTRUM]") < text.index("[SPECTRAL_LOSS]")
    assert text.endswith("weight = 2.0\nwindow = none\nk_min = 2\nk_max = 5\nrel_floor = 0.0\n")
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.spectral_loss) == vars(both.spectral_loss) and again.asINI() == text
    refusals = [("", r"weight is required"), ("weight = 0\n", r"weight.*0"), ("weight = -1\n", r"weight.*-1"),
                ("weight = nan\n", r"weight.*nan"), ("weight = much\n", r"weight.*'much'"),
                ("weight = 1\nwindow = hamming\n", r"window.*hamming"), ("weight = 1\nk_min = 0\n", r"k_min.*0"),
                ("weight = 1\nk_min = x\n", r"k_min.*'x'"), ("weight = 1\nk_min = 3\nk_max = 2\n", r"k_max.*2"),
                ("weight = 1\nk_max = -1\n", r"k_max.*-1"), ("weight = 1\nk_max = 1.5\n", r"k_max.*'1.5'"),
                ("weight = 1\nrel_floor = -1e-3\n", r"rel_floor.*-0.001"), ("weight = 1\nrel_floor = inf\n", r"rel_floor.*inf")]
    for body, pattern in refusals:
        with pytest.raises(ValueError, match=r"\[SPECTRAL_LOSS\] " + pattern):
            Config(_ini_with(tmp_path, "[SPECTRAL_LOSS]\n" + body))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.spectral_loss.present is False and back.spectral_loss.weight is None and back.asINI() == plain


# ---------------------------------------------------------------------------------------------------- 2. the bin set
@pytest.mark.parametrize("dims", [(1, 8), (12, 10), (7, 6), (16, 16), (5, 1)], ids=lambda d: "x".join(map(str, d)))
def test_bin_set_against_an_integer_loop(dims):
    from gan_sr_wind_field_amd.spectral_loss import bin_set

    X, Y = dims
    NK = np_bins(X, Y)[1]
    counts = np_counts(X, Y)
    assert counts.sum() == X * Y
    for k_min, k_max in ((1, 0), (2, 0), (1, NK - 1), (2, NK - 2), (NK - 1, 0)):
        if k_max and k_max < k_min:
            continue
        want = np_bin_set(X, Y, k_min, k_max)
        if len(want) == 0:
            with pytest.raises(ValueError, match="no mode"):
                bin_set(X, Y, k_min, k_max)
            continue
        got = bin_set(X, Y, k_min, k_max)
        assert got.dtype == torch.int64 and got.tolist() == want.tolist(), (k_min, k_max)
    if dims == (1, 8):  # NK = 7, modes only in bins 0, 1, 2, 3, 4: bins 5 and 6 are empty
        assert NK == 7 and bin_set(1, 8).tolist() == [1, 2, 3, 4]
    if dims == (12, 10):
        assert (counts[1:] == 0).any() or len(np_bin_set(12, 10)) == NK - 1
    with pytest.raises(ValueError, match=r"k_min.*0"):
        bin_set(X, Y, 0, 0)
    with pytest.raises(ValueError, match=rf"k_max = {NK}.*{NK - 1}"):
        bin_set(X, Y, 1, NK)


# ---------------------------------------------------------------------------------------------------- 3. the reference
def test_reference_energy_against_a_plain_double_loop():
    from gan_sr_wind_field_amd.spectral_loss import spectral_energy_reference

    B, X, Y, NZ = 1, 5, 4, 3
    HR, SR, _ = random_fields(B, X, Y, NZ, seed=11, mean=2.0, c=4)
    for window in ("hann", "none"):
        got = spectral_energy_reference(HR, SR, window)
        assert got.shape == (B, NZ, np_bins(X, Y)[1], 2) and got.dtype == torch.float64
        w = np_window(X, Y, window)
        bins, NK = np_bins(X, Y)
        want = np.zeros((B, NZ, NK, 2))
        for a, f in enumerate((HR, SR)):
            f = f.double().numpy()
            for z in range(NZ):
                for comp in range(3):
                    g = (f[0, comp, :, :, z] - f[0, comp, :, :, z].mean()) * w
                    for kx in range(X):
                        for ky in range(Y):  # the FULL spectrum: the Hermitian weight is what folds it
                            F = sum(g[i, j] * np.exp(-2j * np.pi * (kx * i / X + ky * j / Y)) for i in range(X) for j in range(Y))
                            kyf = ky if ky <= Y // 2 else Y - ky
                            kxf = kx if ky <= Y // 2 else (X - kx) % X
                            want[0, z, bins[kxf, kyf], a] += abs(F) ** 2 / (2 * X * Y * (w ** 2).sum())
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-15)
        mine, _ = ref_energy(HR, SR, window)
        np.testing.assert_allclose(mine, want, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("dims", [(5, 4, 3), (1, 8, 2)], ids=str)
def test_gradcheck_of_the_reference_and_of_the_loss(dims):
    from gan_sr_wind_field_amd.spectra import mode_counts
    from gan_sr_wind_field_amd.spectral_loss import loss_from_energy, spectral_energy_reference, spectral_loss

    X, Y, NZ = dims
    g = torch.Generator().manual_seed(5)
    HR = torch.randn((1, 3, X, Y, NZ), generator=g, dtype=torch.float64)
    SR = (HR + 0.5 * torch.randn((1, 3, X, Y, NZ), generator=g, dtype=torch.float64)).requires_grad_(True)
    for window in ("hann", "none"):
        assert torch.autograd.gradcheck(lambda s: spectral_energy_reference(HR, s, window)[..., 1], (SR,), atol=1e-8)
        assert torch.autograd.gradcheck(
            lambda s: loss_from_energy(spectral_energy_reference(HR, s, window), mode_counts(X, Y), 1, 0, 1e-3), (SR,),
            atol=1e-8)
    e = spectral_energy_reference(HR, SR, "hann")
    g_hr = torch.autograd.grad(e[..., 0].sum(), SR, allow_unused=True, retain_graph=True)[0]  # only e_sr carries gradient
    assert g_hr is None or not g_hr.any()
    L = spectral_loss(HR, SR, Section())  # (a CPU device: the reference in float64, a float32 scalar out)
    assert L.dtype == torch.float32 and L.dim() == 0
    assert abs(float(L.detach()) - float(truth_loss(e.detach(), X, Y))) <= 1e-6 * float(L.detach())


@pytest.mark.parametrize("dims", [(2, 7, 6, 5), (1, 1, 8, 3), (1, 5, 1, 4), (1, 12, 10, 3), (1, 16, 16, 2)], ids=str)
def test_the_numpy_vjp_against_autograd_of_the_reference(dims):
    from gan_sr_wind_field_amd.spectral_loss import spectral_energy_reference

    B, X, Y, NZ = dims
    NK = np_bins(X, Y)[1]
    HR, SR, _ = random_fields(B, X, Y, NZ, seed=3, mean=1.0, c=4)
    for window in ("hann", "none"):
        gbin = torch.randn((B, NZ, NK), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
        s = SR.double().requires_grad_(True)
        e = spectral_energy_reference(HR.double(), s, window)
        (e[..., 1] * gbin).sum().backward()
        want, _ = ref_vjp(SR, gbin.numpy(), window)
        scale = np.abs(want).max()
        assert np.abs(s.grad[:, :3].numpy() - want).max() <= 1e-13 * scale, (dims, window)
        assert not s.grad[:, 3:].any()  # surplus channels: zero
        assert np.abs(want.sum(axis=(2, 3))).max() <= 1e-13 * scale * X * Y  # every plane sums to zero
        # the quadratic identity, exact for any d: sum G (e_sr(SR + d) - e_sr(SR - d)) = 2 <dsr, d>
        d = torch.randn(SR.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
        ep, _ = ref_energy(HR, SR.double() + d, window)
        em, _ = ref_energy(HR, SR.double() - d, window)
        lhs = float((gbin.numpy() * (ep[..., 1] - em[..., 1])).sum())
        rhs = 2 * float((want * d[:, :3].numpy()).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-30), (dims, window)


# ---------------------------------------------------------------------------------------------------- 4. the loss
def test_the_three_analytic_properties_of_the_loss():
    from gan_sr_wind_field_amd.spectral_loss import spectral_loss

    HR, SR, _ = random_fields(2, 12, 10, 3, seed=21, c=4)
    HR, SR = HR.double(), SR.double()
    for window in ("hann", "none"):
        sec = Section(window=window, rel_floor=0.0)
        assert float(spectral_loss(HR, HR.clone(), sec)) == 0.0
        base = spectral_loss(HR, SR, sec)
        assert float(base) > 0
        shift = torch.randn((2, 4, 1, 1, 3), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
        assert abs(float(spectral_loss(HR, SR + shift, sec)) - float(base)) <= 1e-6 * float(base)
        for a in (0.5, 3.0):
            assert abs(float(spectral_loss(HR, a * HR, sec)) - (2 * math.log(a)) ** 2) <= 1e-6 * (2 * math.log(a)) ** 2
    # empty bins are left out of the mean, not added as log(1): 1 x 8 has bins 1..4 of 1..6
    H8, S8, _ = random_fields(1, 1, 8, 2, seed=4)
    assert abs(float(spectral_loss(H8, 2.0 * H8, Section(rel_floor=0.0))) - (2 * math.log(2.0)) ** 2) < 1e-5
    with pytest.raises(ValueError, match=r"k_max = 9"):
        spectral_loss(HR, SR, Section(k_max=9))  # NK of 12 x 10 is 9: checked at the first batch
    # a large floor switches the term off: the loss falls with it
    assert float(spectral_loss(HR, SR, Section(rel_floor=10.0))) < 1e-2 * float(spectral_loss(HR, SR, Section()))


# ---------------------------------------------------------------------------------------------------- 5. the model
def _cpu_gan(section):
    from test_dist_gloo import _build_gan

    gan, cfg = _build_gan()
    sl = cfg.spectral_loss
    sl.present = section is not None
    for k, v in (section or {}).items():
        setattr(sl, k, v)
    return gan, cfg


def test_update_G_on_a_cpu_device_with_and_without_the_section(monkeypatch):
    from gan_sr_wind_field_amd import spectral_loss as slmod
    from gan_sr_wind_field_amd.config.config import SpectralLossConfig
    from oracle.gan import synthetic_batch
    from test_dist_gloo import _g_iteration

    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    seen = []
    orig = slmod.spectral_energy

    def recorded(hr, sr, window="hann"):
        seen.append((hr.detach().clone(), sr.detach().clone(), window))
        return orig(hr, sr, window)

    monkeypatch.setattr(slmod, "spectral_energy", recorded)
    try:
        gan0, cfg0 = _cpu_gan(None)
        w0, l0 = _g_iteration(gan0, cfg0, LR, HR, Z, x, y)
        assert not seen and "spectral" not in l0  # never called, exactly the old keys
        assert set(l0) == {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}

        gan1, cfg1 = _cpu_gan(dict(weight=0.05, window="hann", k_min=1, k_max=0, rel_floor=1e-6))
        before = {k: v.clone() for k, v in gan1.G.state_dict().items()}
        w1, l1 = _g_iteration(gan1, cfg1, LR, HR, Z, x, y)
        assert len(seen) == 1 and seen[0][2] == "hann" and torch.equal(seen[0][0], HR)
        e, _ = ref_energy(seen[0][0], seen[0][1], "hann")
        want = 0.05 * float(truth_loss(torch.from_numpy(e), HR.shape[2], HR.shape[3]))
        assert abs(l1["spectral"] - want) <= 1e-5 * want and want > 0
        # one more entry of the core vector: the total moves by it, the other terms do not, the step differs
        assert abs((l1["total"] - l0["total"]) - l1["spectral"]) <= 1e-5 * abs(l1["total"])
        assert all(l1[k] == l0[k] for k in l0 if k != "total")
        assert any(not torch.equal(w1[k], w0[k]) for k in w0)

        # a NaN in the spectral term: the total is not finite, the Adam step is skipped, the weights stay bit-equal
        gan2, cfg2 = _cpu_gan(dict(weight=0.05))
        monkeypatch.setattr(slmod, "spectral_energy", lambda hr, sr, window="hann": orig(hr, sr, window) * float("nan"))
        _, l2 = _g_iteration(gan2, cfg2, LR, HR, Z, x, y)
        assert math.isnan(l2["spectral"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, before[k]), k
        # validation logs it too
        monkeypatch.setattr(slmod, "spectral_energy", orig)
        gan1.update_G(LR, HR, Z, 0, False)
        assert float(gan1.get_G_val_loss_dict_ref()["spectral"]) > 0
        assert "spectral" not in gan0.get_G_val_loss_dict_ref()
    finally:
        for k in ("present", "weight", "window", "k_min", "k_max", "rel_floor"):  # (the class-level singleton)
            setattr(cfg0.spectral_loss, k, getattr(SpectralLossConfig, k))


# ---------------------------------------------------------------------------------------------------- 6. the C ABI
def test_exports_are_in_the_header_and_in_EXPORTS():
    from gan_sr_wind_field_amd._lib import EXPORTS

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    names = ("wsr_spectral_energy_workspace_floats", "wsr_spectral_energy_saved_floats", "wsr_spectral_energy",
             "wsr_spectral_energy_bwd")
    for n in names:
        assert n in EXPORTS and re.search(rf"\b{n}\s*\(", header), n
    assert int(re.search(r"#define\s+WSR_ABI_VERSION\s+(\d+)", header).group(1)) == 9
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        assert "spectral_loss.hip" in f.read()
