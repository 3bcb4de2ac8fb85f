"""[SPECTRUM] on the GPU: ``wsr_level_spectra`` (csrc/spectra.hip) against the float64 evaluation of the same formulas
(``ref_spectra`` of tests/test_spectra.py: its own numpy DFT matrices and integer bins, nothing of spectra.py), analytic
identities evaluated on the device, refusals, and ``run.py --train --test`` without the section, with it under ``[EVAL]``
(the device loop) and with it alone (the host loop).  The sums and the workspace of the kernel live in ``Guarded`` buffers.

Bounds (kernel_bounds.py's convention, LAMBDA = 16 untouched): per mode of one (sample, field a, component, level) plane

    delta_a = LAMBDA * 2^-24 * sqrt(X Y) * || w (|f_a| + |m_a|) ||_2

and per (sample, level, bin)

    e_a:  1/2 sum_comp sum_modes h (2 |F_a| delta_a + delta_a^2) / (X Y W2)                      + 2^-100
    c_b:  1/2 sum_comp sum_modes h (|F_HR| delta_b + |F_b| delta_HR + delta_HR delta_b) / (X Y W2) + 2^-100

Each term of the transform carries one rounding of its twiddle, of its product and of the detrend; the sums behave as a
random walk (kernel_bounds' argument, with the l2 norm in place of A because the terms' signs are the twiddles').  delta
is at most 2e-3 of the rms mode amplitude, so one dropped or misplaced mode fails.  Nothing is measured against the code
under test.  The plane wave is held to its analytic value a^2 / 4 with, on top of the bound, what the rounding of the
input to fp32 can move: a relative 2^-24 of every sample changes half the variance by less than 2^-22 of a^2 / 4, and
puts at most 2^-47 a^2 anywhere else.

End to end the spectrum of each loop is held against the float64 spectrum of the fields THAT run pickled (its own SR and
baseline), under the bound above carried through ``spectrum_from_sums`` (``spectrum_bounds``).

Measured on an MI355X when the kernel was written: worst |err| / bound 0.075 for the sums against float64 (at 5 x 1 x 4;
0.069 at 1 x 8 x 3, 0.060 at 7 x 6 x 5, 0.034 at 9 x 5 x 130 and 12 x 10 x 6, 0.026 at 33 x 20, below 0.02 at 16 x 16, 64 x 64 and
128 x 128; 0.091 for ``gan.level_spectra`` at 2 x 12 x 8 x 5), 5.7e-3 for the plane waves against float64 and 4.5e-5 against
a^2 / 4, 2.6e-3 for Parseval, 0.011 for the spectra end to end.  The whole file ran in 12.3 s.
"""
import csv
import math
import os
import pickle
import time

import numpy as np
import pytest
import torch

from kernel_bounds import Guarded, assert_guards_intact, assert_within
from test_spectra import NS, np_bins, plane_wave, random_fields, ref_spectra, spectrum_bounds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
WINDOW_CODES = {"none": 0, "hann": 1}


def _launch(hip, HR, SR, TL, window, label=""):
    """the C entry on device copies of the operands, sums and workspace in guarded buffers -> (B, NZ, NK, 5) float64 on
    the host; a second launch and the wrapper must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    ops = [t.to(DEV).contiguous() for t in (HR, SR, TL)]
    NK = int(hip.wsr_level_spectra_bins(X, Y))
    assert NK == np_bins(X, Y)[1]
    n_ws = int(hip.wsr_level_spectra_workspace_floats(B, X, Y, NZ))
    assert n_ws > 2 * B * 9 * X * (Y // 2 + 1) * NZ
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, NK, 2 * NS), torch.float32, DEV)  # (B, NZ, NK, 5) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_spectra(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1], hip_ops._p(ops[2]),
                                    TL.shape[1], B, X, Y, NZ, WINDOW_CODES[window], hip_ops._p(ws.t), hip_ops._p(out.t),
                                    hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_spectra {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, NK, NS)
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), f"{label}: two calls differ"
    wrapped = hip_ops.level_spectra(*ops, window)  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(wrapped.cpu().view(torch.int64), got[0].view(torch.int64)), label
    return got[0]


def _poisoned(t, c):
    """``c`` channels: the first three of t, the surplus ones NaN (they must never be read)"""
    if c == 3:
        return t[:, :3].contiguous()
    return torch.cat([t[:, :3], torch.full((t.shape[0], c - 3) + tuple(t.shape[2:]), float("nan"))], dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------- sums against float64
# (B, X, Y, NZ): odd sizes and two samples; a power of two; 12 x 10; the two unit axes; X past one slab and no multiple of
# it, Y odd; more levels than one z chunk of any pass (130); the e2e tests' shape; 128 x 128 (two kx chunks per workgroup)
SUM_CASES = [(2, 7, 6, 5), (1, 16, 16, 10), (1, 12, 10, 6), (1, 1, 8, 3), (1, 5, 1, 4), (1, 33, 20, 3), (1, 9, 5, 130),
             (1, 64, 64, 10), (1, 128, 128, 4)]


@pytest.mark.parametrize("window", ["hann", "none"])
@pytest.mark.parametrize("dims", SUM_CASES, ids=lambda d: "x".join(map(str, d)))
def test_sums_against_float64(hip, dims, window):
    B, X, Y, NZ = dims
    for mean in (0.0, 8.0):
        for noise in (None, 1e-3):
            HR, SR, TL = random_fields(B, X, Y, NZ, seed=X * 7 + NZ + int(mean), noise=noise, mean=mean)
            ref, bnd = (torch.from_numpy(v) for v in ref_spectra(HR, SR, TL, window))
            for c in (3, 5):
                got = _launch(hip, _poisoned(HR, c), _poisoned(SR, c), _poisoned(TL, 8 - c), window, f"{dims} c={c}")
                assert_within(got, ref, bnd, f"level_spectra vs float64[{dims} {window} mean={mean} noise={noise} c={c}]",
                              kind="sums")


# ---------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("dims,pq", [((16, 16), (3, 2)), ((12, 10), (2, 3))], ids=str)
def test_a_plane_wave_lands_in_its_bin(hip, dims, pq):
    (X, Y), (p, q), a, NZ = dims, pq, 0.75, 3
    HR = plane_wave(X, Y, NZ, p, q, a)
    zero = torch.zeros_like(HR)
    got = _launch(hip, HR, HR.clone(), zero, "none", f"plane wave {dims}")[0]
    ref, bnd = (torch.from_numpy(v)[0] for v in ref_spectra(HR, HR, zero, "none"))
    assert_within(got, ref, bnd, f"plane wave vs float64[{dims}]", kind="sums")
    k = int(np_bins(X, Y)[0][p, q])
    want = torch.zeros_like(got)
    want[:, k, [0, 1, 3]] = a * a / 4
    slack = torch.full_like(got, 2.0 ** -47 * a * a)
    slack[:, k, :] = 2.0 ** -22 * a * a / 4
    assert_within(got, want, bnd + slack, f"plane wave vs a^2 / 4[{dims}]", kind="sums")
    assert bool((got[..., [2, 4]] == 0).all())  # (a zero baseline has no energy and no co-spectrum)


@pytest.mark.parametrize("window", ["hann", "none"])
def test_parseval_against_the_float64_variance(hip, window):
    from test_spectra import np_window

    for (B, X, Y, NZ) in ((2, 7, 6, 5), (1, 33, 20, 3), (1, 64, 64, 10)):
        fields = random_fields(B, X, Y, NZ, seed=X + NZ, mean=3.0)
        got = _launch(hip, *fields, window, f"parseval {(B, X, Y, NZ)}")
        _, bnd = ref_spectra(*fields, window)
        w = np_window(X, Y, window)[None, None, :, :, None]
        for a, f in enumerate(fields):
            f = f.double().numpy()
            d = (f - f.mean(axis=(2, 3), keepdims=True)) * w
            want = torch.from_numpy(0.5 * (d ** 2).sum(axis=(1, 2, 3)) / (w ** 2).sum())  # (B, NZ)
            allowed = torch.from_numpy(bnd[..., a].sum(axis=-1)) + 2.0 ** -48 * want  # (+ the float64 sums themselves)
            assert_within(got[..., a].sum(dim=-1), want, allowed, f"parseval[{(B, X, Y, NZ)} {window} field {a}]", kind="sums")


def test_identical_and_negated_fields_give_equal_bits(hip):
    for dims in ((1, 7, 6, 5), (1, 9, 5, 130), (1, 64, 64, 10)):
        HR, _, TL = random_fields(*dims, seed=33, mean=1.0)
        same = _launch(hip, HR, HR.clone(), TL, "hann", f"SR = HR {dims}")
        i64 = same.view(torch.int64)
        assert torch.equal(i64[..., 1], i64[..., 0]) and torch.equal(i64[..., 3], i64[..., 0]), dims
        assert bool((same[..., 0].sum(dim=-1) > 0).all())
        neg = _launch(hip, HR, -HR, TL, "hann", f"SR = -HR {dims}")
        assert torch.equal(neg[..., 1].view(torch.int64), i64[..., 0]) and torch.equal(neg[..., 3], -same[..., 0]), dims
        assert torch.equal(neg[..., [2, 4]].view(torch.int64), same[..., [2, 4]].view(torch.int64)), dims


def test_gan_level_spectra_builds_the_baseline_and_calls_the_kernel(hip):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from test_spectra import gan_stub

    HR, SR, _ = (t.to(DEV) for t in random_fields(2, 12, 8, 5, seed=4))
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5)).to(DEV)
    for window in ("hann", "none"):
        got = wind_field_GAN_3D.level_spectra(gan_stub(), HR, SR, LR, window)
        TL = hip_ops.trilinear_xy(LR, 4)
        want = hip_ops.level_spectra(HR, SR, TL, window)
        assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got.view(torch.int64), want.view(torch.int64))
        ref, bnd = (torch.from_numpy(v) for v in ref_spectra(HR, SR, TL, window))
        assert_within(got, ref, bnd, f"gan.level_spectra vs float64[(2, 12, 8, 5) {window}]", kind="sums")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 4, 4, 3
    HR, SR, TL = (t.to(DEV) for t in random_fields(B, X, Y, NZ, seed=1))
    NK = int(hip.wsr_level_spectra_bins(X, Y))
    n_ws = int(hip.wsr_level_spectra_workspace_floats(B, X, Y, NZ))
    out = Guarded((B, NZ, NK, 2 * NS), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, b=B, nx=X, ny=Y, nz=NZ, win=1, w=ws.t, o=out.t):
        return hip.wsr_level_spectra(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, b, nx, ny, nz, win, p(w), p(o), hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(tl=None), dict(w=None), dict(o=None), dict(hr_c=2), dict(sr_c=2),
               dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(win=2), dict(win=-1)]
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(nx=1025), dict(ny=1025), dict(b=65536), dict(nz=65536), dict(nx=1024, ny=1024, nz=2048)):
        assert call(**kw) == -2, kw
    assert hip.wsr_level_spectra_workspace_floats(1, 1025, 4, 3) == 0 == hip.wsr_level_spectra_workspace_floats(0, 4, 4, 3)
    assert hip.wsr_level_spectra_bins(1025, 4) == 0 == hip.wsr_level_spectra_bins(4, 0)
    assert hip.wsr_level_spectra_bins(1024, 1024) == 725 and hip.wsr_level_spectra_bins(1, 8) == 7
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    ok = hip_ops.level_spectra(HR, SR, TL)
    assert ok.shape == (B, NZ, NK, NS) and bool(torch.isfinite(ok).all())
    into = torch.empty((B, NZ, NK, NS), dtype=torch.float64, device=DEV)
    assert hip_ops.level_spectra(HR, SR, TL, "hann", out=into) is into and torch.equal(into, ok)
    bad = [(HR[:, :2].contiguous(), SR, TL), (HR.double(), SR, TL), (HR, SR[..., :2], TL), (HR, SR[..., :2].contiguous(), TL),
           (HR, SR, TL[:, :, :1].contiguous()), (HR, SR, torch.cat([TL, TL]))]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_spectra(*args)
    with pytest.raises(ValueError, match="window.*hamming"):
        hip_ops.level_spectra(HR, SR, TL, "hamming")
    wide = torch.zeros((1, 3, 1025, 1, 1), device=DEV)
    with pytest.raises(ValueError, match="1025"):
        hip_ops.level_spectra(wide, wide, wide)
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_spectra(HR, SR, TL, out=torch.empty((B, NZ, NK, NS), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_spectra(HR.cpu(), SR, TL)


# ---------------------------------------------------------------------------------------------------- run.py
def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _float64_sums(run_dir, names, window):
    """(sums, bounds) (NZ, NK, 5) of the fields a run pickled, in float64 from its own HR / SR / TL"""
    total = bound = None
    for name in names:
        p = pickle.load(open(os.path.join(run_dir, "fields", f"test_fields_{name}.pkl"), "rb"))
        HR, SR, TL = (torch.from_numpy(np.asarray(p[k]))[None] for k in ("HR", "SR", "TL"))
        s, b = ref_spectra(HR, SR, TL, window)
        total = s[0] if total is None else total + s[0]
        bound = b[0] if bound is None else bound + b[0]
    return total, bound


def _check_columns(tag, rows, sums, bnd, nplanes, uvw, N, d, counts):
    """the rows ``bin,columns`` of a file against ``spectrum_from_sums`` of the float64 ``sums`` (NK, 5) -> worst ratio"""
    from gan_sr_wind_field_amd.spectra import SPECTRUM_COLUMNS, spectrum_from_sums

    want = spectrum_from_sums(torch.from_numpy(sums), nplanes, uvw, N, d, counts)
    allowed = spectrum_bounds(sums, bnd, nplanes, uvw)
    worst = 0.0
    for k, row in enumerate(rows):
        got = dict(zip(SPECTRUM_COLUMNS, map(float, row)))
        assert got["wavelength_m"] == want["wavelength_m"][k] and got["n_modes"] == want["n_modes"][k], (tag, k)
        for col, b in allowed.items():
            w = want[col][k]
            if math.isnan(w):  # (an empty bin: 0 / 0 in both)
                assert counts[k] == 0 and math.isnan(got[col]), (tag, col, k, got[col])
                continue
            lim = b[k] + 2.0 ** -45 * abs(w)  # (+ the double arithmetic of the two evaluations)
            worst = max(worst, abs(got[col] - w) / lim)
            assert abs(got[col] - w) <= lim, (tag, col, k, got[col], w, lim)
    return worst


def test_run_train_and_test_without_and_with_the_section_in_both_loops(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.spectra import SPECTRUM_COLUMNS, grid_spacing, mode_counts, n_bins

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_spectra

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_spectra", counted)

    def run(name, flags, section, interpolate_z=False, **env):
        ini = str(tmp_path / f"{name}.ini")
        cfg = _write_ini(ini)
        cfg.name = name
        cfg.gan_config.interpolate_z = interpolate_z
        for k, v in env.items():
            setattr(cfg.env, k, v)
        with open(ini, "w") as f:
            f.write(cfg.asINI() + section)
        runmod.main(flags + ["--cfg", ini])
        return cfg, os.path.join(str(tmp_path), "runs", name)

    spec = "\n[SPECTRUM]\nenergy_spectrum = True\nper_level = True\nwindow = hann\n"
    cfg_a, dir_a = run("plain", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n")
    assert calls["n"] == 0 and not any("energy_spectrum" in f for f in os.listdir("test_output"))  # never without the section
    _, dir_b = run("dev", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n" + spec)
    n_test = len(_read("dev", "metrics")) - 1
    assert n_test > 1 and calls["n"] == -(-n_test // 2), calls  # once per batch
    _, dir_c = run("host", ["--train", "--test"], spec)
    assert calls["n"] == -(-n_test // 2), calls  # the host loop composes torch ops
    with open(os.path.join(dir_b, "config.ini")) as f:
        assert f.read().endswith(spec)

    # the existing files of the first two runs: text-equal
    with open("test_output/plain____metrics.csv") as fa, open("test_output/dev____metrics.csv") as fb:
        assert fa.read() == fb.read()
    av = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert [r.split(",")[0] for r in av[1:]] == ["plain", "dev", "host"] and av[1].split(",", 1)[1] == av[2].split(",", 1)[1]
    assert sorted(os.listdir(os.path.join(dir_a, "fields"))) == sorted(os.listdir(os.path.join(dir_b, "fields")))

    _, te, _, _, _ = runmod.prepare_data(cfg_a)
    uvw = float(te.UVW_MAX)
    names = [te[i][3] for i in range(len(te))]
    X, Y, NZ = te[0][1].shape[1:]
    NK, N, counts = n_bins(X, Y), max(X, Y), mode_counts(X, Y).tolist()
    d = grid_spacing(np.asarray(te.x), np.asarray(te.y))
    worst = 0.0
    for name, run_dir in (("dev", dir_b), ("host", dir_c)):
        sums, bnd = _float64_sums(run_dir, names, "hann")
        rows = _read(name, "energy_spectrum")
        assert rows[0] == ["bin"] + list(SPECTRUM_COLUMNS) and [r[0] for r in rows[1:]] == [str(k) for k in range(NK)]
        worst = max(worst, _check_columns(name, [r[1:] for r in rows[1:]], sums.sum(axis=0), bnd.sum(axis=0),
                                          n_test * NZ, uvw, N, d, counts))
        per = _read(name, "energy_spectrum_levels")
        assert per[0] == ["level", "bin"] + list(SPECTRUM_COLUMNS) and len(per) == 1 + NZ * NK
        for lvl in range(NZ):
            block = per[1 + lvl * NK:1 + (lvl + 1) * NK]
            assert [r[:2] for r in block] == [[str(lvl), str(k)] for k in range(NK)]
            worst = max(worst, _check_columns(f"{name} level {lvl}", [r[2:] for r in block], sums[lvl], bnd[lvl], n_test,
                                              uvw, N, d, counts))
    print(f"[e2e] energy spectra of both loops against float64: worst |err| / bound {worst:.3g}")

    # reverse interpolation: the second pair, on the raw levels, from the same checkpoint
    load = dict(generator_load_path=os.path.join(dir_a, "G_6.pth"), discriminator_load_path=os.path.join(dir_a, "D_6.pth"),
                state_load_path=os.path.join(dir_a, "state_6.pth"))
    before = calls["n"]
    run("rev", ["--test"], "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n" + spec, interpolate_z=True, **load)
    assert calls["n"] - before == 2 * -(-n_test // 2)
    for what in ("energy_spectrum", "energy_spectrum_reverse_interpolate"):
        rows = _read("rev", what)
        assert rows[0] == ["bin"] + list(SPECTRUM_COLUMNS) and len(rows) == 1 + NK, what
        assert all(math.isfinite(float(r[1 + SPECTRUM_COLUMNS.index("E_SR")])) for r in rows[1:]), what
    assert _read("rev", "energy_spectrum") != _read("rev", "energy_spectrum_reverse_interpolate")
    assert len(_read("rev", "energy_spectrum_levels_reverse_interpolate")) == 1 + NZ * NK
    print(f"[time] tests/test_spectra_gpu.py up to here: {time.time() - T0:.1f} s")
