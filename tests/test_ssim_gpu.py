"""[SSIM] on the GPU: ``wsr_level_ssim`` (csrc/ssim.hip) against the float64 evaluation of the same formulas
(``ref_ssim`` of tests/ssim_bounds.py: numpy sliding windows, nothing of ssim.py but the tap table), bit identities and
closed forms evaluated on the device, refusals, ``gan.level_ssim``, and ``run.py --train --test`` with ``[EVAL]`` alone,
with ``[EVAL]`` and ``[SSIM]`` (the device loop) and with ``[SSIM]`` alone (the host loop), validation epochs included.
The sums and the workspace of the kernel live in ``Guarded`` buffers.

The bound is derived in tests/ssim_bounds.py (LAMBDA = 16 of kernel_bounds.py, untouched) and shown on the CPU to hold
for a torch fp32 evaluation and to reject an evaluation that is one voxel off (tests/test_ssim.py).  End to end the CSV
columns and the validation metrics are means of the sums, so their bounds are the same means of the sums' bounds
(``columns_from_sums`` is linear with positive weights), against the float64 sums of the fields THAT run pickled.

Measured on an MI355X when the kernel was written: worst |err| / bound 0.014 for the sums against float64 (one position,
3 x 3 x 4; 0.012 at 13 x 12 x 128, 0.0085 at 16 x 16 x 10, 0.0070 at 2 x 7 x 6 x 5, 0.0051 at 17 x 15 x 256, below 0.004 at
40 x 12 x 8, 35 x 35 x 200 and 70 x 66 x 6; 0.0063 for ``gan.level_ssim`` at 2 x 12 x 8 x 5), 0.0097 for ``SR = alpha HR`` and
0.0032 for constant planes against the closed forms, 2.0e-4 for the CSV columns end to end.  The whole file ran in 11 s
before the end-to-end test, which takes 21 s.
"""
import csv
import math
import os
import pickle
import re
import time

import numpy as np
import pytest
import torch

from kernel_bounds import Guarded, assert_guards_intact, assert_within
from ssim_bounds import GPU_CASES, NS, case_data, case_id, constant_planes, fields, poisoned, ref_ssim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
C1, C2 = 0.02 ** 2, 0.06 ** 2  # data_range 2


def _launch(hip, HR, SR, TL, win, sigma, label=""):
    """the C entry on device copies of the operands, sums and workspace in guarded buffers -> (B, NZ, 3, 4) float64 on
    the host; a second launch, the wrapper and the wrapper with ``out=`` must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops, ssim
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    ops = [t.to(DEV).contiguous() for t in (HR, SR, TL)]
    taps = ssim.taps(win, sigma).to(DEV)
    n_ws = int(hip.wsr_level_ssim_workspace_floats(B, X, Y, NZ, win))
    assert n_ws >= B * NZ * 3 * NS
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, 3, 2 * NS), torch.float32, DEV)  # (B, NZ, 3, 4) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_ssim(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1], hip_ops._p(ops[2]),
                                 TL.shape[1], hip_ops._p(taps), win, C1, C2, B, X, Y, NZ, hip_ops._p(ws.t),
                                 hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_ssim {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, 3, NS)
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), f"{label}: two calls differ"
    wrapped = hip_ops.level_ssim(*ops, win, sigma)  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(wrapped.cpu().view(torch.int64), got[0].view(torch.int64)), label
    into = torch.full((B, NZ, 3, NS), float("nan"), dtype=torch.float64, device=DEV)
    assert hip_ops.level_ssim(*ops, win, sigma, out=into) is into
    assert torch.equal(into.cpu().view(torch.int64), got[0].view(torch.int64)), label
    return got[0]


# ---------------------------------------------------------------------------------------------------- sums against float64
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_sums_against_float64(hip, case, kind):
    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, TL, ref, bnd = case_data(case, kind)
    for c in (3, 5):
        got = _launch(hip, poisoned(HR, c), poisoned(SR, c), poisoned(TL, 8 - c), win, sigma, f"{case_id(case)} c={c}")
        assert_within(got, ref, bnd, f"level_ssim vs float64[{case_id(case)} {kind} c={c}]", kind="sums")


# ---------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_equal_fields_give_exactly_the_number_of_positions(hip, case):
    (B, X, Y, NZ), (win, sigma) = case
    npos = float((X - win + 1) * (Y - win + 1))
    for kind in ("uniform", "smooth"):
        HR, SR, TL, ref, _ = case_data(case, kind)
        same_sr = _launch(hip, HR, HR.clone(), TL, win, sigma, f"SR = HR {case_id(case)}")
        assert bool((same_sr[..., :2] == npos).all()), (case, kind, same_sr[..., :2].flatten()[:8])
        same_tl = _launch(hip, HR, SR, HR.clone(), win, sigma, f"TL = HR {case_id(case)}")
        assert bool((same_tl[..., 2:] == npos).all()), (case, kind, same_tl[..., 2:].flatten()[:8])
        # the other pair is untouched by the first: the bits of the plain call
        plain = _launch(hip, HR, SR, TL, win, sigma, f"plain {case_id(case)}")
        assert torch.equal(same_sr[..., 2:].view(torch.int64), plain[..., 2:].view(torch.int64))
        assert torch.equal(same_tl[..., :2].view(torch.int64), plain[..., :2].view(torch.int64))


def test_constant_planes_and_a_scaled_field_match_the_closed_forms(hip):
    from ssim_bounds import _windowed

    from gan_sr_wind_field_amd.ssim import taps

    for (B, X, Y, NZ), (win, sigma) in (GPU_CASES[0], GPU_CASES[3], GPU_CASES[5]):
        npos = (X - win + 1) * (Y - win + 1)
        ones = torch.ones((B, 3, X, Y, NZ))
        p, q = 0.5, -0.25
        got = _launch(hip, p * ones, q * ones, p * ones, win, sigma, "constant planes")
        ref, bnd = ref_ssim(p * ones, q * ones, p * ones, win, sigma)
        l, cs = constant_planes(p, q, win, sigma)
        assert abs(l - (2 * p * q + C1) / (p * p + q * q + C1)) < 1e-6 and abs(cs - 1) < 1e-3  # (W = 1: the issue's form)
        want = torch.empty_like(ref)
        want[..., 0], want[..., 1], want[..., 2:] = npos * l * cs, npos * cs, npos
        assert float((ref - want).abs().max()) < 1e-10 * npos
        assert_within(got, want, bnd + 1e-10 * npos, f"constant planes[{(B, X, Y, NZ)}]", kind="sums")
        # SR = alpha HR (exact in fp32): mu_s = alpha mu_a, var_s = alpha^2 var_a, cov = alpha var_a
        HR = fields(B, X, Y, NZ, seed=5, kind="uniform")[0]
        alpha = 0.5
        got = _launch(hip, HR, alpha * HR, HR, win, sigma, "SR = alpha HR")
        _, bnd = ref_ssim(HR, alpha * HR, HR, win, sigma)
        g = taps(win, sigma).double().numpy()
        a = np.ascontiguousarray(HR.double().numpy().transpose(0, 4, 1, 2, 3))
        mu = _windowed(a, g)
        var = _windowed(a * a, g) - mu * mu
        l = (2 * alpha * mu * mu + C1) / ((1 + alpha * alpha) * mu * mu + C1)
        cs = (2 * alpha * var + C2) / ((1 + alpha * alpha) * var + C2)
        want = torch.stack([torch.from_numpy((l * cs).sum(axis=(-2, -1))), torch.from_numpy(cs.sum(axis=(-2, -1)))], dim=-1)
        assert_within(got[..., :2], want, bnd[..., :2] + 1e-12 * npos, f"SR = alpha HR[{(B, X, Y, NZ)}]", kind="sums")
        assert bool((got[..., 2:] == npos).all())


def test_a_constant_added_to_one_plane_moves_l_and_leaves_cs(hip):
    (B, X, Y, NZ), (win, sigma) = GPU_CASES[3]
    HR, SR, TL = (torch.round(t * 4096) / 4096 for t in fields(B, X, Y, NZ, seed=21, kind="smooth"))  # (SR + d is exact)
    d, (b, c, z) = 0.25, (0, 1, 2)
    moved = SR.clone()
    moved[b, c, :, :, z] += d
    assert torch.equal((moved - SR)[b, c, :, :, z], torch.full((X, Y), d))
    before = _launch(hip, HR, SR, TL, win, sigma, "before the shift")
    after = _launch(hip, HR, moved, TL, win, sigma, "after the shift")
    mask = torch.ones((B, NZ, 3), dtype=torch.bool)
    mask[b, z, c] = False
    assert torch.equal(after[mask].view(torch.int64), before[mask].view(torch.int64))  # every other plane: the same bits
    assert torch.equal(after[b, z, c, 2:].view(torch.int64), before[b, z, c, 2:].view(torch.int64))  # the TL pair too
    ref0, _ = ref_ssim(HR, SR, TL, win, sigma)
    ref1, bnd1 = ref_ssim(HR, moved, TL, win, sigma)
    want_ssim, want_cs = _shifted_plane(HR[b, c, :, :, z], SR[b, c, :, :, z], d, win, sigma)
    assert abs(want_ssim - float(ref1[b, z, c, 0])) < 1e-10 and abs(want_cs - float(ref1[b, z, c, 1])) < 1e-10
    npos = (X - win + 1) * (Y - win + 1)
    # cs does not see a constant (up to 1 - W of the fp32 taps, far below the bound); l follows the formula with mu_s + d W
    assert abs(want_cs - float(ref0[b, z, c, 1])) < 1e-6 * npos < 0.1 * float(bnd1[b, z, c, 1])
    assert abs(float(after[b, z, c, 1]) - want_cs) <= float(bnd1[b, z, c, 1]) + 1e-10
    assert abs(float(after[b, z, c, 0]) - want_ssim) <= float(bnd1[b, z, c, 0]) + 1e-10
    assert abs(want_ssim - float(ref0[b, z, c, 0])) > 100 * float(bnd1[b, z, c, 0])  # (and l did move)


def _shifted_plane(a, s, d, win, sigma):
    """(sum of l cs, sum of cs) of the planes a and s + d in float64, from the moments of a and s: with W the sum of the 2-D
    window, mu_s -> mu_s + d W, S_ss -> S_ss + 2 d mu_s + d^2 W, S_as -> S_as + d mu_a"""
    from ssim_bounds import _windowed

    from gan_sr_wind_field_amd.ssim import taps

    g = taps(win, sigma).double().numpy()
    W = float(g.sum()) ** 2
    a, s = a.double().numpy(), s.double().numpy()
    mua, mus, Saa, Sss, Sas = (_windowed(v, g) for v in (a, s, a * a, s * s, a * s))
    mus1, Sss1, Sas1 = mus + d * W, Sss + 2 * d * mus + d * d * W, Sas + d * mua
    va, vs1, cov1 = Saa - mua * mua, Sss1 - mus1 * mus1, Sas1 - mua * mus1
    l1 = (2 * mua * mus1 + C1) / (mua * mua + mus1 * mus1 + C1)
    cs1 = (2 * cov1 + C2) / (va + vs1 + C2)
    return float((l1 * cs1).sum()), float(cs1.sum())


def test_gan_level_ssim_builds_the_baseline_and_calls_the_kernel(hip):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from test_ssim import gan_stub

    HR, SR, _ = (t.to(DEV) for t in fields(2, 12, 8, 5, seed=4, kind="uniform"))
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5)).to(DEV)
    got = wind_field_GAN_3D.level_ssim(gan_stub(window_size=5, sigma=1.2), HR, SR, LR)
    TL = hip_ops.trilinear_xy(LR, 4)
    want = hip_ops.level_ssim(HR, SR, TL, 5, 1.2, 2.0)
    assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got.view(torch.int64), want.view(torch.int64))
    ref, bnd = ref_ssim(HR, SR, TL, 5, 1.2)
    assert_within(got, ref, bnd, "gan.level_ssim vs float64[(2, 12, 8, 5)]", kind="sums")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops, ssim

    B, X, Y, NZ, WIN = 1, 6, 5, 3, 3
    HR, SR, TL = (t.to(DEV) for t in fields(B, X, Y, NZ, seed=1, kind="uniform"))
    TAPS = ssim.taps(15, 2.0).to(DEV)  # (long enough for every window the calls below name)
    n_ws = int(hip.wsr_level_ssim_workspace_floats(B, X, Y, NZ, WIN))
    assert n_ws > 0
    out = Guarded((B, NZ, 3, 2 * NS), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, taps=TAPS, win=WIN, c1=C1, c2=C2, b=B, nx=X, ny=Y, nz=NZ, w=ws.t,
             o=out.t):
        return hip.wsr_level_ssim(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, p(taps), win, c1, c2, b, nx, ny, nz, p(w), p(o),
                                  hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(tl=None), dict(taps=None), dict(w=None), dict(o=None), dict(hr_c=2),
               dict(sr_c=2), dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(win=4), dict(win=1),
               dict(win=17), dict(win=-3), dict(win=7), dict(nx=2), dict(win=5, ny=4), dict(c1=0.0), dict(c2=-1.0)]
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(nz=257), dict(b=65536), dict(nx=32769), dict(ny=32769), dict(nx=32768, ny=32768, nz=2)):
        assert call(**kw) == -2, kw
    wsf = hip.wsr_level_ssim_workspace_floats
    assert wsf(0, X, Y, NZ, 3) == wsf(1, X, Y, 257, 3) == wsf(1, X, Y, NZ, 4) == wsf(1, X, 2, NZ, 3) == wsf(1, X, Y, NZ, 7) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    ok = hip_ops.level_ssim(HR, SR, TL, 3, 1.0)
    assert ok.shape == (B, NZ, 3, NS) and bool(torch.isfinite(ok).all())
    bad = [(HR[:, :2].contiguous(), SR, TL), (HR.double(), SR, TL), (HR, SR[..., :2], TL), (HR, SR[..., :2].contiguous(), TL),
           (HR, SR, TL[:, :, :3].contiguous()), (HR, SR, torch.cat([TL, TL]))]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_ssim(*args, 3, 1.0)
    for win, sigma, rng, pattern in ((4, 1.0, 2.0, "window.*4"), (17, 1.0, 2.0, "17"), (3, 0.0, 2.0, "sigma"),
                                     (3, 1.0, 0.0, "data_range"), (7, 1.0, 2.0, "6 x 5.*7 x 7")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.level_ssim(HR, SR, TL, win, sigma, rng)
    deep = torch.zeros((1, 3, 3, 3, 257), device=DEV)
    with pytest.raises(ValueError, match="257"):
        hip_ops.level_ssim(deep, deep, deep, 3, 1.0)
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_ssim(HR, SR, TL, 3, 1.0, out=torch.empty((B, NZ, 3, NS), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_ssim(HR.cpu(), SR, TL, 3, 1.0)
    # the taps are uploaded once per (device, window, sigma)
    n = len(hip_ops._ssim_taps)
    hip_ops.level_ssim(HR, SR, TL, 3, 1.0)
    hip_ops.level_ssim(HR, SR, TL, 3, 1.0)
    assert len(hip_ops._ssim_taps) == n
    hip_ops.level_ssim(HR, SR, TL, 3, 0.9)
    assert len(hip_ops._ssim_taps) == n + 1


# ---------------------------------------------------------------------------------------------------- run.py
def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _float64_sums(run_dir, names, win, sigma):
    """[(sums, bounds)] (NZ, 3, 4) per field a run pickled, in float64 from its own HR / SR / TL"""
    res = []
    for name in names:
        p = pickle.load(open(os.path.join(run_dir, "fields", f"test_fields_{name}.pkl"), "rb"))
        HR, SR, TL = (torch.from_numpy(np.asarray(p[k]))[None] for k in ("HR", "SR", "TL"))
        s, b = ref_ssim(HR, SR, TL, win, sigma)
        res.append((s[0], b[0]))
    return res


def _check_row(tag, row, sums, bnd, npos):
    """a CSV row of ``SSIM_COLUMNS`` against the columns of the float64 ``sums`` -> worst ratio"""
    from gan_sr_wind_field_amd.ssim import columns_from_sums

    want, allowed = columns_from_sums(sums, npos), columns_from_sums(bnd, npos)
    worst = 0.0
    for k, (g, w, a) in enumerate(zip(map(float, row), want, allowed)):
        lim = a + 2.0 ** -45 * abs(w)  # (+ the double arithmetic of the two evaluations)
        worst = max(worst, abs(g - w) / lim)
        assert abs(g - w) <= lim, (tag, k, g, w, lim)
    return worst


def _val_lines(path):
    """the validation averages the status log holds: [(iteration, {key: value})] per validation epoch"""
    out = []
    with open(path) as f:
        for line in f:
            m = re.search(r"train\.py: it: (\d+) (.*)$", line)
            if m:
                out.append((int(m.group(1)), {k: float(v) for k, v in re.findall(r"(\w+): (\S+)", m.group(2))}))
    return out


def test_run_train_and_test_three_ways_with_validation(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod
    from gan_sr_wind_field_amd.ssim import SSIM_COLUMNS, n_positions

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_ssim

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_ssim", counted)
    cls = gmod.wind_field_GAN_3D
    orig_val, orig_val_ssim = cls.validation, cls._val_ssim
    val = {}  # run name -> [(metrics of the batch, its float64 means and their bounds or None)]
    WIN, SIGMA = 11, 1.5

    def rec_val_ssim(self, LR, HR, fake_HR):
        orig_val_ssim(self, LR, HR, fake_HR)
        TL = hip_ops.trilinear_xy(LR.detach().float().contiguous(), self.cfg.scale)
        s, b = ref_ssim(HR, fake_HR.detach().float(), TL, WIN, SIGMA)
        n = 3 * HR.shape[0] * HR.shape[4] * n_positions(HR.shape[2], HR.shape[3], WIN)
        self._ssim_ref = (s.sum(dim=(0, 1, 2)) / n, b.sum(dim=(0, 1, 2)) / n)

    def rec_val(self, LR, HR, Z, it):
        self._ssim_ref = None
        orig_val(self, LR, HR, Z, it)
        m = self.get_metrics_dict_ref()
        types = {k: (torch.is_tensor(v) and v.is_cuda, getattr(v, "dtype", None)) for k, v in m.items() if "SSIM" in k}
        val.setdefault(self.cfg.name, []).append(({k: float(v) for k, v in m.items()}, self._ssim_ref, types, int(it)))

    monkeypatch.setattr(cls, "_val_ssim", rec_val_ssim)
    monkeypatch.setattr(cls, "validation", rec_val)

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
        # (read now: the loggers keep the file handlers of earlier runs, so a later run also writes into this file)
        log = os.path.join(str(tmp_path), "log", f"{name}.log")  # (a --test run alone writes none)
        logs[name] = [(it, e) for it, e in _val_lines(log) if "val_PSNR" in e] if os.path.exists(log) else []
        return cfg, os.path.join(str(tmp_path), "runs", name)

    logs = {}
    sec = "\n[SSIM]\nper_level = True\n"
    cfg_a, dir_a = run("plain", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n")
    assert calls["n"] == 0 and not any("ssim" in f for f in os.listdir("test_output"))  # never without the section
    _, dir_b = run("dev", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n" + sec)
    n_test, n_val = len(_read("dev", "metrics")) - 1, len(val["dev"])
    assert n_test > 1 and n_val > 0 and calls["n"] == n_val + -(-n_test // 2), calls  # once per batch
    _, dir_c = run("host", ["--train", "--test"], sec)
    assert calls["n"] == 2 * n_val + -(-n_test // 2), calls  # (validation on a GPU: the kernel; the host loop: torch ops)

    # the existing files of the first two runs: text-equal
    with open("test_output/plain____metrics.csv") as fa, open("test_output/dev____metrics.csv") as fb:
        assert fa.read() == fb.read()
    av = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert [r.split(",")[0] for r in av[1:]] == ["plain", "dev", "host"] and av[1].split(",", 1)[1] == av[2].split(",", 1)[1]
    assert sorted(os.listdir(os.path.join(dir_a, "fields"))) == sorted(os.listdir(os.path.join(dir_b, "fields")))

    _, te, _, _, _ = runmod.prepare_data(cfg_a)
    names = [te[i][3] for i in range(len(te))]
    X, Y, NZ = te[0][1].shape[1:]
    npos = n_positions(X, Y, WIN)
    worst = 0.0
    avs = open(os.path.join("test_output", "averages_ssim.csv")).read().strip().splitlines()
    assert avs[0] == "Name," + ",".join("Average " + k for k in SSIM_COLUMNS[:4]) and [r.split(",")[0] for r in avs[1:]] == ["dev", "host"]
    for at, (name, run_dir) in enumerate((("dev", dir_b), ("host", dir_c))):
        per_field = _float64_sums(run_dir, names, WIN, SIGMA)
        rows = _read(name, "ssim")
        assert rows[0] == ["field"] + list(SSIM_COLUMNS) and [r[0] for r in rows[1:]] == names
        for r, (s, b) in zip(rows[1:], per_field):
            worst = max(worst, _check_row(f"{name} {r[0]}", r[1:], s, b, npos))
        means = [float(v) for v in avs[1 + at].split(",")[1:]]
        for k, m in enumerate(means):  # the means of the per-field rows reproduce the averages
            assert m == pytest.approx(sum(float(r[1 + k]) for r in rows[1:]) / n_test, rel=1e-12)
        per = _read(name, "ssim_levels")
        assert per[0] == ["level"] + list(SSIM_COLUMNS) and [r[0] for r in per[1:]] == [str(k) for k in range(NZ)]
        total, total_b = sum(s for s, _ in per_field), sum(b for _, b in per_field)
        for lvl in range(NZ):
            worst = max(worst, _check_row(f"{name} level {lvl}", per[1 + lvl][1:], total[lvl:lvl + 1], total_b[lvl:lvl + 1],
                                          npos * n_test))
        for k in range(len(SSIM_COLUMNS)):  # the means over the levels reproduce the means over the fields
            assert sum(float(r[1 + k]) for r in per[1:]) / NZ == pytest.approx(
                sum(float(r[1 + k]) for r in rows[1:]) / n_test, rel=1e-12)
    print(f"[e2e] ssim.csv and ssim_levels.csv of both loops against float64: worst |err| / bound {worst:.3g}")

    # validation: the four keys without the section; with it two more, from the kernel, as device tensors, within the bound
    keys = ["val_PSNR", "Trilinear_PSNR", "pix_loss_unscaled", "trilinear_pix_loss"]
    assert all(list(m) == keys and ref is None for m, ref, _, _ in val["plain"])
    worst = 0.0
    for name in ("dev", "host"):
        assert len(val[name]) == n_val
        for m, (ref, bnd), types, _ in val[name]:
            assert list(m) == keys + ["val_SSIM", "Trilinear_SSIM"]
            assert set(types.values()) == {(True, torch.float64)}, types  # no read per key
            for key, j in (("val_SSIM", 0), ("Trilinear_SSIM", 2)):
                lim = float(bnd[j]) + 2.0 ** -45
                worst = max(worst, abs(m[key] - float(ref[j])) / lim)
                assert abs(m[key] - float(ref[j])) <= lim, (name, key, m[key], float(ref[j]), lim)
        logged = logs[name]
        assert logged and all("val_SSIM" in e and "Trilinear_SSIM" in e for _, e in logged)
        for it, entry in logged:  # the epoch's mean is the mean of its batches
            batch = [m for m, _, _, at in val[name] if at == it]
            assert batch
            for key in ("val_SSIM", "Trilinear_SSIM"):
                assert entry[key] == pytest.approx(sum(m[key] for m in batch) / len(batch), rel=1e-12), (name, it, key)
    assert logs["plain"] and all("SSIM" not in k for _, e in logs["plain"] for k in e)
    print(f"[e2e] val_SSIM and Trilinear_SSIM of every validation batch against float64: worst |err| / bound {worst:.3g}")

    # reverse interpolation: the second set of files, on the raw levels, from the same checkpoint
    load = dict(generator_load_path=os.path.join(dir_a, "G_6.pth"), discriminator_load_path=os.path.join(dir_a, "D_6.pth"),
                state_load_path=os.path.join(dir_a, "state_6.pth"))
    before = calls["n"]
    run("rev", ["--test"], "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n" + sec, interpolate_z=True, **load)
    assert calls["n"] - before == 2 * -(-n_test // 2)
    for what in ("ssim", "ssim_reverse_interpolate"):
        rows = _read("rev", what)
        assert rows[0] == ["field"] + list(SSIM_COLUMNS) and len(rows) == 1 + n_test, what
        assert all(math.isfinite(float(v)) and -1 <= float(v) <= 1 for r in rows[1:] for v in r[1:]), what
    assert _read("rev", "ssim") != _read("rev", "ssim_reverse_interpolate")
    assert len(_read("rev", "ssim_levels_reverse_interpolate")) == 1 + NZ
    rv = open(os.path.join("test_output", "averages_ssim_reverse_interpolate.csv")).read().strip().splitlines()
    assert len(rv) == 2 and rv[1].startswith("rev,")
    print(f"[time] tests/test_ssim_gpu.py up to here: {time.time() - T0:.1f} s")
