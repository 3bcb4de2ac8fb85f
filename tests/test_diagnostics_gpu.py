"""[DIAGNOSTICS] on the GPU: ``wsr_level_diagnostics`` (csrc/diagnostics.hip) against the float64 evaluation of the same
formulas (``ref_level_sums`` of tests/test_diagnostics.py, its own stencil code), analytic identities evaluated on the
device, refusals, and ``run.py --train --test`` without the section, with it under ``[EVAL]`` (the device loop) and with
it alone (the host loop).  The sums and the workspace of the kernel live in ``Guarded`` buffers.

Bounds (kernel_bounds.py's convention, LAMBDA = 16 untouched): per (sample, level, k)

    |got - ref| <= LAMBDA * sqrt(X * Y) * 2^-24 * A + 2^-100

with A the float64 sum of the term magnitudes listed in tests/test_diagnostics.py.  Nothing is measured against the code
under test.  The identities compare with analytic values: a linear field on dyadic coordinates (every product exact in
fp32) has div = a + b + c at every level; SR = HR turned about z by phi, formed in float64 and rounded once to fp32 - each
component moves by at most 2^-24 of itself, the horizontal vector and its angle by at most 2^-23 - has direction error
phi, speed bias 0 and an error vector of length 2 sin(phi / 2) h.

End to end the profile of each loop is held against the float64 profile of the fields THAT run pickled (its own SR and
baseline), under the bound above carried through ``profile_from_sums``; the two loops then agree within the sum of their
two bounds plus the distance of those two float64 profiles (the triangle inequality: the device loop's SR comes from a
forward of two fields, its baseline from ``wsr_trilinear_xy``).

Measured on an MI355X when the kernel was written: worst |err| / bound 0.076 for the sums against float64 (at 3 x 1 x 4;
0.071 at 4 x 3 x 256, 0.046 at 7 x 6 x 5, below 0.02 at the other shapes; the composed fp32 path on the device 0.067), 2.5e-4 for
the linear-field identity, 1.2e-4 for the profiles end to end; direction errors of the two rotations 0.29999996 .. 0.3 and
2.4999996 .. 2.5000002.  The whole file ran in 13.2 s.
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
from test_diagnostics import linear_case, profile_bounds, random_case, ref_level_sums, rotated, sum_bounds
from test_eval import metric_bounds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
NS = 15


def _launch(hip, HR, SR, TL, x, y, Z, label=""):
    """the C entry on device copies of the operands, sums and workspace in guarded buffers -> (B, NZ, 15) float64 on the
    host; a second launch must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    ops = [t.to(DEV).contiguous() for t in (HR, SR, TL, Z, x, y)]
    n_ws = int(hip.wsr_level_diagnostics_workspace_floats(B, X, Y, NZ))
    assert 0 < n_ws <= B * 1024 * NZ * NS
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, 2 * NS), torch.float32, DEV)  # (B, NZ, 15) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_diagnostics(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1], hip_ops._p(ops[2]),
                                        TL.shape[1], hip_ops._p(ops[3]), hip_ops._p(ops[4]), hip_ops._p(ops[5]), B, X, Y, NZ,
                                        hip_ops._p(ws.t), hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_diagnostics {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, NS)
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), f"{label}: two calls differ"
    wrapped = hip_ops.level_diagnostics(*ops[:3], ops[4], ops[5], ops[3])  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(wrapped.cpu().view(torch.int64), got[0].view(torch.int64)), label
    return got[0]


def _poisoned(t, c):
    """``c`` channels: the first three of t, the surplus ones NaN (they must never be read)"""
    if c == 3:
        return t[:, :3].contiguous()
    return torch.cat([t[:, :3], torch.full((t.shape[0], c - 3) + tuple(t.shape[2:]), float("nan"))], dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------- sums against float64
# (B, X, Y, NZ): NZ not dividing 256 and a partly filled last chunk; 12 x 10 x 6; 16 x 16 x 10; two columns per workgroup;
# several workgroups per sample (1600 columns in chunks of 32: 50 rows); a unit axis; NZ = 1; the largest NZ; and more
# chunks than WSR_LEVEL_DIAG_MAX_ROWS, the stride loop (NZ = 200: one column per pass, 1225 chunks on 1024 workgroups)
SUM_CASES = [(2, 7, 6, 5), (1, 12, 10, 6), (1, 16, 16, 10), (1, 9, 5, 128), (1, 40, 40, 8), (1, 3, 1, 4), (1, 5, 4, 1),
             (1, 4, 3, 256), (1, 35, 35, 200)]


@pytest.mark.parametrize("noise", [None, 1e-3], ids=["independent", "noise1e-3"])
@pytest.mark.parametrize("dims", SUM_CASES, ids=lambda d: "x".join(map(str, d)))
def test_sums_against_float64(hip, dims, noise):
    B, X, Y, NZ = dims
    HR, SR, TL, x, y, Z = random_case(B, X, Y, NZ, seed=X * 7 + NZ, noise=noise)
    ref, A = ref_level_sums(HR, SR, TL, x, y, Z)
    bnd = sum_bounds(A, X * Y)
    for c in (3, 5):
        got = _launch(hip, _poisoned(HR, c), _poisoned(SR, c), _poisoned(TL, 8 - c), x, y, Z, f"{dims} c={c}")
        assert_within(got, ref, bnd, f"level_diagnostics vs float64[{dims} noise={noise} c={c}]", kind="sums")
    if min(X, Y, NZ) >= 2:  # the composed torch path on the device, in fp32: the same bound
        from gan_sr_wind_field_amd.diagnostics import level_sums_reference

        dev = level_sums_reference(*(t.to(DEV) for t in (HR, SR, TL, x, y, Z)), dtype=torch.float32)
        assert_within(dev, ref, bnd, f"level_sums_reference fp32 on the device[{dims} noise={noise}]", kind="sums")


# ---------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("dims,abc", [((7, 6, 5), (0.5, -0.25, 1.5)), ((40, 40, 8), (1.0, 0.5, -0.25)), ((3, 1, 4), (2.0, 0.75, -0.5)),
                                      ((5, 4, 1), (1.0, 1.0, 3.0)), ((9, 5, 128), (-0.5, 0.25, 2.0))],
                         ids=lambda v: "x".join(map(str, v)))
def test_linear_field_has_rms_divergence_a_plus_b_plus_c(hip, dims, abc):
    X, Y, NZ = dims
    HR, x, y, Z = linear_case(X, Y, NZ, seed=X + NZ, abc=abc)
    got = _launch(hip, HR, HR, HR, x, y, Z, f"linear {dims}")[0]
    _, A = ref_level_sums(HR, HR, HR, x, y, Z)
    bnd = sum_bounds(A, X * Y)[0]
    want = sum(v for v, n in zip(abc, dims) if n > 1)  # (an axis of length 1 contributes 0)
    n = X * Y
    worst = 0.0
    for k in (10, 11, 12):
        err = (got[:, k] - n * want * want).abs()
        worst = max(worst, float((err / bnd[:, k]).max()))
        assert bool((err <= bnd[:, k]).all()), (dims, k, got[:, k].tolist(), n * want * want)
    rms = torch.sqrt(got[:, 10] / n)
    print(f"[identity] linear field {dims}: rms div in [{float(rms.min()):.9g}, {float(rms.max()):.9g}], |a + b + c| = "
          f"{abs(want)}, worst |err| / bound {worst:.3g}")


@pytest.mark.parametrize("phi", [0.3, 2.5])
def test_rotation_about_z_gives_direction_error_phi(hip, phi):
    B, X, Y, NZ = 1, 12, 10, 6
    HR, _, TL, x, y, Z = random_case(B, X, Y, NZ, seed=21)
    SR = rotated(HR, phi)
    got = _launch(hip, HR, SR, TL, x, y, Z, f"rotation {phi}")[0]
    ref, A = ref_level_sums(HR, SR, TL, x, y, Z)
    b = sum_bounds(A, X * Y)[0]
    s0, s7 = ref[0, :, 0], ref[0, :, 7]  # (float64 sums of the inputs: the size of the 2^-23 input rounding terms)
    c = 2 * math.sin(phi / 2)
    checks = {"direction": ((got[:, 8] - phi * got[:, 7]).abs(), b[:, 8] + phi * b[:, 7] + 2.0 ** -23 * s7),
              "speed bias": (got[:, 3].abs(), b[:, 3] + 2.0 ** -23 * s0),
              "pix": ((got[:, 1] - c * got[:, 7]).abs(), b[:, 1] + c * b[:, 7] + 2.0 ** -23 * s0)}
    for name, (err, allowed) in checks.items():
        assert bool((err <= allowed).all()), (name, phi, err.tolist(), allowed.tolist())
    print(f"[identity] rotation by {phi}: direction error per level {(got[:, 8] / got[:, 7]).tolist()}")


def test_sr_equal_hr_gives_exact_zeros(hip):
    for dims in ((1, 7, 6, 5), (1, 9, 5, 128)):
        B, X, Y, NZ = dims
        HR, _, TL, x, y, Z = random_case(B, X, Y, NZ, seed=33)
        got = _launch(hip, HR, HR.clone(), TL, x, y, Z, f"SR = HR {dims}")
        assert bool((got[..., [1, 3, 5, 8]] == 0).all()), dims
        assert torch.equal(got[..., 10].view(torch.int64), got[..., 11].view(torch.int64)), dims
        assert bool((got[..., 14][:, 0] == 0).all()) and bool((got[..., 2] > 0).all())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 2, 2, 257
    HR, SR, TL, x, y, Z = (t.to(DEV).contiguous() for t in random_case(B, X, Y, NZ, seed=1))
    out = Guarded((B, NZ, 2 * NS), torch.float32, DEV)
    ws = Guarded((B * 4 * NZ * NS,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, zc=Z, xs=x, ys=y, b=B, nx=X, ny=Y, nz=4, w=ws.t, o=out.t):
        return hip.wsr_level_diagnostics(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, p(zc), p(xs), p(ys), b, nx, ny, nz, p(w), p(o),
                                         hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(tl=None), dict(zc=None), dict(xs=None), dict(ys=None), dict(w=None),
               dict(o=None), dict(hr_c=2), dict(sr_c=2), dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0)]
    for kw in invalid:
        assert call(**kw) == -1, kw
    assert call(nz=257) == -2 and call(b=65536) == -2 and call(nx=32769) == -2 and call(nx=32768, ny=32768, nz=2) == -2
    assert hip.wsr_level_diagnostics_workspace_floats(1, 2, 2, 257) == 0 == hip.wsr_level_diagnostics_workspace_floats(0, 2, 2, 4)
    assert hip.wsr_level_diagnostics_workspace_floats(2, 7, 6, 5) == 2 * 1 * 5 * NS  # 42 columns: one chunk of 51
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    H4, S4, T4, Z4 = HR[..., :4].contiguous(), SR[..., :4].contiguous(), TL[..., :4].contiguous(), Z[..., :4].contiguous()
    ok = hip_ops.level_diagnostics(H4, S4, T4, x, y, Z4)
    assert ok.shape == (B, 4, NS) and bool(torch.isfinite(ok).all())
    bad = [(HR, SR, TL, x, y, Z), (H4[:, :2].contiguous(), S4, T4, x, y, Z4), (H4.double(), S4, T4, x, y, Z4),
           (H4, S4[..., :3], T4, x, y, Z4), (H4, S4[..., :3].contiguous(), T4, x, y, Z4), (H4, S4, T4[:, :, :1].contiguous(), x, y, Z4),
           (H4, S4, T4, x[:1], y, Z4), (H4, S4, T4, x, y.double(), Z4), (H4, S4, T4, x, y, H4), (H4, S4, T4, x, y, Z4[..., :2].contiguous())]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_diagnostics(*args)
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_diagnostics(H4, S4, T4, x, y, Z4, out=torch.empty((B, 4, NS), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_diagnostics(H4.cpu(), S4, T4, x, y, Z4)


def test_gan_level_diagnostics_builds_the_baseline_and_calls_the_kernel(hip):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from test_diagnostics import gan_stub

    HR, SR, _, x, y, Z = (t.to(DEV) for t in random_case(2, 12, 8, 5, seed=4))
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5)).to(DEV)
    got = wind_field_GAN_3D.level_diagnostics(gan_stub(x.cpu(), y.cpu()), HR, SR, LR, Z)  # (coordinates from anywhere)
    want = hip_ops.level_diagnostics(HR, SR, hip_ops.trilinear_xy(LR, 4), x, y, Z)
    assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got.view(torch.int64), want.view(torch.int64))
    ref, A = ref_level_sums(HR, SR, hip_ops.trilinear_xy(LR, 4), x, y, Z)
    assert_within(got, ref, sum_bounds(A, 12 * 8), "gan.level_diagnostics vs float64[(2, 12, 8, 5)]", kind="sums")


# ---------------------------------------------------------------------------------------------------- run.py
def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _float64_profile(run_dir, names, x, y, uvw):
    """(profile, bounds, sums) of the fields a run pickled, in float64 from its own HR / SR / TL / Z"""
    from gan_sr_wind_field_amd.diagnostics import profile_from_sums

    total = bound = None
    for name in names:
        p = pickle.load(open(os.path.join(run_dir, "fields", f"test_fields_{name}.pkl"), "rb"))
        HR, SR, TL, Z = (torch.from_numpy(np.asarray(p[k]))[None] for k in ("HR", "SR", "TL", "Z"))
        if Z.dim() == 4:
            Z = Z[:, None]
        s, A = ref_level_sums(HR, SR, TL, x, y, Z)
        b = sum_bounds(A, HR.shape[2] * HR.shape[3])
        total = s[0] if total is None else total + s[0]
        bound = b[0] if bound is None else bound + b[0]
    ncols = len(names) * HR.shape[2] * HR.shape[3]
    return profile_from_sums(total, ncols, uvw), profile_bounds(total, bound, ncols, uvw), total


def test_run_train_and_test_without_and_with_the_section_in_both_loops(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.diagnostics import PROFILE_COLUMNS
    from gan_sr_wind_field_amd.test import METRIC_NAMES

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_diagnostics

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_diagnostics", counted)

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

    diag = "\n[DIAGNOSTICS]\nlevel_profile = True\nper_field = True\n"
    cfg_a, dir_a = run("plain", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n")
    assert calls["n"] == 0 and not any("level_profile" in f for f in os.listdir("test_output"))  # never without the section
    _, dir_b = run("dev", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n" + diag)
    n_test = len(_read("dev", "metrics")) - 1
    assert n_test > 1 and calls["n"] == -(-n_test // 2), calls  # once per batch
    _, dir_c = run("host", ["--train", "--test"], diag)
    assert calls["n"] == -(-n_test // 2), calls  # the host loop composes torch ops
    with open(os.path.join(dir_b, "config.ini")) as f:
        assert f.read().endswith("\n[DIAGNOSTICS]\nlevel_profile = True\nper_field = True\n")

    # the existing files of the first two runs: text-equal
    with open("test_output/plain____metrics.csv") as fa, open("test_output/dev____metrics.csv") as fb:
        assert fa.read() == fb.read()
    av = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert [r.split(",")[0] for r in av[1:]] == ["plain", "dev", "host"] and av[1].split(",", 1)[1] == av[2].split(",", 1)[1]
    assert sorted(os.listdir(os.path.join(dir_a, "fields"))) == sorted(os.listdir(os.path.join(dir_b, "fields")))

    _, te, _, _, _ = runmod.prepare_data(cfg_a)
    x, y = (torch.from_numpy(np.asarray(v)).float() for v in (te.x, te.y))  # (the whole test domain)
    uvw = float(te.UVW_MAX)
    names = [te[i][3] for i in range(len(te))]
    NZ, nvox = te[0][1].shape[-1], math.prod(te[0][1].shape[1:])
    worst = 0.0
    prof, f64 = {}, {}
    for name, d in (("dev", dir_b), ("host", dir_c)):
        rows = _read(name, "level_profile")
        assert rows[0] == ["level"] + list(PROFILE_COLUMNS) and [r[0] for r in rows[1:]] == [str(k) for k in range(NZ)]
        prof[name] = {k: [float(r[1 + i]) for r in rows[1:]] for i, k in enumerate(PROFILE_COLUMNS)}
        assert all(math.isfinite(v) for col in prof[name].values() for v in col), name
        f64[name] = _float64_profile(d, names, x, y, uvw)
        want, bnd, _ = f64[name]
        for k in PROFILE_COLUMNS:
            for lvl in range(NZ):
                err = abs(prof[name][k][lvl] - want[k][lvl])
                allowed = bnd[k][lvl] + 2.0 ** -50 * abs(want[k][lvl])  # (+ the double arithmetic of the two evaluations)
                worst = max(worst, err / allowed)
                assert err <= allowed, (name, k, lvl, prof[name][k][lvl], want[k][lvl], allowed)
    # the two loops agree: their two bounds and the distance of the float64 profiles of their own inputs
    for k in PROFILE_COLUMNS:
        for lvl in range(NZ):
            allowed = (f64["dev"][1][k][lvl] + f64["host"][1][k][lvl] + abs(f64["dev"][0][k][lvl] - f64["host"][0][k][lvl])
                       + 2.0 ** -50 * abs(f64["host"][0][k][lvl]))
            assert abs(prof["dev"][k][lvl] - prof["host"][k][lvl]) <= allowed, (k, lvl)
    print(f"[e2e] level profiles of both loops against float64: worst |err| / bound {worst:.3g}")

    # the mean over levels of three columns is the run's averages.csv entry
    for name, row in (("dev", av[2]), ("host", av[3])):
        avg = dict(zip(METRIC_NAMES, map(float, row.split(",")[1:])))
        bnd = metric_bounds(avg, nvox)
        rel = sum_bounds(torch.tensor(1.0), nvox // NZ).item()  # (non-negative terms: the bound is relative to the sum)
        for k in ("pix", "trilinear_pix", "average_wind_speed"):
            mean = sum(prof[name][k]) / NZ
            assert abs(mean - avg[k]) <= bnd[k] + (rel + 2.0 ** -22) * abs(avg[k]), (name, k, mean, avg[k])

    # per field: fields x NZ rows, and their means (root mean squares for the divergences) reproduce the profile
    for name in ("dev", "host"):
        per = _read(name, "level_profile_fields")
        assert per[0] == ["field", "level"] + list(PROFILE_COLUMNS) and len(per) == 1 + n_test * NZ
        assert [r[0] for r in per[1::NZ]] == names and [r[1] for r in per[1:1 + NZ]] == [str(k) for k in range(NZ)]
        for i, k in enumerate(PROFILE_COLUMNS):
            for lvl in range(NZ):
                col = [float(r[2 + i]) for r in per[1:] if int(r[1]) == lvl]
                got = prof[name][k][lvl]
                if k.startswith("direction"):  # (a speed-weighted mean of the fields' angles)
                    assert min(col) * (1 - 1e-12) <= got <= max(col) * (1 + 1e-12), (name, k, lvl)
                    continue
                want = math.sqrt(sum(v * v for v in col) / len(col)) if k.startswith("rms_div") else sum(col) / len(col)
                assert got == pytest.approx(want, rel=1e-12, abs=1e-12), (name, k, lvl)

    # reverse interpolation: the second file, on the raw levels, from the same checkpoint
    load = dict(generator_load_path=os.path.join(dir_a, "G_6.pth"), discriminator_load_path=os.path.join(dir_a, "D_6.pth"),
                state_load_path=os.path.join(dir_a, "state_6.pth"))
    before = calls["n"]
    run("rev", ["--test"], "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n" + diag, interpolate_z=True, **load)
    assert calls["n"] - before == 2 * -(-n_test // 2)
    for what in ("level_profile", "level_profile_reverse_interpolate"):
        rows = _read("rev", what)
        assert rows[0] == ["level"] + list(PROFILE_COLUMNS) and len(rows) == 1 + NZ, what
        assert all(math.isfinite(float(v)) for r in rows[1:] for v in r[1:]), what
    assert _read("rev", "level_profile") != _read("rev", "level_profile_reverse_interpolate")
    assert len(_read("rev", "level_profile_fields_reverse_interpolate")) == 1 + n_test * NZ
    print(f"[time] tests/test_diagnostics_gpu.py up to here: {time.time() - T0:.1f} s")
