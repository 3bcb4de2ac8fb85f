"""[DISTRIBUTION] on the GPU: ``wsr_level_distribution`` (csrc/distribution.hip) against
``distribution.level_distribution_reference`` evaluated on the CPU.  The counts are integers and the classes are defined
by fp32 operations in a fixed order, so every comparison of tables is ``torch.equal`` on the float64 values: no tolerance.
The counts and the workspace of the kernel live in ``Guarded`` buffers whose sentinel is no count: a call that leaves an
element of ``out`` unwritten fails the comparison.

The shapes: smaller than any tile, the reference's patch, level chunks with a remainder, and one level more than the
chunk a workgroup counts at each parameter set (``hip_ops.distribution_level_chunk``, from the header's
``WSR_DISTRIBUTION_LDS_COUNTERS``).  tools/distribution_host_check.cpp ran clean under the address and
undefined-behaviour sanitisers at these shapes and parameter sets, with the special voxels of ``distribution_cases``.

End to end the HR columns of the new files are the same text in the device loop and in the host loop; the SR and
baseline frequencies may differ by 2 / n (one voxel that changes class, n voxels): SR differs in its low digits between
batch sizes, the baseline between ``F.interpolate`` and ``wsr_trilinear_xy``.
"""
import csv
import os
import time
from types import SimpleNamespace

import pytest
import torch

from distribution_cases import CALMS, NAN, PARAMS, fields, plant_specials, tables
from kernel_bounds import Guarded, assert_guards_intact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
CASES = [(ns, nd, calm) for ns, nd in PARAMS for calm in CALMS]


def case_id(c):
    return f"{c[0]}x{c[1]}_calm{c[2]}"


def _bits(t):
    return t.contiguous().view(torch.int64)


def _launch(hip, HR, SR, TL, t, label=""):
    """the C entry on device copies of the operands, counts and workspace in guarded buffers -> (B, NZ, 3, NS, ND + 1)
    float64 on the host; a second launch, the wrapper and the wrapper with ``out=`` must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    ns, nd = t.speed_bins, t.sectors
    ops = [None if f is None else f.to(DEV).contiguous() for f in (HR, SR, TL)]
    edge2, bx, by = (v.to(DEV) for v in (t.edge2, t.bx, t.by))
    n_ws = int(hip.wsr_level_distribution_workspace_floats(B, X, Y, NZ, ns, nd))
    assert n_ws == B * NZ * 3 * ns * (nd + 1)
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, 3, ns, 2 * (nd + 1)), torch.float32, DEV)  # (B, NZ, 3, NS, ND + 1) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_distribution(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1],
                                         hip_ops._p(ops[2]), 0 if TL is None else TL.shape[1], hip_ops._p(edge2), ns,
                                         hip_ops._p(bx), hip_ops._p(by), nd, t.calm2, B, X, Y, NZ, hip_ops._p(ws.t),
                                         hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_distribution {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, 3, ns, nd + 1)
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    wrapped = hip_ops.level_distribution(*ops, t)  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(_bits(wrapped.cpu()), _bits(got[0])), label
    into = torch.full((B, NZ, 3, ns, nd + 1), NAN, dtype=torch.float64, device=DEV)
    assert hip_ops.level_distribution(*ops, t, out=into) is into
    assert torch.equal(_bits(into.cpu()), _bits(got[0])), label
    return got[0]


def _check(hip, HR, SR, TL, t, label):
    from gan_sr_wind_field_amd.distribution import level_distribution_reference

    want = level_distribution_reference(HR, SR, TL, t)
    got = _launch(hip, HR, SR, TL, t, label)
    B, _, X, Y, NZ = HR.shape
    assert bool((want[:, :, :2].sum(dim=(3, 4)) == X * Y).all())
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{label}: {bad.shape[0]} counts differ, the first at (b, z, source, bin, sector) = "
                             f"{bad[0].tolist()}: {float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}")
    return got


def _shapes(ns, nd):
    from gan_sr_wind_field_amd import hip_ops

    chunk = hip_ops.distribution_level_chunk(10 ** 6, ns, nd)
    assert chunk == hip_ops.DISTRIBUTION_LDS_COUNTERS // (ns * (nd + 1))
    return [(1, 5, 7, 3), (3, 16, 16, 10), (2, 33, 17, 37), (1, 8, 8, 130), (1, 3, 2, chunk + 1)]


# ---------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_counts_equal_the_reference(hip, case):
    ns, nd, calm = case
    t = tables(ns, nd, calm)
    for k, shape in enumerate(_shapes(ns, nd)):
        HR, SR, TL = fields(*shape, seed=10 + k, channels=(4, 3, 3))
        got = _check(hip, HR, SR, TL, t, f"{case_id(case)} {shape}")
        assert not torch.equal(got[:, :, 0], got[:, :, 1])  # (the sources differ)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_special_voxels(hip, case):
    """ties, bin edges, zeros, NaN and +-Inf at the first and the last voxels and across a level-chunk boundary"""
    from gan_sr_wind_field_amd import hip_ops

    ns, nd, calm = case
    t = tables(ns, nd, calm)
    for shape in ((2, 9, 5, 37), (1, 6, 5, hip_ops.distribution_level_chunk(10 ** 6, ns, nd) + 1)):
        chunk = hip_ops.distribution_level_chunk(shape[3], ns, nd)
        HR, SR, TL = plant_specials(fields(*shape, seed=21, channels=(4, 3, 3)), chunk, ns)
        assert bool(torch.isnan(HR[:, :2]).any()) and bool(torch.isinf(SR[:, :2]).any())
        _check(hip, HR, SR, TL, t, f"special voxels {case_id(case)} {shape}")


def test_concentration_and_one_level_apart(hip):
    """every voxel of a level the same vector: one counter holds X * Y (every lane adds to one address); then one level
    holds another vector than all the others"""
    B, X, Y, NZ = 2, 33, 17, 37
    for ns, nd, calm in ((32, 16, 0.5), (64, 36, 0.0)):
        t = tables(ns, nd, calm)
        f = torch.zeros((B, 3, X, Y, NZ))
        f[:, 0], f[:, 1] = 0.2, -0.1
        got = _check(hip, f, f.clone(), f.clone(), t, "concentration")
        assert float(got.max()) == X * Y and int((got != 0).sum()) == B * NZ * 3
        for z in (0, 5, NZ - 1):  # (also the last level of a chunk with a remainder)
            g = f.clone()
            g[:, 0, :, :, z], g[:, 1, :, :, z] = -0.3, 0.4
            got = _check(hip, f, g, f, t, f"level {z} apart")
            same = [k for k in range(NZ) if k != z]
            assert torch.equal(got[:, same, 1], got[:, same, 0]) and not torch.equal(got[:, z, 1], got[:, z, 0])
            assert float(got[:, z, 1].max()) == X * Y


# ---------------------------------------------------------------------------------------------------- completeness
def test_no_baseline_and_another_stream(hip):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.distribution import level_distribution_reference

    t = tables()
    HR, SR, TL = fields(2, 33, 17, 37, seed=4, channels=(3, 4, 3))
    got = _check(hip, HR, SR, None, t, "tl = NULL")
    assert float(got[:, :, 2].abs().sum()) == 0 and float(got[:, :, :2].sum()) == 2 * 2 * 33 * 17 * 37
    # another stream: the operand is written on that stream just before the launch
    want = level_distribution_reference(HR, SR, TL, t)
    ops = [f.to(DEV) for f in (HR, SR, TL)]
    stale = torch.zeros_like(ops[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stale.copy_(ops[0], non_blocking=True)
        assert hip_ops._stream().value == s.cuda_stream
        out = hip_ops.level_distribution(stale, ops[1], ops[2], t)
    s.synchronize()
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ, ns, nd = 1, 6, 5, 3, 32, 16
    t = tables(ns, nd, 0.5)
    HR, SR, TL = (f.to(DEV) for f in fields(B, X, Y, NZ, seed=1, channels=(3, 3, 3)))
    big = tables(64, 36, 0.5)  # (long enough for every table size the calls below name)
    E2, BX, BY = (v.to(DEV) for v in (big.edge2, big.bx, big.by))
    n_ws = int(hip.wsr_level_distribution_workspace_floats(B, X, Y, NZ, ns, nd))
    assert n_ws > 0
    out = Guarded((B, NZ, 3, ns, 2 * (nd + 1)), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, e2=E2, n_s=ns, b_x=BX, b_y=BY, n_d=nd, b=B, nx=X, ny=Y, nz=NZ,
             w=ws.t, o=out.t):
        return hip.wsr_level_distribution(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, p(e2), n_s, p(b_x), p(b_y), n_d, t.calm2, b,
                                          nx, ny, nz, p(w), p(o), hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(e2=None), dict(b_x=None), dict(b_y=None), dict(w=None), dict(o=None),
               dict(hr_c=2), dict(sr_c=2), dict(tl_c=2), dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0),
               dict(n_s=1), dict(n_s=65), dict(n_s=-4), dict(n_d=2), dict(n_d=5), dict(n_d=15), dict(n_d=38), dict(n_d=0)]
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(b=65536), dict(nx=65536, ny=32768), dict(nx=32768, ny=32768, nz=2)):
        assert call(**kw) == -2, kw
    wsf = hip.wsr_level_distribution_workspace_floats
    assert wsf(0, X, Y, NZ, ns, nd) == wsf(1, X, Y, NZ, 65, nd) == wsf(1, X, Y, NZ, ns, 7) == wsf(65536, X, Y, NZ, ns, nd) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    ok = hip_ops.level_distribution(HR, SR, TL, t)
    assert ok.shape == (B, NZ, 3, ns, nd + 1) and float(ok.sum()) == 3 * X * Y * NZ
    bad = [(HR[:, :2].contiguous(), SR, TL), (HR.double(), SR, TL), (HR, SR[..., :2], TL), (HR, SR[..., :2].contiguous(), TL),
           (HR, SR, TL[:, :, :3].contiguous()), (HR, SR, torch.cat([TL, TL]))]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_distribution(*args, t)
    for kw, pattern in ((dict(speed_bins=65), "speed_bins.*65"), (dict(sectors=5), "sectors.*5"),
                        (dict(bin_width=0.0), "bin_width"), (dict(calm=-1.0), "calm.*-1"),
                        (dict(edge2=t.edge2[:-1]), "31 edges")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.level_distribution(HR, SR, TL, t._replace(**kw))
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_distribution(HR, SR, TL, t, out=torch.empty((B, NZ, 3, ns, nd + 1), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_distribution(HR.cpu(), SR, TL, t)
    # the tables are uploaded once per (device, parameters)
    n = len(hip_ops._distribution_tables)
    hip_ops.level_distribution(HR, SR, TL, t)
    hip_ops.level_distribution(HR, SR, TL, tables(ns, nd, 0.5))
    assert len(hip_ops._distribution_tables) == n
    hip_ops.level_distribution(HR, SR, TL, tables(ns, nd, 0.25))
    assert len(hip_ops._distribution_tables) == n + 1


# ---------------------------------------------------------------------------------------------------- the model's entry
def gan_stub(scale=4, **section):
    """what ``wind_field_GAN_3D.level_distribution`` uses of its object: the scale and the section"""
    from gan_sr_wind_field_amd.config.config import DistributionConfig

    dc = DistributionConfig()
    dc.setDistributionConfig(None)
    for k, v in section.items():
        setattr(dc, k, v)
    return SimpleNamespace(cfg=SimpleNamespace(scale=scale, distribution=dc))


def test_gan_level_distribution(hip):
    import torch.nn.functional as F

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.distribution import level_distribution_reference
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    HR, SR, _ = fields(2, 12, 8, 5, seed=4, channels=(3, 3, 3))
    LR = 0.25 * torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    for stub, t in ((gan_stub(), tables(32, 16, 0.5, 1.0, 20.0)),  # (no section: its defaults, bin_width 1.0)
                    (gan_stub(present=True, bin_width=0.5, speed_bins=40, sectors=12, calm=0.2), tables(40, 12, 0.2, 0.5, 20.0))):
        got = wind_field_GAN_3D.level_distribution(stub, HR.to(DEV), SR.to(DEV), LR.to(DEV), 20.0)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (2, 5, 3, t.speed_bins, t.sectors + 1)
        TL_dev = hip_ops.trilinear_xy(LR.to(DEV), 4).cpu()
        want = level_distribution_reference(HR, SR, TL_dev, t)
        assert torch.equal(got.cpu(), want)  # HR, SR and the device baseline: exact
        # the baseline of F.interpolate differs in its low digits (a matter of [EVAL]): HR and SR are compared
        host = level_distribution_reference(HR, SR, F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear",
                                                                   align_corners=True), t)
        assert torch.equal(host[:, :, :2], got.cpu()[:, :, :2])
        print(f"[gan] baseline counts, F.interpolate against wsr_trilinear_xy: summed |difference| "
              f"{float((host[:, :, 2] - got.cpu()[:, :, 2]).abs().sum()):g}")
        # on a CPU device the same entry is the reference
        assert torch.equal(wind_field_GAN_3D.level_distribution(stub, HR, SR, LR, 20.0), host)


# ---------------------------------------------------------------------------------------------------- run.py
def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _earlier_files(name, run_dir):
    """the files a run without the section writes: path relative to the run -> bytes"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____") and "____wind_" not in f:
            with open(os.path.join("test_output", f), "rb") as fh:
                out[f[len(name):]] = fh.read()
    for f in sorted(os.listdir(os.path.join(run_dir, "fields"))):
        with open(os.path.join(run_dir, "fields", f), "rb") as fh:
            out["fields/" + f] = fh.read()
    return out


def test_run_test_device_loop_against_host_loop(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.distribution import ROSE_COLUMNS, SPEED_COLUMNS, SUMMARY_COLUMNS

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_distribution

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_distribution", counted)

    def run(name, flags, section, **env):
        ini = str(tmp_path / f"{name}.ini")
        cfg = _write_ini(ini)
        cfg.name = name
        cfg.gan_config.interpolate_z = True
        for k, v in env.items():
            setattr(cfg.env, k, v)
        with open(ini, "w") as f:
            f.write(cfg.asINI() + section)
        runmod.main(flags + ["--cfg", ini])
        return cfg, os.path.join(str(tmp_path), "runs", name)

    dev_loop = "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n"
    host_loop = "\n[EVAL]\ndevice_metrics = False\nreverse_interpolate = True\n"
    sec = "\n[DISTRIBUTION]\nbin_width = 0.5\nspeed_bins = 40\nsectors = 12\ncalm = 0.25\nper_level = True\n"
    cfg_t, dir_t = run("trained", ["--train"], "")
    load = dict(generator_load_path=os.path.join(dir_t, "G_6.pth"), discriminator_load_path=os.path.join(dir_t, "D_6.pth"),
                state_load_path=os.path.join(dir_t, "state_6.pth"))
    _, dir_a = run("plain", ["--test"], dev_loop, **load)
    assert calls["n"] == 0 and not any("wind_" in f.split("____")[-1] or "distribution" in f for f in os.listdir("test_output"))
    _, dir_b = run("dev", ["--test"], dev_loop + sec, **load)
    n_test = len(_read("dev", "metrics")) - 1
    assert n_test > 1 and calls["n"] == 2 * -(-n_test // 2), calls  # once per batch and set of levels
    _, dir_c = run("host", ["--test"], host_loop + sec, **load)
    assert calls["n"] == 2 * -(-n_test // 2), calls  # (the host loop: torch ops)

    # every earlier file: byte for byte those of the run without the section
    a, b = _earlier_files("plain", dir_a), _earlier_files("dev", dir_b)
    assert sorted(a) == sorted(b) and len(a) >= 2 + n_test // 2
    for k in a:
        assert a[k] == b[k], k
    av = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert [r.split(",")[0] for r in av[1:]] == ["plain", "dev", "host"] and av[1].split(",", 1)[1] == av[2].split(",", 1)[1]

    _, te, _, _, _ = runmod.prepare_data(cfg_t)
    X, Y, NZ = te[0][1].shape[1:]
    n = n_test * X * Y * NZ
    worst = 0.0
    for suffix in ("", "_reverse_interpolate"):
        for what, first, columns, rows_n in (("wind_distribution", "bin", SPEED_COLUMNS, 40), ("wind_rose", "sector", ROSE_COLUMNS, 13)):
            d, h = _read("dev", what + suffix), _read("host", what + suffix)
            assert d[0] == h[0] == [first] + list(columns) and len(d) == len(h) == 1 + rows_n, (what, suffix)
            assert [r[:4] for r in d] == [r[:4] for r in h], (what, suffix)  # the labels, the edges and f_HR: the same text
            assert sum(float(r[3]) for r in d[1:]) == pytest.approx(1, abs=1e-12)
            for rd, rh in zip(d[1:], h[1:]):
                for k in (4, 5):  # f_SR, f_trilinear
                    worst = max(worst, abs(float(rd[k]) - float(rh[k])) * n / 2)
                    assert abs(float(rd[k]) - float(rh[k])) <= 2 / n * (1 + 1e-9), (what, suffix, rd, rh)
        lv = _read("dev", "wind_distribution_levels" + suffix)
        assert lv[0] == ["level"] + list(SUMMARY_COLUMNS) and [r[0] for r in lv[1:]] == [str(k) for k in range(NZ)]
        avd = open(os.path.join("test_output", f"averages_distribution{suffix}.csv")).read().strip().splitlines()
        assert avd[0] == "Name," + ",".join(SUMMARY_COLUMNS) and [r.split(",")[0] for r in avd[1:]] == ["dev", "host"]
        dv, hv = ([float(v) for v in r.split(",")[1:]] for r in avd[1:])
        hr_cols = [k for k, c in enumerate(SUMMARY_COLUMNS) if c.endswith("_HR")]
        assert [dv[k] for k in hr_cols] == [hv[k] for k in hr_cols]
        assert 0 < dv[0] <= 1 and 0 < dv[1] <= 1
    assert _read("dev", "wind_distribution") != _read("dev", "wind_distribution_reverse_interpolate")
    print(f"[e2e] f_SR, f_trilinear of the device loop against the host loop: worst |difference| / (2 / n) {worst:.3g}")
    print(f"[time] tests/test_distribution_gpu.py up to here: {time.time() - T0:.1f} s")
