"""[FSS] on the GPU: ``wsr_level_fss`` (csrc/fss.hip) against ``fss.level_fss_reference`` evaluated on the CPU.  The sums
are integers and the events are defined by fp32 operations in a fixed order, so every comparison of tables is
``torch.equal`` on the float64 values: no tolerance.  The sums and the workspace of the kernel live in ``Guarded`` buffers
whose sentinel is no sum: a call that leaves an element of ``out`` unwritten fails the comparison.

The shapes: a plane smaller than every halo, the reference's patch, odd sizes with tile and chunk remainders, more levels
than any chunk, a plane where the halo of n = 33 reaches past the neighbouring tile, and a launch large enough for the
six-level chunk (``hip_ops.fss_level_chunk``; smaller launches stage two levels per workgroup).
tools/fss_host_check.cpp ran clean under the address and undefined-behaviour sanitisers at these shapes and parameter
sets, with the special voxels of ``fss_cases``.

End to end the HR-only columns (``f_HR``, ``FSS_uniform``) of the new files are the same text in the device loop and in
the host loop; SR differs in its low digits between batch sizes and the baseline between ``F.interpolate`` and
``wsr_trilinear_xy``, so a few voxels next to a threshold change sides: the SR and baseline scores are compared with
``E2E_FLIPS`` voxels' worth of change.
"""
import csv
import math
import os
import time
from types import SimpleNamespace

import pytest
import torch

from fss_cases import DEFAULT_SCALES, NAN, PARAMS, SEEDS, SHAPES, fields, plant_specials, tables, tie_tables
from kernel_bounds import Guarded, assert_guards_intact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
BIG = (64, 8, 8, 48)  # 512 workgroups at the widest halo: the chunk of six levels
#: The SR and baseline scores of the device loop against the host loop: |difference| <= E2E_FLIPS * 4 / (events of HR at
#: the row's threshold in the whole set).  A voxel of SR or of the baseline that changes sides of a threshold moves hits,
#: misses or false alarms by 1, so a contingency score - a ratio whose denominator holds the events of HR - by at most
#: 2 / events; at a neighbourhood n it moves n^2 counts by 1, srd by at most sum (2 |c_SR - c_HR| + 1) <= 2 (hr2 + sr2) /
#: (mean count) + n^2, which is again of the order of 2 / events of the score: 4 / events covers both.  Measured on an
#: MI355X when the test was written: no voxel changed sides, every score the same text (worst |difference| 0).
E2E_FLIPS = 2

_reference = {}


def case_id(c):
    return f"{len(c[0])}thr_{len(c[1])}scales"


def _bits(t):
    return t.contiguous().view(torch.int64)


def _inputs(shape, seed):
    """HR, SR, TL of ``fields`` (HR with a fourth channel of NaN), made once per shape"""
    key = ("fields", shape, seed)
    if key not in _reference:
        _reference[key] = fields(*shape, seed=seed, channels=(4, 3, 3))
    return _reference[key]


def _want(shape, seed, thresholds, scales, tl=True):
    """the CPU reference of ``_inputs(shape, seed)``, computed once and shared"""
    from gan_sr_wind_field_amd.fss import level_fss_reference

    key = ("sums", shape, seed, thresholds, scales, tl)
    if key not in _reference:
        HR, SR, TL = _inputs(shape, seed)
        _reference[key] = level_fss_reference(HR, SR, TL if tl else None, tables(thresholds), scales)
    return _reference[key]


def _launch(hip, HR, SR, TL, t, scales, label=""):
    """the C entry on device copies of the operands, sums and workspace in guarded buffers -> (B, NZ, NT, NN, 5) float64
    on the host; a second launch, the wrapper and the wrapper with ``out=`` must give the same bits"""
    import ctypes

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    nt, nn = t.thr2.numel(), len(scales)
    ops = [None if f is None else f.to(DEV).contiguous() for f in (HR, SR, TL)]
    thr2 = t.thr2.to(DEV)
    n_ws = int(hip.wsr_level_fss_workspace_floats(B, X, Y, NZ, nt, nn, scales[-1]))
    assert n_ws == 2 * B * NZ * nt * nn * 5
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, nt, nn, 2 * 5), torch.float32, DEV)  # (B, NZ, NT, NN, 5) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_fss(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1], hip_ops._p(ops[2]),
                                0 if TL is None else TL.shape[1], hip_ops._p(thr2), nt, (ctypes.c_int32 * nn)(*scales), nn,
                                B, X, Y, NZ, hip_ops._p(out.t), hip_ops._p(ws.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_fss {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, nt, nn, 5)
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    wrapped = hip_ops.level_fss(*ops, t, scales)  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(_bits(wrapped.cpu()), _bits(got[0])), label
    into = torch.full((B, NZ, nt, nn, 5), NAN, dtype=torch.float64, device=DEV)
    assert hip_ops.level_fss(*ops, t, scales, out=into) is into
    assert torch.equal(_bits(into.cpu()), _bits(got[0])), label
    return got[0]


def _compare(got, want, label):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{label}: {bad.shape[0]} sums differ, the first at (b, z, threshold, scale, sum) = "
                             f"{bad[0].tolist()}: {float(got[tuple(bad[0])])} != {float(want[tuple(bad[0])])}")


# ---------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("case", PARAMS, ids=case_id)
def test_sums_equal_the_reference(hip, case):
    from gan_sr_wind_field_amd import hip_ops

    thresholds, scales = case
    t = tables(thresholds)
    shapes = SHAPES + ((BIG,) if len(scales) == 2 else ())
    for k, shape in enumerate(shapes):
        HR, SR, TL = _inputs(shape, SEEDS[k])
        want = _want(shape, SEEDS[k], thresholds, scales)
        got = _launch(hip, HR, SR, TL, t, scales, f"{case_id(case)} {shape}")
        _compare(got, want, f"{case_id(case)} {shape}")
        assert not torch.equal(got[..., 0], got[..., 1]) and not torch.equal(got[..., 0], got[..., 3])  # (the sources differ)
        if len(thresholds) == 4:  # no comparison skips a cell: every (sample, level, threshold, scale) has events
            assert bool((got[..., 0] + got[..., 1] > 0).all()), shape
    assert hip_ops.fss_level_chunk(*BIG, (1, 33)) == 6 and hip_ops.fss_level_chunk(*SHAPES[3], (1, 33)) == 2


def test_special_voxels(hip):
    """the tie, its fp32 neighbours, zeros, NaN and +-Inf at the first and the last voxels, on either side of a tile
    boundary along x and y, and on either side of a level-chunk boundary (chunks of two and of six levels)"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.fss import level_fss_reference

    t = tie_tables()
    assert float(t.thr2[1]) == 0.0625
    for shape, scales in (((2, 40, 36, 7), (1, 3, 33)), (BIG, (1, 33))):
        chunk = hip_ops.fss_level_chunk(*shape, scales)
        assert chunk < shape[3]
        HR, SR, TL = plant_specials(fields(*shape, seed=21, channels=(4, 3, 3)), hip_ops.FSS_TILE, chunk)
        assert bool(torch.isnan(HR[:, :2]).any()) and bool(torch.isinf(SR[:, :2]).any())
        assert bool(((HR[:, 0] == 0.25) & (HR[:, 1] == 0)).any())
        want = level_fss_reference(HR, SR, TL, t, scales)
        _compare(_launch(hip, HR, SR, TL, t, scales, f"special voxels {shape}"), want, f"special voxels {shape}")
    # one voxel, every special value in turn, alone in the corner of a plane
    f = torch.zeros((1, 3, 3, 3, 1))
    for (u, v), event in (((0.25, 0.0), 1), ((0.0, -0.25), 1), ((NAN, 1.0), 0), ((float("inf"), 0.0), 1), ((0.2, 0.0), 0)):
        f[0, 0, 0, 0, 0], f[0, 1, 0, 0, 0] = u, v
        got = _launch(hip, f, f, None, tables((8.0,), 32.0), (1, 3), f"one voxel {u}, {v}")
        assert got[0, 0, 0].tolist() == [[event, event, 0, 0, 0], [4 * event, 4 * event, 0, 0, 0]], (u, v)


def test_equal_fields_and_a_displaced_event(hip):
    """SR = HR: srd = 0 exactly; one event displaced by two cells across a tile boundary: FSS(n) = max(0, 1 - 2 / n)"""
    from gan_sr_wind_field_amd.fss import fss_from_sums

    HR, _, _ = _inputs(SHAPES[2], SEEDS[2])
    t = tables()
    got = _launch(hip, HR, HR.clone(), HR.clone(), t, DEFAULT_SCALES, "equal fields")
    assert float(got[..., 2].abs().sum()) == 0 and float(got[..., 4].abs().sum()) == 0 and torch.equal(got[..., 0], got[..., 1])
    X, Y = 70, 40
    a, b = torch.zeros((1, 3, X, Y, 2)), torch.zeros((1, 3, X, Y, 2))
    a[0, 0, 31, 20], b[0, 0, 33, 20] = 0.5, 0.5
    got = _launch(hip, a, b, None, tables((10.0,)), (1, 3, 5, 9), "displaced")
    col = fss_from_sums(got[0, 0], (1, 3, 5, 9), (10.0,), 1.0, X * Y)
    assert col["fss"]["FSS"] == [0.0, 1 - 2 / 3, 1 - 2 / 5, 1 - 2 / 9]


# ---------------------------------------------------------------------------------------------------- completeness
def test_no_baseline_and_another_stream(hip):
    from gan_sr_wind_field_amd import hip_ops

    shape, (thresholds, scales) = SHAPES[2], PARAMS[1]
    t = tables(thresholds)
    HR, SR, TL = _inputs(shape, SEEDS[2])
    got = _launch(hip, HR, SR, None, t, scales, "tl = NULL")
    _compare(got, _want(shape, SEEDS[2], thresholds, scales, tl=False), "tl = NULL")
    assert float(got[..., 3:].abs().sum()) == 0 and float(got[..., :3].sum()) > 0
    # another stream: the operand is written on that stream just before the launch
    want = _want(shape, SEEDS[2], thresholds, scales)
    ops = [f.to(DEV) for f in (HR, SR, TL)]
    stale = torch.zeros_like(ops[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stale.copy_(ops[0], non_blocking=True)
        assert hip_ops._stream().value == s.cuda_stream
        out = hip_ops.level_fss(stale, ops[1], ops[2], t, scales)
    s.synchronize()
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    import ctypes

    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 6, 5, 3
    thresholds, scales = (5.0, 10.0, 15.0, 20.0), (1, 3, 5)
    t = tables(thresholds)
    nt, nn = 4, 3
    HR, SR, TL = (f.to(DEV) for f in fields(B, X, Y, NZ, seed=1, channels=(3, 3, 3)))
    THR = tables((1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)).thr2.to(DEV)  # (long enough for every nt the calls below name)
    n_ws = int(hip.wsr_level_fss_workspace_floats(B, X, Y, NZ, nt, nn, 5))
    assert n_ws > 0
    out = Guarded((B, NZ, nt, nn, 2 * 5), torch.float32, DEV)
    ws = Guarded((n_ws + 2,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, thr=THR, n_t=nt, sc=scales, n_n=None, b=B, nx=X, ny=Y, nz=NZ,
             w=ws.t, o=out.t):
        arr = None if sc is None else (ctypes.c_int32 * max(len(sc), 1))(*sc)
        return hip.wsr_level_fss(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, p(thr), n_t, arr, len(sc or ()) if n_n is None else n_n,
                                 b, nx, ny, nz, p(o), p(w), hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(thr=None), dict(sc=None, n_n=3), dict(w=None), dict(o=None),
               dict(hr_c=2), dict(sr_c=2), dict(tl_c=2), dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0),
               dict(n_t=0), dict(n_t=9), dict(n_t=-1), dict(sc=(), n_n=0), dict(sc=(1, 3, 5, 7, 9, 11, 13, 15, 17)),
               dict(sc=(3, 5)), dict(sc=(1, 4)), dict(sc=(1, 5, 3)), dict(sc=(1, 3, 3)), dict(sc=(1, 35)), dict(sc=(1, -3)),
               dict(w=ws.t[1:])]  # (a workspace that is not 8-byte aligned)
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(b=65536), dict(nx=65536, ny=32768), dict(nx=32768, ny=32768, nz=2)):
        assert call(**kw) == -2, kw
    wsf = hip.wsr_level_fss_workspace_floats
    assert wsf(0, X, Y, NZ, nt, nn, 5) == wsf(1, X, Y, NZ, 9, nn, 5) == wsf(1, X, Y, NZ, nt, nn, 4) == 0
    assert wsf(1, X, Y, NZ, nt, nn, 35) == wsf(65536, X, Y, NZ, nt, nn, 5) == wsf(1, X, Y, NZ, nt, 9, 33) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError naming what is wrong
    ok = hip_ops.level_fss(HR, SR, TL, t, scales)
    assert ok.shape == (B, NZ, nt, nn, 5) and float(ok[..., 0].sum()) > 0
    bad = [(HR[:, :2].contiguous(), SR, TL), (HR.double(), SR, TL), (HR, SR[..., :2], TL), (HR, SR[..., :2].contiguous(), TL),
           (HR, SR, TL[:, :, :3].contiguous()), (HR, SR, torch.cat([TL, TL]))]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_fss(*args, t, scales)
    for sc, pattern in (((3, 5), "scales must begin with 1"), ((1, 4), "scales must be odd"), ((1, 35), "scales .*35"),
                        ((1, 5, 3), "scales must be strictly"), (tuple(range(1, 19, 2)), "scales must hold")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.level_fss(HR, SR, TL, t, sc)
    for kw, pattern in ((dict(thresholds=(10.0, 5.0)), "thresholds must be strictly"), (dict(thresholds=()), "thresholds must hold"),
                        (dict(thr2=t.thr2[:-1]), "4 squared thresholds, got 3")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.level_fss(HR, SR, TL, t._replace(**kw), scales)
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_fss(HR, SR, TL, t, scales, out=torch.empty((B, NZ, nt, nn, 5), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_fss(HR.cpu(), SR, TL, t, scales)
    # the thresholds are uploaded once per (device, parameters)
    n = len(hip_ops._fss_tables)
    hip_ops.level_fss(HR, SR, TL, t, scales)
    hip_ops.level_fss(HR, SR, TL, tables(thresholds), (1,))
    assert len(hip_ops._fss_tables) == n
    hip_ops.level_fss(HR, SR, TL, tables((5.0, 11.0)), scales)
    assert len(hip_ops._fss_tables) == n + 1


# ---------------------------------------------------------------------------------------------------- the model's entry
def gan_stub(scale=4, **section):
    """what ``wind_field_GAN_3D.level_fss`` uses of its object: the scale and the section"""
    from gan_sr_wind_field_amd.config.config import FssConfig

    fc = FssConfig()
    fc.setFssConfig(None)
    for k, v in section.items():
        setattr(fc, k, v)
    return SimpleNamespace(cfg=SimpleNamespace(scale=scale, fss=fc))


def test_gan_level_fss(hip):
    import torch.nn.functional as F

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.fss import level_fss_reference
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    HR, SR, _ = fields(2, 12, 8, 5, seed=4, channels=(3, 3, 3))
    LR = 0.3 * torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    for stub, t, scales in ((gan_stub(), tables((5.0, 10.0, 15.0, 20.0), 20.0), DEFAULT_SCALES),  # (no section: its defaults)
                            (gan_stub(present=True, thresholds=[3.0, 6.0], scales=[1, 5]), tables((3.0, 6.0), 20.0), (1, 5))):
        got = wind_field_GAN_3D.level_fss(stub, HR.to(DEV), SR.to(DEV), LR.to(DEV), 20.0)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (2, 5, t.thr2.numel(), len(scales), 5)
        TL_dev = hip_ops.trilinear_xy(LR.to(DEV), 4).cpu()
        assert torch.equal(got.cpu(), level_fss_reference(HR, SR, TL_dev, t, scales))  # HR, SR and the device baseline: exact
        # the baseline of F.interpolate differs in its low digits (a matter of [EVAL]): HR and SR are compared
        host = level_fss_reference(HR, SR, F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear",
                                                         align_corners=True), t, scales)
        assert torch.equal(host[..., :3], got.cpu()[..., :3])
        print(f"[gan] baseline sums, F.interpolate against wsr_trilinear_xy: summed |difference| "
              f"{float((host[..., 3:] - got.cpu()[..., 3:]).abs().sum()):g}")
        # on a CPU device the same entry is the reference
        assert torch.equal(wind_field_GAN_3D.level_fss(stub, HR, SR, LR, 20.0), host)


# ---------------------------------------------------------------------------------------------------- run.py
def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _earlier_files(name, run_dir):
    """the files a run without the section writes: path relative to the run -> bytes"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____") and "____fss" not in f and "____exceedance" not in f:
            with open(os.path.join("test_output", f), "rb") as fh:
                out[f[len(name):]] = fh.read()
    for f in sorted(os.listdir(os.path.join(run_dir, "fields"))):
        with open(os.path.join(run_dir, "fields", f), "rb") as fh:
            out["fields/" + f] = fh.read()
    return out


def _close(a, b):
    """|a - b| of two printed scores; two nan are equal, one nan is infinitely far"""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
    return abs(a - b)


def test_run_test_device_loop_against_host_loop(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.fss import EXCEEDANCE_COLUMNS, FSS_COLUMNS

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_fss

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_fss", counted)

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
    cfg_t, dir_t = run("trained", ["--train"], "")
    _, te, _, _, _ = runmod.prepare_data(cfg_t)
    uvw = float(te.UVW_MAX)
    thresholds = [round(f * uvw, 6) for f in (0.05, 0.1, 0.2)]
    sec = f"\n[FSS]\nthresholds = {thresholds}\nscales = [1, 3, 9, 33]\nper_level = True\n"
    load = dict(generator_load_path=os.path.join(dir_t, "G_6.pth"), discriminator_load_path=os.path.join(dir_t, "D_6.pth"),
                state_load_path=os.path.join(dir_t, "state_6.pth"))
    _, dir_a = run("plain", ["--test"], dev_loop, **load)
    assert calls["n"] == 0 and not any("fss" in f or "exceedance" in f for f in os.listdir("test_output"))
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

    worst = 0.0  # |difference| / bound
    for suffix, truth in (("", te[0][1]), ("_reverse_interpolate", te[0][4])):
        npos = n_test * truth.shape[1] * truth.shape[2] * truth.shape[3]
        d, h = _read("dev", "exceedance" + suffix), _read("host", "exceedance" + suffix)
        assert d[0] == h[0] == ["threshold"] + list(EXCEEDANCE_COLUMNS) and len(d) == len(h) == 1 + 3
        bound = {}
        for rd, rh in zip(d[1:], h[1:]):
            assert rd[:2] == rh[:2], (suffix, rd, rh)  # threshold and f_HR: the same text
            assert 0 < float(rd[1]) < 1
            events = float(rd[1]) * npos
            bound[rd[0]] = E2E_FLIPS * 4 / events
            for k, c in enumerate(d[0]):
                if c.startswith(("f_", "bias", "CSI", "POD", "FAR", "ETS")):
                    worst = max(worst, _close(rd[k], rh[k]) / bound[rd[0]])
                    assert _close(rd[k], rh[k]) <= bound[rd[0]], (suffix, c, rd[k], rh[k], bound[rd[0]])
                elif c.startswith("useful"):
                    print(f"[e2e] exceedance{suffix} {rd[0]} {c}: device {rd[k]} host {rh[k]}")
            print(f"[e2e] exceedance{suffix} {rd[0]}: {events:.0f} events of HR in {npos} positions, bound {bound[rd[0]]:.3g}")
        d, h = _read("dev", "fss" + suffix), _read("host", "fss" + suffix)
        assert d[0] == h[0] == ["threshold", "scale"] + list(FSS_COLUMNS) and len(d) == len(h) == 1 + 3 * 4
        for rd, rh in zip(d[1:], h[1:]):
            assert rd[:3] == rh[:3] and rd[5] == rh[5], (suffix, rd, rh)  # threshold, scale, scale_m, FSS_uniform: the same text
            for k in (3, 4):
                print(f"[e2e] fss{suffix} {rd[0]} {rd[1]} {d[0][k]}: device {rd[k]} host {rh[k]}")
                worst = max(worst, _close(rd[k], rh[k]) / bound[rd[0]])
                assert _close(rd[k], rh[k]) <= bound[rd[0]], (suffix, rd, rh, bound[rd[0]])
        lv = _read("dev", "fss_levels" + suffix)
        assert lv[0] == ["level", "threshold", "scale"] + list(FSS_COLUMNS) and len(lv) == 1 + truth.shape[3] * 12
        assert [r[0] for r in lv[1::12]] == [str(k) for k in range(truth.shape[3])]
    assert _read("dev", "fss") != _read("dev", "fss_reverse_interpolate")
    print(f"[e2e] SR and baseline scores of the device loop against the host loop: worst |difference| / bound {worst:.3g}")
    print(f"[time] tests/test_fss_gpu.py up to here: {time.time() - T0:.1f} s")
