"""[INCREMENTS] on the GPU: ``wsr_level_increments`` (csrc/increments.hip) against a float64 evaluation of the definition
of ``increments.py`` from the same fp32 inputs (``f64_sums`` below: its own code, index_select instead of the reference's
slices).  The sums and the workspace of the kernel live in ``Guarded`` buffers whose sentinel is a NaN: a call that leaves
an element of ``out`` unwritten fails the comparison.

The bound of every entry: ``LAMBDA sqrt(pairs) 2^-24 A + 2^-100`` with A the float64 sum of |delta|^p over the entry's
pairs and ``LAMBDA`` = 16 of ``kernel_bounds``.  Why it holds for the kernel's order: a term carries at most 2 p roundings
(delta 1; delta^2 3; delta^3 5; delta^4 7, each relative 2^-24); a workgroup adds its fp32 terms in a chain of at most 96
additions whatever the plane (at most 64 in a thread, 16 in a group of slots, 16 groups; csrc/increments_kernels.h), and
never more than the entry has pairs, because a zero partial adds exactly; the rows of the tiles are added in double.  So
the error is at most (min(pairs, 96) + 8) 2^-24 A (1 + small), and 16 sqrt(pairs) >= min(pairs, 96) + 8 for every
pairs >= 1.  Measured on an MI355X when the test was written: see ``WORST`` in DESIGN 30.

tools/increments_host_check.cpp ran clean under the address and undefined-behaviour sanitisers at these shapes and
separation lists, with and without a baseline.
"""
import csv
import math
import os
import pickle
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from increments_cases import LISTS, NAN, SEEDS, SHAPES, alternating_field, fields, pairs_table, ramp_field
from kernel_bounds import LAMBDA, TINY, Guarded, assert_guards_intact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
U_FP32 = 2.0 ** -24

_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int64)


def f64_sums(HR, SR, TL, separations):
    """(sums, A) float64 (B, NZ, 3, R, 2, 3, 3): the definition with every operation in float64 on the fp32 values, and
    the sums of |delta|^p; gathers by index, one (direction, kind) at a time"""
    B, _, X, Y, NZ = HR.shape
    nr = len(separations)
    sums = torch.zeros((B, NZ, 3, nr, 2, 3, 3), dtype=torch.float64)
    mags = torch.zeros_like(sums)
    for s, f in enumerate((HR, SR, TL)):
        if f is None:
            continue
        for a, n in enumerate((X, Y)):
            dim = 1 + a  # of a (B, X, Y, NZ) component
            for kind, chan in enumerate(((0, 1, 2), (1, 0, 2))[a]):
                c = f[:, chan].double()
                for k, r in enumerate(separations):
                    if r >= n:
                        continue
                    lo = torch.arange(0, n - r)
                    delta = c.index_select(dim, lo + r) - c.index_select(dim, lo)
                    q = delta * delta
                    for o, (term, mag) in enumerate(((q, q), (q * delta, q * delta.abs()), (q * q, q * q))):
                        sums[:, :, s, k, a, kind, o] = term.sum(dim=(1, 2))
                        mags[:, :, s, k, a, kind, o] = mag.sum(dim=(1, 2))
    return sums, mags


def sum_bounds(A, X, Y, separations):
    """the bound of the module docstring for every entry of a (B, NZ, 3, R, 2, 3, 3) table"""
    pairs = pairs_table(X, Y, separations)[None, None, None, :, :, None, None]
    return LAMBDA * pairs.sqrt() * U_FP32 * A + TINY


def _inputs(k, independent):
    key = ("fields", k, independent)
    if key not in _cache:
        _cache[key] = fields(*SHAPES[k], seed=SEEDS[k], independent=independent)
    return _cache[key]


def _want(k, independent, separations):
    """(sums, A) of ``_inputs(k, independent)`` in float64, computed once and shared"""
    key = ("sums", k, independent, separations)
    if key not in _cache:
        _cache[key] = f64_sums(*_inputs(k, independent), separations)
    return _cache[key]


def _launch(hip, HR, SR, TL, separations, label=""):
    """the C entry on device copies of the operands, sums and workspace in guarded buffers -> (B, NZ, 3, R, 2, 3, 3)
    float64 on the host; a second launch, the wrapper and the wrapper with ``out=`` must give the same bits"""
    import ctypes

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    nr = len(separations)
    ops = [None if f is None else f.to(DEV).contiguous() for f in (HR, SR, TL)]
    arr = (ctypes.c_int32 * nr)(*separations)
    n_ws = int(hip.wsr_level_increments_workspace_floats(B, X, Y, NZ, arr, nr))
    assert n_ws > 0 and n_ws % (9 * B * nr * 6) == 0
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, 3, nr, 2, 3, 2 * 3), torch.float32, DEV)  # (B, NZ, 3, R, 2, 3, 3) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_level_increments(hip_ops._p(ops[0]), HR.shape[1], hip_ops._p(ops[1]), SR.shape[1], hip_ops._p(ops[2]),
                                       0 if TL is None else TL.shape[1], arr, nr, B, X, Y, NZ, hip_ops._p(ws.t),
                                       hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"level_increments {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, 3, nr, 2, 3, 3)
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    wrapped = hip_ops.level_increments(*ops, separations)  # the wrapper: the same launch
    assert wrapped.dtype == torch.float64 and torch.equal(_bits(wrapped.cpu()), _bits(got[0])), label
    into = torch.full((B, NZ, 3, nr, 2, 3, 3), NAN, dtype=torch.float64, device=DEV)
    assert hip_ops.level_increments(*ops, separations, out=into) is into
    assert torch.equal(_bits(into.cpu()), _bits(got[0])), label
    return got[0]


def _check(got, want, A, X, Y, separations, label):
    """-> the worst |err| / bound; entries without pairs are exactly 0"""
    bnd = sum_bounds(A, X, Y, separations)
    err = (got - want).abs()
    if not bool((err <= bnd).all()):  # (a NaN fails)
        bad = (~(err <= bnd)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{label}: {bad.shape[0]} sums outside the bound, the first at (b, z, source, separation, "
                             f"direction, kind, order) = {i}: got {float(got[i])!r} want {float(want[i])!r} bound "
                             f"{float(bnd[i]):.3g}")
    none = (pairs_table(X, Y, separations) == 0)[None, None, None, :, :, None, None].expand_as(got)
    assert bool((_bits(got[none]) == 0).all()), f"{label}: an entry without pairs is not +0"
    s2 = got[..., 0]
    assert bool((s2[~none[..., 0]] > 0).all()), f"{label}: an S2 entry with pairs is not positive"
    return float((err / bnd)[~none].max()) if bool((~none).any()) else 0.0


# ---------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=lambda k: "x".join(map(str, SHAPES[k])))
def test_sums_within_the_bound_of_float64(hip, k):
    B, X, Y, NZ = SHAPES[k]
    for independent in (True, False):
        HR, SR, TL = _inputs(k, independent)
        assert HR.shape[1] == 4 and bool(torch.isnan(HR[:, 3]).all())  # a surplus channel of NaN: never read
        for separations in LISTS:
            label = f"{SHAPES[k]} {separations} {'independent' if independent else 'close'}"
            want, A = _want(k, independent, separations)
            got = _launch(hip, HR, SR, TL, separations, label)
            worst = _check(got, want, A, X, Y, separations, label)
            assert not torch.equal(got[:, :, 0], got[:, :, 1]) and not torch.equal(got[:, :, 0], got[:, :, 2])
            print(f"[bound] {label}: worst |err| / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- exactness
def test_exact_identities(hip):
    """every term a power of two times a small integer: any summation order is exact, so ``torch.equal``"""
    B, X, Y, NZ = 2, 70, 40, 5
    sp = (1, 2, 4, 8)
    pairs = pairs_table(X, Y, sp)
    f = ramp_field(B, X, Y, NZ)
    got = _launch(hip, f, f.clone(), None, sp, "ramp")
    want = torch.zeros_like(got)
    for k, r in enumerate(sp):
        for o, p in enumerate((2, 3, 4)):
            want[:, :, :2, k, 0, 0, o] = pairs[k, 0] * (r * 2.0 ** -6) ** p
    assert torch.equal(got, want)
    for k, r in enumerate(sp):  # skewness and flatness of the x direction: exactly 1
        m2, m3, m4 = (float(got[0, 0, 0, k, 0, 0, o]) / float(pairs[k, 0]) for o in range(3))
        assert m4 / m2 ** 2 == 1.0 and m3 / m2 ** 1.5 == 1.0
    f = alternating_field(B, X, Y, NZ)
    got = _launch(hip, f, f.clone(), f.clone(), sp, "alternating")
    want = torch.zeros_like(got)
    want[:, :, :, 0, 0, 0, 0] = pairs[0, 0] * 2.0 ** -4
    want[:, :, :, 0, 0, 0, 1] = 0.0 if (X - 1) % 2 == 0 else -(2.0 ** -6) * Y  # the cubes cancel in pairs: X - 1 = 69 is odd
    want[:, :, :, 0, 0, 0, 2] = pairs[0, 0] * 2.0 ** -8
    assert torch.equal(got, want)
    f = torch.full((B, 3, X, Y, NZ), 0.7)
    got = _launch(hip, f, f.clone(), f.clone(), LISTS[2], "constant")
    assert bool((_bits(got) == 0).all())
    # SR = HR (and TL = HR) on random fields: equal slices, bit for bit
    HR = fields(2, 33, 40, 7, seed=77)[0]
    got = _launch(hip, HR, HR[:, :3].contiguous(), HR.clone(), LISTS[2], "equal fields")
    assert torch.equal(_bits(got[:, :, 0]), _bits(got[:, :, 1])) and torch.equal(_bits(got[:, :, 0]), _bits(got[:, :, 2]))
    assert bool((got[..., :6, :, :, 0] > 0).all())
    # Y = 1: a y direction without pairs
    HR, SR, TL = fields(1, 40, 1, 3, seed=78)
    got = _launch(hip, HR, SR, TL, sp, "Y = 1")
    assert bool((_bits(got[:, :, :, :, 1]) == 0).all()) and bool((got[:, :, :, :, 0, :, 0] > 0).all())


# ---------------------------------------------------------------------------------------------------- completeness
def test_no_baseline_and_another_stream(hip):
    from gan_sr_wind_field_amd import hip_ops

    k, separations = 2, LISTS[1]
    HR, SR, TL = _inputs(k, True)
    full = _launch(hip, HR, SR, TL, separations, "with tl")
    got = _launch(hip, HR, SR, None, separations, "tl = NULL")
    assert torch.equal(_bits(got[:, :, :2]), _bits(full[:, :, :2])) and bool((_bits(got[:, :, 2]) == 0).all())
    # another stream: the operand is written on that stream just before the launch
    ops = [f.to(DEV) for f in (HR, SR, TL)]
    stale = torch.zeros_like(ops[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stale.copy_(ops[0], non_blocking=True)
        assert hip_ops._stream().value == s.cuda_stream
        out = hip_ops.level_increments(stale, ops[1], ops[2], separations)
    s.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(full))


def test_nan_voxels_poison_their_pairs_only(hip):
    """a NaN at the first and the last voxel, on either side of a tile boundary along x and along y and of a level-chunk
    boundary: exactly the entries the reference names are non-finite, the rest are the bits of the clean call"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.increments import level_increments_reference

    B, X, Y, NZ = 1, 40, 40, 8
    sp = LISTS[1]
    T, chunk = hip_ops.INCREMENTS_TILE, hip_ops.increments_level_chunk(NZ, sp)
    assert X > T and Y > T and chunk == 4
    HR, SR, TL = fields(B, X, Y, NZ, seed=31, channels=(3, 3, 3))
    ops = [f.to(DEV) for f in (HR, SR, TL)]
    clean = hip_ops.level_increments(*ops, sp).cpu()
    assert bool(torch.isfinite(clean).all())
    places = [(0, 0, 0), (X - 1, Y - 1, NZ - 1), (T - 1, 5, 1), (T, 5, 1), (7, T - 1, 2), (7, T, 2), (3, 4, chunk - 1),
              (3, 4, chunk), (T, T, chunk), (T - 1, T - 1, chunk - 1)]
    for n, (x, y, z) in enumerate(places):
        src, comp = n % 3, (n // 3) % 3
        dirty = [f.clone() for f in (HR, SR, TL)]
        dirty[src][0, comp, x, y, z] = NAN if n % 2 == 0 else float("inf")
        want_bad = ~torch.isfinite(level_increments_reference(*dirty, sp))
        got = hip_ops.level_increments(*[f.to(DEV) for f in dirty], sp).cpu()
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, want_bad), (x, y, z, int(bad.sum()), int(want_bad.sum()))
        assert 0 < int(bad.sum()) <= 3 * len(sp) * 2 * 2 and bool(bad[0, z, src].any()) and int(bad.sum()) == int(bad[0, z, src].sum())
        assert torch.equal(_bits(got[~bad]), _bits(clean[~bad])), (x, y, z)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    import ctypes

    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 6, 5, 3
    sp = (1, 2, 4)
    HR, SR, TL = (f.to(DEV) for f in fields(B, X, Y, NZ, seed=1, channels=(3, 3, 3)))
    wsf = hip.wsr_level_increments_workspace_floats
    n_ws = int(wsf(B, X, Y, NZ, (ctypes.c_int32 * 3)(*sp), 3))
    assert n_ws > 0
    out = Guarded((B, NZ, 3, 3, 2, 3, 2 * 3), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws)]
    p = hip_ops._p

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, s=sp, n=None, b=B, nx=X, ny=Y, nz=NZ, w=ws.t, o=out.t):
        arr = None if s is None else (ctypes.c_int32 * max(len(s), 1))(*s)
        return hip.wsr_level_increments(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, arr, len(s or ()) if n is None else n, b, nx,
                                        ny, nz, p(w), p(o), hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(s=None, n=3), dict(w=None), dict(o=None), dict(hr_c=2), dict(sr_c=2),
               dict(tl_c=2), dict(tl_c=0), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(s=(), n=0), dict(n=-1),
               dict(s=tuple(range(1, 10))), dict(s=(0, 1)), dict(s=(1, 33)), dict(s=(2, 1)), dict(s=(1, 1)), dict(s=(-1,))]
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(b=65536), dict(nx=65536, ny=32768), dict(nx=32768, ny=32768, nz=2)):
        assert call(**kw) == -2, kw
    arr = (ctypes.c_int32 * 3)(*sp)
    assert wsf(0, X, Y, NZ, arr, 3) == wsf(1, X, Y, NZ, arr, 9) == wsf(1, X, Y, NZ, None, 3) == wsf(65536, X, Y, NZ, arr, 3) == 0
    assert wsf(1, X, Y, NZ, (ctypes.c_int32 * 2)(2, 1), 2) == wsf(1, 32768, 32768, 2, arr, 3) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError naming what is wrong
    ok = hip_ops.level_increments(HR, SR, TL, sp)
    assert ok.shape == (B, NZ, 3, 3, 2, 3, 3) and float(ok[..., 0].sum()) > 0
    bad = [(HR[:, :2].contiguous(), SR, TL), (HR.double(), SR, TL), (HR, SR[..., :2], TL), (HR, SR[..., :2].contiguous(), TL),
           (HR, SR, TL[:, :, :3].contiguous()), (HR, SR, torch.cat([TL, TL]))]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.level_increments(*args, sp)
    for s, pattern in (((2, 1), "separations must be strictly"), ((1, 33), "separations must lie in 1 .. 32"),
                       ((0,), "separations must lie"), (tuple(range(1, 10)), "separations must hold 1 .. 8 entries, not 9"),
                       ((), "separations must hold"), ((1, 2.5), "separations must be a list of integers")):
        with pytest.raises(ValueError, match="level_increments: " + pattern):
            hip_ops.level_increments(HR, SR, TL, s)
    with pytest.raises(ValueError, match="out"):
        hip_ops.level_increments(HR, SR, TL, sp, out=torch.empty((B, NZ, 3, 3, 2, 3, 3), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.level_increments(HR.cpu(), SR, TL, sp)


# ---------------------------------------------------------------------------------------------------- the model's entry
def gan_stub(scale=4, **section):
    """what ``wind_field_GAN_3D.level_increments`` uses of its object: the scale and the section"""
    from gan_sr_wind_field_amd.config.config import IncrementsConfig

    ic = IncrementsConfig()
    ic.setIncrementsConfig(None)
    for k, v in section.items():
        setattr(ic, k, v)
    return SimpleNamespace(cfg=SimpleNamespace(scale=scale, increments=ic))


def test_gan_level_increments(hip):
    import torch.nn.functional as F

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.increments import DEFAULT_SEPARATIONS, level_increments_reference
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    HR, SR, _ = fields(2, 12, 8, 5, seed=4, channels=(3, 3, 3))
    LR = 0.3 * torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    for stub, sp in ((gan_stub(), DEFAULT_SEPARATIONS), (gan_stub(present=True, separations=[1, 3]), (1, 3))):
        got = wind_field_GAN_3D.level_increments(stub, HR.to(DEV), SR.to(DEV), LR.to(DEV))
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (2, 5, 3, len(sp), 2, 3, 3)
        TL_dev = hip_ops.trilinear_xy(LR.to(DEV), 4)
        assert torch.equal(_bits(got), _bits(hip_ops.level_increments(HR.to(DEV), SR.to(DEV), TL_dev, sp)))  # bit for bit
        want, A = f64_sums(HR, SR, TL_dev.cpu(), sp)
        assert bool(((got.cpu() - want).abs() <= sum_bounds(A, 12, 8, sp)).all())
        # on a CPU device the same entry is the reference
        host = level_increments_reference(HR, SR, F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear",
                                                                align_corners=True), sp)
        assert torch.equal(wind_field_GAN_3D.level_increments(stub, HR, SR, LR), host)


# ---------------------------------------------------------------------------------------------------- run.py
def column_bounds(t, b, separations, nplanes, X, Y, uvw):
    """the bounds ``b`` (3, R, 2, 3, 3) of the sums ``t`` carried through ``increments_from_sums`` -> a list per column"""
    from gan_sr_wind_field_amd.increments import INCREMENT_COLUMNS, KINDS, SOURCES

    def ratio(a, ea, d, ed):  # |(a + ea') / (d + ed') - a / d| for |ea'| <= ea, |ed'| <= ed, d > ed
        return (ea + abs(a / d) * ed) / (d - ed) if d > ed else math.inf

    out = {c: [] for c in INCREMENT_COLUMNS}
    T, Bd = t.tolist(), b.tolist()
    for k, r in enumerate(separations):
        nx, ny = nplanes * max(X - r, 0) * Y, nplanes * X * max(Y - r, 0)
        n = nx + ny
        for c in ("r", "r_m", "pairs"):
            out[c].append(0.0)
        m2, e2 = {}, {}
        for s, src in enumerate(SOURCES):
            for kind, kn in enumerate(KINDS):
                m = [(T[s][k][0][kind][o] + T[s][k][1][kind][o]) / n for o in range(3)]
                e = [(Bd[s][k][0][kind][o] + Bd[s][k][1][kind][o]) / n for o in range(3)]
                m2[src, kn], e2[src, kn] = m[0], e[0]
                out[f"S2{kn}_{src}"].append(uvw * uvw * e[0])
                out[f"flatness_{kn}_{src}"].append(ratio(m[2], e[2], m[0] ** 2, 2 * m[0] * e[0] + e[0] ** 2))
                if kind == 0:
                    out[f"skewness_L_{src}"].append(ratio(m[1], e[1], m[0] ** 1.5, (m[0] + e[0]) ** 1.5 - m[0] ** 1.5))
            out[f"anisotropy_{src}"].append(ratio(T[s][k][0][0][0] / nx, Bd[s][k][0][0][0] / nx, T[s][k][1][0][0] / ny,
                                                  Bd[s][k][1][0][0] / ny))
        for kn in KINDS:
            for twin, src in (("", "SR"), ("_trilinear", "trilinear")):
                out[f"S2{kn}_ratio{twin}"].append(ratio(m2[src, kn], e2[src, kn], m2["HR", kn], e2["HR", kn]))
    return out


def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _earlier_files(name, run_dir):
    """the files a run without the section writes: path relative to the run -> bytes"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____") and "structure_functions" not in f:
            with open(os.path.join("test_output", f), "rb") as fh:
                out[f[len(name):]] = fh.read()
    for f in sorted(os.listdir(os.path.join(run_dir, "fields"))):
        with open(os.path.join(run_dir, "fields", f), "rb") as fh:
            out["fields/" + f] = fh.read()
    return out


def _float64_columns(run_dir, names, separations, uvw, d, raw):
    """(columns, bounds) of the fields a run pickled, in float64 from its own HR / SR / TL (flat levels), or for ``raw``
    from its raw truth alone (SR = TL = HR: the HR-only columns)"""
    from gan_sr_wind_field_amd.increments import increments_from_sums

    total = bound = None
    for name in names:
        with open(os.path.join(run_dir, "fields", f"test_fields_{name}.pkl"), "rb") as f:
            p = pickle.load(f)
        keys = ("HR_orig", "HR_orig", "HR_orig") if raw else ("HR", "SR", "TL")
        HR, SR, TL = (torch.from_numpy(np.asarray(p[k]))[None].float() for k in keys)
        s, A = f64_sums(HR, SR, TL, separations)
        bd = sum_bounds(A, HR.shape[2], HR.shape[3], separations)
        total = s[0].sum(dim=0) if total is None else total + s[0].sum(dim=0)
        bound = bd[0].sum(dim=0) if bound is None else bound + bd[0].sum(dim=0)
    X, Y, NZ = HR.shape[2:]
    nplanes = len(names) * NZ
    return (increments_from_sums(total, separations, nplanes, X, Y, uvw, d),
            column_bounds(total, bound, separations, nplanes, X, Y, uvw))


def test_run_test_device_loop_against_host_loop(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.increments import INCREMENT_COLUMNS
    from gan_sr_wind_field_amd.spectra import grid_spacing

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.level_increments

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "level_increments", counted)

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
    d = grid_spacing(np.asarray(te.x), np.asarray(te.y))
    sp = [1, 2, 4, 8, 16]
    sec = f"\n[INCREMENTS]\nseparations = {sp}\nper_level = True\n"
    load = dict(generator_load_path=os.path.join(dir_t, "G_6.pth"), discriminator_load_path=os.path.join(dir_t, "D_6.pth"),
                state_load_path=os.path.join(dir_t, "state_6.pth"))
    _, dir_a = run("plain", ["--test"], dev_loop, **load)
    assert calls["n"] == 0 and not any("structure_functions" in f for f in os.listdir("test_output"))
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

    names = [te[i][3] for i in range(len(te))]
    NZ = te[0][1].shape[3]
    hr_only = [c for c in INCREMENT_COLUMNS[3:] if c.endswith("_HR")]
    worst = 0.0
    for suffix, raw in (("", False), ("_reverse_interpolate", True)):
        rows = {n: _read(n, "structure_functions" + suffix) for n in ("dev", "host")}
        f64 = {n: _float64_columns(dd, names, sp, uvw, d, raw) for n, dd in (("dev", dir_b), ("host", dir_c))}
        for n in rows:
            assert rows[n][0] == list(INCREMENT_COLUMNS) and len(rows[n]) == 1 + len(sp)
            lv = _read(n, "structure_functions_levels" + suffix)
            assert lv[0] == ["level"] + list(INCREMENT_COLUMNS) and len(lv) == 1 + NZ * len(sp)
            assert [r[0] for r in lv[1::len(sp)]] == [str(z) for z in range(NZ)]
        avg = open(os.path.join("test_output", f"averages_structure_functions{suffix}.csv")).read().strip().splitlines()
        assert avg[0] == "Name," + ",".join(INCREMENT_COLUMNS)
        assert [r.split(",")[0] for r in avg[1:]] == ["dev"] * len(sp) + ["host"] * len(sp)
        for k, r in enumerate(sp):
            rd, rh = rows["dev"][1 + k], rows["host"][1 + k]
            assert rd[:3] == rh[:3] and int(rd[0]) == r and float(rd[1]) == r * d and float(rd[2]) > 0, (suffix, rd[:3], rh[:3])
            for i, c in enumerate(INCREMENT_COLUMNS):
                if i < 3 or (raw and c not in hr_only):
                    continue
                dv, hv = float(rd[i]), float(rh[i])
                assert math.isfinite(dv) and math.isfinite(hv), (suffix, c, k)
                own = 0.0
                for n, v in (("dev", dv), ("host", hv)):  # each loop against the float64 columns of its own fields
                    want, bnd = f64[n][0][c][k], f64[n][1][c][k] + 2.0 ** -40 * abs(f64[n][0][c][k])
                    worst = max(worst, abs(v - want) / bnd)
                    assert abs(v - want) <= bnd, (suffix, n, c, k, v, want, bnd)
                    own += bnd
                assert abs(dv - hv) <= own + abs(f64["dev"][0][c][k] - f64["host"][0][c][k]), (suffix, c, k, dv, hv)
    assert _read("dev", "structure_functions") != _read("dev", "structure_functions_reverse_interpolate")
    print(f"[e2e] structure-function columns of both loops against float64: worst |err| / bound {worst:.3g}")
    print(f"[time] tests/test_increments_gpu.py up to here: {time.time() - T0:.1f} s")
