"""[HUB_HEIGHT] on the GPU: ``wsr_hub_height`` (csrc/hub_height.hip) against ``hub_height.hub_height_reference`` in float64
on the CPU, identities with analytic values, special columns, refusals, the model's entry and ``run.py --test`` without
the section, with it in the device loop and with it in the host loop.  Sums, planes and workspace of the kernel live in
``Guarded`` buffers; a second launch, the wrapper and the wrapper with ``out=`` must give the same bits.

The bound (kernel_bounds.py's convention, LAMBDA = 16 untouched), per (sample, height, sum) over K = n_valid columns:

    |got - ref| <= LAMBDA sqrt(K) 2^-24 A + 2^-100,      A = sum over the valid columns of (|term| + e / 2^-24)

with e the error the kernel's arithmetic carries INTO the term, derived here from what csrc/hub_height_kernels.h does
(u0 = 2^-24; nothing is measured against the code under test).  Validity and the interval are the same fp32 comparisons
on both sides, so no term changes its interval; n_valid and the validity plane must be exact.

    weight      t is formed in double from the same fp32 heights as in the reference: identical operations in linear
                mode, two ``log`` of at most 1 ulp each and a division in log mode - a relative error EPS = 2^-49
                covers either, and the double roundings of the blend
    component   c = fl32(f_j + t (f_{j+1} - f_j)), rounded ONCE:   dc = u0 |c| + EPS (|c| + t |f_{j+1} - f_j|)
    speed       V = sqrtf(fl(fl(u u) + fl(v v))): |dV/dc| <= 1 and three roundings that each move V by at most u0 V
                (the products and the sum enter under the root, which halves them; the root is allowed a whole ulp):
                dV = dc_u + dc_v + 3 u0 V
    power       P = fl32(np.interp(V)) in double, rounded once; the curve is continuous with largest slope S:
                dP = S dV + u0 |P|
    terms       V: dV.   |V_s - V_hr|: dV_s + dV_hr + u0 |.|.   (V_s - V_hr)^2: (2 |d| + dV_s + dV_hr)(dV_s + dV_hr) + 3 u0 d^2.
                V^3: 3.1 V^2 dV + 2 u0 V^3.   P: dP.   |P_s - P_hr|: dP_s + dP_hr + u0 |.|.
                V_hr angle: cross and dot are each within (2 u0 + r_a + r_b) |a||b| of their values (two products and a
                sum, and components that moved by r = (dc_u + dc_v) / V relative to the vector), the gradient of atan2
                is 1 / (|a||b|), atan2f is allowed 6 ulp: dth = 2 (2 u0 + r_a + r_b) + 12 u0 th, and the term carries
                dV_hr th + V_hr dth + u0 V_hr th
    planes      |V - ref| <= 1.001 dV, |P - ref| <= 1.001 dP per element (the factor: second-order terms)

Measured on an MI355X when the kernel was written: worst |err| / bound of the sums 0.0107 (at 2 x 7 x 6 x 5 in log mode; 0.0092
there in linear mode, 0.003 with eight heights, below 0.001 at every larger shape - A holds the carried errors at full weight
and LAMBDA sqrt(K) on top, so the sums sit far inside it; the planes are held per element and sit at about half of theirs in
the fp32 torch path), 1.1e-5 for the columns end to end; direction errors of the two rotations 0.29999997 .. 0.29999999 and
2.4999999 .. 2.5000002.  The whole file ran in 10.3 s.

End to end the two loops cannot print the same text for the HR-only columns: the host loop is the float64 reference, the
device loop the kernel's fp32 partial sums.  ``valid_fraction`` is exact and must be the same text; every other column of
the flat levels - HR-only ones included - is held against the float64 columns of the fields THAT run pickled, under the
bound above carried through ``hub_height_from_sums`` (``column_bounds``), and the two loops agree within their two bounds
plus the distance of their float64 columns (the triangle inequality of test_diagnostics_gpu.py).  The raw levels' SR
and baseline are not pickled: there the files' shape, ``valid_fraction`` and the HR-only columns (two bounds, distance 0)
are checked.
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

from hub_height_cases import CASES, HEIGHTS, KNOT_V, MODES, NAN, case, make, plant_specials, tables, terrain_of
from kernel_bounds import LAMBDA, TINY, U_FP32, Guarded, assert_guards_intact, assert_within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
NS, PLANES = 18, 7
EPS = 2.0 ** -49
TL_SUMS = [3, 5, 7, 10, 13, 15, 17]

_reference = {}


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def magnitudes(HR, SR, TL, Z, terrain, t, interp):
    """-> (A (B, NH, 18), dV, dP (B, NH, 3, X, Y)): the A of the module docstring and the per-element bounds of the
    planes (0 for an invalid column and an absent baseline), in float64 on the CPU"""
    from gan_sr_wind_field_amd.hub_height import column_values

    u0 = U_FP32
    cv, cp = t.curve_v.double(), t.curve_p.double()
    slope = float(((cp[1:] - cp[:-1]) / (cv[1:] - cv[:-1])).abs().max())
    B, _, X, Y, _ = HR.shape
    nh = t.heights.numel()
    A = torch.zeros((B, nh, NS), dtype=torch.float64)
    dVs, dPs = torch.zeros((B, nh, 3, X, Y), dtype=torch.float64), torch.zeros((B, nh, 3, X, Y), dtype=torch.float64)
    for k, c in enumerate(column_values(HR, SR, TL, Z, terrain, t, interp)):
        valid, w = c["valid"], c["t"]

        def total(x):
            return torch.where(valid, x, torch.zeros_like(x)).sum(dim=(1, 2))

        dV, dP, rel = [None] * 3, [None] * 3, [None] * 3
        for s in range(3):
            if c["V"][s] is None:
                continue
            dc = [u0 * f.abs() + EPS * (f.abs() + w * sp) for f, sp in zip(c["uv"][s], c["span"][s])]
            V, P = c["V"][s], c["P"][s]
            dV[s] = dc[0] + dc[1] + 3 * u0 * V
            dP[s] = slope * dV[s] + u0 * P.abs()
            rel[s] = torch.where(V > 0, (dc[0] + dc[1]) / V.clamp(min=1e-300), torch.zeros_like(V))
            dVs[:, k, s], dPs[:, k, s] = torch.where(valid, dV[s], 0.0), torch.where(valid, dP[s], 0.0)
        A[:, k, 0] = valid.double().sum(dim=(1, 2))
        V0, P0 = c["V"][0], c["P"][0]
        for s in range(3):
            if c["V"][s] is None:
                continue
            V, P = c["V"][s], c["P"][s]
            A[:, k, 1 + s] = total(V + dV[s] / u0)
            A[:, k, 8 + s] = total(V ** 3 + (3.1 * V * V * dV[s]) / u0 + 2 * V ** 3)
            A[:, k, 11 + s] = total(P.abs() + dP[s] / u0)
            if s:
                d, e = (V - V0).abs(), dV[s] + dV[0]
                A[:, k, 3 + s] = total(d + e / u0 + d)
                A[:, k, 5 + s] = total(d * d + (2 * d + e) * e / u0 + 3 * d * d)
                dp = (P - P0).abs()
                A[:, k, 13 + s] = total(dp + (dP[s] + dP[0]) / u0 + dp)
                (au, av), (bu, bv) = c["uv"][0], c["uv"][s]
                th = torch.atan2((au * bv - av * bu).abs(), au * bu + av * bv)
                dth = 2 * (2 * u0 + rel[0] + rel[s]) + 12 * u0 * th
                A[:, k, 15 + s] = total(V0 * th + (dV[0] * th + V0 * dth) / u0 + V0 * th)
    return A, dVs, dPs


def sum_bounds(A):
    K = A[..., :1].clamp(min=1.0)
    b = LAMBDA * torch.sqrt(K) * U_FP32 * A + TINY
    b[..., 0] = TINY  # n_valid: exact (asserted apart)
    return b


def _want(key, inputs, t, interp):
    """reference sums, planes, bounds of ``inputs``, computed once per ``key`` and shared"""
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    key = (key, interp, tuple(t.heights_m), tuple(t.curve_speeds), inputs[2] is None)
    if key not in _reference:
        sums, cols = hub_height_reference(*inputs, t, interp, with_columns=True)
        A, dV, dP = magnitudes(*inputs, t, interp)
        _reference[key] = (sums, cols, sum_bounds(A), dV, dP)
    return _reference[key]


def _launch(hip, HR, SR, TL, Z, terrain, t, interp, with_cols, label=""):
    """the C entry on device copies of the operands; sums, planes and workspace in guarded buffers -> (sums (B, NH, 18)
    float64, planes (B, NH, 7, X, Y) fp32 or None) on the host; a second launch, the wrapper and the wrapper with
    ``out=`` must give the same bits"""
    import ctypes

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    nh, nk = t.heights.numel(), t.curve_v.numel()
    ops = [None if f is None else f.to(DEV).contiguous() for f in (HR, SR, TL, Z, terrain)]
    arr = [(ctypes.c_float * a.numel())(*a.tolist()) for a in (t.heights, t.curve_v, t.curve_p)]
    n_ws = int(hip.wsr_hub_height_workspace_floats(B, X, Y, NZ, nh))
    cps = hip_ops.hub_height_columns_per_chunk(NZ, nh)
    assert n_ws == B * min(-(-X * Y // cps), 2048) * nh * NS
    got, planes = [], []
    p = hip_ops._p
    for _ in range(2):
        out = Guarded((B, nh, 2 * NS), torch.float32, DEV)  # (B, NH, 18) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        cols = Guarded((B, nh, PLANES, X, Y), torch.float32, DEV) if with_cols else None
        check(hip.wsr_hub_height(p(ops[0]), HR.shape[1], p(ops[1]), SR.shape[1], p(ops[2]), 0 if TL is None else TL.shape[1],
                                 p(ops[3]), p(ops[4]), arr[0], nh, arr[1], arr[2], nk, int(interp == "log"), B, X, Y, NZ,
                                 p(ws.t), p(out.t), p(None if cols is None else cols.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(*(g for g in (out, ws, cols) if g is not None), label=f"hub_height {label}")
        got.append(out.t.view(torch.float64).cpu())
        planes.append(None if cols is None else cols.t.cpu())
    assert got[0].shape == (B, nh, NS)
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    wrapped = hip_ops.hub_height(*ops, t, interp, with_cols)  # the wrapper: the same launch
    into = torch.full((B, nh, NS), NAN, dtype=torch.float64, device=DEV)
    res = hip_ops.hub_height(*ops, t, interp, with_cols, out=into)
    if with_cols:
        assert torch.equal(_bits(planes[0]), _bits(planes[1])), f"{label}: the planes of two calls differ"
        assert not torch.isnan(planes[0]).any(), f"{label}: an element of the planes was not written"
        assert torch.equal(_bits(wrapped[1].cpu()), _bits(planes[0])) and torch.equal(_bits(res[1].cpu()), _bits(planes[0]))
        wrapped, res = wrapped[0], res[0]
    assert res is into and wrapped.dtype == torch.float64
    assert torch.equal(_bits(wrapped.cpu()), _bits(got[0])) and torch.equal(_bits(into.cpu()), _bits(got[0])), label
    return got[0], planes[0]


def _check(got, planes, want, label):
    """sums within the bound, n_valid and the validity plane exact, the planes within their element bounds"""
    sums, cols, bnd, dV, dP = want
    assert torch.equal(got[..., 0], sums[..., 0]), f"{label}: n_valid {got[..., 0].tolist()} != {sums[..., 0].tolist()}"
    worst = assert_within(got, sums, bnd, f"hub_height vs float64[{label}]", kind="sums")
    if planes is not None:
        assert torch.equal(planes[:, :, 6].double(), cols[:, :, 6]), f"{label}: the validity plane differs"
        for name, sl, d in (("V", slice(0, 3), dV), ("P", slice(3, 6), dP)):
            err = (planes[:, :, sl].double() - cols[:, :, sl]).abs()
            assert bool((err <= 1.001 * d + TINY).all()), f"{label}: plane {name}: {float((err - 1.001 * d).max())} above its bound"
    return worst


# ---------------------------------------------------------------------------------------------------- sums against float64
@pytest.mark.parametrize("interp", MODES)
@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: "x".join(map(str, CASES[k][0])))
def test_sums_and_planes_against_float64(hip, k, interp):
    inputs, t = case(k), tables()
    want = _want(k, inputs, t, interp)
    for with_cols in (True, False):
        got, planes = _launch(hip, *inputs, t, interp, with_cols, f"{CASES[k][0]} {interp}")
        _check(got, planes, want, f"{CASES[k][0]} {interp} planes={with_cols}")
    assert bool((got[..., 0] > 0).all()) and not torch.isnan(got).any()  # (the surplus channels are NaN: never read)
    assert not torch.equal(got[..., 1], got[..., 2]) and not torch.equal(got[..., 1], got[..., 3])  # (the sources differ)


def test_eight_heights_and_a_two_knot_curve(hip):
    inputs = case(5)
    t = tables((2.5, 10.0, 30.0, 50.0, 100.0, 150.0, 300.0, 590.0), curve=([0.0, 20.0], [0.0, 1.0]))
    for interp in MODES:
        got, planes = _launch(hip, *inputs, t, interp, True, f"8 heights {interp}")
        _check(got, planes, _want("8h", inputs, t, interp), f"8 heights {interp}")


# ---------------------------------------------------------------------------------------------------- identities
def test_equal_fields_give_exact_zeros(hip):
    HR, _, _, Z, terrain = case(0)
    for interp in MODES:
        got, planes = _launch(hip, HR, HR.clone(), HR.clone(), Z, terrain, tables(), interp, True, f"equal fields {interp}")
        assert float(got[..., [4, 5, 6, 7, 14, 15, 16, 17]].abs().sum()) == 0
        for a, b, c in ((1, 2, 3), (8, 9, 10), (11, 12, 13)):
            assert torch.equal(_bits(got[..., a]), _bits(got[..., b])) and torch.equal(_bits(got[..., a]), _bits(got[..., c]))
        assert torch.equal(planes[:, :, 0], planes[:, :, 1]) and torch.equal(planes[:, :, 3], planes[:, :, 5])
        assert float(got[..., 1].min()) > 0


def test_constant_field_on_between_and_beyond_the_knots(hip):
    """a field constant in space: every valid column has that V, and P = np.interp of it.  Dyadic speeds and knots:
    every value and every partial sum is exact"""
    (B, X, Y, NZ) = (1, 16, 16, 10)
    _, _, _, Z, terrain = case(1)
    t = tables(curve=([4.0, 8.0, 16.0, 24.0], [0.0, 0.25, 1.0, 0.5]))  # at UVW_MAX 32: 0.125, 0.25, 0.5, 0.75
    cv, cp = t.curve_v.double().numpy(), t.curve_p.double().numpy()
    speeds = (0.0625, 0.25, 0.375, 0.875)  # below, on, between, beyond
    f = [torch.zeros((B, 3, X, Y, NZ)) for _ in range(3)]
    for a, b, c in ((0, 1, 2), (1, 2, 3), (3, 0, 1)):
        for s, i in enumerate((a, b, c)):
            f[s][:, 0], f[s][:, 1] = speeds[i], 0.0
        f[1][:, 0], f[1][:, 1] = 0.0, -speeds[b]  # (SR along -v)
        for interp in MODES:
            got, planes = _launch(hip, *f, Z, terrain, t, interp, True, f"constant {interp}")
            n = got[0, :, 0]
            assert bool((n > 0).all())
            for s, i in enumerate((a, b, c)):
                P = float(np.interp(speeds[i], cv, cp))
                valid = planes[0, :, 6] == 1
                assert bool((planes[0, :, s][valid] == speeds[i]).all()) and bool((planes[0, :, 3 + s][valid] == P).all())
                assert bool((planes[0, :, s][~valid] == 0).all())
                assert torch.equal(got[0, :, 1 + s], n * speeds[i]) and torch.equal(got[0, :, 11 + s], n * P)
                assert torch.equal(got[0, :, 8 + s], n * speeds[i] ** 3)
            assert torch.equal(got[0, :, 4], n * abs(speeds[b] - speeds[a]))
            assert (float(np.interp(0.375, cv, cp)), float(np.interp(0.875, cv, cp)), float(np.interp(0.0625, cv, cp))) == (0.625, 0.5, 0.0)


def _dyadic_columns(B, X, Y, NZ, seed):
    """levels 8 m apart from a lowest level that is a multiple of 0.25 m in 1 .. 8.75 m: with a terrain of multiples of
    0.25 m every altitude, every height above ground and every weight of a dyadic height is exact"""
    gen = torch.Generator().manual_seed(seed)
    terrain = terrain_of(X, Y)
    h0 = 1.0 + 0.25 * torch.randint(0, 32, (B, X, Y, 1), generator=gen).float()
    h = h0 + 8.0 * torch.arange(NZ).float()
    return h, (terrain[None, :, :, None] + h)[:, None].contiguous(), terrain


def test_linear_profile_is_interpolated_exactly(hip):
    """u = 1/8 + h / 1024 on dyadic levels, linear mode, dyadic heights: every interpolated value - a multiple of 2^-12
    below 1, whose square is exact in fp32 - comes back exactly"""
    B, X, Y, NZ = 2, 7, 6, 5
    h, Z, terrain = _dyadic_columns(B, X, Y, NZ, 3)
    f = torch.zeros((B, 3, X, Y, NZ))
    f[:, 0] = 0.125 + h / 1024.0
    heights = (9.0, 12.5, 20.25, 30.0)
    assert torch.equal(Z[:, 0] - terrain[None, :, :, None], h)
    got, planes = _launch(hip, f, f.clone(), None, Z, terrain, tables(heights), "linear", True, "linear profile")
    for k, q in enumerate(heights):
        valid = planes[:, k, 6] == 1
        assert torch.equal(valid, (h[..., 0] <= q) & (q <= h[..., -1])) and bool(valid.any())
        assert bool((planes[:, k, 0][valid] == 0.125 + q / 1024.0).all()), q
        assert torch.equal(got[:, k, 1], got[:, k, 0] * (0.125 + q / 1024.0))
    assert float(got[..., TL_SUMS].abs().sum()) == 0


def test_log_law_profile(hip):
    """u = a ln(h / z0), rounded to fp32 at the levels: log mode returns a ln(q / z0) up to the knots' rounding (a convex
    combination of two values each within u0 of the law) and the kernel's own dV <= 4 u0 V - 6 u0 times the column's
    top value covers both; linear mode lies strictly below the law at every height that is no level (the law is concave)"""
    B, X, Y, NZ = 1, 9, 5, 10
    a, z0 = 0.05, 0.25
    h, Z, terrain = _dyadic_columns(B, X, Y, NZ, 4)
    f = torch.zeros((B, 3, X, Y, NZ))
    f[:, 0] = (a * torch.log(h.double() / z0)).float()
    heights = (9.5, 20.0, 41.125, 60.0)
    t = tables(heights)
    on_level = [((h - q) == 0).any(dim=-1) for q in heights]
    got, planes = _launch(hip, f, f.clone(), f.clone(), Z, terrain, t, "log", True, "log law, log")
    _, lin = _launch(hip, f, f.clone(), f.clone(), Z, terrain, t, "linear", True, "log law, linear")
    for k, q in enumerate(heights):
        valid = planes[:, k, 6] == 1
        law = a * math.log(q / z0)
        err = (planes[:, k, 0].double() - law).abs()
        assert bool(valid.any()) and bool((err[valid] <= 6 * U_FP32 * f[:, 0, ..., -1].double()[valid]).all()), (q, float(err[valid].max()))
        off = valid & ~on_level[k]
        assert bool(off.any()) and bool((lin[:, k, 0].double()[off] < law).all()), q
        assert torch.equal(lin[:, k, 6], planes[:, k, 6])


@pytest.mark.parametrize("phi", [0.3, 2.5])
def test_rotation_about_z_gives_direction_error_phi(hip, phi):
    """SR = HR turned about z by phi, formed in float64 and rounded once to fp32 at the levels.  Interpolation is linear,
    so SR at the height is the turned HR up to the knots' roundings: each component within u0 (|c| + |f_{j+1} - f_j|),
    summed over the valid columns in R"""
    from gan_sr_wind_field_amd.hub_height import column_values

    HR, _, TL, Z, terrain = case(1)
    h = HR.double()
    SR = HR.clone()
    SR[:, 0] = (math.cos(phi) * h[:, 0] - math.sin(phi) * h[:, 1]).float()
    SR[:, 1] = (math.sin(phi) * h[:, 0] + math.cos(phi) * h[:, 1]).float()
    t = tables()
    for interp in MODES:
        got, _ = _launch(hip, HR, SR, TL, Z, terrain, t, interp, False, f"rotation {phi} {interp}")
        _, _, b, _, _ = _want(("rot", phi), (HR, SR, TL, Z, terrain), t, interp)
        R = torch.stack([torch.where(c["valid"], sum(f.abs() + sp for f, sp in zip(c["uv"][1], c["span"][1])), 0.0).sum(dim=(1, 2))
                         for c in column_values(HR, SR, TL, Z, terrain, t, interp)], dim=1) * U_FP32
        err = (got[..., 16] - phi * got[..., 1]).abs()
        assert bool((err <= b[..., 16] + phi * b[..., 1] + 2 * R).all()), (phi, interp, err.tolist())
        bias = (got[..., 2] - got[..., 1]).abs()
        assert bool((bias <= b[..., 2] + b[..., 1] + R).all()), (phi, interp, bias.tolist())
        print(f"[identity] rotation by {phi} ({interp}): direction error per height {(got[0, :, 16] / got[0, :, 1]).tolist()}")


# ---------------------------------------------------------------------------------------------------- special columns
@pytest.mark.parametrize("k", [1, 2, 5], ids=lambda k: "x".join(map(str, CASES[k][0])))
def test_special_columns(hip, k):
    """a height exactly on a level and on the top level, one fp32 step outside and inside either end, a column that
    begins above the height, a lowest level at or below the ground (log mode), NaN altitudes - at the first and the last
    column, on both sides of the first staging boundary and at every fifth column"""
    from gan_sr_wind_field_amd import hip_ops

    (B, X, Y, NZ), _, _ = CASES[k]
    cps = hip_ops.hub_height_columns_per_chunk(NZ, len(HEIGHTS))
    HR, SR, TL, Z, terrain, kinds = plant_specials(case(k), cps)
    assert bool(torch.isnan(Z).any()) == bool((kinds >= 9).any()) and bool((kinds[:, [0, cps - 1, cps, X * Y - 1]] >= 0).all())
    t = tables()
    for interp in MODES:
        want = _want(("special", k), (HR, SR, TL, Z, terrain), t, interp)
        got, planes = _launch(hip, HR, SR, TL, Z, terrain, t, interp, True, f"special columns {CASES[k][0]} {interp}")
        _check(got, planes, want, f"special columns {CASES[k][0]} {interp}")
        # a height on a level, or on the top level: that level's value bit for bit (``KNOT_UV`` there: V is exact)
        h = (Z[:, 0] - terrain[None, :, :, None]).reshape(B, X * Y, NZ)
        for b, c in ((kinds == 0) | (kinds == 1)).nonzero().tolist():
            qi = (c + b) % 2
            assert float(h[b, c, NZ // 2 if kinds[b, c] == 0 else NZ - 1]) == HEIGHTS[qi]
            if planes[b, qi, 6].reshape(-1)[c] != 1:  # (log mode: the column begins below the ground)
                assert interp == "log" and float(h[b, c, 0]) <= 0
                continue
            assert tuple(float(planes[b, qi, s].reshape(-1)[c]) for s in range(3)) == KNOT_V, (b, c)
        if interp == "log":
            lin = _want(("special", k), (HR, SR, TL, Z, terrain), t, "linear")
            assert float(lin[0][..., 0].sum()) > float(want[0][..., 0].sum())  # (h_0 <= 0: valid in linear mode only)


# ---------------------------------------------------------------------------------------------------- completeness
def test_no_baseline_and_another_stream(hip):
    from gan_sr_wind_field_amd import hip_ops

    HR, SR, TL, Z, terrain = case(5)
    t = tables()
    got, planes = _launch(hip, HR, SR, None, Z, terrain, t, "log", True, "tl = NULL")
    _check(got, planes, _want(5, (HR, SR, None, Z, terrain), t, "log"), "tl = NULL")
    assert float(got[..., TL_SUMS].abs().sum()) == 0 and float(planes[:, :, [2, 5]].abs().sum()) == 0
    full = _want(5, (HR, SR, TL, Z, terrain), t, "log")
    # another stream: the operand is written on that stream just before the launch
    ops = [f.to(DEV) for f in (HR, SR, TL, Z, terrain)]
    base = hip_ops.hub_height(*ops, t, "log")
    stale = torch.zeros_like(ops[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        stale.copy_(ops[0], non_blocking=True)
        assert hip_ops._stream().value == s.cuda_stream
        out = hip_ops.hub_height(stale, *ops[1:], t, "log")
    s.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(base.cpu()))
    assert_within(out.cpu(), full[0], full[2], "hub_height on another stream[(3, 33, 17, 10)]", kind="sums")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(hip):
    import ctypes

    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 6, 5, 4
    t = tables()
    nh, nk = 4, t.curve_v.numel()
    HR, SR, TL, Z, terrain = (f.to(DEV) for f in make(B, X, Y, NZ, seed=1, channels=(3, 3, 3)))
    n_ws = int(hip.wsr_hub_height_workspace_floats(B, X, Y, NZ, nh))
    assert n_ws == nh * NS
    out = Guarded((B, nh, 2 * NS), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    cols = Guarded((B, nh, PLANES, X, Y), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws, cols)]
    p = hip_ops._p
    H8 = tuple(float(v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 9))
    V33 = tuple(i / 64.0 for i in range(33))

    def floats(v):
        return None if v is None else (ctypes.c_float * max(len(v), 1))(*v)

    def call(hr=HR, hr_c=3, sr=SR, sr_c=3, tl=TL, tl_c=3, z=Z, g=terrain, hs=HEIGHTS, n_h=None, cv=tuple(t.curve_v.tolist()),
             cp=tuple(t.curve_p.tolist()), n_k=None, log=1, b=B, nx=X, ny=Y, nz=NZ, w=ws.t, o=out.t, c=cols.t):
        return hip.wsr_hub_height(p(hr), hr_c, p(sr), sr_c, p(tl), tl_c, p(z), p(g), floats(hs), len(hs or ()) if n_h is None else n_h,
                                  floats(cv), floats(cp), len(cv or ()) if n_k is None else n_k, log, b, nx, ny, nz, p(w), p(o),
                                  p(c), hip_ops._stream())

    invalid = [dict(hr=None), dict(sr=None), dict(z=None), dict(g=None), dict(hs=None, n_h=4), dict(cv=None, n_k=nk),
               dict(cp=None, n_k=nk), dict(w=None), dict(o=None), dict(hr_c=2), dict(sr_c=2), dict(tl_c=2), dict(tl_c=0),
               dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nz=1), dict(hs=(), n_h=0), dict(hs=H8, n_h=9), dict(n_h=-1),
               dict(hs=(50.0, 10.0)), dict(hs=(50.0, 50.0)), dict(hs=(0.0, 50.0)), dict(hs=(-1.0,)), dict(hs=(NAN,)),
               dict(hs=(10.0, float("inf"))), dict(cv=(0.5,), cp=(1.0,)), dict(cv=V33, cp=V33), dict(cv=(0.5, 0.25), cp=(0.0, 1.0)),
               dict(cv=(0.5, 0.5), cp=(0.0, 1.0)), dict(cv=(-0.1, 0.5), cp=(0.0, 1.0)), dict(cv=(0.1, NAN), cp=(0.0, 1.0)),
               dict(log=2), dict(log=-1)]
    for kw in invalid:
        assert call(**kw) == -1, kw
    for kw in (dict(nz=129), dict(b=65536), dict(nx=32769), dict(nx=32768, ny=32768, nz=2)):
        assert call(**kw) == -2, kw
    wsf = hip.wsr_hub_height_workspace_floats
    assert wsf(0, X, Y, NZ, nh) == wsf(B, X, Y, 1, nh) == wsf(B, X, Y, 129, nh) == wsf(B, X, Y, NZ, 9) == wsf(65536, X, Y, NZ, nh) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws, cols), before):
        assert torch.equal(g.base.view(torch.int32), b4)
    assert call() == 0 and call(tl=None, tl_c=0, c=None) == 0  # (the arguments the refusals vary are fine)
    torch.cuda.synchronize()

    # the wrapper: every refusal a ValueError naming what is wrong
    ok = hip_ops.hub_height(HR, SR, TL, Z, terrain, t, "log")
    assert ok.shape == (B, nh, NS) and float(ok[..., 0].sum()) > 0
    bad = [((HR[:, :2].contiguous(), SR, TL, Z, terrain), "HR"), ((HR.double(), SR, TL, Z, terrain), "HR"),
           ((HR, SR[..., :2], TL, Z, terrain), "SR"), ((HR, SR[..., :2].contiguous(), TL, Z, terrain), "SR"),
           ((HR, SR, torch.cat([TL, TL]), Z, terrain), "TL"), ((HR, SR, TL, HR, terrain), "levels Z"),
           ((HR, SR, TL, Z[..., :2].contiguous(), terrain), "levels Z"), ((HR, SR, TL, Z.double(), terrain), "Z"),
           ((HR, SR, TL, Z, terrain[:, :3].contiguous()), "terrain"), ((HR, SR, TL, Z, terrain.double()), "terrain"),
           ((HR, SR, TL, Z, terrain.t()), "terrain")]
    for args, pattern in bad:
        with pytest.raises(ValueError, match=pattern):
            hip_ops.hub_height(*args, t, "log")
    with pytest.raises(ValueError, match="interp must be linear or log"):
        hip_ops.hub_height(HR, SR, TL, Z, terrain, t, "cubic")
    for kw, pattern in ((dict(heights_m=(50.0, 10.0)), "heights must be strictly"), (dict(heights_m=()), "heights must hold"),
                        (dict(curve_speeds=(1.0,), curve_power=(1.0,)), "curve_speeds must hold"),
                        (dict(curve_power=t.curve_power[:-1]), "curve_power must hold one value per knot"),
                        (dict(heights=t.heights[:-1]), "4 heights and 12 knots, got 3")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.hub_height(HR, SR, TL, Z, terrain, t._replace(**kw), "log")
    one = tuple(f[..., :1].contiguous() for f in (HR, SR, TL, Z))
    with pytest.raises(ValueError, match="2 .. 128 levels, not 1"):
        hip_ops.hub_height(*one, terrain, t, "log")
    with pytest.raises(ValueError, match="out"):
        hip_ops.hub_height(HR, SR, TL, Z, terrain, t, "log", out=torch.empty((B, nh, NS), device=DEV))
    with pytest.raises(RuntimeError):
        hip_ops.hub_height(HR.cpu(), SR, TL, Z, terrain, t, "log")
    # the tables are converted once per (device, parameters)
    n = len(hip_ops._hub_height_tables)
    hip_ops.hub_height(HR, SR, TL, Z, terrain, tables(), "linear")
    assert len(hip_ops._hub_height_tables) == n
    hip_ops.hub_height(HR, SR, TL, Z, terrain, tables((10.0, 60.0)), "log")
    assert len(hip_ops._hub_height_tables) == n + 1


# ---------------------------------------------------------------------------------------------------- the model's entry
def test_gan_hub_height(hip):
    import torch.nn.functional as F

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.config.config import HubHeightConfig
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    HR, SR, _, Z, terrain = make(2, 12, 8, 5, seed=4, channels=(3, 3, 3))
    LR = 0.3 * torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    hc = HubHeightConfig()
    hc.load(None)
    stub = SimpleNamespace(cfg=SimpleNamespace(scale=4, hub_height=hc))
    try:
        for section, t, interp in ((dict(), tables((50.0, 100.0, 150.0), 20.0), "log"),  # (no section: its defaults)
                                   (dict(present=True, heights=[10.0, 60.0], interp="linear"), tables((10.0, 60.0), 20.0), "linear")):
            for key, v in section.items():
                setattr(hc, key, v)
            got, cols = wind_field_GAN_3D.hub_height(stub, HR.to(DEV), SR.to(DEV), LR.to(DEV), Z.to(DEV), terrain, 20.0, True)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (2, t.heights.numel(), NS) and cols.is_cuda
            TL_dev = hip_ops.trilinear_xy(LR.to(DEV), 4).cpu()
            want = _want(("gan", interp), (HR, SR, TL_dev, Z, terrain), t, interp)
            _check(got.cpu(), cols.cpu(), want, f"gan.hub_height {interp}")
            # on a CPU device the same entry is the reference
            TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
            assert torch.equal(wind_field_GAN_3D.hub_height(stub, HR, SR, LR, Z, terrain, 20.0),
                               hub_height_reference(HR, SR, TL, Z, terrain, t, interp))
    finally:
        hc.load(None)


# ---------------------------------------------------------------------------------------------------- run.py
def column_bounds(s, b, t, rho, ncols):
    """the bounds ``b`` (NH, 18) of the sums ``s`` carried through ``hub_height_from_sums`` -> a list per column"""
    from gan_sr_wind_field_amd.hub_height import COLUMNS

    uvw = t.UVW_MAX
    out = {c: [] for c in COLUMNS}
    src = {"HR": 0, "SR": 1, "trilinear": 2}
    prev = None
    for k in range(s.shape[0]):
        n = max(float(s[k, 0]), 1.0)
        S, Bd = s[k].tolist(), b[k].tolist()
        out["height_m"].append(0.0), out["valid_fraction"].append(0.0)

        def ratio(a, h):  # |(a + ea) / (h + eh) - a / h|
            return (Bd[a] + abs(S[a] / S[h]) * Bd[h]) / max(S[h] - Bd[h], 1e-300) if S[h] > 0 else math.inf

        rel_v = {}
        for tag, i in src.items():
            out["speed_" + tag].append(Bd[1 + i] / n * uvw)
            out["power_density_" + tag].append(0.5 * rho * Bd[8 + i] / n * uvw ** 3)
            out["capacity_factor_" + tag].append(Bd[11 + i] / n)
            rel_v[tag] = Bd[1 + i] / max(S[1 + i] - Bd[1 + i], 1e-300)  # |ln(1 + x)| <= x / (1 - x)
            q = t.heights_m[k]
            out["shear_exponent_" + tag].append(0.0 if prev is None else (rel_v[tag] + prev[1][tag]) / math.log(q / prev[0]))
        for twin, i in (("", 1), ("_trilinear", 2)):
            out["speed_bias" + twin].append((Bd[1 + i] + Bd[1]) / n * uvw)
            out["speed_mae" + twin].append(Bd[3 + i] / n * uvw)
            x, e = S[5 + i] / n, Bd[5 + i] / n
            out["speed_rmse" + twin].append((e / math.sqrt(x - e) if x > 4 * e else math.sqrt(e)) * uvw)
            out["direction_error_deg" + twin].append(math.degrees(ratio(15 + i, 1)))
            out["power_density_rel_error" + twin].append(ratio(8 + i, 8))
            out["capacity_factor_error" + twin].append((Bd[11 + i] + Bd[11]) / n)
            out["power_mae" + twin].append(Bd[13 + i] / n)
        prev = (t.heights_m[k], rel_v)
    return out


def _read(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return list(csv.reader(f))


def _earlier_files(name, run_dir):
    """the files a run without the section writes: path relative to the run -> bytes"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____") and "hub_height" not in f:
            with open(os.path.join("test_output", f), "rb") as fh:
                out[f[len(name):]] = fh.read()
    for f in sorted(os.listdir(os.path.join(run_dir, "fields"))):
        with open(os.path.join(run_dir, "fields", f), "rb") as fh:
            out["fields/" + f] = fh.read()
    return out


def _float64_columns(run_dir, names, terrain, t, interp, rho, raw):
    """(columns, bounds) of the fields a run pickled, in float64 from its own HR / SR / TL / Z (flat levels), or for
    ``raw`` from its raw truth alone (SR = TL = HR: the HR-only columns)"""
    from gan_sr_wind_field_amd.hub_height import hub_height_from_sums, hub_height_reference

    total = bound = None
    for name in names:
        with open(os.path.join(run_dir, "fields", f"test_fields_{name}.pkl"), "rb") as f:
            p = pickle.load(f)
        keys = ("HR_orig", "HR_orig", "HR_orig", "Z_orig") if raw else ("HR", "SR", "TL", "Z")
        HR, SR, TL, Z = (torch.from_numpy(np.asarray(p[k]))[None] for k in keys)
        Z = Z[:, None] if Z.dim() == 4 else Z
        s = hub_height_reference(HR, SR, TL, Z, terrain, t, interp)
        bd = sum_bounds(magnitudes(HR, SR, TL, Z, terrain, t, interp)[0])
        total = s[0] if total is None else total + s[0]
        bound = bd[0] if bound is None else bound + bd[0]
    ncols = len(names) * HR.shape[2] * HR.shape[3]
    return hub_height_from_sums(total, t, rho, ncols), column_bounds(total, bound, t, rho, ncols)


def test_run_test_device_loop_against_host_loop(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.hub_height import COLUMNS

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.hub_height

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "hub_height", counted)

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
    uvw, rho = float(te.UVW_MAX), 1.2
    terrain = torch.from_numpy(np.asarray(te.terrain)).float()
    # heights from the level range of the raw columns: 10 m, a third of the way up, and the height 30 % of the raw column
    # tops stay below - every height is valid in part of the raw domain (2 m, the lowest level, is on either side too)
    tops = torch.cat([te[i][5][0, ..., -1] - terrain for i in range(len(te))]).flatten()
    heights = [10.0, round(float(tops.mean()) / 3, 2), round(float(tops.quantile(0.3)), 2)]
    sec = (f"\n[HUB_HEIGHT]\nheights = {heights}\ninterp = log\nair_density = {rho}\nper_field = True\nwrite_maps = True\n")
    load = dict(generator_load_path=os.path.join(dir_t, "G_6.pth"), discriminator_load_path=os.path.join(dir_t, "D_6.pth"),
                state_load_path=os.path.join(dir_t, "state_6.pth"))
    _, dir_a = run("plain", ["--test"], dev_loop, **load)
    assert calls["n"] == 0 and not any("hub_height" in f for f in os.listdir("test_output"))
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

    t = tables(heights, uvw)
    names = [te[i][3] for i in range(len(te))]
    X, Y = te[0][1].shape[1:3]
    hr_only = [c for c in COLUMNS[2:] if c.endswith("_HR")]
    worst = 0.0
    for suffix, raw in (("", False), ("_reverse_interpolate", True)):
        rows = {n: _read(n, "hub_height" + suffix) for n in ("dev", "host")}
        f64 = {n: _float64_columns(d, names, terrain, t, "log", rho, raw) for n, d in (("dev", dir_b), ("host", dir_c))}
        for n in rows:
            assert rows[n][0] == list(COLUMNS) and len(rows[n]) == 1 + 3
            per = _read(n, "hub_height_fields" + suffix)
            assert per[0] == ["field"] + list(COLUMNS) and len(per) == 1 + 3 * n_test and [r[0] for r in per[1::3]] == names
        avg = open(os.path.join("test_output", f"averages_hub_height{suffix}.csv")).read().strip().splitlines()
        assert avg[0] == "Name," + ",".join(COLUMNS) and [r.split(",")[0] for r in avg[1:]] == ["dev"] * 3 + ["host"] * 3
        for k in range(3):
            rd, rh = rows["dev"][1 + k], rows["host"][1 + k]
            assert rd[:2] == rh[:2] and float(rd[0]) == heights[k], (suffix, rd[:2], rh[:2])  # height and valid_fraction: text
            assert 0 < float(rd[1]) <= 1 and (not raw or k < 2 or float(rd[1]) < 1), (suffix, k, rd[1])
            for i, c in enumerate(COLUMNS):
                if i < 2 or (raw and c not in hr_only):
                    continue
                d, h = float(rd[i]), float(rh[i])
                if math.isnan(d) or math.isnan(h):  # (the shear exponent of the first height)
                    assert math.isnan(d) and math.isnan(h) and k == 0 and c.startswith("shear"), (suffix, c, k)
                    continue
                own = 0.0
                for n, v in (("dev", d), ("host", h)):  # each loop against the float64 columns of its own fields
                    want, bnd = f64[n][0][c][k], f64[n][1][c][k] + 2.0 ** -40 * abs(f64[n][0][c][k])
                    worst = max(worst, abs(v - want) / bnd)
                    assert abs(v - want) <= bnd, (suffix, n, c, k, v, want, bnd)
                    own += bnd
                assert abs(d - h) <= own + abs(f64["dev"][0][c][k] - f64["host"][0][c][k]), (suffix, c, k, d, h)
    assert _read("dev", "hub_height") != _read("dev", "hub_height_reverse_interpolate")
    print(f"[e2e] hub-height columns of both loops against float64: worst |err| / bound {worst:.3g}")

    # the maps: keys, shapes, and their mean is the file's speed where every column is valid in every field
    for suffix in ("", "_reverse_interpolate"):
        m = np.load(os.path.join("test_output", f"dev____hub_height_maps{suffix}.npz"))
        assert sorted(m.files) == ["capacity_factor", "heights", "speed", "valid_fraction", "x", "y"]
        assert m["heights"].tolist() == heights and m["x"].shape == (X,) and m["y"].shape == (Y,)
        assert m["valid_fraction"].shape == (3, X, Y) and m["speed"].shape == m["capacity_factor"].shape == (3, 3, X, Y)
        rows = _read("dev", "hub_height" + suffix)
        for k in range(3):
            assert float(m["valid_fraction"][k].mean()) == pytest.approx(float(rows[1 + k][1]), rel=1e-12)
            if float(rows[1 + k][1]) == 1.0:  # (the same fp32 values: the map adds them in double, the file's sums within
                rel = LAMBDA * math.sqrt(n_test * X * Y) * U_FP32 + 1e-12  # LAMBDA sqrt(K) 2^-24 of their non-negative terms)
                for s in range(3):
                    assert float(m["speed"][k, s].mean()) == pytest.approx(float(rows[1 + k][2 + s]), rel=rel)
                    assert float(m["capacity_factor"][k, s].mean()) == pytest.approx(float(rows[1 + k][18 + s]), rel=rel, abs=1e-300)
    print(f"[time] tests/test_hub_height_gpu.py up to here: {time.time() - T0:.1f} s")
