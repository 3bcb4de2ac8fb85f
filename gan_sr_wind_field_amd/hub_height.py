"""Hub-height wind resource (``[HUB_HEIGHT]``): the wind at fixed heights above ground, its power density and the yield of
a turbine, for the truth (HR), the super-resolved field (SR) and the trilinear baseline (TL).  Every other evaluation
section works on the model's own levels, whose height above ground differs from column to column on the raw grid; a
wind-resource user wants the field at a turbine's hub height, and in units of power - which goes with V^3, so a field
that is a few percent too smooth looks fine point-wise and is visibly wrong in energy yield.

Everything is built from NS = 18 sums per sample and height: on a GPU ``hip_ops.hub_height`` takes them in one fused
launch on the native layout (csrc/hub_height.hip), ``hub_height_reference`` composes the same quantities from torch ops
on any device (the path of a CPU device and of the host loop, and the oracle of the tests).  ``hub_height_from_sums``
turns a table of sums into the columns of the files, defined once for every caller.

This module is the single place where the quantities are defined.  Operands are HR, SR and TL, each (B, C >= 2, X, Y,
NZ), of which only channels 0 (u) and 1 (v) are read, as normalised values (w is not part of the wind-resource speed, as
in ``[DISTRIBUTION]``); ``Z`` (B, 1, X, Y, NZ), the raw altitude, taken as strictly increasing along z (documented, not
checked); ``terrain`` (X, Y), the ground altitude.  With fl() the rounding to fp32, for every column (b, i, j) and
height q (metres above ground, rounded once to fp32 by ``hub_height_tables``):

    height      h_k = fl(Z[b, 0, i, j, k] - terrain[i, j]): ONE fp32 subtraction, in the reference too, which only then
                widens - so validity and the choice of the interval are the same comparisons of the same fp32 numbers
    validity    the column is valid for q iff h_0 <= q <= h_{NZ-1} (fp32 comparisons: false for a NaN), no h_k is a NaN,
                and in ``log`` mode h_0 > 0.  No extrapolation; an invalid column enters no sum for that height
    interval    j = the largest index with h_j <= q.  j = NZ - 1 (q on the top level): the top level's value.  Else the
                weight, in double from the fp32 heights: ``linear`` t = (q - h_j) / (h_{j+1} - h_j) (np.interp, as the
                re-levelling), ``log`` t = ln(q / h_j) / ln(h_{j+1} / h_j) (exact for a log-law profile)
    value       every component c in {u, v}: f_j + t (f_{j+1} - f_j), so t = 0 returns the knot's value bit for bit (the
                kernel evaluates this in double and rounds once to fp32)
    speed       V = sqrt(u^2 + v^2), normalised units;  P = curve(V): piecewise linear between the knots
                (curve_speeds / UVW_MAX, curve_power), the end values outside - ``np.interp``
    sums        over the valid columns, index 0 .. 17 (``SUMS``): n_valid;  sum V of HR, SR, TL;  sum |V_s - V_HR| for
                s = SR, TL;  sum (V_s - V_HR)^2;  sum V^3 of HR, SR, TL;  sum P of HR, SR, TL;  sum |P_s - P_HR|;
                sum V_HR angle(HR, s) with angle(a, b) = atan2(|a x b|, a . b), 0 for two zero vectors
                (``diagnostics.level_sums_reference``): direction errors are weighted by the true horizontal speed, so
                calm air needs no threshold

The sums form a float64 (B, NH, 18) table; without TL its entries are zeros.  The optional per-column planes are
(B, NH, 7, X, Y): V of HR, SR, TL, P of HR, SR, TL, and validity as 1.0 / 0.0, with zeros in the six value planes of an
invalid column.

The curve is continuous by construction, with the end values clamped; a cut-out is a steep segment the user writes (the
default falls from 1 at 25 m/s to 0 at 26 m/s).  That keeps every reported quantity Lipschitz in the inputs.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

NS = 18                # WSR_HUB_HEIGHT_SUMS
PLANES = 7             # WSR_HUB_HEIGHT_PLANES
MAX_HEIGHTS = 8        # WSR_HUB_HEIGHT_MAX_HEIGHTS
MIN_KNOTS, MAX_KNOTS = 2, 32  # WSR_HUB_HEIGHT_MAX_KNOTS
MAX_NZ = 128           # WSR_HUB_HEIGHT_MAX_NZ
INTERP = ("linear", "log")

SUMS = ("n_valid", "V_HR", "V_SR", "V_TL", "absdV_SR", "absdV_TL", "sqdV_SR", "sqdV_TL", "V3_HR", "V3_SR", "V3_TL",
        "P_HR", "P_SR", "P_TL", "absdP_SR", "absdP_TL", "angle_SR", "angle_TL")
#: the columns of ``<name>____hub_height.csv``
COLUMNS = ("height_m", "valid_fraction", "speed_HR", "speed_SR", "speed_trilinear", "speed_bias", "speed_bias_trilinear",
           "speed_mae", "speed_mae_trilinear", "speed_rmse", "speed_rmse_trilinear", "direction_error_deg",
           "direction_error_deg_trilinear", "power_density_HR", "power_density_SR", "power_density_trilinear",
           "power_density_rel_error", "power_density_rel_error_trilinear", "capacity_factor_HR", "capacity_factor_SR",
           "capacity_factor_trilinear", "capacity_factor_error", "capacity_factor_error_trilinear", "power_mae",
           "power_mae_trilinear", "shear_exponent_HR", "shear_exponent_SR", "shear_exponent_trilinear")


class HubHeightTables(NamedTuple):
    """What ``hub_height_tables`` returns: fp32 host tensors ``heights`` (NH,) in metres, ``curve_v`` (NK,) in normalised
    units and ``curve_p`` (NK,), and the parameters they were made from"""

    heights: torch.Tensor
    curve_v: torch.Tensor
    curve_p: torch.Tensor
    heights_m: tuple
    curve_speeds: tuple
    curve_power: tuple
    UVW_MAX: float


def _numbers(values, name, what):
    try:
        return [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a list of numbers, not {values!r}") from None


def check_heights(heights, what="hub_height") -> list:
    """The range of ``heights``: 1 .. 8 finite numbers > 0 in metres above ground, strictly ascending, else a ValueError
    naming ``heights`` -> a list of floats"""
    hs = _numbers(heights, "heights", what)
    if not 1 <= len(hs) <= MAX_HEIGHTS:
        raise ValueError(f"{what}: heights must hold 1 .. {MAX_HEIGHTS} entries, not {len(hs)}")
    if not all(v > 0 and math.isfinite(v) for v in hs):
        raise ValueError(f"{what}: heights must be finite numbers > 0 (metres above ground), not {hs}")
    if any(b <= a for a, b in zip(hs, hs[1:])):
        raise ValueError(f"{what}: heights must be strictly ascending, not {hs}")
    return hs


def check_curve(curve_speeds, curve_power, what="hub_height"):
    """The range of the power curve: 2 .. 32 knots, speeds in m/s finite, >= 0 and strictly ascending, power a fraction
    of rated in [0, 1], else a ValueError naming the key -> two lists of floats"""
    cs, cp = _numbers(curve_speeds, "curve_speeds", what), _numbers(curve_power, "curve_power", what)
    if not MIN_KNOTS <= len(cs) <= MAX_KNOTS:
        raise ValueError(f"{what}: curve_speeds must hold {MIN_KNOTS} .. {MAX_KNOTS} knots, not {len(cs)}")
    if len(cp) != len(cs):
        raise ValueError(f"{what}: curve_power must hold one value per knot of curve_speeds ({len(cs)}), not {len(cp)}")
    if not all(v >= 0 and math.isfinite(v) for v in cs):
        raise ValueError(f"{what}: curve_speeds must be finite numbers >= 0 (m/s), not {cs}")
    if any(b <= a for a, b in zip(cs, cs[1:])):
        raise ValueError(f"{what}: curve_speeds must be strictly ascending, not {cs}")
    if not all(0 <= v <= 1 for v in cp):
        raise ValueError(f"{what}: curve_power must be fractions of rated power in [0, 1], not {cp}")
    return cs, cp


def check_interp(interp, what="hub_height") -> str:
    if interp not in INTERP:
        raise ValueError(f"{what}: interp must be linear or log, not {interp!r}")
    return interp


def hub_height_tables(UVW_MAX: float, heights, curve_speeds, curve_power) -> HubHeightTables:
    """The tables of the module docstring, built once per parameter set: the heights and, divided by ``UVW_MAX`` in
    Python doubles, the curve's speeds, each rounded once to fp32 and still strictly ascending afterwards"""
    hs = check_heights(heights, "hub_height_tables")
    cs, cp = check_curve(curve_speeds, curve_power, "hub_height_tables")
    uvw = float(UVW_MAX)
    if not (uvw > 0 and math.isfinite(uvw)):
        raise ValueError(f"hub_height_tables: UVW_MAX must be a finite number > 0, not {UVW_MAX}")
    h32 = torch.tensor(hs, dtype=torch.float64).float()
    v32 = torch.tensor([v / uvw for v in cs], dtype=torch.float64).float()
    for name, t in (("heights", h32), ("curve_speeds", v32)):
        if not (bool(torch.isfinite(t).all()) and bool((t[1:] > t[:-1]).all())):
            raise ValueError(f"hub_height_tables: {name} are not finite, strictly ascending fp32 numbers "
                             f"(UVW_MAX = {UVW_MAX}): {t.tolist()}")
    return HubHeightTables(h32, v32, torch.tensor(cp, dtype=torch.float64).float(), tuple(hs), tuple(cs), tuple(cp), uvw)


def curve_reference(V: torch.Tensor, curve_v: torch.Tensor, curve_p: torch.Tensor) -> torch.Tensor:
    """``np.interp(V, curve_v, curve_p)`` in V's dtype: the end values outside, slope * (V - v_i) + p_i inside"""
    cv, cp = curve_v.to(V.dtype), curve_p.to(V.dtype)
    nk = cv.numel()
    i = (V.unsqueeze(-1) >= cv[1:nk - 1]).sum(dim=-1) if nk > 2 else torch.zeros_like(V, dtype=torch.long)
    x0, x1, y0, y1 = cv[i], cv[i + 1], cp[i], cp[i + 1]
    inside = (y1 - y0) / (x1 - x0) * (V - x0) + y0
    P = torch.where(V >= cv[-1], cp[-1], torch.where(V > cv[0], inside, cp[0]))
    return torch.where(torch.isnan(V), V, P)


def _angle(au, av, bu, bv):
    return torch.atan2((au * bv - av * bu).abs(), au * bu + av * bv)  # (atan2(0, 0) = 0)


def _check_operands(HR, SR, TL, Z, terrain, interp, who):
    check_interp(interp, who)
    if HR.dim() != 5 or HR.shape[1] < 2:
        raise ValueError(f"{who} wants HR as (B, C >= 2, X, Y, NZ), not {tuple(HR.shape)}")
    B, _, X, Y, NZ = HR.shape
    if SR is None:
        raise ValueError(f"{who}: SR must be given")
    for name, f in (("SR", SR), ("TL", TL)):
        if f is not None and (f.dim() != 5 or (f.shape[0],) + tuple(f.shape[2:]) != (B, X, Y, NZ) or f.shape[1] < 2):
            raise ValueError(f"{who}: {name} {tuple(f.shape)} does not match HR {tuple(HR.shape)}")
    if tuple(Z.shape) != (B, 1, X, Y, NZ) or tuple(terrain.shape) != (X, Y):
        raise ValueError(f"{who} wants Z ({B}, 1, {X}, {Y}, {NZ}) and terrain ({X}, {Y}), not {tuple(Z.shape)} and "
                         f"{tuple(terrain.shape)}")
    if NZ < 2:
        raise ValueError(f"{who} needs at least 2 levels, not {NZ}")
    return B, X, Y, NZ


def column_values(HR, SR, TL, Z, terrain, tables: HubHeightTables, interp, dtype=torch.float64):
    """Steps 1 and 2 of the module docstring and the speeds, for one height after the other: yields per height a dict of
    (B, X, Y) tensors - ``valid`` (bool), ``t`` (the weight, 0 where invalid or on the top level), and per source HR,
    SR, TL (None for an absent TL) the lists ``uv`` ((u, v) at the height), ``span`` ((|u_{j+1} - u_j|, |v_{j+1} - v_j|)
    of the interval), ``V`` and ``P``.  Heights above ground, validity and the interval come from fp32 comparisons,
    everything after them is in ``dtype``."""
    B, X, Y, NZ = _check_operands(HR, SR, TL, Z, terrain, interp, "hub_height_reference")
    dev = HR.device
    h = Z[:, 0].float() - terrain.to(dev).float()[None, :, :, None]  # (B, X, Y, NZ): the ONE fp32 subtraction
    has_nan = torch.isnan(h).any(dim=-1)
    h0, htop, hd = h[..., 0], h[..., -1], h.to(dtype)
    comps = [None if f is None else (f[:, 0].to(dtype), f[:, 1].to(dtype)) for f in (HR, SR, TL)]
    cv, cp = tables.curve_v.to(dev), tables.curve_p.to(dev)
    zero = torch.zeros((), dtype=dtype, device=dev)
    for k in range(tables.heights.numel()):
        q = tables.heights[k].to(dev)  # fp32
        valid = (h0 <= q) & (q <= htop) & ~has_nan
        if interp == "log":
            valid = valid & (h0 > 0)
        j = ((h <= q).sum(dim=-1) - 1).clamp(0, NZ - 1)
        j1 = (j + 1).clamp(max=NZ - 1)
        hj, hj1 = hd.gather(-1, j[..., None])[..., 0], hd.gather(-1, j1[..., None])[..., 0]
        qd = q.to(dtype)
        t = torch.log(qd / hj) / torch.log(hj1 / hj) if interp == "log" else (qd - hj) / (hj1 - hj)
        t = torch.where(valid & (j < NZ - 1), t, zero)
        res = {"valid": valid, "t": t, "uv": [], "span": [], "V": [], "P": []}
        for c in comps:
            if c is None:
                for key in ("uv", "span", "V", "P"):
                    res[key].append(None)
                continue
            ends = [(f.gather(-1, j[..., None])[..., 0], f.gather(-1, j1[..., None])[..., 0]) for f in c]
            u, v = (a + t * (d - a) for a, d in ends)
            res["uv"].append((u, v))
            res["span"].append(tuple((d - a).abs() for a, d in ends))
            res["V"].append(torch.sqrt(u * u + v * v))
            res["P"].append(curve_reference(res["V"][-1], cv, cp))
        yield res


def hub_height_reference(HR, SR, TL, Z, terrain, tables: HubHeightTables, interp, with_columns=False,
                         dtype=torch.float64):
    """The sums of the module docstring, composed from torch ops on the tensors' device (``column_values``, then the
    sums over the valid columns).  HR, SR, TL (B, C >= 2, X, Y, NZ; channels 0 and 1), Z (B, 1, X, Y, NZ), terrain
    (X, Y) -> float64 (B, NH, 18), with ``with_columns`` followed by the planes (B, NH, 7, X, Y) in ``dtype``.  ``TL``
    None: zeros in its sums and planes."""
    B, X, Y, NZ = _check_operands(HR, SR, TL, Z, terrain, interp, "hub_height_reference")
    dev, nh = HR.device, tables.heights.numel()
    sums = torch.zeros((B, nh, NS), dtype=torch.float64, device=dev)
    cols = torch.zeros((B, nh, PLANES, X, Y), dtype=dtype, device=dev) if with_columns else None
    zero = torch.zeros((), dtype=dtype, device=dev)
    for k, c in enumerate(column_values(HR, SR, TL, Z, terrain, tables, interp, dtype)):
        valid, uv, V, P = c["valid"], c["uv"], c["V"], c["P"]

        def total(x):
            return torch.where(valid, x, zero).double().sum(dim=(1, 2))

        sums[:, k, 0] = valid.double().sum(dim=(1, 2))
        for s in range(3):
            if V[s] is None:
                continue
            sums[:, k, 1 + s] = total(V[s])
            sums[:, k, 8 + s] = total(V[s] * V[s] * V[s])
            sums[:, k, 11 + s] = total(P[s])
            if s:
                dV = V[s] - V[0]
                sums[:, k, 3 + s] = total(dV.abs())
                sums[:, k, 5 + s] = total(dV * dV)
                sums[:, k, 13 + s] = total((P[s] - P[0]).abs())
                sums[:, k, 15 + s] = total(V[0] * _angle(*uv[0], *uv[s]))
            if cols is not None:
                cols[:, k, s] = torch.where(valid, V[s], zero)
                cols[:, k, 3 + s] = torch.where(valid, P[s], zero)
        if cols is not None:
            cols[:, k, 6] = valid.to(dtype)
    return (sums, cols) if with_columns else sums


def _ratio(a, b):
    return a / b if b else math.nan


def hub_height_from_sums(table, tables: HubHeightTables, air_density: float, ncols: float) -> dict:
    """``COLUMNS`` from a (NH, 18) table of sums (a tensor or nested lists; sum over the fields first), in double: one
    list per column, one entry per height.  ``ncols``: the number of columns that were looked at (X * Y times the
    fields).  With n = n_valid, a value is nan where n is 0:

        ``valid_fraction`` = n / ncols;  ``speed_*`` = mean V times UVW_MAX (m/s);  ``speed_bias`` = speed_SR - speed_HR,
        ``speed_mae`` = mean |V_SR - V_HR|, ``speed_rmse`` = sqrt(mean (V_SR - V_HR)^2), in m/s;
        ``direction_error_deg`` = the mean angle between HR and SR weighted by the true speed, sum V_HR angle / sum V_HR,
        in degrees;  ``power_density_*`` = 0.5 rho mean(V^3) UVW_MAX^3 (W/m^2), ``power_density_rel_error`` =
        (SR - HR) / HR;  ``capacity_factor_*`` = mean P, ``capacity_factor_error`` = SR - HR, ``power_mae`` =
        mean |P_SR - P_HR|;  ``shear_exponent_*`` = ln(Vbar_q / Vbar_q') / ln(q / q') against the next lower listed
        height q', nan for the first;  every error with its ``_trilinear`` twin (nan for a table without baseline)"""
    c = torch.as_tensor(table, dtype=torch.float64)
    nh = tables.heights.numel()
    if c.dim() != 2 or tuple(c.shape) != (nh, NS):
        raise ValueError(f"hub_height_from_sums wants a (NH, {NS}) = ({nh}, {NS}) table, not {tuple(c.shape)}")
    rho, uvw, ncols = float(air_density), tables.UVW_MAX, float(ncols)
    out = {k: [] for k in COLUMNS}
    nan = math.nan
    prev = None  # (height, the three mean speeds) of the next lower height
    for k, row in enumerate(c.tolist()):
        n = row[0]
        r = dict(zip(SUMS, row))
        # zeros in the baseline's sums beside a moving truth are a table without one
        absent = r["V_TL"] == 0 and r["absdV_TL"] == 0 and r["V_HR"] > 0
        q = float(tables.heights_m[k])
        out["height_m"].append(q)
        out["valid_fraction"].append(_ratio(n, ncols))
        mean_v = {}
        for tag, s in (("HR", "HR"), ("SR", "SR"), ("trilinear", "TL")):
            gone = nan if (s == "TL" and absent) else 1.0
            mean_v[tag] = _ratio(r["V_" + s], n) * gone
            out["speed_" + tag].append(mean_v[tag] * uvw)
            out["power_density_" + tag].append(0.5 * rho * _ratio(r["V3_" + s], n) * uvw ** 3 * gone)
            out["capacity_factor_" + tag].append(_ratio(r["P_" + s], n) * gone)
            if prev is None or not (mean_v[tag] > 0 and prev[1][tag] > 0):
                out["shear_exponent_" + tag].append(nan)
            else:
                out["shear_exponent_" + tag].append(math.log(mean_v[tag] / prev[1][tag]) / math.log(q / prev[0]))
        for twin, s, tag in (("", "SR", "SR"), ("_trilinear", "TL", "trilinear")):
            gone = nan if (s == "TL" and absent) else 1.0
            out["speed_bias" + twin].append(out["speed_" + tag][-1] - out["speed_HR"][-1])
            out["speed_mae" + twin].append(_ratio(r["absdV_" + s], n) * uvw * gone)
            out["speed_rmse" + twin].append(math.sqrt(max(_ratio(r["sqdV_" + s], n), 0.0)) * uvw * gone if n else nan)
            out["direction_error_deg" + twin].append(math.degrees(_ratio(r["angle_" + s], r["V_HR"])) * gone if n else nan)
            out["power_density_rel_error" + twin].append(
                _ratio(out["power_density_" + tag][-1] - out["power_density_HR"][-1], out["power_density_HR"][-1]))
            out["capacity_factor_error" + twin].append(out["capacity_factor_" + tag][-1] - out["capacity_factor_HR"][-1])
            out["power_mae" + twin].append(_ratio(r["absdP_" + s], n) * gone)
        prev = (q, mean_v)
    return out
