"""Structure functions (``[INCREMENTS]``): two-point statistics of the wind in physical space, up to fourth order.  The
second-order structure function S2(r) = <(f(p + r) - f(p))^2> is twice the semivariogram with which Stengel et al. (2020)
validate a GAN super-resolver; the flatness S4 / S2^2 of the velocity increments measures intermittency - whether the
strong gradients have the truth's heavy tails - and the skewness S3 / S2^1.5 of the longitudinal increments the direction
of the energy transfer.  A blurred field has too small an S2 at one or two cells; a field with invented ripple can have
the right S2 (and the right spectrum, which is second order too) and the wrong flatness.  No detrending, no taper and no
periodicity are needed: the sums hold on non-square domains and up to the domain edge.

Everything is built from sums of powers of increments per sample, z level, source, separation, direction, kind and order:
on a GPU ``hip_ops.level_increments`` takes them in one fused launch on the native layout (csrc/increments.hip),
``level_increments_reference`` composes them from torch slices on any device (the path of a CPU device and of the host
loop, and the oracle of the tests).  ``increments_from_sums`` turns a table of sums into the columns of the files,
defined once for every caller.

This module is the single place where the statistics are defined.

    operands      HR, SR and the trilinear baseline TL, each (B, C >= 3, X, Y, NZ), normalised components; channels 0, 1,
                  2 (u, v, w) are read, surplus channels never.  ``TL`` None: zeros in its slices
    separations   1 .. 8 integers in HR grid cells, strictly ascending, each 1 .. 32 (``check_separations``)
    pairs         per level plane, direction a in (x, y) and separation r: every pair (p, p + r e_a) with both ends
                  inside the plane.  No padding: pairs_x(r) = max(X - r, 0) * Y, pairs_y(r) = X * max(Y - r, 0)
                  (``pair_counts``; analytic, so not stored).  z is never paired: the levels are terrain-following and
                  unevenly spaced
    kinds         L, T, W: L the component along a (u for x, v for y), T the horizontal component across a (v for x, u
                  for y), W = w
    increment     delta = f(p + r e_a) - f(p): ONE fp32 subtraction
    orders        2, 3, 4: q = delta * delta, c = q * delta, f = q * q; every product rounded to fp32, nothing contracted
    sums          float64 (B, NZ, 3, R, 2, 3, 3): (sample, level, source HR / SR / TL, separation, direction, kind,
                  order).  An entry without pairs is exactly 0.  A NaN or Inf operand makes the entries whose pairs
                  contain it non-finite and changes no other entry
"""
from __future__ import annotations

import math

import torch

MAX_SEPARATIONS = 8   # WSR_INCREMENTS_MAX_SEPARATIONS
MAX_SEPARATION = 32   # WSR_INCREMENTS_MAX_SEPARATION
DEFAULT_SEPARATIONS = (1, 2, 4, 8, 16)
SOURCES = ("HR", "SR", "trilinear")
DIRECTIONS = ("x", "y")
KINDS = ("L", "T", "W")
ORDERS = (2, 3, 4)
#: the channel a (direction, kind) reads: x: L = u, T = v; y: L = v, T = u; W = w
COMPONENT = ((0, 1, 2), (1, 0, 2))

_PER_SOURCE = ("S2L", "S2T", "S2W", "skewness_L", "flatness_L", "flatness_T", "flatness_W", "anisotropy")
#: the columns of ``<name>____structure_functions.csv``, one row per separation
INCREMENT_COLUMNS = (("r", "r_m", "pairs") + tuple(f"{c}_{s}" for s in SOURCES for c in _PER_SOURCE) +
                     tuple(f"S2{k}_ratio{twin}" for k in KINDS for twin in ("", "_trilinear")))


def check_separations(separations, who="increments") -> list:
    """The range of ``separations``: 1 .. 8 integers, strictly ascending, each 1 .. 32, else a ValueError naming
    ``separations`` -> a list of ints.  The one place that refuses a bad list."""
    try:
        sp = [int(v) for v in separations]
        same = all(s == v and not isinstance(v, bool) for s, v in zip(sp, separations))
    except (TypeError, ValueError):
        sp, same = [], False
    if not same:
        raise ValueError(f"{who}: separations must be a list of integers, not {separations!r}")
    if not 1 <= len(sp) <= MAX_SEPARATIONS:
        raise ValueError(f"{who}: separations must hold 1 .. {MAX_SEPARATIONS} entries, not {len(sp)}")
    if any(r < 1 or r > MAX_SEPARATION for r in sp):
        raise ValueError(f"{who}: separations must lie in 1 .. {MAX_SEPARATION} grid cells, not {sp}")
    if any(b <= a for a, b in zip(sp, sp[1:])):
        raise ValueError(f"{who}: separations must be strictly ascending, not {sp}")
    return sp


def pair_counts(X: int, Y: int, separations) -> list:
    """[(pairs_x(r), pairs_y(r)) for r in separations] of one X x Y plane"""
    return [(max(int(X) - r, 0) * int(Y), int(X) * max(int(Y) - r, 0)) for r in check_separations(separations, "pair_counts")]


def level_increments_reference(HR, SR, TL, separations, dtype=torch.float64) -> torch.Tensor:
    """The sums of the module docstring composed from torch slices (``f[:, :, r:] - f[:, :, :-r]``) on the tensors'
    device: the operands converted to ``dtype``, differences and powers in ``dtype``, the sums in float64.  With the
    default float64 this is the exact-arithmetic value of the definition up to 2^-53 per operation; with
    ``torch.float32`` every term is rounded as the definition rounds it.  HR, SR, TL (B, C >= 3, X, Y, NZ; channels 0, 1
    and 2) -> float64 (B, NZ, 3, R, 2, 3, 3).  ``TL`` None: zeros in its slices."""
    sp = check_separations(separations, "level_increments_reference")
    if HR.dim() != 5 or HR.shape[1] < 3:
        raise ValueError(f"level_increments_reference wants HR as (B, C >= 3, X, Y, NZ), got {tuple(HR.shape)}")
    if SR is None:
        raise ValueError("level_increments_reference: SR must be given")
    B, _, X, Y, NZ = HR.shape
    out = torch.zeros((B, NZ, 3, len(sp), 2, 3, 3), dtype=torch.float64, device=HR.device)
    for s, f in enumerate((HR, SR, TL)):
        if f is None:
            continue
        if f.dim() != 5 or (f.shape[0],) + tuple(f.shape[2:]) != (B, X, Y, NZ) or f.shape[1] < 3:
            raise ValueError(f"level_increments_reference: {SOURCES[s]} {tuple(f.shape)} does not match HR "
                             f"{tuple(HR.shape)}")
        comp = [f[:, c].to(dtype) for c in range(3)]  # (B, X, Y, NZ)
        for k, r in enumerate(sp):
            for a in range(2):
                if r >= (X, Y)[a]:
                    continue  # no pairs: exact zeros
                for kind in range(3):
                    c = comp[COMPONENT[a][kind]]
                    delta = c[:, r:] - c[:, :-r] if a == 0 else c[:, :, r:] - c[:, :, :-r]
                    q = delta * delta
                    for o, term in enumerate((q, q * delta, q * q)):
                        out[:, :, s, k, a, kind, o] = term.sum(dim=(1, 2), dtype=torch.float64)
    return out


def _ratio(a, b):
    return a / b if b and not math.isnan(b) else math.nan


def increments_from_sums(sums, separations, nfields: float, X: int, Y: int, UVW_MAX: float, d: float) -> dict:
    """Columns from a (3, R, 2, 3, 3) table of sums (a tensor or nested lists; sum over fields - and over levels for a
    pooled table - first), in double.  ``separations``: those of the table's second axis; ``nfields``: the number of
    planes that were summed (fields, times levels for a pooled table); ``X``, ``Y``: the plane; ``UVW_MAX``: the
    normalisation of the components in m/s; ``d``: the grid spacing in metres (``spectra.grid_spacing``).  Returns one
    list per name of ``INCREMENT_COLUMNS``, one entry per separation:

        ``r``, ``r_m`` = r d, ``pairs`` = nfields (pairs_x(r) + pairs_y(r))
        per source s in (HR, SR, trilinear), pooled over both directions (sums added, pair counts added):
            ``S2L_s``, ``S2T_s``, ``S2W_s`` in m^2/s^2: UVW_MAX^2 sum / pairs (the semivariogram is half of it)
            ``skewness_L_s`` = S3L / S2L^1.5;  ``flatness_L_s``, ``flatness_T_s``, ``flatness_W_s`` = S4 / S2^2
            (UVW_MAX cancels);  ``anisotropy_s`` = S2L along x / S2L along y, each over its own pair count
        ``S2L_ratio``, ``S2T_ratio``, ``S2W_ratio``: SR over HR, each with its ``_trilinear`` twin

    A column is nan where its denominator is 0 or its pair count is 0."""
    sp = check_separations(separations, "increments_from_sums")
    t = torch.as_tensor(sums, dtype=torch.float64)
    if tuple(t.shape) != (3, len(sp), 2, 3, 3):
        raise ValueError(f"increments_from_sums wants a (3, R, 2, 3, 3) = (3, {len(sp)}, 2, 3, 3) table, not "
                         f"{tuple(t.shape)}")
    t, nf, U, d = t.tolist(), float(nfields), float(UVW_MAX), float(d)
    col = {c: [] for c in INCREMENT_COLUMNS}
    for k, (r, (px, py)) in enumerate(zip(sp, pair_counts(X, Y, sp))):
        nx, ny = nf * px, nf * py
        n = nx + ny
        col["r"].append(r), col["r_m"].append(r * d), col["pairs"].append(n)
        s2 = {}
        for s, src in enumerate(SOURCES):
            e = t[s][k]  # [direction][kind][order]
            for kind, kn in enumerate(KINDS):
                m2 = _ratio(e[0][kind][0] + e[1][kind][0], n)
                m4 = _ratio(e[0][kind][2] + e[1][kind][2], n)
                s2[src, kn] = m2
                col[f"S2{kn}_{src}"].append(U * U * m2)
                col[f"flatness_{kn}_{src}"].append(_ratio(m4, m2 * m2))
            m2, m3 = s2[src, "L"], _ratio(e[0][0][1] + e[1][0][1], n)
            col[f"skewness_L_{src}"].append(_ratio(m3, m2 ** 1.5) if m2 == m2 and m2 >= 0 else math.nan)
            col[f"anisotropy_{src}"].append(_ratio(_ratio(e[0][0][0], nx), _ratio(e[1][0][0], ny)))
        for kn in KINDS:
            col[f"S2{kn}_ratio"].append(_ratio(s2["SR", kn], s2["HR", kn]))
            col[f"S2{kn}_ratio_trilinear"].append(_ratio(s2["trilinear", kn], s2["HR", kn]))
    return col
