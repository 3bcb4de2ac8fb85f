"""Fractions skill score (``[FSS]``): are the strong-wind areas of the super-resolved field where the truth has them, and
from which spatial scale on?  The neighbourhood verification of Roberts & Lean (2008, Mon. Wea. Rev. 136): per exceedance
threshold of the horizontal wind speed and per neighbourhood size the fraction of events in a box around every position
is compared between the truth (HR) and the super-resolved field (SR), and between HR and the trilinear baseline (TL).  A
point-wise score charges a sharp field with a slightly misplaced gust front twice (a miss and a false alarm); the FSS
does not once the neighbourhood is wider than the displacement.  The contingency-table scores (CSI, POD, FAR, ETS,
frequency bias) fall out of the same sums at neighbourhood 1.

Everything is built from five exact integers per sample, z level, threshold and neighbourhood: on a GPU
``hip_ops.level_fss`` takes them in one fused launch on the native layout (csrc/fss.hip), ``level_fss_reference``
composes the same integers from torch ops on any device (the path of a CPU device and of the host loop, and the oracle of
the tests).  ``fss_from_sums`` turns a table of sums into the columns of the files, defined once for every caller.

This module is the single place where the score is defined.  Operands are HR, SR and TL, each (B, C >= 2, X, Y, NZ); only
channels 0 (u) and 1 (v) are read, as normalised values; ``UVW_MAX`` enters through the table alone.  z is never
windowed: the levels are terrain-following and unevenly spaced.  With fl() the rounding to fp32:

    tables      ``fss_tables``: thr2[t] = fl((thresholds[t] / UVW_MAX)^2), computed in Python doubles and rounded once;
                finite, positive and strictly ascending after the rounding
    event       hs2 = fl(fl(u u) + fl(v v)), nothing contracted, no sqrt (the hs2 of ``distribution.py``);
                I_t = hs2 >= thr2[t]: a NaN is no event, a tie is an event, +Inf is an event
    count       n an odd neighbourhood, r = (n - 1) / 2: c_f,t,n(x, y) = the number of events of source f in the n x n box
                centred on (x, y) of the level's plane; cells outside the plane count 0 (the zero padding of Roberts &
                Lean and of pysteps).  An integer 0 .. n^2
    sums        over ALL X * Y positions of the plane, index 0 .. 4:
                hr2 = sum c_HR^2,  sr2 = sum c_SR^2,  srd = sum (c_SR - c_HR)^2,  tl2 = sum c_TL^2,
                tld = sum (c_TL - c_HR)^2

The sums form a float64 (B, NZ, NT, NN, 5) table of exact integers (each far below 2^53); without TL entries 3 and 4 are
zeros.  The n^4 of the fractions' normalisation cancels in every score, so the counts are never divided.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

MAX_THRESHOLDS = 8  # WSR_FSS_MAX_THRESHOLDS
MAX_SCALES = 8      # WSR_FSS_MAX_SCALES
MAX_SCALE = 33      # WSR_FSS_MAX_SCALE
DEFAULT_SCALES = (1, 3, 5, 9, 17, 33)

SUMS = ("hr2", "sr2", "srd", "tl2", "tld")
#: the columns of ``<name>____fss.csv`` after ``threshold,scale``
FSS_COLUMNS = ("scale_m", "FSS", "FSS_trilinear", "FSS_uniform")
#: the columns of ``<name>____exceedance.csv`` after ``threshold``
EXCEEDANCE_COLUMNS = ("f_HR", "f_SR", "f_trilinear", "bias", "bias_trilinear", "CSI", "CSI_trilinear", "POD",
                      "POD_trilinear", "FAR", "FAR_trilinear", "ETS", "ETS_trilinear", "useful_scale_m",
                      "useful_scale_m_trilinear")


class FssTables(NamedTuple):
    """What ``fss_tables`` returns: ``thr2`` an fp32 host tensor (NT,), and the parameters it was made from"""

    thr2: torch.Tensor
    thresholds: tuple
    UVW_MAX: float


def check_thresholds(thresholds, what="fss") -> list:
    """The range of ``thresholds``: 1 .. 8 finite numbers > 0 in m/s, strictly ascending, else a ValueError naming
    ``thresholds`` -> a list of floats"""
    try:
        th = [float(v) for v in thresholds]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: thresholds must be a list of numbers, not {thresholds!r}") from None
    if not 1 <= len(th) <= MAX_THRESHOLDS:
        raise ValueError(f"{what}: thresholds must hold 1 .. {MAX_THRESHOLDS} entries, not {len(th)}")
    if not all(v > 0 and math.isfinite(v) for v in th):
        raise ValueError(f"{what}: thresholds must be finite numbers > 0 (m/s), not {th}")
    if any(b <= a for a, b in zip(th, th[1:])):
        raise ValueError(f"{what}: thresholds must be strictly ascending, not {th}")
    return th


def check_scales(scales, what="fss") -> list:
    """The range of ``scales``: 1 .. 8 odd integers, strictly ascending, the first one 1, the last one <= 33, else a
    ValueError naming ``scales`` -> a list of ints"""
    try:
        sc = [int(v) for v in scales]
        same = all(s == v for s, v in zip(sc, scales))
    except (TypeError, ValueError):
        sc, same = [], False
    if not same:
        raise ValueError(f"{what}: scales must be a list of integers, not {scales!r}")
    if not 1 <= len(sc) <= MAX_SCALES:
        raise ValueError(f"{what}: scales must hold 1 .. {MAX_SCALES} entries, not {len(sc)}")
    if any(n < 1 or n % 2 == 0 for n in sc):
        raise ValueError(f"{what}: scales must be odd and >= 1, not {sc}")
    if any(b <= a for a, b in zip(sc, sc[1:])):
        raise ValueError(f"{what}: scales must be strictly ascending, not {sc}")
    if sc[0] != 1:
        raise ValueError(f"{what}: scales must begin with 1 (the contingency table is its row), not {sc[0]}")
    if sc[-1] > MAX_SCALE:
        raise ValueError(f"{what}: scales must not exceed {MAX_SCALE}, not {sc[-1]}")
    return sc


def fss_tables(UVW_MAX: float, thresholds) -> FssTables:
    """The squared normalised thresholds of the module docstring: Python doubles, rounded once to fp32"""
    th = check_thresholds(thresholds, "fss_tables")
    uvw = float(UVW_MAX)
    if not (uvw > 0 and math.isfinite(uvw)):
        raise ValueError(f"fss_tables: UVW_MAX must be a finite number > 0, not {UVW_MAX}")
    thr2 = torch.tensor([(v / uvw) ** 2 for v in th], dtype=torch.float64).float()
    if not (bool(torch.isfinite(thr2).all()) and float(thr2[0]) > 0 and bool((thr2[1:] > thr2[:-1]).all())):
        raise ValueError(f"fss_tables: the squares of thresholds = {th} at UVW_MAX = {UVW_MAX} are not finite, positive, "
                         f"strictly ascending fp32 numbers")
    return FssTables(thr2, tuple(th), uvw)


def _window_counts(events: torch.Tensor, radii):
    """``events`` int64 (B, X, Y, NZ) of 0 / 1 -> for every radius the (B, X, Y, NZ) int64 number of events in the
    (2 r + 1)^2 box on the plane, zero outside it: one 2-D table of integer running sums, four look-ups per radius"""
    B, X, Y, NZ = events.shape
    P = torch.zeros((B, X + 1, Y + 1, NZ), dtype=torch.int64, device=events.device)
    P[:, 1:, 1:] = events.cumsum(dim=1).cumsum(dim=2)
    ax, ay = torch.arange(X, device=events.device), torch.arange(Y, device=events.device)
    for r in radii:
        x0, x1 = (ax - r).clamp(min=0), (ax + r + 1).clamp(max=X)
        y0, y1 = (ay - r).clamp(min=0), (ay + r + 1).clamp(max=Y)
        hi, lo = P.index_select(1, x1), P.index_select(1, x0)
        yield hi.index_select(2, y1) - hi.index_select(2, y0) - lo.index_select(2, y1) + lo.index_select(2, y0)


def level_fss_reference(HR, SR, TL, tables: FssTables, scales=DEFAULT_SCALES) -> torch.Tensor:
    """The five sums per sample, level, threshold and neighbourhood, composed from torch ops on the tensors' device: the
    events from fp32 ops in the order of the module docstring, the counts and sums in int64 (exact).  HR, SR, TL
    (B, C >= 2, X, Y, NZ; channels 0 and 1) -> float64 (B, NZ, NT, NN, 5).  ``TL`` None: zeros in entries 3 and 4."""
    sc = check_scales(scales, "level_fss_reference")
    B, _, X, Y, NZ = HR.shape
    dev = HR.device
    thr2 = tables.thr2.to(dev)
    nt, nn = thr2.numel(), len(sc)
    radii = [(n - 1) // 2 for n in sc]
    hs2 = []
    for s, f in enumerate((HR, SR, TL)):
        if f is None:
            hs2.append(None)
            continue
        if f.dim() != 5 or (f.shape[0],) + tuple(f.shape[2:]) != (B, X, Y, NZ) or f.shape[1] < 2:
            raise ValueError(f"level_fss_reference: {('HR', 'SR', 'TL')[s]} {tuple(f.shape)} does not match HR "
                             f"{tuple(HR.shape)}")
        u, v = f[:, 0].float(), f[:, 1].float()
        hs2.append(u * u + v * v)
    if hs2[1] is None:
        raise ValueError("level_fss_reference: SR must be given")
    out = torch.zeros((B, NZ, nt, nn, 5), dtype=torch.int64, device=dev)
    for t in range(nt):
        c = [None if h is None else list(_window_counts((h >= thr2[t]).long(), radii)) for h in hs2]
        for k in range(nn):
            ch, cs = c[0][k], c[1][k]
            out[:, :, t, k, 0] = (ch * ch).sum(dim=(1, 2))
            out[:, :, t, k, 1] = (cs * cs).sum(dim=(1, 2))
            out[:, :, t, k, 2] = ((cs - ch) ** 2).sum(dim=(1, 2))
            if c[2] is not None:
                ct = c[2][k]
                out[:, :, t, k, 3] = (ct * ct).sum(dim=(1, 2))
                out[:, :, t, k, 4] = ((ct - ch) ** 2).sum(dim=(1, 2))
    return out.double()


def _ratio(a, b):
    return a / b if b else math.nan


def fss_from_sums(table, scales, thresholds, d: float, npos: float) -> dict:
    """Columns from a (NT, NN, 5) table of sums (a tensor or nested lists; sum over levels and fields first), in double.
    ``scales``: the neighbourhoods of the table's second axis, the first one 1; ``thresholds``: in m/s; ``d``: the grid
    spacing in metres; ``npos``: the number of positions that were summed (X * Y times levels times fields).  Returns
    Python floats and lists:

        ``fss``         one entry per (threshold, scale), thresholds outermost: ``threshold``, ``scale``, and
                        ``FSS_COLUMNS`` - ``scale_m`` = n d, ``FSS`` = 1 - srd / (hr2 + sr2) (nan where nobody has an
                        event), ``FSS_trilinear`` the same with tld and tl2, ``FSS_uniform`` = 0.5 + f_HR / 2
        ``exceedance``  one entry per threshold: ``threshold`` and ``EXCEEDANCE_COLUMNS`` - from the n = 1 row, where a
                        count is 0 or 1: hits = (hr2 + sr2 - srd) / 2, misses = hr2 - hits, false_alarms = sr2 - hits;
                        f = events / npos; bias = (hits + false_alarms) / (hits + misses); CSI = hits / (hits + misses +
                        false_alarms); POD = hits / (hits + misses); FAR = false_alarms / (hits + false_alarms); ETS =
                        (hits - chance) / (hits + misses + false_alarms - chance) with chance = (hits + misses)(hits +
                        false_alarms) / npos; a score is nan where its denominator is 0; ``useful_scale_m``: the
                        smallest listed scale whose FSS reaches FSS_uniform, in metres, nan if none does; every score
                        with its ``_trilinear`` twin (all nan for a table without baseline)"""
    c = torch.as_tensor(table, dtype=torch.float64)
    sc, th = [int(n) for n in scales], [float(v) for v in thresholds]
    if c.dim() != 3 or tuple(c.shape) != (len(th), len(sc), 5):
        raise ValueError(f"fss_from_sums wants a (NT, NN, 5) = ({len(th)}, {len(sc)}, 5) table, not {tuple(c.shape)}")
    if not sc or sc[0] != 1:
        raise ValueError(f"fss_from_sums: scales must begin with 1, not {sc}")
    c, d, npos = c.tolist(), float(d), float(npos)
    fss = {k: [] for k in ("threshold", "scale") + FSS_COLUMNS}
    exc = {k: [] for k in ("threshold",) + EXCEEDANCE_COLUMNS}
    for t, thr in enumerate(th):
        hr2, sr2, srd, tl2, tld = c[t][0]
        row = {"f_HR": _ratio(hr2, npos), "f_SR": _ratio(sr2, npos), "f_trilinear": _ratio(tl2, npos)}
        uniform = 0.5 + row["f_HR"] / 2
        for tag, i2, idiff in (("", 1, 2), ("_trilinear", 3, 4)):
            a2, ad = c[t][0][i2], c[t][0][idiff]
            # a baseline without events has tld = hr2: zeros in both entries beside events of HR are a table without one
            absent = bool(tag) and a2 == 0 and ad == 0 and hr2 > 0
            hits = (hr2 + a2 - ad) / 2
            misses, false_alarms = hr2 - hits, a2 - hits
            chance = _ratio((hits + misses) * (hits + false_alarms), npos)
            scores = {"bias": _ratio(hits + false_alarms, hits + misses),
                      "CSI": _ratio(hits, hits + misses + false_alarms),
                      "POD": _ratio(hits, hits + misses),
                      "FAR": _ratio(false_alarms, hits + false_alarms),
                      "ETS": _ratio(hits - chance, hits + misses + false_alarms - chance)}
            useful = math.nan
            for k, n in enumerate(sc):
                denom = c[t][k][0] + c[t][k][i2]
                score = 1 - c[t][k][idiff] / denom if denom and not absent else math.nan
                if not tag:
                    fss["threshold"].append(thr), fss["scale"].append(n), fss["scale_m"].append(n * d)
                    fss["FSS"].append(score), fss["FSS_uniform"].append(uniform)
                else:
                    fss["FSS_trilinear"].append(score)
                if math.isnan(useful) and score >= uniform:
                    useful = n * d
            for k, v in scores.items():
                row[k + tag] = math.nan if absent else v
            row["useful_scale_m" + tag] = useful
            if absent:
                row["f_trilinear"] = math.nan
        exc["threshold"].append(thr)
        for k in EXCEEDANCE_COLUMNS:
            exc[k].append(row[k])
    return {"fss": fss, "exceedance": exc}
