"""Wind-speed distribution and wind rose (``[DISTRIBUTION]``): the joint frequency table of the horizontal wind speed
(bins of ``bin_width`` m/s, the last one open-ended) and of the direction the wind comes from (``sectors`` sectors, sector
0 centred on the grid's +y, counted clockwise, plus a calm class), for the truth, the super-resolved field and the
trilinear baseline.  It is what a Weibull fit and a wind rose are made from, and it shows whether SR keeps HR's share of
strong wind where a blurred field loses it.

Everything is built from one count table per sample, z level and source: on a GPU ``hip_ops.level_distribution`` takes
it in one fused launch on the native layout (csrc/distribution.hip), ``level_distribution_reference`` composes the same
counts from torch ops on any device (the path of a CPU device and of the host loop, and the oracle of the tests).
``distribution_from_counts`` turns a table of counts into the columns of the files, defined once for every caller.

This module is the single place where the classes are defined.  A voxel's class is a function of fp32 operations in a
fixed order - every product and every sum rounded, nothing contracted, no sqrt and no atan2 - so host, device and the
torch reference agree on every voxel, ties included.  Only channels 0 (u, along x) and 1 (v, along y) are read, as
normalised values; ``UVW_MAX`` enters through the tables alone.  With fl() the rounding to fp32:

    tables      ``distribution_tables``: computed in Python doubles and rounded once,
                edge2[j - 1] = fl((j bin_width / UVW_MAX)^2), j = 1 .. NS - 1;   calm2 = fl((calm / UVW_MAX)^2);
                bx[k] = fl(sin beta_k), by[k] = fl(cos beta_k), beta_k = -pi / ND + 2 pi k / ND, k = 0 .. ND / 2 - 1
                (half of the sector boundaries; the other half are their negatives)
    hs2         fl(fl(u u) + fl(v v))
    speed bin   j = the number of i with hs2 >= edge2[i]: 0 .. NS - 1, a NaN gives 0
    sector      p = (-u, -v), where the wind comes from;  cross_k(q) = fl(fl(by[k] q.x) - fl(bx[k] q.y));
                second = cross_0(p) < 0 or (cross_0(p) == 0 and cross_1(p) > 0);  q = second ? -p : p;
                cnt = the number of k with cross_k(q) >= 0;  sector = max(cnt, 1) - 1 + (second ? ND / 2 : 0);
                if not hs2 > calm2: the calm class ND (a zero vector at calm = 0 and a NaN are calm).
                Always 0 .. ND, for every bit pattern.  A vector exactly on a boundary goes to the clockwise sector:
                cross_k = 0 counts, and the second clause of ``second`` is the one tie that cross_0 < 0 alone would
                send the other way, p opposite to boundary 0 (then cross_1(p) > 0; along boundary 0 it is < 0).

The counts form a float64 (B, NZ, 3, NS, ND + 1) table, source 0 HR, 1 SR, 2 TL; every (b, level, source) slice sums to
X * Y.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

SOURCES = ("HR", "SR", "trilinear")

MIN_SPEED_BINS, MAX_SPEED_BINS = 2, 64  # WSR_DISTRIBUTION_MAX_SPEED_BINS
MIN_SECTORS, MAX_SECTORS = 4, 36        # WSR_DISTRIBUTION_MAX_SECTORS

#: the columns of ``<name>____wind_distribution.csv`` after ``bin``, of ``<name>____wind_rose.csv`` after ``sector``
SPEED_COLUMNS = ("speed_lo", "speed_hi", "f_HR", "f_SR", "f_trilinear")
ROSE_COLUMNS = ("dir_lo_deg", "dir_hi_deg", "f_HR", "f_SR", "f_trilinear")
#: the summary scalars: of ``averages_distribution.csv`` after ``Name``, of the per-level file after ``level``
SUMMARY_COLUMNS = ("PSS", "PSS_trilinear", "W1", "W1_trilinear", "rose_tv", "rose_tv_trilinear",
                   "p50_HR", "p50_SR", "p50_trilinear", "p90_HR", "p90_SR", "p90_trilinear",
                   "p99_HR", "p99_SR", "p99_trilinear", "f_overflow_HR")


class DistributionTables(NamedTuple):
    """What ``distribution_tables`` returns: fp32 host tensors ``edge2`` (NS - 1,), ``bx``, ``by`` (ND / 2,), ``calm2`` a
    Python float holding an fp32 value, and the parameters they were made from"""

    edge2: torch.Tensor
    bx: torch.Tensor
    by: torch.Tensor
    calm2: float
    speed_bins: int
    sectors: int
    bin_width: float
    UVW_MAX: float
    calm: float


def check_parameters(bin_width, speed_bins, sectors, calm, what="distribution") -> None:
    """The ranges of ``[DISTRIBUTION]``, else a ValueError with the number"""
    if bin_width is None or not (float(bin_width) > 0 and math.isfinite(float(bin_width))):
        raise ValueError(f"{what}: bin_width must be a finite number > 0, not {bin_width}")
    if int(speed_bins) != speed_bins or not MIN_SPEED_BINS <= speed_bins <= MAX_SPEED_BINS:
        raise ValueError(f"{what}: speed_bins must be {MIN_SPEED_BINS} .. {MAX_SPEED_BINS}, not {speed_bins}")
    if int(sectors) != sectors or sectors % 2 or not MIN_SECTORS <= sectors <= MAX_SECTORS:
        raise ValueError(f"{what}: sectors must be even and {MIN_SECTORS} .. {MAX_SECTORS}, not {sectors}")
    if not (float(calm) >= 0 and math.isfinite(float(calm))):
        raise ValueError(f"{what}: calm must be a finite number >= 0, not {calm}")


def distribution_tables(UVW_MAX: float, bin_width: float, speed_bins: int = 32, sectors: int = 16,
                        calm: float = 0.5) -> DistributionTables:
    """The bin edges and sector boundaries of the module docstring: Python doubles, rounded once to fp32"""
    check_parameters(bin_width, speed_bins, sectors, calm, "distribution_tables")
    uvw = float(UVW_MAX)
    if not (uvw > 0 and math.isfinite(uvw)):
        raise ValueError(f"distribution_tables: UVW_MAX must be a finite number > 0, not {UVW_MAX}")
    ns, nd = int(speed_bins), int(sectors)
    edge2 = torch.tensor([(j * float(bin_width) / uvw) ** 2 for j in range(1, ns)], dtype=torch.float64).float()
    if not (bool(torch.isfinite(edge2).all()) and float(edge2[0]) > 0 and bool((edge2[1:] > edge2[:-1]).all())):
        raise ValueError(f"distribution_tables: the squared edges of bin_width = {bin_width} at UVW_MAX = {UVW_MAX} are "
                         f"not distinct positive fp32 numbers")
    beta = [-math.pi / nd + 2.0 * math.pi * k / nd for k in range(nd // 2)]
    bx = torch.tensor([math.sin(b) for b in beta], dtype=torch.float64).float()
    by = torch.tensor([math.cos(b) for b in beta], dtype=torch.float64).float()
    calm2 = float(torch.tensor((float(calm) / uvw) ** 2, dtype=torch.float64).float())
    return DistributionTables(edge2, bx, by, calm2, ns, nd, float(bin_width), uvw, float(calm))


def classify(u: torch.Tensor, v: torch.Tensor, tables: DistributionTables):
    """(speed bin, sector) of fp32 tensors ``u``, ``v`` of one shape -> two int64 tensors of that shape, the sector
    ND for the calm class: elementwise fp32 ops in the order of the module docstring, on the tensors' device"""
    dev = u.device
    edge2, bx, by = (t.to(dev) for t in (tables.edge2, tables.bx, tables.by))
    nd = tables.sectors
    hs2 = u * u + v * v
    # the number of edges <= hs2 (the edges ascend); a NaN compares false with every edge
    j = torch.bucketize(hs2, edge2, right=True)
    j = torch.where(hs2 != hs2, torch.zeros_like(j), j)
    c0, c1 = by[0] * (-u) - bx[0] * (-v), by[1] * (-u) - bx[1] * (-v)
    second = (c0 < 0) | ((c0 == 0) & (c1 > 0))
    qx, qy = torch.where(second, u, -u), torch.where(second, v, -v)
    cnt = torch.zeros_like(j)
    for k in range(nd // 2):
        cnt += (by[k] * qx - bx[k] * qy) >= 0
    sector = cnt.clamp(min=1) - 1 + second.to(cnt.dtype) * (nd // 2)
    sector = torch.where(hs2 > tables.calm2, sector, torch.full_like(sector, nd))
    return j, sector


def level_distribution_reference(HR, SR, TL, tables: DistributionTables) -> torch.Tensor:
    """The counts per sample, level and source, composed from torch fp32 ops on the tensors' device: HR, SR, TL
    (B, C >= 2, X, Y, NZ; channels 0 and 1) -> float64 (B, NZ, 3, NS, ND + 1).  ``TL`` None: zeros in its slices."""
    B, _, X, Y, NZ = HR.shape
    ns, nd1 = tables.speed_bins, tables.sectors + 1
    T = ns * nd1
    base = (torch.arange(B, device=HR.device).view(B, 1, 1, 1) * NZ + torch.arange(NZ, device=HR.device)) * T
    out = torch.zeros((B, NZ, 3, ns, nd1), dtype=torch.float64, device=HR.device)
    for s, f in enumerate((HR, SR, TL)):
        if f is None:
            continue
        if (f.shape[0],) + tuple(f.shape[2:]) != (B, X, Y, NZ) or f.shape[1] < 2:
            raise ValueError(f"level_distribution_reference: {SOURCES[s]} {tuple(f.shape)} does not match HR "
                             f"{tuple(HR.shape)}")
        j, sector = classify(f[:, 0].float(), f[:, 1].float(), tables)
        idx = (base + (j * nd1 + sector)).reshape(-1)
        out[:, :, s] = torch.bincount(idx, minlength=B * NZ * T).view(B, NZ, ns, nd1).double()
    return out


def _quantile(f, F, p, bw):
    """the p-quantile of the speed from the bin frequencies ``f`` and their running sums ``F``: linear inside the bin,
    the lower edge of the open bin when it falls there"""
    last = len(f) - 1
    for j in range(last):
        if F[j] >= p and f[j] > 0:
            return bw * (j + (p - (F[j] - f[j])) / f[j])
    return bw * last


def distribution_from_counts(counts, bin_width: float) -> dict:
    """Columns and summary scalars from a (3, NS, ND + 1) table of counts (a tensor or nested lists; sum over levels and
    fields first), in double.  Returns Python floats and lists:

        ``speed``    per speed bin: ``SPEED_COLUMNS`` (``speed_hi`` of the last bin is inf)
        ``rose``     per sector and, last, the calm class: ``ROSE_COLUMNS`` (degrees clockwise from +y, 0 .. 360; nan
                     for the calm class)
        ``summary``  ``SUMMARY_COLUMNS``: for SR and the baseline against HR the Perkins score ``PSS`` = sum_jk
                     min(c_a, c_HR) / n on the joint table, ``W1`` = bin_width sum_{j < NS - 1} |F_a(j) - F_HR(j)| on the
                     speed marginals in m/s, ``rose_tv`` = 1/2 sum_k |r_a - r_HR| on the direction marginals with the
                     calm class; ``p50``, ``p90``, ``p99`` of the three speed marginals; ``f_overflow_HR`` the share of
                     HR in the open bin (where W1 and the quantiles are truncated)

    A source without voxels (the baseline of a launch without one) has frequencies 0 and scores nan."""
    c = torch.as_tensor(counts, dtype=torch.float64)
    if c.dim() != 3 or c.shape[0] != 3 or c.shape[1] < 2 or c.shape[2] < 3:
        raise ValueError(f"distribution_from_counts wants a (3, NS, ND + 1) table, not {tuple(c.shape)}")
    bw, ns, nd = float(bin_width), c.shape[1], c.shape[2] - 1
    n = [float(c[s].sum()) for s in range(3)]
    f = [(c[s].sum(dim=1) / n[s]).tolist() if n[s] else [0.0] * ns for s in range(3)]
    r = [(c[s].sum(dim=0) / n[s]).tolist() if n[s] else [0.0] * (nd + 1) for s in range(3)]
    F = [torch.tensor(f[s], dtype=torch.float64).cumsum(0).tolist() for s in range(3)]
    width = 360.0 / nd
    out = {
        "speed": {"speed_lo": [bw * j for j in range(ns)], "speed_hi": [bw * (j + 1) for j in range(ns - 1)] + [math.inf],
                  "f_HR": f[0], "f_SR": f[1], "f_trilinear": f[2]},
        "rose": {"dir_lo_deg": [((k - 0.5) * width) % 360.0 for k in range(nd)] + [math.nan],
                 "dir_hi_deg": [(k + 0.5) * width for k in range(nd)] + [math.nan],
                 "f_HR": r[0], "f_SR": r[1], "f_trilinear": r[2]},
    }
    summary = {}
    for s, tag in ((1, ""), (2, "_trilinear")):
        ok = n[s] > 0 and n[0] > 0
        summary["PSS" + tag] = float(torch.minimum(c[s], c[0]).sum()) / n[0] if ok else math.nan
        summary["W1" + tag] = bw * math.fsum(abs(a - b) for a, b in zip(F[s][:-1], F[0][:-1])) if ok else math.nan
        summary["rose_tv" + tag] = 0.5 * math.fsum(abs(a - b) for a, b in zip(r[s], r[0])) if ok else math.nan
    for p, name in ((0.5, "p50"), (0.9, "p90"), (0.99, "p99")):
        for s, tag in enumerate(("_HR", "_SR", "_trilinear")):
            summary[name + tag] = _quantile(f[s], F[s], p, bw) if n[s] else math.nan
    summary["f_overflow_HR"] = f[0][-1]
    out["summary"] = {k: summary[k] for k in SUMMARY_COLUMNS}
    return out
