"""The wind-speed distribution loss of generator training (``[DISTRIBUTION_LOSS]``): "have the truth's share of strong
wind".  Every other content term of the generator is a point-wise distance (pix, the gradients, the divergences), fixes the
energy per wavenumber (``[SPECTRAL_LOSS]``) or the local structure (``[SSIM_LOSS]``); none of them acts on the marginal
distribution of the horizontal speed, and a field can satisfy all of them with clipped tails.  This is the ``W1`` that
``[DISTRIBUTION]`` reports at evaluation, made trainable: hard class counts are piecewise constant, so the histogram here
is a soft (linearly binned) one, and the trained ``W1`` is NOT the bit pattern of the ``W1`` ``[DISTRIBUTION]`` logs from
its hard bins.

This module is the single place where the term is defined.  Only channels 0 (u) and 1 (v) are read, as normalised
values; ``UVW_MAX`` enters through ``c`` alone.  With ``NS = speed_bins``, ``c = fl(UVW_MAX / bin_width)`` (a Python
double rounded once to fp32) and fp32 throughout with nothing contracted, per voxel:

    hs2 = fl(fl(u u) + fl(v v))
    r   = sqrt(hs2)                        correctly rounded
    t   = fl(fl(r c) - 0.5)                the position in units of bins, measured from the centre of bin 0
    t   = min(max(t, 0), NS - 1)
    k0  = min(floor(t), NS - 2);   f = t - k0   in [0, 1]

The voxel gives the weight ``1 - f`` to bin ``k0`` and ``f`` to bin ``k0 + 1``.  The centres are ``(k + 1/2) bin_width``;
everything below the first centre goes to bin 0, everything above the last centre to bin ``NS - 1``, the open bin.
Between the two, linear binning preserves the voxel's speed: sum_k weight_k centre_k = r UVW_MAX.  A voxel whose ``hs2`` is
not finite enters no bin; it is counted in a column of its own:

    H(X) -> (B, NZ, NS + 1) float64 per source; column NS holds the number of such voxels; every (b, z) row sums to X Y.

The device form is fixed point (csrc/distribution_loss.hip): ``fi = rint(f 65536)``, bin ``k0`` gets the integer
``65536 - fi`` and bin ``k0 + 1`` gets ``fi``, column ``NS`` counts in units of 65536 too, so every row sums to exactly
``X Y 65536`` and ``H = (double)count / 65536``.  Integer adds commute: the same bits on every call.

    its vector-Jacobian product, towards SR only: given G = dL/dH_sr[b, z, :NS], for a voxel with 0 < t < NS - 1 strictly
    (t before the clamp) and r > 0
        dL/du = (G[k0 + 1] - G[k0]) c u / r,   dL/dv likewise;
    0 for clamped, calm (r = 0) and non-finite voxels and for every other channel.

    the loss, composed in torch from the two small tables (``loss_from_counts``; its form stays editable here, its
    derivative autograd's): with ``pool = level`` every (b, z) row is a distribution, with ``pool = sample`` the rows of a
    sample are summed over z first;
        p = H[..., :NS] / H[..., :NS].sum(-1)
        W1 = bin_width sum_{k < NS - 1} |cumsum(p_sr)[k] - cumsum(p_hr)[k]|
        L_dist = the mean of W1 over the rows, in m/s.
    NaN when any entry of column NS of either table is > 0 (``torch.where`` on the device, no host read): a non-finite SR
    skips the Adam step exactly like a non-finite ``pix``.  Exactly 0, with an exactly zero gradient, for SR = HR.

``L_dist`` is a plain mean over samples: under data parallelism equal shards average exactly as ``pix`` does, and no
collective is added.

On a GPU the tables are ``hip_ops.speed_soft_counts`` (one counting launch for both sources, one backward launch that
recomputes ``t``); on a CPU device (in float64), and under ``WSR_FUSED_DISTRIBUTION_LOSS=0`` (in fp32 on the device),
``soft_counts_reference`` composes the unquantised tables from torch ops and autograd differentiates them.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import torch

from .config.config import DistributionLossConfig
from .distribution import MAX_SPEED_BINS, MIN_SPEED_BINS

#: the keys of ``[DISTRIBUTION_LOSS]`` and their defaults, as ``DistributionLossConfig`` declares them
DISTRIBUTION_LOSS = {k: getattr(DistributionLossConfig, k) for k, _ in DistributionLossConfig._schema}
POOLS = ("level", "sample")
ONE = 65536  # the fixed-point unit of the device tables


class SoftTables(NamedTuple):
    """What ``soft_tables`` returns: ``c`` a Python float holding the fp32 value fl(UVW_MAX / bin_width), and the
    parameters it was made from"""

    c: float
    speed_bins: int
    bin_width: float
    UVW_MAX: float


def check_parameters(bin_width, speed_bins, what="distribution_loss") -> None:
    """The ranges of ``[DISTRIBUTION_LOSS]``, else a ValueError with the number"""
    if bin_width is None or not (float(bin_width) > 0 and math.isfinite(float(bin_width))):
        raise ValueError(f"{what}: bin_width must be a finite number > 0, not {bin_width}")
    if int(speed_bins) != speed_bins or not MIN_SPEED_BINS <= speed_bins <= MAX_SPEED_BINS:
        raise ValueError(f"{what}: speed_bins must be {MIN_SPEED_BINS} .. {MAX_SPEED_BINS}, not {speed_bins}")


def soft_tables(UVW_MAX: float, bin_width: float, speed_bins: int = 32) -> SoftTables:
    """``c`` of the module docstring: a Python double, rounded once to fp32"""
    check_parameters(bin_width, speed_bins, "soft_tables")
    uvw = float(UVW_MAX)
    if not (uvw > 0 and math.isfinite(uvw)):
        raise ValueError(f"soft_tables: UVW_MAX must be a finite number > 0, not {UVW_MAX}")
    c = float(torch.tensor(uvw / float(bin_width), dtype=torch.float64).float())
    if not (c > 0 and math.isfinite(c)):
        raise ValueError(f"soft_tables: UVW_MAX / bin_width = {UVW_MAX} / {bin_width} is not a positive fp32 number")
    return SoftTables(c, int(speed_bins), float(bin_width), uvw)


def fused() -> bool:
    """the run-time switch ``WSR_FUSED_DISTRIBUTION_LOSS`` (0: the composed torch path on every device)"""
    return os.environ.get("WSR_FUSED_DISTRIBUTION_LOSS", "1") != "0"


def _check_pair(HR, SR, what):
    for name, t in (("HR", HR), ("SR", SR)):
        if t.dim() != 5 or t.shape[1] < 2 or t.numel() == 0 or not t.is_floating_point():
            raise ValueError(f"{what} wants {name} as a floating-point (B, C >= 2, X, Y, NZ) tensor, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if (SR.shape[0],) + tuple(SR.shape[2:]) != (HR.shape[0],) + tuple(HR.shape[2:]):
        raise ValueError(f"{what}: SR {tuple(SR.shape)} does not match HR {tuple(HR.shape)}")


def soft_positions(u: torch.Tensor, v: torch.Tensor, tables: SoftTables):
    """(t before the clamp, k0, f, finite) of tensors ``u``, ``v`` of one shape and dtype: elementwise ops in that dtype,
    in the order of the module docstring.  A voxel that is not ``finite`` is given u = v = 0 first, and a calm one a unit
    radicand whose root is discarded, so neither carries a NaN or an infinite derivative into the graph."""
    ns = tables.speed_bins
    hs2 = u * u + v * v
    finite = torch.isfinite(hs2)
    zero = torch.zeros_like(u)
    u, v = torch.where(finite, u, zero), torch.where(finite, v, zero)
    hs2 = u * u + v * v
    moving = hs2 > 0
    r = torch.where(moving, torch.sqrt(torch.where(moving, hs2, torch.ones_like(hs2))), zero)
    t = r * tables.c - 0.5
    tc = t.clamp(0.0, float(ns - 1))
    k0 = tc.detach().floor().clamp(max=ns - 2)
    return t, k0.long(), tc - k0, finite


def soft_counts_reference(HR, SR, tables: SoftTables, dtype=torch.float64) -> torch.Tensor:
    """``H`` of both sources -> float64 (2, B, NZ, NS + 1), source 0 HR (detached), 1 SR: the per-voxel weights ``1 - f``
    and ``f`` in ``dtype`` on the tensors' device, unquantised, added into a float64 table by ``index_add``;
    differentiable by autograd.  The path of a CPU device and of ``WSR_FUSED_DISTRIBUTION_LOSS=0``, and the oracle of the
    tests."""
    _check_pair(HR, SR, "soft_counts_reference")
    B, _, X, Y, NZ = HR.shape
    ns = tables.speed_bins
    T = ns + 1
    dev = HR.device
    base = ((torch.arange(B, device=dev).view(B, 1, 1, 1) * NZ + torch.arange(NZ, device=dev)) * T).expand(B, X, Y, NZ)
    tabs = []
    for f in (HR.detach(), SR):
        _, k0, frac, finite = soft_positions(f[:, 0].to(dtype), f[:, 1].to(dtype), tables)
        lo = torch.where(finite, base + k0, base + ns).reshape(-1)
        hi = torch.where(finite, base + k0 + 1, base + ns).reshape(-1)
        w_hi = torch.where(finite, frac, torch.zeros_like(frac))  # (a non-finite voxel: one whole count in column NS)
        w_lo = 1.0 - w_hi
        H = torch.zeros(B * NZ * T, dtype=torch.float64, device=dev)
        H = H.index_add(0, lo, w_lo.reshape(-1).double()).index_add(0, hi, w_hi.reshape(-1).double())
        tabs.append(H.view(B, NZ, T))
    return torch.stack(tabs)


def soft_counts_vjp(SR, G, tables: SoftTables, dtype=torch.float64) -> torch.Tensor:
    """The closed form of the module docstring: ``SR`` (B, C, X, Y, NZ), ``G`` = dL/dH_sr[..., :NS] (B, NZ, NS) ->
    dL/dSR in ``dtype``, zero in every channel but 0 and 1"""
    ns = tables.speed_bins
    u, v = SR[:, 0].to(dtype), SR[:, 1].to(dtype)
    t, k0, _, finite = soft_positions(u, v, tables)
    r = torch.sqrt(u * u + v * v)
    live = finite & (t > 0) & (t < ns - 1) & (r > 0)
    Gx = G.to(dtype).unsqueeze(1).unsqueeze(1).expand(-1, SR.shape[2], SR.shape[3], -1, -1)  # (B, X, Y, NZ, NS)
    d = (Gx.gather(4, (k0 + 1).unsqueeze(-1)) - Gx.gather(4, k0.unsqueeze(-1))).squeeze(-1)
    safe = torch.where(live, r, torch.ones_like(r))
    out = torch.zeros(SR.shape, dtype=dtype, device=SR.device)
    out[:, 0] = torch.where(live, d * tables.c * u / safe, torch.zeros_like(u))
    out[:, 1] = torch.where(live, d * tables.c * v / safe, torch.zeros_like(v))
    return out


def soft_counts(HR, SR, tables: SoftTables) -> torch.Tensor:
    """``H`` of both sources, float64 (2, B, NZ, NS + 1): the kernel pair on a GPU; the reference under
    ``WSR_FUSED_DISTRIBUTION_LOSS=0`` (its weights in fp32 on the device, the precision of the kernels) and on a CPU
    device (in float64)"""
    if HR.is_cuda and fused():
        from . import hip_ops
        return hip_ops.speed_soft_counts(HR, SR, tables)
    return soft_counts_reference(HR, SR, tables, dtype=torch.float32 if HR.is_cuda else torch.float64)


def loss_from_counts(H_hr: torch.Tensor, H_sr: torch.Tensor, bin_width: float, pool: str = "level") -> torch.Tensor:
    """``L_dist`` of the module docstring from the two (B, NZ, NS + 1) tables -> a scalar in their dtype"""
    if pool not in POOLS:
        raise ValueError(f"loss_from_counts: pool must be level or sample, not {pool!r}")
    ns = H_hr.shape[-1] - 1
    bad = (H_hr[..., ns] > 0).any() | (H_sr[..., ns] > 0).any()
    cdf = []
    for H in (H_hr, H_sr):
        h = H[..., :ns]
        if pool == "sample":
            h = h.sum(dim=1)
        cdf.append((h / h.sum(dim=-1, keepdim=True)).cumsum(dim=-1)[..., :ns - 1])
    w1 = float(bin_width) * (cdf[1] - cdf[0]).abs().sum(dim=-1)
    L = w1.mean()
    return torch.where(bad, torch.full_like(L, math.nan), L)


def distribution_loss(HR, SR, cfg_section, tables: SoftTables) -> torch.Tensor:
    """``L_dist`` (un-weighted, a float32 scalar, m/s) of a batch ``HR``, ``SR`` (B, C >= 2, X, Y, NZ) under the keys of
    ``cfg_section`` (``pool``: a ``DistributionLossConfig`` or anything with that attribute) and ``tables`` =
    ``soft_tables(UVW_MAX, bin_width, speed_bins)``"""
    H = soft_counts(HR, SR, tables)
    return loss_from_counts(H[0], H[1], tables.bin_width, str(cfg_section.pool)).float()
