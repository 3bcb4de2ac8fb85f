"""The coarse-grained consistency loss of generator training (``[CONSISTENCY_LOSS]``): "coarse-grained again, the
downscaled field is the coarse field".  Every other content term of the generator is a voxel-wise distance at HR
resolution (pix, the gradients, the divergences), fixes the energy per wavenumber (``[SPECTRAL_LOSS]``, blind to phase
and to the plane mean), the local structure inside a window (``[SSIM_LOSS]``) or the marginal speed distribution
(``[DISTRIBUTION_LOSS]``); a generator can satisfy all of them and still drift in its cell averages.  This term acts only
on what the low-resolution model resolves and leaves the sub-grid scales to the detail-restoring terms: the
downscaling-consistency constraint, with the operator the project already owns - the anti-aliased coarse-graining ``D``
of ``[DEGRADATION]`` (degradation.py), here applied to the output and given its adjoint.

This module is the single place where the term is defined.

- ``HR``, ``SR`` are ``(B, C >= 3, X, Y, NZ)``.  Only channels 0..2 are read.  ``s`` is the factor.
- ``t = degradation.taps(kernel, s, sigma)``, with radius ``R <= degradation.MAX_RADIUS``.
- ``wx = degradation.axis_weights(X, s, t)`` has shape ``(XL, 2R+1)``, ``wy = degradation.axis_weights(Y, s, t)`` has
  shape ``(YL, 2R+1)``; ``XL = ceil(X / s)`` and ``YL = ceil(Y / s)``.
- The fp32 tables are exactly those of ``[DEGRADATION]`` (``degradation.tables``); nothing is re-derived here.
- z is never filtered.
- Everything is fp32 and nothing is contracted.  Accumulators start from ``+0.0f``, indices ascend, and taps outside
  ``[0, n)`` are skipped and never read.

Forward:

    e[x, y, z]  = fl(SR - HR)
    g[i, y, z]  = sum_{d asc} fl(wx[i, d] * e[s i + d - R, y, z])
    r[i, j, z]  = sum_{d asc} fl(wy[j, d] * g[i, s j + d - R, z])        -> (B, 3, XL, YL, NZ) fp32

Vector-Jacobian product, towards SR only, with ``G = dL/dr``; every ``(i, d)`` with ``x = s i + d - R`` is in range by
construction:

    t[x; j, z]    = sum_{i asc} fl(wx[i, x - s i + R] * G[i, j, z])
    dSR[x, y, z]  = sum_{j asc} fl(wy[j, y - s j + R] * t[x; j, z])
    channels >= 3: 0

``L_cons`` is the mean of ``|r|`` (``norm = l1``) or of ``r^2`` (``norm = l2``) over samples, the three wind components,
coarse cells and levels, in normalised units like ``pix``.

Consequences:

- ``r`` is exactly 0, with an exactly zero gradient, for SR = HR.
- ``coarse_residual(0, F)`` carries the bits of ``degradation.degrade_lr(F, s, spec)`` for the same kernel.
- ``L_cons`` of ``SR = HR + c`` is ``|c|`` (``c^2``) up to rounding, because every weight row sums to 1.
- A non-finite voxel of SR makes every coarse cell whose footprint holds it non-finite.  The core total is then
  non-finite and the Adam step is skipped, like a non-finite ``pix``.  No extra guard is added.

``L_cons`` is a plain mean over samples: under data parallelism equal shards average exactly as ``pix`` does, and no
collective is added.

On a GPU ``r`` is ``hip_ops.coarse_residual`` (one launch forward, one backward that needs only ``G`` and the tables); on
a CPU device (in float64), and under ``WSR_FUSED_CONSISTENCY_LOSS=0`` (in fp32 on the device),
``coarse_residual_reference`` composes it from whole-array torch ops, one per tap, and autograd differentiates them.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import degradation
from .config.config import ConsistencyLossConfig

#: the keys of ``[CONSISTENCY_LOSS]`` and their defaults, as ``ConsistencyLossConfig`` declares them
CONSISTENCY_LOSS = {k: getattr(ConsistencyLossConfig, k) for k, _ in ConsistencyLossConfig._schema}
NORMS = ("l1", "l2")
MIN_FACTOR, MAX_FACTOR = 2, 32


class CoarseTables(NamedTuple):
    """What ``coarse_tables`` returns: the fp32 tables ``wx`` (XL, 2R+1) and ``wy`` (YL, 2R+1) of
    ``degradation.tables`` as tensors on the device, the radius and the factor"""

    wx: torch.Tensor
    wy: torch.Tensor
    R: int
    s: int


def check_parameters(kernel, sigma, s, what="consistency_loss") -> None:
    """The ranges of ``[CONSISTENCY_LOSS]``, else a ValueError with the number"""
    if kernel not in degradation.KERNELS:
        raise ValueError(f"{what}: kernel must be box or gaussian, not {kernel!r}")
    if kernel == "gaussian" and (sigma is None or not 0.0 < float(sigma) <= 10.0):
        raise ValueError(f"{what}: sigma must be > 0 and <= 10 with kernel = gaussian, not {sigma}")
    if int(s) != s or not MIN_FACTOR <= s <= MAX_FACTOR:
        raise ValueError(f"{what}: the coarse-graining factor must be {MIN_FACTOR} .. {MAX_FACTOR}, not {s}")
    degradation.taps(kernel, int(s), None if kernel == "box" else float(sigma))  # (refuses a radius above MAX_RADIUS)


_tables: dict = {}


def coarse_tables(kernel: str, sigma, s: int, X: int, Y: int, device="cpu") -> CoarseTables:
    """The tables of ``[DEGRADATION]`` for an ``X x Y`` plane at factor ``s`` on ``device``: ``degradation.tables``,
    copied once per (kernel, sigma, s, X, Y, device)"""
    check_parameters(kernel, sigma, s, "coarse_tables")
    device = torch.device(device)
    sigma = float(sigma) if kernel == "gaussian" else None
    key = (kernel, sigma, int(s), int(X), int(Y), str(device))
    hit = _tables.get(key)
    if hit is None:
        if len(_tables) >= 16:
            _tables.clear()
        wx, wy, R = degradation.tables(degradation.DegradationSpec(kernel, sigma), int(s), int(X), int(Y))
        hit = CoarseTables(torch.from_numpy(np.array(wx)).to(device), torch.from_numpy(np.array(wy)).to(device), int(R),
                           int(s))
        _tables[key] = hit
    return hit


def fused() -> bool:
    """the run-time switch ``WSR_FUSED_CONSISTENCY_LOSS`` (0: the composed torch path on every device)"""
    return os.environ.get("WSR_FUSED_CONSISTENCY_LOSS", "1") != "0"


def _check_pair(HR, SR, what):
    for name, t in (("HR", HR), ("SR", SR)):
        if t.dim() != 5 or t.shape[1] < 3 or t.numel() == 0 or not t.is_floating_point():
            raise ValueError(f"{what} wants {name} as a floating-point (B, C >= 3, X, Y, NZ) tensor, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if (SR.shape[0],) + tuple(SR.shape[2:]) != (HR.shape[0],) + tuple(HR.shape[2:]):
        raise ValueError(f"{what}: SR {tuple(SR.shape)} does not match HR {tuple(HR.shape)}")


def _check_tables(tables: CoarseTables, X: int, Y: int, what: str) -> None:
    s, K = tables.s, 2 * tables.R + 1
    if tuple(tables.wx.shape) != (-(-X // s), K) or tuple(tables.wy.shape) != (-(-Y // s), K):
        raise ValueError(f"{what}: the tables {tuple(tables.wx.shape)}, {tuple(tables.wy.shape)} are not those of a "
                         f"{X} x {Y} plane at factor {s} with radius {tables.R}")


def _tap_range(d: int, n: int, n_out: int, s: int, R: int):
    """the outputs [lo, hi) whose tap ``d`` falls inside [0, n): s i + d - R >= 0 and <= n - 1"""
    return max(0, -(-(R - d) // s)), min(n_out, (n - 1 - d + R) // s + 1)


def _pass(f: torch.Tensor, w: torch.Tensor, s: int, R: int, axis: int) -> torch.Tensor:
    """one 1-D pass along ``axis`` (2 or 3) of f (B, 3, ., ., NZ): whole-array operations in f's dtype, one product and
    one sum per tap, taps ascending (``degradation._pass`` with a batch axis, in torch)"""
    n, n_out = f.shape[axis], w.shape[0]
    shape = list(f.shape)
    shape[axis] = n_out
    out = torch.zeros(shape, dtype=f.dtype, device=f.device)
    wshape = [1, 1, 1, 1, 1]
    wshape[axis] = -1
    for d in range(2 * R + 1):
        lo, hi = _tap_range(d, n, n_out, s, R)
        if hi <= lo:
            continue
        src = [slice(None)] * 5
        dst = [slice(None)] * 5
        src[axis] = slice(s * lo + d - R, s * (hi - 1) + d - R + 1, s)
        dst[axis] = slice(lo, hi)
        prod = w[lo:hi, d].reshape(wshape) * f[tuple(src)]
        out[tuple(dst)] = out[tuple(dst)] + prod  # (a sum saves nothing for autograd: the slice may be overwritten)
    return out


def _pass_t(G: torch.Tensor, w: torch.Tensor, n: int, s: int, R: int, axis: int) -> torch.Tensor:
    """the adjoint of ``_pass`` along ``axis``: out[x] = sum_{i asc} w[i, x - s i + R] G[i].  Whole-array operations, one
    per tap; a given x receives its terms from the taps d = x - s i + R in DESCENDING order, which is i ascending."""
    n_out = w.shape[0]
    shape = list(G.shape)
    shape[axis] = n
    out = torch.zeros(shape, dtype=G.dtype, device=G.device)
    wshape = [1, 1, 1, 1, 1]
    wshape[axis] = -1
    for d in range(2 * R, -1, -1):
        lo, hi = _tap_range(d, n, n_out, s, R)
        if hi <= lo:
            continue
        src = [slice(None)] * 5
        dst = [slice(None)] * 5
        src[axis] = slice(lo, hi)
        dst[axis] = slice(s * lo + d - R, s * (hi - 1) + d - R + 1, s)
        out[tuple(dst)] = out[tuple(dst)] + w[lo:hi, d].reshape(wshape) * G[tuple(src)]
    return out


def coarse_residual_reference(HR, SR, tables: CoarseTables, dtype=torch.float64) -> torch.Tensor:
    """``r`` of the module docstring -> (B, 3, XL, YL, NZ) in ``dtype`` on the tensors' device: whole-array torch ops, one
    product and one sum per tap, in the defined order; HR detached; differentiable by autograd.  The path of a CPU device
    and of ``WSR_FUSED_CONSISTENCY_LOSS=0``, and the oracle of the tests (in fp32 it is the kernel's arithmetic)."""
    _check_pair(HR, SR, "coarse_residual_reference")
    _check_tables(tables, HR.shape[2], HR.shape[3], "coarse_residual_reference")
    e = SR[:, :3].to(dtype) - HR[:, :3].detach().to(dtype)
    wx, wy = tables.wx.to(device=e.device, dtype=dtype), tables.wy.to(device=e.device, dtype=dtype)
    return _pass(_pass(e, wx, tables.s, tables.R, 2), wy, tables.s, tables.R, 3)


def coarse_residual_vjp(G, tables: CoarseTables, shape, dtype=torch.float64) -> torch.Tensor:
    """The closed form of the module docstring: ``G`` = dL/dr (B, 3, XL, YL, NZ) and the ``shape`` (B, C, X, Y, NZ) of
    SR -> dL/dSR in ``dtype``, zero in every channel from 3 on (in fp32 it is the backward kernel's arithmetic)"""
    B, C_, X, Y, NZ = (int(v) for v in shape)
    _check_tables(tables, X, Y, "coarse_residual_vjp")
    if tuple(G.shape) != (B, 3, tables.wx.shape[0], tables.wy.shape[0], NZ):
        raise ValueError(f"coarse_residual_vjp: G {tuple(G.shape)} does not belong to SR {tuple(shape)}")
    G = G.detach().to(dtype)
    wx, wy = tables.wx.to(device=G.device, dtype=dtype), tables.wy.to(device=G.device, dtype=dtype)
    t = _pass_t(G, wx, X, tables.s, tables.R, 2)
    out = torch.zeros((B, C_, X, Y, NZ), dtype=dtype, device=G.device)
    out[:, :3] = _pass_t(t, wy, Y, tables.s, tables.R, 3)
    return out


def coarse_residual(HR, SR, tables: CoarseTables) -> torch.Tensor:
    """``r``: the kernel pair on a GPU (fp32); the reference under ``WSR_FUSED_CONSISTENCY_LOSS=0`` (fp32 on the device)
    and on a CPU device (float64)"""
    if HR.is_cuda and fused():
        from . import hip_ops
        _check_tables(tables, HR.shape[2], HR.shape[3], "coarse_residual")
        return hip_ops.coarse_residual(HR, SR, tables.wx, tables.wy, tables.s)
    return coarse_residual_reference(HR, SR, tables, dtype=torch.float32 if HR.is_cuda else torch.float64)


def loss_from_residual(r: torch.Tensor, norm: str = "l1") -> torch.Tensor:
    """``L_cons`` of the module docstring from ``r`` -> a scalar in its dtype"""
    if norm not in NORMS:
        raise ValueError(f"loss_from_residual: norm must be l1 or l2, not {norm!r}")
    return r.abs().mean() if norm == "l1" else (r * r).mean()


def section_tables(HR, cfg_section, scale) -> CoarseTables:
    """``coarse_tables`` for a batch under the keys of ``cfg_section`` and ``[DEFAULT] scale``, which ``factor = 0``
    stands for; a factor larger than the patch is refused with the numbers"""
    s = int(cfg_section.factor) if cfg_section.factor else int(scale)
    X, Y = int(HR.shape[2]), int(HR.shape[3])
    if s > min(X, Y):
        raise ValueError(f"[CONSISTENCY_LOSS] the coarse-graining factor {s} is larger than the {X} x {Y} patch it is to "
                         f"coarse-grain: lower factor or train on larger patches")
    return coarse_tables(str(cfg_section.kernel), cfg_section.sigma, s, X, Y, HR.device)


def consistency_loss(HR, SR, cfg_section, scale) -> torch.Tensor:
    """``L_cons`` (un-weighted, a float32 scalar) of a batch ``HR``, ``SR`` (B, C >= 3, X, Y, NZ) under the keys of
    ``cfg_section`` (``kernel``, ``sigma``, ``factor``, ``norm``: a ``ConsistencyLossConfig`` or anything with those
    attributes) and ``[DEFAULT] scale``"""
    _check_pair(HR, SR, "consistency_loss")
    tables = section_tables(HR, cfg_section, scale)
    return loss_from_residual(coarse_residual(HR, SR, tables), str(cfg_section.norm)).float()
