"""Inputs, float64 references and derived error bounds for the ``[CONSISTENCY_LOSS]`` kernels (csrc/consistency_loss.hip),
shared by tests/test_consistency_loss.py (CPU) and tests/test_consistency_loss_gpu.py.  A plain helper module, like
distribution_loss_bounds.py.  u = 2^-24 is the unit roundoff of fp32, gamma_k = k u / (1 - k u), R the tap radius, s the
factor.  Both sides read the SAME fp32 weight tables (``degradation.tables``), whose entries are non-negative; the float64
reference evaluates the definition at the same fp32 inputs with errors of 2^-53, which are ignored.

The inputs
----------
Normalised winds of magnitude at most 1 with |x| >= 2^-20 or x = 0 (``wind_fields`` snaps what lies below to 0), and
upstream gradients of the same kind.  The smallest weight of a test is above 2^-13 (the end tap of a gaussian with
sigma = 10 is exp(-4.5) / 25).  A difference e = fl(SR - HR) of two such numbers is 0 or at least 2^-20 2^-23 = 2^-43 in
magnitude (one unit in the last place of the smaller operand), so the smallest product is above 2^-56 and the smallest
product of the second pass above 2^-69: nothing is subnormal, and every rounding is a relative one.

Forward
-------
e32 = fl(SR - HR) = e (1 + d), |d| <= u.  A coarse cell is a sum over its footprint of wy wx e32, and every term passes
one product and at most 2 R + 1 sums per pass (the first sum, to +0.0f, is exact): at most n = 2 (2 R + 2) roundings on
its path, each 1 + d_k with |d_k| <= u, whose product is 1 + theta with |theta| <= gamma_n.  With |D| the filter with
its (non-negative) weights applied to absolute values, per coarse cell

    |r32 - r64| <= u |D|(|SR - HR|) + gamma_n |D|(|e32|) <= (u + gamma_n (1 + u)) |D|(|SR - HR|)       ``ref_forward``

The operator is linear: there is no switch, no clamp and no division, so no voxel is left out of the comparison.

Backward
--------
The same count for the adjoint: an element of dSR is a sum over at most m = ceil((2 R + 1) / s) coarse columns and as
many coarse rows, every term one product and at most m sums per pass: n' = 2 (m + 1), and

    |dSR32 - dSR64| <= gamma_n' |D^T|(|G|)                                                             ``ref_backward``

with G the fp32 upstream gradient both sides read.  Again nothing is left out.

The loss
--------
``loss_from_residual`` on an r that is within b = ``ref_forward``'s bound of r64, N = r.numel():

    l1:  ||r32| - |r64|| <= b
    l2:  |fl(r32^2) - r64^2| <= b (2 |r64| + b) + u (|r64| + b)^2
    the fp32 mean of N numbers in ANY order is within gamma_N of the mean of their magnitudes             ``loss_bound``

For the gradient the upstream table is G = sign(r) / N (l1) or 2 r / N (l2), formed in fp32 from r32.  l1: as long as
every |r64| exceeds its bound b - or is exactly 0 because its whole footprint is (``signs_are_safe``: asserted by the
test on its inputs, not assumed) - the signs agree, and G32 differs from G64 by the rounding of 1 / N alone: u |G|.
l2: G32 - G64 = 2 (r32 - r64) / N and two roundings (the product with 2 / N, and 1 / N itself).  The perturbation of G
passes through D^T with non-negative weights, so

    l1:  |dSR32 - dSR64| <= (gamma_n' + 2 u) |D^T|(|G64|)
    l2:  |dSR32 - dSR64| <= (gamma_n' + 4 u) |D^T|(|G64|) + (1 + gamma_n') |D^T|(2 b / N)                ``loss_grad_bound``

(one u more than counted in each, for the final conversion of the scalar loss to fp32, whose backward is a product with
1.0f - exact - kept as slack for a path that scales by the weight).  The composed fp32 path (WSR_FUSED_CONSISTENCY_LOSS=0)
forms the same sums with the same number of non-zero terms per element - autograd adds exact zeros besides - in another
order: the same bounds hold, which is why both paths are held to float64 and not to each other.
"""
import math

import torch

from kernel_bounds import TINY, U_FP32

SNAP = 2.0 ** -20


def gamma(k: int) -> float:
    return k * U_FP32 / (1.0 - k * U_FP32)


def n_forward(R: int) -> int:
    """roundings on the longest path of one term of a coarse cell"""
    return 2 * (2 * R + 2)


def n_backward(R: int, s: int) -> int:
    """roundings on the longest path of one term of an element of dSR"""
    return 2 * (-(-(2 * R + 1) // s) + 1)


def tables_for(kernel, sigma, s, X, Y):
    from gan_sr_wind_field_amd.consistency_loss import coarse_tables

    return coarse_tables(kernel, sigma, s, X, Y, "cpu")


def _snap(f):
    return torch.where(f.abs() < SNAP, torch.zeros_like(f), f).clamp(-1.0, 1.0)


def wind_fields(B, C, X, Y, NZ, seed, zeros=3):
    """fp32 HR, SR (B, C, X, Y, NZ) within [-1, 1], no magnitude below 2^-20 but 0: HR a sum of three plane waves per
    (sample, component) whose phase turns with z, scaled to 0.9 - SR is 0.9 HR plus a smooth and a white error and a
    constant offset per component (the cell averages drift).  ``zeros`` exact zeros are planted in each, and as many
    voxels where SR equals HR bit for bit.  Channels from 3 on hold NaN: they are never read."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 3, X, Y, NZ)
    i = torch.arange(X, dtype=torch.float64).view(1, 1, X, 1, 1)
    j = torch.arange(Y, dtype=torch.float64).view(1, 1, 1, Y, 1)
    k = torch.arange(NZ, dtype=torch.float64).view(1, 1, 1, 1, NZ)

    def waves():
        f = torch.zeros(shape, dtype=torch.float64)
        for _ in range(3):
            fx, fy = (0.3 + 0.7 * torch.rand((B, 3, 1, 1, 1), generator=g, dtype=torch.float64) for _ in range(2))
            ph = torch.rand((B, 3, 1, 1, 1), generator=g, dtype=torch.float64) * 2 * math.pi
            f = f + torch.sin(fx * i + fy * j + 0.21 * k + ph)
        return f / 3.0

    hr = 0.9 * waves()
    off = 0.05 * (torch.rand((B, 3, 1, 1, 1), generator=g, dtype=torch.float64) - 0.5)
    sr = 0.9 * hr + 0.05 * waves() + 0.01 * torch.randn(shape, generator=g, dtype=torch.float64) + off
    hr, sr = _snap(hr.float()).reshape(B, 3, -1), _snap(sr.float()).reshape(B, 3, -1)
    vol = X * Y * NZ
    perm = torch.randperm(vol, generator=g)
    for b in range(B):
        for q in range(zeros):
            c = q % 3
            hr[b, c, int(perm[(3 * q) % vol])] = 0.0
            sr[b, c, int(perm[(3 * q + 1) % vol])] = 0.0
            sr[b, c, int(perm[(3 * q + 2) % vol])] = hr[b, c, int(perm[(3 * q + 2) % vol])]
    out = []
    for f in (hr, sr):
        full = torch.full((B, C, vol), float("nan"))
        full[:, :3] = f
        out.append(full.view(B, C, X, Y, NZ).contiguous())
    return tuple(out)


def random_upstream(B, XL, YL, NZ, seed):
    """an upstream gradient dL/dr as the wrapper hands it over: fp32 (B, 3, XL, YL, NZ), uniform in [-1, 1], no magnitude
    below 2^-20"""
    g = torch.Generator().manual_seed(seed)
    return _snap((torch.rand((B, 3, XL, YL, NZ), generator=g) * 2.0 - 1.0).float()).contiguous()


def ref_forward(HR, SR, tables):
    """(float64 r (B, 3, XL, YL, NZ) at the fp32 inputs, its bound)"""
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_reference

    HR, SR = HR.cpu(), SR.cpu()
    r = coarse_residual_reference(HR, SR, tables, torch.float64)
    mag = (SR[:, :3].double() - HR[:, :3].double()).abs()
    A = coarse_residual_reference(torch.zeros_like(mag), mag, tables, torch.float64)
    return r, (U_FP32 + gamma(n_forward(tables.R)) * (1.0 + U_FP32)) * A + TINY


def ref_backward(G32, tables, shape, extra_u: int = 0):
    """(float64 VJP (B, C, X, Y, NZ) at the fp32 upstream gradient, its bound); ``extra_u``: further relative roundings of
    the upstream gradient itself"""
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_vjp

    G = G32.cpu().double()
    grad = coarse_residual_vjp(G, tables, shape, torch.float64)
    A = coarse_residual_vjp(G.abs(), tables, shape, torch.float64)
    return grad, (gamma(n_backward(tables.R, tables.s)) + extra_u * U_FP32) * A + TINY


def loss_bound(r64, b, norm: str) -> float:
    """|L32 - L64| for ``loss_from_residual`` of an r within ``b`` of ``r64``, the mean taken in fp32 in any order"""
    n = r64.numel()
    if norm == "l1":
        per, mag = b, r64.abs() + b
    else:
        mag = (r64.abs() + b) ** 2
        per = b * (2.0 * r64.abs() + b) + U_FP32 * mag
    return float(per.mean()) + gamma(n) * float(mag.mean()) + U_FP32 * float(mag.mean()) + TINY


def signs_are_safe(r64, b) -> bool:
    """every |r64| exceeds its bound, or is exactly 0 with a zero bound magnitude (SR = HR on its whole footprint)"""
    return bool(((r64.abs() > b) | ((r64 == 0) & (b <= TINY))).all())


def loss_grad_bound(r64, b, tables, shape, norm: str):
    """(float64 dL/dSR of ``loss_from_residual`` through the float64 reference, its bound)"""
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_vjp

    n = r64.numel()
    G = torch.sign(r64) / n if norm == "l1" else 2.0 * r64 / n
    grad = coarse_residual_vjp(G, tables, shape, torch.float64)
    A = coarse_residual_vjp(G.abs(), tables, shape, torch.float64)
    g = gamma(n_backward(tables.R, tables.s))
    if norm == "l1":
        return grad, (g + 2 * U_FP32) * A + TINY
    P = coarse_residual_vjp(2.0 * b / n, tables, shape, torch.float64)
    return grad, (g + 4 * U_FP32) * A + (1.0 + g) * P + TINY
