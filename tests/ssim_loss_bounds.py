"""The float64 evaluation of the [SSIM_LOSS] vector-Jacobian product and its per-element error bound, shared by
tests/test_ssim_loss.py (where the closed form is held against float64 autograd and the bound is shown to be sound and to
have teeth, on the CPU) and tests/test_ssim_loss_gpu.py (where the backward kernel is held to it).  A plain helper module
like ssim_bounds.py, whose moments, moment errors and quotient rule it takes over.  Nothing here is measured against the
code under test, and nothing of the package is used but the tap table.

``ref_vjp`` evaluates, in numpy float64 from the fp32 inputs, the fp32 taps and the float64 ``gout`` (B, NZ, 3, 2) =
(G0, G1),

    h     = G0 l + G1
    alpha = G0 cs (2 mu_a - 2 mu_s l) / D1 + h (2 mu_s cs - 2 mu_a) / D2
    beta  = -h cs / D2,    gamma = 2 h / D2
    dL/dSR(p) = (g2^T alpha)(p) + 2 s(p) (g2^T beta)(p) + a(p) (g2^T gamma)(p)

with g2^T the adjoint of the valid separable window: the coefficient maps padded with win - 1 zeros on every side and
filtered with the reversed taps.

The bound (kernel_bounds.py's convention; LAMBDA = 16 and u = 2^-24 imported, untouched).  The moment errors e_m and the
errors of var, cov, N1, D1, N2, D2 are those of ssim_bounds.py; every product carries |x| dy + |y| dx + dx dy, every
quotient (dN + |N / D| dD) / (D - dD) with D - dD > 0 asserted, every rounded operation a few u of its value:

    dG   = u |G|                                               gout is rounded to fp32
    b_l  = d_l + 4 u |l|,  b_cs = d_cs + 4 u |cs|
    d_h  = |G0| b_l + dG0 (|l| + b_l) + dG1 + 4 u (|G0 l| + |G1|)
    w1 = 2 mu_a - 2 mu_s l      d_w1 = 2 e_mua + 2 (|mu_s| b_l + |l| e_mus + e_mus b_l) + 4 u (|2 mu_a| + |2 mu_s l|)
    v1 = G0 cs                  d_v1 = |G0| b_cs + dG0 (|cs| + b_cs) + 2 u |v1|
    w2 = 2 mu_s cs - 2 mu_a     d_w2 = 2 (|mu_s| b_cs + |cs| e_mus + e_mus b_cs) + 2 e_mua + 4 u (|2 mu_s cs| + |2 mu_a|)
    b_alpha = d(v1 w1 / D1) + d(h w2 / D2) + 4 u (|v1 w1 / D1| + |h w2 / D2|)
    b_beta  = d(h cs / D2) + 4 u |beta|,   b_gamma = d(2 h / D2) + 4 u |gamma|
    B(p) = g2^T b_alpha + 2 |s| g2^T b_beta + |a| g2^T b_gamma
           + LAMBDA win^2 u (g2^T |alpha| + 2 |s| g2^T |beta| + |a| g2^T |gamma|)

What keeps the bound from being vacuous: its mean over the elements is at most ``MEAN_CAP`` = 2e-2 of the rms of the
float64 gradient on every tested case, asserted by the tests.
"""
import functools

import numpy as np
import torch

from kernel_bounds import LAMBDA, U_FP32
from ssim_bounds import _quotient, _windowed, fields

MEAN_CAP = 2e-2

#: (B, X, Y, NZ), (win, sigma): the shapes the bound was stated on; the GPU tests add more (test_ssim_loss_gpu.py)
CASES = [((2, 7, 6, 5), (3, 1.0)), ((1, 11, 11, 3), (11, 1.5)), ((1, 16, 16, 10), (11, 1.5)), ((1, 40, 12, 8), (7, 1.0)),
         ((1, 70, 66, 6), (11, 1.5)), ((1, 17, 15, 4), (15, 2.0))]

#: (B, X, Y, NZ), (win, sigma), seed: where the bound is shown to have teeth; fixed seeds for which both wrong
#: evaluations are at least 10 bounds off somewhere (test_ssim_loss.py)
TEETH_CASES = [((1, 7, 6, 2), (3, 1.0), 7023), ((1, 11, 11, 2), (11, 1.5), 11031), ((1, 16, 16, 2), (11, 1.5), 116031),
               ((1, 40, 12, 2), (7, 1.0), 40027), ((1, 17, 15, 2), (15, 2.0), 17035)]


def case_id(case):
    return "x".join(map(str, case[0])) + f"-w{case[1][0]}"


def adjoint(m, g):
    """g2^T m: m (..., PX, PY) float64 -> (..., PX + win - 1, PY + win - 1), the adjoint of ``ssim_bounds._windowed``"""
    h = g.size - 1
    pad = [(0, 0)] * (m.ndim - 2) + [(h, h), (h, h)]
    return _windowed(np.pad(m, pad), np.ascontiguousarray(g[::-1]))


def random_gout(B, NZ, seed):
    """(B, NZ, 3, 2) float64, N(0, 1) in both columns"""
    return torch.randn((B, NZ, 3, 2), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _prod(x, dx, y, dy):
    """|d(x y)| for |dx|, |dy|, before the rounding of the product itself"""
    return np.abs(x) * dy + np.abs(y) * dx + dx * dy


def ref_vjp(HR, SR, gout, win, sigma, data_range=2.0, drop_alpha=False, crop=False):
    """(grad, bound): float64 tensors (B, 3, X, Y, NZ).  ``drop_alpha`` and ``crop`` are the two WRONG evaluations of the
    teeth test: the alpha term left out, and the adjoint kept only where a pixel lies in all win x win windows."""
    from gan_sr_wind_field_amd.ssim import taps

    g = taps(win, sigma).numpy().astype(np.float64)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    u = U_FP32

    def planes(f):  # (B, C, X, Y, NZ) -> (B, NZ, 3, X, Y) float64
        return np.ascontiguousarray(f[:, :3].detach().cpu().numpy().astype(np.float64).transpose(0, 4, 1, 2, 3))

    a, s = planes(HR), planes(SR)
    G = gout.detach().cpu().numpy().astype(np.float64)
    G0, G1 = G[..., 0, None, None], G[..., 1, None, None]
    dG0, dG1 = u * np.abs(G0), u * np.abs(G1)
    e = LAMBDA * win * u
    mua, mus = _windowed(a, g), _windowed(s, g)
    Saa, Sss, Sas = _windowed(a * a, g), _windowed(s * s, g), _windowed(a * s, g)
    e_mua, e_mus = e * _windowed(np.abs(a), g), e * _windowed(np.abs(s), g)
    e_Saa, e_Sss, e_Sas = e * Saa, e * Sss, e * _windowed(np.abs(a) * np.abs(s), g)
    va, vs, cov = Saa - mua * mua, Sss - mus * mus, Sas - mua * mus
    d_va = e_Saa + 2 * np.abs(mua) * e_mua + e_mua ** 2
    d_vs = e_Sss + 2 * np.abs(mus) * e_mus + e_mus ** 2
    cross = np.abs(mua) * e_mus + np.abs(mus) * e_mua + e_mua * e_mus
    d_cov = e_Sas + cross
    D1 = mua * mua + mus * mus + C1
    dD1 = 2 * np.abs(mua) * e_mua + e_mua ** 2 + 2 * np.abs(mus) * e_mus + e_mus ** 2
    D2, dD2 = va + vs + C2, d_va + d_vs
    l, d_l = _quotient(2 * mua * mus + C1, 2 * cross, D1, dD1)
    cs, d_cs = _quotient(2 * cov + C2, 2 * d_cov, D2, dD2)
    b_l, b_cs = d_l + 4 * u * np.abs(l), d_cs + 4 * u * np.abs(cs)

    h = G0 * l + G1
    d_h = np.abs(G0) * b_l + dG0 * (np.abs(l) + b_l) + dG1 + 4 * u * (np.abs(G0 * l) + np.abs(G1))
    w1 = 2 * mua - 2 * mus * l
    d_w1 = 2 * e_mua + 2 * _prod(mus, e_mus, l, b_l) + 4 * u * (np.abs(2 * mua) + np.abs(2 * mus * l))
    v1 = G0 * cs
    d_v1 = np.abs(G0) * b_cs + dG0 * (np.abs(cs) + b_cs) + 2 * u * np.abs(v1)
    w2 = 2 * mus * cs - 2 * mua
    d_w2 = 2 * _prod(mus, e_mus, cs, b_cs) + 2 * e_mua + 4 * u * (np.abs(2 * mus * cs) + np.abs(2 * mua))
    T1, d_T1 = _quotient(v1 * w1, _prod(v1, d_v1, w1, d_w1) + 2 * u * np.abs(v1 * w1), D1, dD1)
    T2, d_T2 = _quotient(h * w2, _prod(h, d_h, w2, d_w2) + 2 * u * np.abs(h * w2), D2, dD2)
    alpha, b_alpha = T1 + T2, d_T1 + d_T2 + 4 * u * (np.abs(T1) + np.abs(T2))
    hcs, d_beta = _quotient(h * cs, _prod(h, d_h, cs, b_cs) + 2 * u * np.abs(h * cs), D2, dD2)
    beta, b_beta = -hcs, d_beta + 4 * u * np.abs(hcs)
    gamma, d_gamma = _quotient(2 * h, 2 * d_h, D2, dD2)
    b_gamma = d_gamma + 4 * u * np.abs(gamma)
    if drop_alpha:
        alpha = np.zeros_like(alpha)

    A, Bt, Cg = adjoint(alpha, g), adjoint(beta, g), adjoint(gamma, g)
    grad = A + 2 * s * Bt + a * Cg
    if crop:
        X, Y = a.shape[-2:]
        keep = np.zeros((X, Y))
        keep[win - 1:X - win + 1, win - 1:Y - win + 1] = 1.0
        grad = grad * keep
    bound = (adjoint(b_alpha, g) + 2 * np.abs(s) * adjoint(b_beta, g) + np.abs(a) * adjoint(b_gamma, g)
             + LAMBDA * win * win * u * (adjoint(np.abs(alpha), g) + 2 * np.abs(s) * adjoint(np.abs(beta), g)
                                         + np.abs(a) * adjoint(np.abs(gamma), g)))

    def back(v):  # (B, NZ, 3, X, Y) -> (B, 3, X, Y, NZ)
        return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 3, 4, 1)))

    return back(grad), back(bound)


def tightness(grad, bound):
    """mean bound / rms gradient: what ``MEAN_CAP`` limits"""
    return float(bound.mean()) / float(grad.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def case_data(case, kind):
    """(HR, SR, gout, grad, bound) of a case: computed once, shared by the tests, never modified.  The inputs are
    ``ssim_bounds.fields`` with its seeds, gout is N(0, 1) in both columns."""
    (B, X, Y, NZ), (win, sigma) = case
    seed = 1000 * X + 10 * NZ + win
    HR, SR, _ = fields(B, X, Y, NZ, seed=seed, kind=kind)
    gout = random_gout(B, NZ, seed + 1)
    grad, bound = ref_vjp(HR, SR, gout, win, sigma)
    return HR, SR, gout, grad, bound


def autograd_vjp(HR, SR, gout, win, sigma, dtype, data_range=2.0):
    """dL/dSR (B, C, X, Y, NZ) float64 by torch autograd of ``ssim.ssim_maps`` in ``dtype``, L = sum gout * P"""
    from gan_sr_wind_field_amd.ssim_loss import pair_sums_reference

    x = SR.to(dtype).clone().requires_grad_(True)  # (a float64 leaf for a float64 gradient)
    P = pair_sums_reference(HR, x, win, sigma, data_range, dtype=dtype)
    (P * gout.to(P.dtype)).sum().backward()
    return x.grad.double()
