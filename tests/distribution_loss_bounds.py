"""Inputs, float64 references and derived error bounds for the ``[DISTRIBUTION_LOSS]`` kernels (csrc/distribution_loss.hip),
shared by tests/test_distribution_loss.py (CPU) and tests/test_distribution_loss_gpu.py.  A plain helper module, like
ssim_loss_bounds.py.  u = 2^-24 is the unit roundoff of fp32, NS the number of bins, c = fl(UVW_MAX / bin_width) the same
fp32 number on both sides, n = X * Y the voxels of a row.

The position
-----------
The kernel computes t = fl(fl(r c) - 0.5) with r = sqrt_rn(fl(fl(u u) + fl(v v))); the float64 reference computes the same
expression at the same fp32 inputs with errors of 2^-53, which are ignored.  Relative errors, first order in u:

    fl(u u), fl(v v)    1 rounding each, both terms positive: their sum carries <= 1 u, the addition 1 more   -> hs2: 2 u
    sqrt                halves what it is given and rounds once                                              -> r:   2 u
    fl(r c)             1 rounding                                                                           -> r c: 3 u
    fl(. - 0.5)         1 rounding of the result t

so |t32 - t64| <= 3 u (t + 1/2) + u |t|.  Only voxels with t <= NS matter (beyond NS both sides sit on the upper clamp,
whose neighbourhood of width 4 NS u is inside the case t <= NS), hence |t32 - t64| <= (4 NS + 2) u <= 6 NS u for NS >= 2
(second-order terms are below 2^-40).

Forward
-------
The weight a voxel gives to bin k is the hat function max(0, 1 - |clamp(t) - k|) of its position, with the two end bins
flat beyond the clamps: 1-Lipschitz in t and continuous, so a voxel that changes k0 between the two evaluations costs
nothing extra.  The device adds fi / 65536 with fi = rint(f 65536), f = t - k0 exact in fp32 (t <= 63 and k0 <= t): at most
2^-17 from f, and 65536 - fi has the same error.  Summed over the n voxels of a row, per entry

    |H - H64| <= n (2^-17 + 6 NS u)                                                          ``forward_bound``

Column NS (non-finite hs2) is exact: the test inputs hold NaNs or finite values far below the overflow of fp32.

Backward
--------
Per element g = ((d c) x) / r with d = fl(G[k0 + 1] - G[k0]), x = u or v.  G is handed over as fp32 and the reference uses
the same fp32 numbers, so the subtraction is ONE rounding - but its result can be far smaller than its operands, and an
upstream table that differs in its last bit (the loss test below) moves d by u (|G[k0 + 1]| + |G[k0]|).  The bound is
therefore stated on the magnitude with the cancellation undone,

    A = (|G[k0 + 1]| + |G[k0]|) c |x| / r  >=  |g|

and counts the roundings: the subtraction, two multiplications, one division (correctly rounded), and the 2 u of r
above: 6 in all,

    |g32 - g64| <= gamma_6 A + 2^-100,    gamma_k = k u / (1 - k u)                          ``ref_backward``

(2^-100 keeps it positive where A = 0.)  The derivative jumps where t crosses an integer - a bin switch or a clamp, both
integers - so the two evaluations may sit on different sides: voxels whose float64 t lies within 12 NS u (twice the bound
on |t32 - t64|) of an integer are left out of the comparison, and the tests assert that these are at most 1 % of a case.

The loss
--------
``loss_from_counts`` in float64 on tables that are each within ``forward_bound`` of the truth.  The running sums of
p = H[:NS] / n (the rows sum to n exactly on the device) are means over voxels of 1-Lipschitz, continuous functions of t
too (0, 1 - f, 1), so each F(k) is within eps = 2^-17 + 6 NS u of its float64 value, each |F_sr(k) - F_hr(k)| within
2 eps, and

    |L - L64| <= 2 (NS - 1) bin_width eps                                                    ``loss_bound``

For the gradient, dL/dH_sr[k] = a (S_k - const) with a = bin_width / (rows n), S_k the sum of sign(F_sr(j) - F_hr(j)) over
k <= j < NS - 1: as long as no |F_sr(j) - F_hr(j)| is below 2 eps (``signs_are_safe``: asserted by the test on its inputs,
not assumed) the signs agree on both sides, the table differs from the float64 one by float64 rounding only, and its
fp32 rounding by at most one more u on each of G[k0 + 1] and G[k0]: one more unit of A, gamma_7.
"""
import math

import torch

from kernel_bounds import TINY, U_FP32

QUANTUM = 2.0 ** -17


def eps_position(ns: int) -> float:
    """the bound on |t32 - t64|"""
    return 6.0 * ns * U_FP32


def forward_bound(n: int, ns: int) -> float:
    """per entry of H, n = X * Y"""
    return n * (QUANTUM + eps_position(ns))


def loss_bound(ns: int, bin_width: float) -> float:
    return 2.0 * (ns - 1) * float(bin_width) * (QUANTUM + eps_position(ns))


def gamma(k: int) -> float:
    return k * U_FP32 / (1.0 - k * U_FP32)


def tables_for(ns: int, bin_width: float = 1.5, UVW_MAX: float = 32.0):
    from gan_sr_wind_field_amd.distribution_loss import soft_tables

    return soft_tables(UVW_MAX, bin_width, ns)


def wind_fields(B, C, X, Y, NZ, tables, seed, zeros=3, nans=0):
    """fp32 HR, SR (B, C, X, Y, NZ): HR a sum of three plane waves per (sample, component) whose phase turns with z, scaled
    so that its largest speed sits a quarter beyond the last bin centre (the upper clamp) - SR is 0.85 HR plus smooth and
    white noise, a field with too little strong wind.  Both clamps are spanned: ``zeros`` exact zero vectors, as many
    vectors below the first centre and as many far beyond the last one are planted in each, at different voxels.
    ``nans``: that many NaN voxels planted in SR.  Channels from 2 on hold NaN: they are never read."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 2, X, Y, NZ)
    i = torch.arange(X, dtype=torch.float64).view(1, 1, X, 1, 1)
    j = torch.arange(Y, dtype=torch.float64).view(1, 1, 1, Y, 1)
    k = torch.arange(NZ, dtype=torch.float64).view(1, 1, 1, 1, NZ)

    def waves():
        f = torch.zeros(shape, dtype=torch.float64)
        for _ in range(3):
            fx, fy = (0.3 + 0.7 * torch.rand((B, 2, 1, 1, 1), generator=g, dtype=torch.float64) for _ in range(2))
            ph = torch.rand((B, 2, 1, 1, 1), generator=g, dtype=torch.float64) * 2 * math.pi
            f = f + torch.sin(fx * i + fy * j + 0.21 * k + ph)
        return f

    hr = waves()
    top = 1.25 * (tables.speed_bins - 0.5) / tables.c
    hr = hr * (top / float((hr[:, 0] ** 2 + hr[:, 1] ** 2).sqrt().max()))
    sr = 0.85 * hr + 0.05 * top * waves() / 3 + 0.01 * top * torch.randn(shape, generator=g, dtype=torch.float64)
    out = []
    vol = X * Y * NZ
    for f, shift in ((hr, 0), (sr, 1)):
        f = f.float().reshape(B, 2, vol)
        perm = torch.randperm(vol, generator=g)
        at = 0
        for b in range(B):
            for val in ((0.0, 0.0), (0.2 / tables.c, -0.1 / tables.c), (0.0, 3.0 * top)):
                for _ in range(zeros):
                    p = int(perm[(at + shift) % vol])
                    f[b, 0, p], f[b, 1, p] = val
                    at += 2
        full = torch.full((B, C, vol), float("nan"))
        full[:, :2] = f
        out.append(full)
    if nans:
        perm = torch.randperm(vol, generator=g)
        for b in range(B):
            for q in range(nans):
                out[1][b, q % 2, int(perm[q])] = float("nan")
    return tuple(t.view(B, C, X, Y, NZ).contiguous() for t in out)


def reference_tables(HR, SR, tables):
    """float64 H (2, B, NZ, NS + 1) at the fp32 inputs"""
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_reference

    return soft_counts_reference(HR.cpu(), SR.cpu(), tables, torch.float64)


def random_upstream(B, NZ, ns, seed):
    """an upstream table dL/dH_sr[..., :NS] as the wrapper hands it over: fp32 (B, NZ, NS), N(0, 1)"""
    return torch.randn((B, NZ, ns), generator=torch.Generator().manual_seed(seed)).float()


def ref_backward(SR, G32, tables, roundings: int = 6):
    """(float64 VJP (B, C, X, Y, NZ) at the fp32 inputs and the fp32 table, its bound, the mask of the voxels that are
    compared (B, X, Y, NZ))"""
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_vjp, soft_positions

    SR = SR.cpu()
    ns = tables.speed_bins
    grad = soft_counts_vjp(SR, G32.double(), tables, torch.float64)
    u, v = SR[:, 0].double(), SR[:, 1].double()
    t, k0, _, finite = soft_positions(u, v, tables)
    r = torch.sqrt(torch.where(finite, u * u + v * v, torch.zeros_like(u)))
    Gx = G32.double().abs().unsqueeze(1).unsqueeze(1).expand(-1, SR.shape[2], SR.shape[3], -1, -1)
    mag = (Gx.gather(4, (k0 + 1).unsqueeze(-1)) + Gx.gather(4, k0.unsqueeze(-1))).squeeze(-1)
    live = finite & (r > 0)
    safe = torch.where(live, r, torch.ones_like(r))
    bound = torch.full(SR.shape, TINY, dtype=torch.float64)
    for ch, x in ((0, u), (1, v)):
        bound[:, ch] += torch.where(live, gamma(roundings) * mag * tables.c * x.abs() / safe, torch.zeros_like(r))
    near = (t - t.round()).abs() <= 2.0 * eps_position(ns)
    keep = ~(finite & near)
    return grad, bound, keep


def signs_are_safe(H, ns: int, pool: str) -> bool:
    """no |F_sr(k) - F_hr(k)| of the float64 tables ``H`` (2, B, NZ, NS + 1) lies within 2 eps of zero"""
    cdf = []
    for s in (0, 1):
        h = H[s][..., :ns]
        if pool == "sample":
            h = h.sum(dim=1)
        cdf.append((h / h.sum(dim=-1, keepdim=True)).cumsum(dim=-1)[..., :ns - 1])
    return bool(((cdf[1] - cdf[0]).abs() > 2.0 * (QUANTUM + eps_position(ns))).all())
