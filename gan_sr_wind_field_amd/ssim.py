"""Structural similarity (``[SSIM]``): the SSIM of Wang et al. 2004 between the truth and the super-resolved field, and
between the truth and the trilinear baseline, on horizontal planes.  Beside the PSNR it is the other number every
super-resolution result is reported with; its contrast-structure factor ``cs`` falls for a blurred field even where the
point-wise error is small, and it is reported per field, per wind component and per z level.

Everything is built from four sums per sample, z level and component (``SSIM_SUMS``): on a GPU ``hip_ops.level_ssim``
takes them in one fused launch on the native layout (csrc/ssim.hip), ``level_ssim_reference`` composes the same sums
from torch ops on any device (the path of a CPU device and of the host loop, and the oracle of the CPU tests).
``ssim_from_sums`` turns a table of sums into means, defined once for every caller.

Definitions.  For sample b, component c in {u, v, w} (channels 0..2) and level z, a = HR[b, c, :, :, z] and
s = SR[b, c, :, :, z] (likewise with the baseline TL in place of SR).  z is never windowed: the levels are
terrain-following and unevenly spaced.

    g                    the separable gaussian window of odd size ``win`` and standard deviation ``sigma``: 1-D taps
                         exp(-(k - (win - 1) / 2)^2 / (2 sigma^2)) in float64, normalised to sum 1, rounded to fp32
                         (``taps``: one table, read by the reference and handed to the kernel)
    positions            the valid ones only, npos = (X - win + 1) (Y - win + 1) per plane; no padding
    mu_a, mu_s           the windowed sums of a and s;  S_aa, S_ss, S_as those of a a, s s, a s
    var_a = S_aa - mu_a^2,  var_s = S_ss - mu_s^2,  cov = S_as - mu_a mu_s
    l  = (2 mu_a mu_s + C1) / (mu_a^2 + mu_s^2 + C1)
    cs = (2 cov + C2) / (var_a + var_s + C2)
    SSIM = l cs,         C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = ``data_range`` (2.0: a normalised component spans [-1, 1],
                         the range behind the max_diff_squared = 4 of the PSNR)

The four sums over the valid positions - ``ssim_sr``, ``cs_sr``, ``ssim_tl``, ``cs_tl`` - form a float64 (B, NZ, 3, 4) table.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

#: the four sums of one (sample, level, component), in the order of ``wsr_level_ssim``
SSIM_SUMS = ("ssim_sr", "cs_sr", "ssim_tl", "cs_tl")

#: the columns of the SSIM files, after ``field`` (``level`` in the per-level file)
SSIM_COLUMNS = ("SSIM", "SSIM_trilinear", "CS", "CS_trilinear", "SSIM_u", "SSIM_v", "SSIM_w")

MAX_WIN = 15  # WSR_SSIM_MAX_WIN
MAX_NZ = 256


def check_window(win, sigma, what="ssim") -> None:
    """``win`` odd in 3 .. 15 and ``sigma`` > 0, else a ValueError with the numbers"""
    if int(win) != win or win % 2 == 0 or not 3 <= win <= MAX_WIN:
        raise ValueError(f"{what}: the window size must be odd and 3 .. {MAX_WIN}, not {win}")
    if not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise ValueError(f"{what}: sigma must be > 0, not {sigma}")


def taps(win: int, sigma: float) -> torch.Tensor:
    """The 1-D gaussian taps -> fp32 (win,): computed in float64, normalised to sum 1, then rounded"""
    check_window(win, sigma, "ssim.taps")
    k = torch.arange(int(win), dtype=torch.float64) - (int(win) - 1) / 2
    g = torch.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).to(torch.float32)


def constants(data_range: float = 2.0):
    """(C1, C2) as Python floats"""
    if not (float(data_range) > 0 and math.isfinite(float(data_range))):
        raise ValueError(f"ssim: data_range must be > 0, not {data_range}")
    return (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2


def n_positions(X: int, Y: int, win: int) -> int:
    """npos of one plane"""
    return (int(X) - int(win) + 1) * (int(Y) - int(win) + 1)


def check_domain(X, Y, win, what="ssim") -> None:
    if X < win or Y < win:
        raise ValueError(f"{what}: the {X} x {Y} horizontal plane is smaller than the {win} x {win} window "
                         f"([SSIM] window_size)")


def windowed(p: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The valid separable window sums of planes ``p`` (N, X, Y) with taps ``g`` (win,) of p's dtype -> (N, X - win + 1,
    Y - win + 1): along x, then along y"""
    win = g.numel()
    q = F.conv2d(p.unsqueeze(1), g.view(1, 1, win, 1))
    return F.conv2d(q, g.view(1, 1, 1, win)).squeeze(1)


def ssim_maps(a, s, g, C1, C2):
    """(l, cs) maps over the valid positions of planes ``a`` and ``s`` (N, X, Y)"""
    mu_a, mu_s = windowed(a, g), windowed(s, g)
    var_a = windowed(a * a, g) - mu_a * mu_a
    var_s = windowed(s * s, g) - mu_s * mu_s
    cov = windowed(a * s, g) - mu_a * mu_s
    l = (2 * (mu_a * mu_s) + C1) / ((mu_a * mu_a + mu_s * mu_s) + C1)
    cs = (2 * cov + C2) / ((var_a + var_s) + C2)
    return l, cs


def level_ssim_reference(HR, SR, TL, win: int = 11, sigma: float = 1.5, data_range: float = 2.0,
                         dtype=torch.float64) -> torch.Tensor:
    """The four sums of ``SSIM_SUMS`` per sample, level and component, composed from torch ops in ``dtype`` on the
    tensors' device: HR, SR, TL (B, C >= 3, X, Y, NZ; channels 0..2) -> float64 (B, NZ, 3, 4)."""
    B, _, X, Y, NZ = HR.shape
    check_window(win, sigma, "level_ssim_reference")
    check_domain(X, Y, win, "level_ssim_reference")
    C1, C2 = constants(data_range)
    g = taps(win, sigma).to(device=HR.device, dtype=dtype)

    def planes(f):  # (B, 3, X, Y, NZ) -> (B * NZ * 3, X, Y)
        return f[:, :3].to(dtype).permute(0, 4, 1, 2, 3).reshape(B * NZ * 3, X, Y)

    a = planes(HR)
    cols = []
    for f in (SR, TL):
        l, cs = ssim_maps(a, planes(f), g, C1, C2)
        cols += [(l * cs).sum(dim=(1, 2), dtype=torch.float64), cs.sum(dim=(1, 2), dtype=torch.float64)]
    return torch.stack(cols, dim=-1).view(B, NZ, 3, len(SSIM_SUMS))


def ssim_from_sums(table, npos: int) -> dict:
    """Means from a table of sums (..., NZ, 3, 4) (a tensor or nested lists; leading axes, if any, and a sum of tables
    over ``n`` fields count as more planes: pass ``npos`` = positions per plane times n).  Returns Python floats and lists:

        ``levels``      (NZ, 4): the means over components and positions per level, in the order of ``SSIM_SUMS``
        ``mean``        (4,): the means over components, levels and positions
        ``components``  (3, 4): the means over levels and positions per component
    """
    t = torch.as_tensor(table, dtype=torch.float64)
    if t.dim() < 3 or tuple(t.shape[-2:]) != (3, len(SSIM_SUMS)):
        raise ValueError(f"ssim_from_sums wants a (..., NZ, 3, {len(SSIM_SUMS)}) table, not {tuple(t.shape)}")
    t = t.reshape(-1, t.shape[-3], 3, len(SSIM_SUMS)).sum(dim=0)
    NZ, n = t.shape[0], float(npos)
    return {"levels": (t.sum(dim=1) / (3 * n)).tolist(), "mean": (t.sum(dim=(0, 1)) / (3 * NZ * n)).tolist(),
            "components": (t.sum(dim=0) / (NZ * n)).tolist()}


def columns_from_sums(table, npos: int) -> list:
    """``SSIM_COLUMNS`` of one table of sums (NZ, 3, 4) over ``npos`` positions per plane"""
    m = ssim_from_sums(table, npos)
    return [m["mean"][0], m["mean"][2], m["mean"][1], m["mean"][3]] + [m["components"][c][0] for c in range(3)]
