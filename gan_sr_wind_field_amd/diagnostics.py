"""Per-level evaluation diagnostics (``[DIAGNOSTICS]``): what ``run.py --test`` can report per z level on top of its
nine whole-volume metrics - wind speed, error-vector length, speed bias and absolute speed error, direction error, and
the rms divergence of the truth, the super-resolved field and the trilinear baseline.

Everything is built from fifteen sums per level over the X * Y columns of the level (``SUM_NAMES``): on a GPU
``hip_ops.level_diagnostics`` takes them in one pass (csrc/diagnostics.hip), ``level_sums_reference`` composes the same
sums from torch ops on any device (the path of a CPU device, and the oracle of the tests).  ``profile_from_sums`` turns
a table of sums into the columns of ``<name>____level_profile.csv``, defined once for both evaluation loops.
"""
from __future__ import annotations

import math

import torch

from .process_data import calculate_div_z, calculate_gradient_of_wind_field

#: the fifteen sums of one level, in the order of ``wsr_level_diagnostics``
SUM_NAMES = ("speed", "err", "err_tl", "speed_bias", "speed_bias_tl", "speed_abs", "speed_abs_tl", "hspeed",
             "hspeed_angle", "hspeed_angle_tl", "div_sq_hr", "div_sq_sr", "div_sq_tl", "altitude", "height")

#: the columns of the level profile, after ``level`` (and ``field`` in the per-field file)
PROFILE_COLUMNS = ("mean_altitude", "mean_height_above_lowest_level", "average_wind_speed", "pix", "trilinear_pix",
                   "speed_bias", "speed_bias_trilinear", "speed_abs_error", "speed_abs_error_trilinear",
                   "direction_error_deg", "direction_error_deg_trilinear", "rms_div_HR", "rms_div_SR",
                   "rms_div_trilinear")


def _divergence(f: torch.Tensor, x: torch.Tensor, y: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """du/dx + dv/dy + dw/dz of f (B, 3, X, Y, NZ) -> (B, X, Y, NZ): J0 + J4 + J8 of
    ``calculate_gradient_of_wind_field``.  An axis of length 1 has derivative 0 (``torch.gradient`` refuses it), and on a
    GPU the fused gradient is fp32 only: both cases take the torch expressions that function is made of, axis by axis."""
    _, _, X, Y, NZ = f.shape
    if min(X, Y, NZ) >= 2 and (not f.is_cuda or f.dtype == torch.float32):
        J = calculate_gradient_of_wind_field(f, x, y, Z)
        return J[:, 0] + J[:, 4] + J[:, 8]
    div = torch.zeros_like(f[:, 0])
    if X >= 2:
        div = div + torch.gradient(f[:, 0], dim=1, spacing=(x,))[0]
    if Y >= 2:
        div = div + torch.gradient(f[:, 1], dim=2, spacing=(y,))[0]
    if NZ >= 2:
        div = div + calculate_div_z(f[:, 2:3], Z)[:, 0]
    return div


def level_sums_reference(HR, SR, TL, x, y, Z, dtype=torch.float64) -> torch.Tensor:
    """The fifteen sums of ``SUM_NAMES`` per sample and level, composed from torch ops in ``dtype`` on the tensors'
    device: HR, SR, TL (B, C >= 3, X, Y, NZ; channels 0..2), the raw altitude Z (B, 1, X, Y, NZ), coordinates x (X),
    y (Y) -> (B, NZ, 15)."""
    h, s, t = (f[:, :3].to(dtype) for f in (HR, SR, TL))
    x, y, Z = x.to(dtype), y.to(dtype), Z.to(dtype)

    def norm(f):
        return torch.sqrt((f ** 2).sum(dim=1))

    def angle(a, b):
        cross = (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).abs()
        dot = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
        return torch.where((cross == 0) & (dot == 0), torch.zeros_like(dot), torch.atan2(cross, dot))

    nh, ns, nt = norm(h), norm(s), norm(t)
    hs = torch.sqrt(h[:, 0] ** 2 + h[:, 1] ** 2)
    z = Z[:, 0]
    terms = (nh, norm(h - s), norm(h - t), ns - nh, nt - nh, (ns - nh).abs(), (nt - nh).abs(), hs, hs * angle(h, s),
             hs * angle(h, t), _divergence(h, x, y, Z) ** 2, _divergence(s, x, y, Z) ** 2, _divergence(t, x, y, Z) ** 2,
             z, z - z[..., :1])
    return torch.stack([v.sum(dim=(1, 2)) for v in terms], dim=-1)


def profile_from_sums(sums, ncols, UVW_MAX) -> dict:
    """``PROFILE_COLUMNS`` as per-level lists of Python floats from a table ``sums`` (NZ, 15) (nested lists or a tensor)
    summed over ``ncols`` columns (X * Y times the number of fields).  Lengths and speeds in m/s (times ``UVW_MAX``),
    direction errors in degrees, weighted by the true horizontal speed (nan where that is 0 on the whole level), rms
    divergences in 1/s, altitudes as stored."""
    rows = sums.tolist() if torch.is_tensor(sums) else sums
    n, U = float(ncols), float(UVW_MAX)
    out = {k: [] for k in PROFILE_COLUMNS}
    for s in rows:
        s = [float(v) for v in s]
        deg = [(s[k] / s[7] * 180.0 / math.pi) if s[7] != 0 else math.nan for k in (8, 9)]
        vals = (s[13] / n, s[14] / n, s[0] / n * U, s[1] / n * U, s[2] / n * U, s[3] / n * U, s[4] / n * U, s[5] / n * U,
                s[6] / n * U, deg[0], deg[1], math.sqrt(s[10] / n) * U, math.sqrt(s[11] / n) * U,
                math.sqrt(s[12] / n) * U)
        for k, v in zip(PROFILE_COLUMNS, vals):
            out[k].append(v)
    return out
