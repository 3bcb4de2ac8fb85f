"""Anti-aliased LR degradation ([DEGRADATION], opt-in): the low-resolution input is a blurred, then sampled copy of the
full-resolution channels instead of ``HR[:, ::s, ::s, :]``.  One definition for the CPU datasets
(``process_data.CustomizedDataset``, :func:`degrade_lr`) and the device-resident gather (``device_data.ResidentStore``,
csrc/data_gather.hip); both read the weight tables of :func:`axis_weights`, so their batches agree bit for bit.

Taps ``t[-R..R]``, symmetric and centred ON the sample point ``s * i`` (the LR voxels stay where the trilinear
baseline, the tiling and the network expect them):

* ``box``: ``R = s // 2``, all taps 1, the two end taps 1/2 for even ``s`` - a width-``s`` mean centred on the sample;
* ``gaussian``: ``R = ceil(3 sigma)``, ``t[d] = exp(-d^2 / (2 sigma^2))``, sigma in HR grid cells.

Per axis of extent ``n`` (the slice when slicing, else the domain) ``w[i, d] = t[d] / N(i)`` with ``N(i)`` the sum of
the taps inside ``[0, n)``, 0 outside; float64 on the host, rounded once to fp32.  The filter runs on the normalised fp32
full-resolution channel ``f`` of the slice, x pass first, fp32 throughout, every product and every sum rounded (no
fused multiply-add), taps ascending, accumulators from +0.0f, out-of-range taps skipped:

    g[i, y, z]  = sum_d fl(wx[i, d] * f[s i + d - R, y, z])
    LR[i, j, z] = sum_d fl(wy[j, d] * g[i, s j + d - R, z])

z is never filtered; rotation, the u / v exchange and the mirrors come after it; HR and Z are untouched.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

MAX_RADIUS = 32  # (WSR_DEGRADE_MAX_R of csrc/data_gather.hip)
KERNELS = ("box", "gaussian")
CHANNELS = ("all", "wind")


@dataclass(frozen=True)
class DegradationSpec:
    """What a dataset needs of [DEGRADATION]: picklable, so it travels to the loader's worker processes."""

    kernel: str
    sigma: Optional[float] = None
    channels: str = "all"

    def n_filt(self, cin: int) -> int:
        """number of leading LR channels that are filtered (the rest stay point-sampled)"""
        return min(3, cin) if self.channels == "wind" else cin


def taps(kernel: str, s: int, sigma: Optional[float] = None) -> np.ndarray:
    """the float64 taps ``t[-R..R]`` (length 2 R + 1) of ``kernel`` at coarseness ``s``"""
    if s < 1:
        raise ValueError(f"degradation: the coarseness factor must be >= 1, not {s}")
    if kernel == "box":
        R = s // 2
        t = np.ones(2 * R + 1, dtype=np.float64)
        if s % 2 == 0:
            t[0] = t[-1] = 0.5
    elif kernel == "gaussian":
        if sigma is None or not (0.0 < sigma <= 10.0):  # (NaN fails both)
            raise ValueError(f"degradation: sigma must be > 0 and <= 10, not {sigma}")
        R = int(math.ceil(3.0 * sigma))
        d = np.arange(-R, R + 1, dtype=np.float64)
        t = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    else:
        raise ValueError(f"degradation: kernel must be box or gaussian, not {kernel!r}")
    if R > MAX_RADIUS:
        raise ValueError(f"degradation: tap radius {R} > {MAX_RADIUS} ({kernel}, coarseness {s})")
    return t


def axis_weights(n: int, s: int, t: np.ndarray) -> np.ndarray:
    """fp32 (ceil(n / s), 2 R + 1): row ``i`` holds the taps around sample ``s * i`` divided by the sum of those inside
    ``[0, n)``, zeros at the ones outside"""
    t = np.asarray(t, dtype=np.float64)
    R = (t.size - 1) // 2
    if t.size != 2 * R + 1 or R > MAX_RADIUS:
        raise ValueError(f"degradation: taps must have odd length <= {2 * MAX_RADIUS + 1}, not {t.size}")
    i = np.arange(-(-n // s))
    pos = s * i[:, None] + np.arange(-R, R + 1)[None, :]
    w = np.where((pos >= 0) & (pos < n), t[None, :], 0.0)
    return (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


@lru_cache(maxsize=16)
def tables(spec: DegradationSpec, s: int, W: int, H: int):
    """(wx, wy, R): the fp32 weight tables of a ``W x H`` slice at coarseness ``s`` (read-only arrays)"""
    t = taps(spec.kernel, s, spec.sigma)
    wx, wy = axis_weights(W, s, t), axis_weights(H, s, t)
    wx.setflags(write=False)
    wy.setflags(write=False)
    return wx, wy, (t.size - 1) // 2


def _pass(f: np.ndarray, w: np.ndarray, s: int, R: int, axis: int) -> np.ndarray:
    """one 1-D pass along ``axis`` (1 or 2) of f (C, ., ., NZ): whole-array fp32 operations, one per tap"""
    n, n_out = f.shape[axis], w.shape[0]
    shape = list(f.shape)
    shape[axis] = n_out
    out = np.zeros(shape, dtype=np.float32)
    wshape = [1, 1, 1, 1]
    wshape[axis] = -1
    for d in range(2 * R + 1):
        # outputs whose tap d falls inside [0, n): s i + d - R >= 0 and <= n - 1
        lo = max(0, -(-(R - d) // s))
        hi = min(n_out, (n - 1 - d + R) // s + 1)
        if hi <= lo:
            continue
        src = [slice(None)] * 4
        dst = [slice(None)] * 4
        src[axis] = slice(s * lo + d - R, s * (hi - 1) + d - R + 1, s)
        dst[axis] = slice(lo, hi)
        prod = w[lo:hi, d].reshape(wshape) * f[tuple(src)]
        out[tuple(dst)] = out[tuple(dst)] + prod
    return out


def degrade_lr(f: np.ndarray, s: int, spec: DegradationSpec) -> np.ndarray:
    """fp32 (C, W, H, NZ) full-resolution LR channels of a slice -> fp32 (C, ceil(W / s), ceil(H / s), NZ): the first
    ``spec.n_filt(C)`` channels filtered as the module docstring defines, the others ``f[c, ::s, ::s]``"""
    if f.dtype != np.float32 or f.ndim != 4:
        raise ValueError(f"degrade_lr wants a float32 (C, W, H, NZ) array, got {f.dtype} {f.shape}")
    C, W, H, _ = f.shape
    wx, wy, R = tables(spec, int(s), W, H)
    nf = spec.n_filt(C)
    out = np.ascontiguousarray(f[:, ::s, ::s, :])
    if nf:
        out[:nf] = _pass(_pass(f[:nf], wx, s, R, 1), wy, s, R, 2)
    return out
