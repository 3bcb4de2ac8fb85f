"""The energy-spectrum loss of generator training (``[SPECTRAL_LOSS]``): "put as much kinetic energy into every horizontal
wavenumber bin as the truth has there".  Every other content term of the generator (pix, the gradients, the divergences)
is a point-wise distance, which a blurred field minimises; this one compares the binned spectra ``[SPECTRUM]`` reports at
evaluation and prescribes no phases - the pixel term does.

Definitions.  Everything in the module docstring of ``spectra.py`` carries over unchanged: ``g = (f - m) w``,
``F(kx, ky)`` for ``ky = 0 .. Y // 2``, the Hermitian weight ``h``, the integer-decided ``bin``, ``NK``,
``scale = 1 / (2 X Y W2)`` and ``e_a(b, z, k) = scale * sum_comp sum_{modes in k} h |F_a|^2``.  New here:

    E(HR, SR) -> (B, NZ, NK, 2) float64 = [e_hr, e_sr]     channels 0..2 of each tensor are read, surplus ones never;
                                         only e_sr carries gradient, and only towards SR
    its vector-Jacobian product: given G(b, z, k) = dL / de_sr
        u(x, y) = sum_{kx} sum_{ky = 0 .. Y // 2} h(ky) G(bin(kx, ky)) Re( F_sr(kx, ky) exp(+2 pi i (kx x / X + ky y / Y)) )
        v = 2 scale w u
        dL/dSR(b, comp, x, y, z) = v - mean_plane(v)       the last term: the adjoint of the detrend
    the loss, composed in torch from the small (B, NZ, NK) tensors (its form stays editable here, its derivative autograd's):
        K = {k : k_min <= k <= k_max, mode_counts(X, Y)[k] > 0}        empty bins (1 x 8 has four above 0) are left out
        floor(b, z) = rel_floor * sum_k e_hr(b, z, k) + 1e-20          independent of SR
        r = log((e_sr + floor) / (e_hr + floor))
        L_spec = mean over (b, z, k in K) of r^2

``L_spec`` is a plain mean over samples: under data parallelism equal shards average exactly as ``pix`` does, and no
collective is added.  It is 0 for SR = HR, unchanged when a constant is added to any plane of SR, and ``(2 log a)^2`` for
SR = a HR where the floor is negligible.

On a GPU ``E`` is ``hip_ops.spectral_energy`` (csrc/spectral_loss.hip: the six-plane forward of the direct separable DFT
of csrc/spectra.hip and, as backward, the inverse transform above); on a CPU device, and under ``WSR_FUSED_SPECTRAL=0``,
``spectral_energy_reference`` composes it from ``torch.fft.rfft2`` and ``index_add_`` and autograd differentiates it.
"""
from __future__ import annotations

import functools
import os

import torch

from .config.config import SpectralLossConfig
from .spectra import WINDOWS, bin_index, hermitian_weight, mode_counts, n_bins, window_2d

#: the keys of ``[SPECTRAL_LOSS]`` and their defaults, as ``SpectralLossConfig`` declares them (``weight`` has none: the
#: user chooses it)
SPECTRAL_LOSS = {k: getattr(SpectralLossConfig, k) for k, _ in SpectralLossConfig._schema}
ABS_FLOOR = 1e-20


def fused() -> bool:
    """the run-time switch ``WSR_FUSED_SPECTRAL`` (0: the composed ``torch.fft`` path on every device)"""
    return os.environ.get("WSR_FUSED_SPECTRAL", "1") != "0"


def _select(counts, k_min, k_max, planes=""):
    """the non-empty bins k_min <= k <= k_max of ``counts`` (NK,) -> int64 (len K,) on the CPU; the one place the two keys
    are checked against NK"""
    counts = torch.as_tensor(counts).cpu()
    NK = counts.numel()
    k_min, k_max = int(k_min), int(k_max)
    last = NK - 1 if k_max == 0 else k_max
    if k_min < 1:
        raise ValueError(f"[SPECTRAL_LOSS] k_min must be >= 1, not {k_min}")
    if not k_min <= last < NK:
        raise ValueError(f"[SPECTRAL_LOSS] k_max = {k_max} must be 0 or in k_min = {k_min} .. NK - 1 = {NK - 1}{planes}")
    k = torch.arange(NK, dtype=torch.int64)
    K = k[(k >= k_min) & (k <= last) & (counts > 0)]
    if K.numel() == 0:
        raise ValueError(f"[SPECTRAL_LOSS] no mode{planes} lies in the bins k_min = {k_min} .. {last}")
    return K


def bin_set(X: int, Y: int, k_min: int = 1, k_max: int = 0) -> torch.Tensor:
    """K: the non-empty bins k_min <= k <= k_max of an X x Y plane -> int64 (len K,); ``k_max`` = 0: the last bin.
    Refuses ``k_min`` < 1 and a ``k_max`` outside k_min .. NK - 1 with the numbers."""
    return _select(mode_counts(X, Y), k_min, k_max, f" of {X} x {Y} planes")


def loss_from_energy(e: torch.Tensor, counts: torch.Tensor, k_min: int = 1, k_max: int = 0,
                     rel_floor: float = 1e-6) -> torch.Tensor:
    """``L_spec`` of the module docstring from ``e`` (B, NZ, NK, 2) = [e_hr, e_sr] and the modes per bin ``counts``
    (NK,) -> a scalar in ``e``'s dtype"""
    if torch.as_tensor(counts).numel() != e.shape[2]:
        raise ValueError(f"[SPECTRAL_LOSS] {torch.as_tensor(counts).numel()} mode counts for {e.shape[2]} bins")
    return _loss(e, _select(counts, k_min, k_max).to(e.device), rel_floor)


def _loss(e, K, rel_floor):
    e_hr, e_sr = e[..., 0].detach(), e[..., 1]
    floor = float(rel_floor) * e_hr.sum(dim=-1, keepdim=True) + ABS_FLOOR
    r = torch.log((e_sr.index_select(2, K) + floor) / (e_hr.index_select(2, K) + floor))
    return (r * r).mean()


@functools.lru_cache(maxsize=16)
def _bin_set_on(X, Y, k_min, k_max, device):
    return bin_set(X, Y, k_min, k_max).to(device)


def spectral_energy_reference(HR, SR, window: str = "hann", dtype=torch.float64) -> torch.Tensor:
    """``E(HR, SR)`` (B, NZ, NK, 2) composed from ``torch.fft.rfft2`` and ``index_add_`` in ``dtype`` on the tensors'
    device, differentiable by autograd: the path of a CPU device and of ``WSR_FUSED_SPECTRAL=0``"""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, not {window!r}")
    B, _, X, Y, NZ = HR.shape
    dev = HR.device
    w64 = window_2d(X, Y, window)
    W2 = float((w64 ** 2).sum())
    w = w64.to(device=dev, dtype=dtype).view(1, 1, 1, X, Y)
    h = hermitian_weight(Y).to(device=dev, dtype=dtype)
    idx = bin_index(X, Y).flatten().to(dev)
    es = []
    for f in (HR.detach(), SR):
        f = f[:, :3].to(dtype).permute(0, 1, 4, 2, 3)  # (B, 3, NZ, X, Y)
        F = torch.fft.rfft2((f - f.mean(dim=(-2, -1), keepdim=True)) * w)
        modes = ((F.real ** 2 + F.imag ** 2) * h).sum(dim=1).reshape(B, NZ, -1)
        es.append(torch.zeros((B, NZ, n_bins(X, Y)), dtype=dtype, device=dev).index_add(2, idx, modes))
    return torch.stack(es, dim=-1) * (0.5 / (X * Y * W2))


def spectral_energy(HR, SR, window: str = "hann") -> torch.Tensor:
    """``E(HR, SR)``: the kernel pair on a GPU; the reference under ``WSR_FUSED_SPECTRAL=0`` (in fp32 on the device, the
    precision of the kernels' transforms) and on a CPU device (in float64); always float64 out"""
    if HR.is_cuda and fused():
        from . import hip_ops
        return hip_ops.spectral_energy(HR, SR, window)
    return spectral_energy_reference(HR, SR, window, dtype=torch.float32 if HR.is_cuda else torch.float64).double()


def spectral_loss(HR, SR, cfg_section) -> torch.Tensor:
    """``L_spec`` (un-weighted, a float32 scalar) of a batch ``HR``, ``SR`` (B, C >= 3, X, Y, NZ) under the keys of
    ``cfg_section`` (``window``, ``k_min``, ``k_max``, ``rel_floor``: a ``SpectralLossConfig`` or anything with those
    attributes); ``k_max`` is checked against NK of these planes here, at the first batch."""
    X, Y = int(HR.shape[2]), int(HR.shape[3])
    K = _bin_set_on(X, Y, int(cfg_section.k_min), int(cfg_section.k_max), HR.device)  # (refuses a k_max >= NK)
    return _loss(spectral_energy(HR, SR, cfg_section.window), K, cfg_section.rel_floor).float()
