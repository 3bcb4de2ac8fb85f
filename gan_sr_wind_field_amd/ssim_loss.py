"""The SSIM loss of generator training (``[SSIM_LOSS]``): "be structurally similar to the truth on every horizontal plane".
Every other content term of the generator (pix, the gradients, the divergences) is a point-wise distance, which a blurred
field minimises, and ``[SPECTRAL_LOSS]`` says how much energy a wavenumber bin holds but not where it sits; the
contrast-structure factor ``cs`` of SSIM is the local quantity that falls for a blurred field and for misplaced detail.
This is the quantity ``[SSIM]`` reports at evaluation and in validation, made trainable.

Definitions.  Everything in the module docstring of ``ssim.py`` carries over unchanged: the taps ``g``, the valid
positions only (``npos`` per plane, no padding), z never windowed, the five windowed moments, ``l``, ``cs``, ``C1`` and
``C2``.  New here:

    P(HR, SR) -> (B, NZ, 3, 2) float64 = [sum over the valid positions of l cs, sum of cs]   per sample, level, component;
                 channels 0..2 of each tensor are read, surplus ones never; gradient flows only towards SR, from both
                 columns
    its vector-Jacobian product: given G0 = dL/dP[b, z, c, 0], G1 = dL/dP[b, z, c, 1] and, per valid position,
        D1 = mu_a^2 + mu_s^2 + C1,  D2 = var_a + var_s + C2,  h = G0 l + G1
        alpha = G0 cs (2 mu_a - 2 mu_s l) / D1 + h (2 mu_s cs - 2 mu_a) / D2      (through mu_s)
        beta  = -h cs / D2                                                         (through S_ss)
        gamma = 2 h / D2                                                           (through S_as)
        dL/dSR(p) = (g2^T alpha)(p) + 2 s(p) (g2^T beta)(p) + a(p) (g2^T gamma)(p)
        (g2^T m)(px, py) = sum_{i, j} g[i] g[j] m(px - i, py - j) over the valid positions (px - i, py - j): a pixel near
        a plane border lies in fewer windows; nothing is padded or renormalised
    the loss, composed in torch from the small table (its form stays editable here, its derivative autograd's):
        L_ssim = 1 - P[..., 0].sum() / (3 B NZ npos)

``L_ssim`` is a plain mean over samples: under data parallelism equal shards average exactly as ``pix`` does, and no
collective is added.  It is exactly 0 for SR = HR (bit for bit) and lies in (0, 2) otherwise.

On a GPU ``P`` is ``hip_ops.ssim_pair_sums`` (csrc/ssim_loss.hip: the tile kernel of csrc/ssim.hip without the baseline -
both columns carry the bits of ``level_ssim``'s ``ssim_sr`` and ``cs_sr``, so the trained quantity is the logged one -
and, as backward, one launch that recomputes the moments around a tile of pixels); on a CPU device, and under
``WSR_FUSED_SSIM_LOSS=0``, ``pair_sums_reference`` composes it from ``ssim.ssim_maps`` and autograd differentiates it.
"""
from __future__ import annotations

import os

import torch

from . import ssim
from .config.config import SsimLossConfig

#: the keys of ``[SSIM_LOSS]`` and their defaults, as ``SsimLossConfig`` declares them (``weight`` has none)
SSIM_LOSS = {k: getattr(SsimLossConfig, k) for k, _ in SsimLossConfig._schema}
WHAT = "[SSIM_LOSS] window_size"


def fused() -> bool:
    """the run-time switch ``WSR_FUSED_SSIM_LOSS`` (0: the composed torch path on every device)"""
    return os.environ.get("WSR_FUSED_SSIM_LOSS", "1") != "0"


def pair_sums_reference(HR, SR, win: int = 11, sigma: float = 1.5, data_range: float = 2.0,
                        dtype=torch.float64) -> torch.Tensor:
    """``P(HR, SR)`` (B, NZ, 3, 2) composed from ``ssim.ssim_maps`` in ``dtype`` on the tensors' device, differentiable by
    autograd: the path of a CPU device and of ``WSR_FUSED_SSIM_LOSS=0``"""
    B, _, X, Y, NZ = HR.shape
    ssim.check_window(win, sigma, "ssim_loss.pair_sums_reference")
    ssim.check_domain(X, Y, win, WHAT)
    C1, C2 = ssim.constants(data_range)
    g = ssim.taps(win, sigma).to(device=HR.device, dtype=dtype)

    def planes(f):  # (B, C, X, Y, NZ) -> (B * NZ * 3, X, Y)
        return f[:, :3].to(dtype).permute(0, 4, 1, 2, 3).reshape(B * NZ * 3, X, Y)

    l, cs = ssim.ssim_maps(planes(HR.detach()), planes(SR), g, C1, C2)
    cols = [(l * cs).sum(dim=(1, 2), dtype=torch.float64), cs.sum(dim=(1, 2), dtype=torch.float64)]
    return torch.stack(cols, dim=-1).view(B, NZ, 3, 2)


def pair_sums(HR, SR, win: int = 11, sigma: float = 1.5, data_range: float = 2.0) -> torch.Tensor:
    """``P(HR, SR)``: the kernel pair on a GPU; the reference under ``WSR_FUSED_SSIM_LOSS=0`` (in fp32 on the device, the
    precision of the kernels) and on a CPU device (in float64); always float64 out"""
    if HR.is_cuda and fused():
        from . import hip_ops
        return hip_ops.ssim_pair_sums(HR, SR, win, sigma, data_range)
    return pair_sums_reference(HR, SR, win, sigma, data_range,
                               dtype=torch.float32 if HR.is_cuda else torch.float64).double()


def loss_from_sums(P: torch.Tensor, npos: int) -> torch.Tensor:
    """``L_ssim`` of the module docstring from ``P`` (B, NZ, 3, 2) and the positions per plane -> a scalar in P's dtype"""
    return 1.0 - P[..., 0].sum() / float(3 * P.shape[0] * P.shape[1] * npos)


def ssim_loss(HR, SR, cfg_section) -> torch.Tensor:
    """``L_ssim`` (un-weighted, a float32 scalar) of a batch ``HR``, ``SR`` (B, C >= 3, X, Y, NZ) under the keys of
    ``cfg_section`` (``window_size``, ``sigma``, ``data_range``: a ``SsimLossConfig`` or anything with those attributes);
    the window is checked against these planes here, at the first batch."""
    X, Y, win = int(HR.shape[2]), int(HR.shape[3]), int(cfg_section.window_size)
    ssim.check_domain(X, Y, win, WHAT)
    P = pair_sums(HR, SR, win, float(cfg_section.sigma), float(cfg_section.data_range))
    return loss_from_sums(P, ssim.n_positions(X, Y, win)).float()
