"""Tiled whole-domain inference ([TILE]; ``--tile`` of ESRGAN / Real-ESRGAN / BasicSR): the domain is cut into
overlapping tiles in x and y, the generator runs on stacked tiles of the size it was trained on, and the outputs are
blended with a feathering window.  The forward's memory then follows ``tiles_per_forward``, not the domain, and the
network sees the geometry it saw in training.  z is never tiled: the network never up-scales it.

Geometry (``tile_starts``): an axis of ``N`` LR voxels no longer than ``tile`` is one tile of ``N``.  Otherwise
``n = ceil((N - overlap) / (tile - overlap))`` tiles start at ``(i * (N - tile) + (n - 1) // 2) // (n - 1)``: the first
at 0, the last at ``N - tile``, evenly spread and rounded, neighbours overlapping by at least ``overlap``, no coordinate
under more than three tiles.

Blend (``csrc/tiling.hip``, the rule is stated in ``include/windsr_hip.h``): at HR resolution the weight of a tile on one
axis ramps 1, 2, .. ``overlap * scale`` + 1 from each edge that is not the domain's border, the weight of a tile is the
product of both axes', and its share the product of the two axes' normalised weights.  ``overlap = 0`` gives hard seams
(and plain averages where rounded origins make tiles overlap anyway).  The seam map ``sum alpha_T (x_T - out)^2`` says
how far the tiles disagree where they overlap; it is exactly 0 where one tile covers a voxel.
"""
from __future__ import annotations

from typing import Callable, List

from torch import Tensor


def _check(tile, overlap) -> None:
    if isinstance(tile, bool) or not isinstance(tile, int) or tile < 1:
        raise ValueError(f"tile must be an integer >= 1, not {tile!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap <= tile // 2:
        raise ValueError(f"overlap must be an integer in 0 .. tile // 2 = {tile // 2}, not {overlap!r}")


def tile_starts(N: int, tile: int, overlap: int) -> List[int]:
    """origins, in LR voxels, of the tiles along an axis of ``N`` voxels"""
    _check(tile, overlap)
    if isinstance(N, bool) or not isinstance(N, int) or N < 1:
        raise ValueError(f"N must be an integer >= 1, not {N!r}")
    if N <= tile:
        return [0]
    step = tile - overlap
    n = (N - overlap + step - 1) // step
    return [(i * (N - tile) + (n - 1) // 2) // (n - 1) for i in range(n)]


def tiled_forward(fn: Callable[[Tensor, Tensor], Tensor], LR: Tensor, Z: Tensor, scale: int, tile: int, overlap: int,
                  tiles_per_forward: int, with_seam: bool = False):
    """``fn`` on overlapping tiles of ``LR`` (B, C, Xl, Yl, NZ) and of the terrain tensor ``Z`` (B, 1, Xl * scale,
    Yl * scale, NZ), blended into one field.  The tiles are row-major, ``T = ix * ny + iy``; per chunk of at most
    ``tiles_per_forward`` of them the LR tiles and the terrain tiles come from one launch each, ``fn`` is called ONCE on
    the stacked batch ``(n_chunk * B, ...)`` (tile-major) and its (n_chunk * B, 3, tx * scale, ty * scale, NZ) output is
    kept as fp32; one stitch launch after the last chunk.  -> ``SR`` (B, 3, Xl * scale, Yl * scale, NZ), or
    ``(SR, seam)``.

    ``fn`` may return a tuple of such tensors (a mean and a variance): every one is stitched by the same kernel and a
    tuple comes back in place of ``SR``; the seam is that of the first."""
    _check(tile, overlap)
    s = int(scale)
    if isinstance(tiles_per_forward, bool) or not isinstance(tiles_per_forward, int) or tiles_per_forward < 1:
        raise ValueError(f"tiles_per_forward must be an integer >= 1, not {tiles_per_forward!r}")
    if LR.dim() != 5 or Z.dim() != 5 or s < 1 or tuple(Z.shape) != (LR.shape[0], 1, LR.shape[2] * s, LR.shape[3] * s,
                                                                   LR.shape[4]):
        raise ValueError(f"tiled_forward wants LR (B, C, X, Y, NZ) and Z (B, 1, X * {s}, Y * {s}, NZ), got "
                         f"{tuple(LR.shape)} and {tuple(Z.shape)}")
    import torch

    from . import hip_ops

    B, _, Xl, Yl, NZ = LR.shape
    xs, ys = tile_starts(Xl, tile, overlap), tile_starts(Yl, tile, overlap)
    tx, ty = min(tile, Xl), min(tile, Yl)
    origins = [(x, y) for x in xs for y in ys]
    want = (3, tx * s, ty * s, NZ)
    bufs = None
    multi = False
    for k0 in range(0, len(origins), tiles_per_forward):
        chunk = origins[k0:k0 + tiles_per_forward]
        n = len(chunk)
        x0, y0 = [x for x, _ in chunk], [y for _, y in chunk]
        LR_t = hip_ops.tile_gather(LR, x0, y0, tx, ty)
        Z_t = hip_ops.tile_gather(Z, [x * s for x in x0], [y * s for y in y0], tx * s, ty * s)
        res = fn(LR_t.view((n * B,) + tuple(LR_t.shape[2:])), Z_t.view((n * B,) + tuple(Z_t.shape[2:])))
        multi = isinstance(res, (tuple, list))
        res = tuple(res) if multi else (res,)
        for out in res:
            if not torch.is_tensor(out) or tuple(out.shape) != (n * B,) + want:
                got = tuple(out.shape) if torch.is_tensor(out) else type(out).__name__
                raise ValueError(f"tiled_forward: fn returned {got} for a batch of {n} tiles x {B}, wanted "
                                 f"{(n * B,) + want}")
        if bufs is None:
            bufs = [torch.empty((len(origins), B) + want, dtype=torch.float32, device=LR.device) for _ in res]
        for buf, out in zip(bufs, res):
            buf[k0:k0 + n] = out.detach().float().view((n, B) + want)
    hx, hy = [x * s for x in xs], [y * s for y in ys]
    R = overlap * s
    first = hip_ops.tile_stitch(bufs[0], hx, hy, Xl * s, Yl * s, R, R, with_seam=with_seam)
    SR, seam = first if with_seam else (first, None)
    if multi:
        SR = (SR,) + tuple(hip_ops.tile_stitch(b, hx, hy, Xl * s, Yl * s, R, R) for b in bufs[1:])
    return (SR, seam) if with_seam else SR
