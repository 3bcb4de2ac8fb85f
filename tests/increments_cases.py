"""What tests/test_increments.py and tests/test_increments_gpu.py share: the separation lists, the shapes, the inputs,
a plain Python loop over the definition of ``increments.py`` and the fields of the exact identities.  Nothing here is a
tolerance."""
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
#: the separation lists of every comparison: one, the powers of two, and a list most of which has no pairs in a small plane
LISTS = ((1,), (1, 2, 4, 8), (1, 2, 3, 5, 8, 13, 21, 32))
#: (B, X, Y, NZ) of the GPU tests: smaller than a tile, the reference's patch, odd sizes with a second tile along x, more
#: levels than any chunk, three tiles along x and two along y, a y direction without pairs, one level, a second tile in
#: both directions, many level chunks under four tiles, and three tiles in both directions with a remainder in every tile
#: and in the last level chunk of every separation list (17 levels in chunks of 9, 6 and 3)
SHAPES = ((2, 7, 6, 5), (1, 16, 16, 10), (1, 33, 17, 37), (1, 8, 8, 130), (1, 70, 40, 2), (1, 3, 1, 4), (1, 5, 4, 1),
          (1, 40, 40, 8), (1, 35, 35, 200), (2, 65, 66, 17))
#: the seed of ``fields`` per shape; with gaussian components every S2 entry with pairs is strictly positive - checked with
#: the CPU reference in tests/test_increments.py
SEEDS = tuple(range(40, 40 + len(SHAPES)))


def fields(B, X, Y, NZ, seed, channels=(4, 3, 3), independent=False, sd=0.3):
    """HR, SR, TL: HR gaussian wind of standard deviation ``sd`` in three channels, NaN in any further channel (it must
    never be read); SR is HR plus 1e-3 noise or, with ``independent``, another gaussian field; TL a 3 x 3 horizontal box
    blur of HR"""
    gen = torch.Generator().manual_seed(seed)
    HR = sd * torch.randn((B, 3, X, Y, NZ), generator=gen)
    noise = torch.randn((B, 3, X, Y, NZ), generator=gen)
    SR = sd * noise if independent else HR + 1e-3 * noise
    planes = HR.permute(0, 1, 4, 2, 3).reshape(B * 3 * NZ, 1, X, Y)
    TL = F.avg_pool2d(F.pad(planes, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
    TL = TL.reshape(B, 3, NZ, X, Y).permute(0, 1, 3, 4, 2)
    out = []
    for f, c in zip((HR, SR, TL), channels):
        if c > 3:
            f = torch.cat([f, torch.full((B, c - 3, X, Y, NZ), NAN)], dim=1)
        out.append(f.contiguous())
    return out


def loop_reference(HR, SR, TL, separations):
    """The definition of ``increments.py`` in plain Python on nested lists: the fp32 values as exact doubles, every pair
    visited one by one, Python float arithmetic (float64) -> (B, NZ, 3, R, 2, 3, 3).  For tiny shapes."""
    B, _, X, Y, NZ = HR.shape
    out = torch.zeros((B, NZ, 3, len(separations), 2, 3, 3), dtype=torch.float64)
    for s, f in enumerate((HR, SR, TL)):
        if f is None:
            continue
        v = f[:, :3].double().tolist()
        for b in range(B):
            for z in range(NZ):
                for k, r in enumerate(separations):
                    for a, (dx, dy) in enumerate(((r, 0), (0, r))):
                        for kind in range(3):
                            c = 2 if kind == 2 else (kind if a == 0 else 1 - kind)
                            sums = [0.0, 0.0, 0.0]
                            for x in range(X - dx):
                                for y in range(Y - dy):
                                    delta = v[b][c][x + dx][y + dy][z] - v[b][c][x][y][z]
                                    q = delta * delta
                                    sums[0] += q
                                    sums[1] += q * delta
                                    sums[2] += q * q
                            out[b, z, s, k, a, kind] = torch.tensor(sums, dtype=torch.float64)
    return out


def pairs_table(X, Y, separations):
    """(R, 2) float64: the pairs of every (separation, direction)"""
    return torch.tensor([[max(X - r, 0) * Y, X * max(Y - r, 0)] for r in separations], dtype=torch.float64)


def ramp_field(B, X, Y, NZ):
    """u = 2^-6 i along x, v = w = 0: every x increment of u is r 2^-6, exactly, and every power a power of two times an
    integer"""
    f = torch.zeros((B, 3, X, Y, NZ))
    f[:, 0] = (torch.arange(X, dtype=torch.float32) * 2.0 ** -6)[None, :, None, None]
    return f


def alternating_field(B, X, Y, NZ):
    """u = 2^-3 (-1)^i along x: delta = +-2^-2 at odd r and 0 at even r"""
    f = torch.zeros((B, 3, X, Y, NZ))
    f[:, 0] = (0.125 * (1 - 2 * (torch.arange(X) % 2)).float())[None, :, None, None]
    return f


def is_nan(v):
    return isinstance(v, float) and math.isnan(v)
