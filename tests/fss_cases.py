"""What tests/test_fss.py and tests/test_fss_gpu.py share: the parameter sets, the inputs, the special voxels (those of
tools/fss_host_check.cpp) and a plain Python loop over the definition of ``fss.py``.  Every comparison of sums in those
tests is exact; nothing here is a tolerance."""
import math

import torch
import torch.nn.functional as F

UVW = 30.0
DEFAULT_SCALES = (1, 3, 5, 9, 17, 33)
#: (thresholds in m/s, scales)
PARAMS = (((10.0,), (1,)),
          ((5.0, 10.0, 15.0, 20.0), DEFAULT_SCALES),
          ((2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0), (1, 33)))
SHAPES = ((1, 5, 7, 3), (3, 16, 16, 10), (2, 33, 17, 37), (1, 8, 8, 130), (1, 70, 40, 2))
#: the seed of ``fields`` per shape (and of one more shape of the GPU tests): chosen so that at the thresholds 5, 10, 15,
#: 20 m/s every (sample, level) of every shape holds an event of HR or SR - checked with the CPU reference; seed 13 leaves
#: a level of the 8 x 8 x 130 shape without one at 20 m/s
SEEDS = (10, 11, 12, 14, 15, 16)
NAN, INF = float("nan"), float("inf")


def tables(thresholds=(5.0, 10.0, 15.0, 20.0), uvw=UVW):
    from gan_sr_wind_field_amd.fss import fss_tables

    return fss_tables(uvw, thresholds)


def fields(B, X, Y, NZ, seed, channels=(4, 3, 3), sd=0.3):
    """HR, SR, TL: HR gaussian wind of standard deviation ``sd`` in three channels (with ``UVW`` = 30 the thresholds 5, 10,
    15, 20 m/s have base rates of about 0.86, 0.54, 0.25 and 0.09), NaN in any further channel (it must never be read);
    SR is HR plus noise, TL a 3 x 3 horizontal box blur of HR"""
    gen = torch.Generator().manual_seed(seed)
    HR = sd * torch.randn((B, 3, X, Y, NZ), generator=gen)
    SR = HR + 0.05 * torch.randn((B, 3, X, Y, NZ), generator=gen)
    planes = HR.permute(0, 1, 4, 2, 3).reshape(B * 3 * NZ, 1, X, Y)
    TL = F.avg_pool2d(F.pad(planes, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
    TL = TL.reshape(B, 3, NZ, X, Y).permute(0, 1, 3, 4, 2)
    out = []
    for f, c in zip((HR, SR, TL), channels):
        if c > 3:
            f = torch.cat([f, torch.full((B, c - 3, X, Y, NZ), NAN)], dim=1)
        out.append(f.contiguous())
    return out


def special_voxels():
    """(u, v) pairs for thr2 = 2^-4 (``tie_tables``: UVW_MAX 32, threshold 8 m/s, an exact square): the tie itself, its
    neighbours in fp32, zeros, NaN, +-Inf, the smallest and the largest magnitudes"""
    below = float(torch.nextafter(torch.tensor(0.25), torch.tensor(0.0)))
    above = float(torch.nextafter(torch.tensor(0.25), torch.tensor(1.0)))
    return [(0.25, 0.0), (0.0, -0.25), (below, 0.0), (above, 0.0), (0.0, 0.0), (-0.0, 0.0), (NAN, 0.9), (0.9, NAN),
            (NAN, NAN), (INF, 0.0), (0.0, -INF), (-INF, INF), (INF, NAN), (1e-30, -1e-30), (3e38, 3e38), (0.125, 0.0)]


def tie_tables():
    """thresholds 4, 8, 12 m/s at UVW_MAX 32: thr2[1] = 2^-4 exactly, the square of u = 0.25"""
    return tables((4.0, 8.0, 12.0), 32.0)


def plant(f, voxels, at, rot=0):
    """writes ``voxels`` (rotated by ``rot``) into channels 0 and 1 of every sample of ``f`` at the flat (x, y, z) indices
    ``at``, ``at + 1``, ... (wrapping inside the volume)"""
    B, _, X, Y, NZ = f.shape
    vol = X * Y * NZ
    u, v = f[:, 0].reshape(B, vol), f[:, 1].reshape(B, vol)  # (views: f is contiguous)
    for k in range(len(voxels)):
        pu, pv = voxels[(k + rot) % len(voxels)]
        u[:, (at + k) % vol], v[:, (at + k) % vol] = pu, pv
    return f


def plant_specials(fs, tile, chunk):
    """the special voxels at the first and the last voxels of the volume and, where the plane has more than one tile or
    the levels more than one chunk, on either side of the first tile boundary along x and along y and of the first chunk
    boundary; another rotation per source"""
    vox = special_voxels()
    for s, f in enumerate(fs):
        B, _, X, Y, NZ = f.shape
        plant(f, vox, 0, rot=s)
        plant(f, vox, X * Y * NZ - len(vox), rot=s + 5)
        for k in range(len(vox)):
            pair = [vox[(k + s) % len(vox)], vox[(k + s + 1) % len(vox)]]
            if X > tile:  # (tile - 1, y, z) and (tile, y, z)
                for d in (0, 1):
                    plant(f, pair[d:d + 1], ((tile - 1 + d) * Y + k % Y) * NZ + k % NZ)
            if Y > tile:
                for d in (0, 1):
                    plant(f, pair[d:d + 1], ((k % X) * Y + tile - 1 + d) * NZ + (k + 1) % NZ)
            if chunk < NZ:  # (x, y, chunk - 1) and (x, y, chunk): consecutive in memory
                plant(f, pair, (k % (X * Y)) * NZ + chunk - 1)
    return fs


def loop_reference(HR, SR, TL, thr2, scales):
    """The definition of ``fss.py`` in plain Python on nested lists: hs2 from torch in fp32 and compared as the
    exact doubles of those values, every box clipped to the plane position by position -> float64 (B, NZ, NT, NN, 5).  For tiny shapes."""
    B, _, X, Y, NZ = HR.shape
    nt, nn = len(thr2), len(scales)
    out = torch.zeros((B, NZ, nt, nn, 5), dtype=torch.float64)
    hs2 = []
    for f in (HR, SR, TL):
        if f is None:
            hs2.append(None)
            continue
        u, v = f[:, 0].float(), f[:, 1].float()
        hs2.append(((u * u) + (v * v)).tolist())
    thr = [float(t) for t in thr2]
    for b in range(B):
        for z in range(NZ):
            for t in range(nt):
                ev = [None if h is None else [[1 if h[b][x][y][z] >= thr[t] else 0 for y in range(Y)] for x in range(X)]
                      for h in hs2]
                for k, n in enumerate(scales):
                    r = (n - 1) // 2
                    sums = [0] * 5
                    for x in range(X):
                        for y in range(Y):
                            c = [0 if e is None else sum(e[xx][yy] for xx in range(max(0, x - r), min(X, x + r + 1))
                                                         for yy in range(max(0, y - r), min(Y, y + r + 1))) for e in ev]
                            sums[0] += c[0] ** 2
                            sums[1] += c[1] ** 2
                            sums[2] += (c[1] - c[0]) ** 2
                            if ev[2] is not None:
                                sums[3] += c[2] ** 2
                                sums[4] += (c[2] - c[0]) ** 2
                    out[b, z, t, k] = torch.tensor(sums, dtype=torch.float64)
    return out


def is_nan(v):
    return isinstance(v, float) and math.isnan(v)
