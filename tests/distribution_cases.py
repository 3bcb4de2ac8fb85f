"""What tests/test_distribution.py and tests/test_distribution_gpu.py share: the parameter sets, the inputs, the special
voxels (those of tools/distribution_host_check.cpp) and an independent float64 classification (hypot, atan2, floor).
Every comparison of counts in those tests is exact; nothing here is a tolerance."""
import math

import numpy as np
import torch

UVW = 32.0
PARAMS = ((5, 4), (32, 16), (64, 36))  # (speed_bins, sectors)
CALMS = (0.0, 0.5)
NAN, INF = float("nan"), float("inf")


def special_voxels(speed_bins=32):
    """(u, v) pairs: the axis directions, the |u| = |v| ties, vectors on a bin edge (bin_width 1 at UVW_MAX 32), zeros,
    NaN, +-Inf, the smallest and the largest magnitudes"""
    e = 1.0 / 32.0
    return [(0.0, -0.25), (-0.25, 0.0), (0.0, 0.25), (0.25, 0.0),
            (0.25, 0.25), (-0.25, 0.25), (0.25, -0.25), (-0.25, -0.25),
            (e, 0.0), (2 * e, 0.0), (0.0, 3 * e), (-(speed_bins - 1) * e, 0.0),
            (0.0, 0.0), (-0.0, 0.0), (NAN, 0.1), (0.1, NAN), (NAN, NAN),
            (INF, 0.0), (0.0, -INF), (INF, INF), (-INF, INF), (INF, NAN), (1e-30, -1e-30), (3e38, 3e38)]


def tables(speed_bins=32, sectors=16, calm=0.5, bin_width=1.0, uvw=UVW):
    from gan_sr_wind_field_amd.distribution import distribution_tables

    return distribution_tables(uvw, bin_width, speed_bins, sectors, calm)


def fields(B, X, Y, NZ, seed, channels=(4, 3, 3), sd=0.25):
    """HR, SR, TL: gaussian wind of standard deviation ``sd`` in the first three channels, NaN in any further one (it
    must never be read); SR and TL are HR plus noise, so the three tables differ"""
    gen = torch.Generator().manual_seed(seed)
    HR = sd * torch.randn((B, 3, X, Y, NZ), generator=gen)
    out = []
    for k, c in enumerate(channels):
        f = HR + (0.05 * k) * torch.randn((B, 3, X, Y, NZ), generator=gen)
        if c > 3:
            f = torch.cat([f, torch.full((B, c - 3, X, Y, NZ), NAN)], dim=1)
        out.append(f.contiguous())
    return out


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


def plant_specials(fs, chunk, speed_bins):
    """the special voxels at the first and the last voxels of the volume and, where the levels split into chunks of
    ``chunk``, on both sides of the first chunk boundary of the first columns; another rotation per source"""
    vox = special_voxels(speed_bins)
    for s, f in enumerate(fs):
        B, _, X, Y, NZ = f.shape
        vol = X * Y * NZ
        plant(f, vox, 0, rot=s)
        plant(f, vox, vol - len(vox), rot=s + 5)
        if chunk < NZ:
            for k in range(min(X * Y, len(vox))):
                plant(f, vox[k:k + 2], k * NZ + chunk - 1, rot=0)
    return fs


def classify_f64(u, v, speed_bins, sectors, calm, bin_width=1.0, uvw=UVW):
    """The independent classification, in float64 with hypot / atan2 / floor -> (speed bin, sector, near) numpy arrays:
    ``near`` flags the voxels within 1e-4 m/s of a speed edge or of ``calm``, or within 1e-5 rad of a sector boundary."""
    u, v = np.asarray(u, dtype=np.float64) * uvw, np.asarray(v, dtype=np.float64) * uvw
    speed = np.hypot(u, v)
    x = speed / bin_width
    j = np.minimum(np.floor(x), speed_bins - 1).astype(np.int64)
    width = 2.0 * math.pi / sectors
    theta = np.arctan2(-u, -v)  # clockwise from +y, of where the wind comes from
    y = (theta + width / 2) / width
    sector = np.floor(y).astype(np.int64) % sectors
    sector = np.where(speed > calm, sector, sectors)
    near_edge = (np.abs(x - np.round(x)) * bin_width < 1e-4) & (np.round(x) >= 1) & (np.round(x) <= speed_bins - 1)
    near = near_edge | (np.abs(speed - calm) < 1e-4) | ((np.abs(y - np.round(y)) * width < 1e-5) & (speed > calm))
    return j, sector, near


def counts_f64(f, speed_bins, sectors, calm):
    """(counts (B, NZ, NS, ND + 1) float64, the number of flagged voxels) of one field by ``classify_f64``"""
    B, _, X, Y, NZ = f.shape
    j, sector, near = classify_f64(f[:, 0].numpy(), f[:, 1].numpy(), speed_bins, sectors, calm)
    T = speed_bins * (sectors + 1)
    base = (np.arange(B).reshape(B, 1, 1, 1) * NZ + np.arange(NZ)) * T
    idx = (base + j * (sectors + 1) + sector).reshape(-1)
    counts = np.bincount(idx, minlength=B * NZ * T).reshape(B, NZ, speed_bins, sectors + 1)
    return torch.from_numpy(counts.astype(np.float64)), int(near.sum())
