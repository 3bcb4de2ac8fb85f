"""[TILE] on the CPU: the tile origins, the config section, test.py's switch, and the float64 reference of the blend the
kernels of csrc/tiling.hip are held to on the GPU (tests/test_tiling_gpu.py imports it from here).

The weight rule (include/windsr_hip.h), restated here and nowhere else in the tests.  On one axis a tile at origin ``a``
of side ``T`` on an axis of length ``N`` with ramp ``R`` weighs ``w(p) = min(L(p), Rr(p))`` at ``p = i - a``:
``L(p) = R + 1`` if ``a == 0`` else ``min(p + 1, R + 1)``, ``Rr(p) = R + 1`` if ``a + T == N`` else
``min(T - p, R + 1)``.  The share of tile ``(ix, iy)`` is ``(wx / Wx) * (wy / Wy)``, ``Wx`` the sum of ``wx`` over the x
tiles covering ``i``; ``out = sum alpha x``, ``seam = sum alpha (x - out)^2``.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_ema import SHIPPED

CFG_DIR = os.path.join(REPO, "gan_sr_wind_field_amd", "config")
LOCAL_INI = os.path.join(CFG_DIR, "wind_field_GAN_3D_config_local.ini")


# ------------------------------------------------------------------------------------------------- shared references
def axis_weights(starts, T, N, R):
    """(n, N) float64: the integer weight of every tile of an axis at every coordinate, 0 outside the tile"""
    w = np.zeros((len(starts), N))
    for k, a in enumerate(starts):
        for p in range(T):
            left = R + 1 if a == 0 else min(p + 1, R + 1)
            right = R + 1 if a + T == N else min(T - p, R + 1)
            w[k, a + p] = min(left, right)
    return w


def shares(xs, ys, X, Y, Tx, Ty, Rx, Ry):
    """alpha (nx, ny, X, Y) float64 - one division of exact integers per share - and the cover count (X, Y)"""
    wx, wy = axis_weights(xs, Tx, X, Rx), axis_weights(ys, Ty, Y, Ry)
    assert (wx.sum(0) >= 1).all() and (wy.sum(0) >= 1).all(), "an origin list that leaves a coordinate uncovered"
    num = wx[:, None, :, None] * wy[None, :, None, :]
    alpha = num / (wx.sum(0)[:, None] * wy.sum(0)[None, :])
    ncov = (wx > 0).sum(0)[:, None] * (wy > 0).sum(0)[None, :]
    return alpha, ncov


def ref_stitch(tiles, xs, ys, X, Y, Rx, Ry):
    """float64 blend of ``tiles`` (nx * ny, B, C, Tx, Ty, NZ), tile ``ix * ny + iy`` at ``(xs[ix], ys[iy])``.
    -> dict: ``out``, ``seam`` (B, C, X, Y, NZ); ``A_out = sum alpha |x|`` and ``A_seam = sum alpha (|x| + |out|)^2``, the
    magnitudes the bounds of the GPU tests scale with; ``ncov`` (X, Y) the number of tiles over every column"""
    tiles = np.asarray(tiles, dtype=np.float64)
    n, B, C, Tx, Ty, NZ = tiles.shape
    assert n == len(xs) * len(ys)
    alpha, ncov = shares(xs, ys, X, Y, Tx, Ty, Rx, Ry)
    out, A_out = np.zeros((B, C, X, Y, NZ)), np.zeros((B, C, X, Y, NZ))
    each = [(ix, iy, slice(a, a + Tx), slice(b, b + Ty)) for ix, a in enumerate(xs) for iy, b in enumerate(ys)]
    for ix, iy, sx, sy in each:
        al = alpha[ix, iy, sx, sy][None, None, :, :, None]
        out[:, :, sx, sy] += al * tiles[ix * len(ys) + iy]
        A_out[:, :, sx, sy] += al * np.abs(tiles[ix * len(ys) + iy])
    seam, A_seam = np.zeros_like(out), np.zeros_like(out)
    for ix, iy, sx, sy in each:
        al = alpha[ix, iy, sx, sy][None, None, :, :, None]
        t = tiles[ix * len(ys) + iy]
        seam[:, :, sx, sy] += al * (t - out[:, :, sx, sy]) ** 2
        A_seam[:, :, sx, sy] += al * (np.abs(t) + np.abs(out[:, :, sx, sy])) ** 2
    return {"out": out, "seam": seam, "A_out": A_out, "A_seam": A_seam, "ncov": ncov}


def cut_tiles(F, xs, ys, Tx, Ty):
    """the tiles of one field (B, C, X, Y, NZ), row-major -> (nx * ny, B, C, Tx, Ty, NZ)"""
    return np.stack([F[:, :, a:a + Tx, b:b + Ty] for a in xs for b in ys])


def _ini_with(tmp_path, extra: str, name="c.ini") -> str:
    with open(LOCAL_INI) as f:
        text = f.read()
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text + "\n" + extra)
    return path


# ------------------------------------------------------------------------------------------------- 1. tile origins
def test_tile_starts_properties_for_every_small_case():
    from gan_sr_wind_field_amd.tiling import tile_starts

    cases = 0
    for N in range(1, 61):
        for tile in range(1, 17):
            for overlap in range(0, tile // 2 + 1):
                s = tile_starts(N, tile, overlap)
                cases += 1
                if N <= tile:
                    assert s == [0], (N, tile, overlap)
                    continue
                key = (N, tile, overlap, s)
                assert s[0] == 0, key
                assert s[-1] == N - tile, key
                assert all(b > a for a, b in zip(s, s[1:])), key
                assert all(b - a <= tile - overlap for a, b in zip(s, s[1:])), key
                assert len(s) == -(-(N - overlap) // (tile - overlap)), key
                cover = np.zeros(N, dtype=int)
                for a in s:
                    cover[a:a + tile] += 1
                assert cover.min() >= 1 and cover.max() <= 3, key
    assert cases == 4800


def test_tile_starts_sample_values():
    from gan_sr_wind_field_amd.tiling import tile_starts

    assert tile_starts(13, 8, 4) == [0, 3, 5]
    assert tile_starts(11, 4, 1) == [0, 2, 5, 7]
    assert tile_starts(32, 16, 4) == [0, 8, 16]
    assert tile_starts(8, 8, 4) == [0] and tile_starts(5, 8, 4) == [0]


def test_tile_starts_refuses_bad_values_naming_the_key():
    from gan_sr_wind_field_amd.tiling import tile_starts

    for tile, overlap in ((8, 5), (1, 1), (8, -1), (7, 4)):
        with pytest.raises(ValueError, match="overlap"):
            tile_starts(20, tile, overlap)
    for tile in (0, -4, 2.5, None, True):
        with pytest.raises(ValueError, match="tile must be"):
            tile_starts(20, tile, 0)
    for N in (0, -3):
        with pytest.raises(ValueError, match="N must be"):
            tile_starts(N, 8, 2)


def test_tiled_forward_refuses_bad_arguments_before_it_touches_a_device():
    from gan_sr_wind_field_amd.tiling import tiled_forward

    LR, Z = torch.zeros(1, 4, 6, 6, 5), torch.zeros(1, 1, 24, 24, 5)
    with pytest.raises(ValueError, match="tiles_per_forward"):
        tiled_forward(lambda a, b: a, LR, Z, 4, 4, 1, 0)
    with pytest.raises(ValueError, match="overlap"):
        tiled_forward(lambda a, b: a, LR, Z, 4, 4, 3, 1)
    with pytest.raises(ValueError, match=r"\(1, 1, 24, 20, 5\)"):
        tiled_forward(lambda a, b: a, LR, torch.zeros(1, 1, 24, 20, 5), 4, 4, 1, 1)


# ------------------------------------------------------------------------------------------- 2. the reference blend
# (X, Y, tile, overlap, scale): overlap 0; a triple-coverage axis (13, 8, 4); one axis shorter than the tile; 3 x 3 tiles
REF_CASES = [(20, 12, 8, 0, 1), (13, 8, 8, 4, 1), (13, 6, 8, 4, 2), (11, 11, 4, 1, 3), (32, 32, 16, 4, 1)]


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reference_shares_sum_to_one_and_identical_tiles_give_the_field_back(case):
    from gan_sr_wind_field_amd.tiling import tile_starts

    Xl, Yl, tile, overlap, s = case
    X, Y, R = Xl * s, Yl * s, overlap * s
    xs, ys = [a * s for a in tile_starts(Xl, tile, overlap)], [a * s for a in tile_starts(Yl, tile, overlap)]
    Tx, Ty = min(tile, Xl) * s, min(tile, Yl) * s
    alpha, ncov = shares(xs, ys, X, Y, Tx, Ty, R, R)
    assert np.abs(alpha.sum((0, 1)) - 1.0).max() <= 1e-15
    assert (alpha >= 0).all() and ncov.min() >= 1 and ncov.max() <= 9
    single = ncov == 1
    assert (np.sort(alpha.reshape(-1, X, Y), axis=0)[-1][single] == 1.0).all()  # one tile: its share is exactly 1
    if (case[0], case[2], case[3]) == (13, 8, 4):
        assert ((axis_weights(xs, Tx, X, R) > 0).sum(0) == 3).any()  # the triple-coverage axis
    F = np.random.default_rng(sum(case)).standard_normal((2, 3, X, Y, 4))
    ref = ref_stitch(cut_tiles(F, xs, ys, Tx, Ty), xs, ys, X, Y, R, R)
    assert np.abs(ref["out"] - F).max() <= 1e-15
    assert ref["seam"].max() <= 1e-29 and (ref["seam"] >= 0).all()
    assert (ref["out"][:, :, single] == F[:, :, single]).all() and (ref["seam"][:, :, single] == 0).all()


def test_reference_weights_ramp_only_at_inner_edges_and_overlap_zero_is_a_hard_seam():
    # (13, 8, 4) at scale 1: origins 0, 3, 5; the first tile ramps down at its right edge only, the last up at its left
    w = axis_weights([0, 3, 5], 8, 13, 4)
    assert w[0].tolist() == [5, 5, 5, 5, 4, 3, 2, 1, 0, 0, 0, 0, 0]
    assert w[1].tolist() == [0, 0, 0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 0]
    assert w[2].tolist() == [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 5, 5, 5]
    # overlap 0 without rounding overlap: every coordinate under one tile, a hard seam
    w = axis_weights([0, 8, 16], 8, 24, 0)
    assert ((w > 0).sum(0) == 1).all() and set(np.unique(w)) == {0.0, 1.0}
    # overlap 0 where the rounded origins overlap anyway: a plain average
    alpha, ncov = shares([0, 6, 12], [0], 20, 4, 8, 4, 0, 0)
    assert (alpha[:2, 0, 6:8, 0] == 0.5).all() and (alpha[2, 0, 6:8, 0] == 0).all() and ncov[6, 0] == 2


# ---------------------------------------------------------------------------------------------------- 3. config
def test_file_without_the_section_prints_the_pinned_text():
    """every shipped ini prints the text pinned before the extensions existed (the digests of test_ema.py); a fresh
    interpreter, because the section objects are class-level singletons"""
    code = ("import json, os, sys\n"
            "from gan_sr_wind_field_amd.config.config import Config\n"
            "out = {}\n"
            "for name in sys.argv[2:]:\n"
            "    cfg = Config(os.path.join(sys.argv[1], name))\n"
            "    t = cfg.tile\n"
            "    assert t.present is False and (t.tile, t.overlap, t.tiles_per_forward, t.write_seam) == (None, 4, 8, False)\n"
            "    out[name] = cfg.asINI()\n"
            "print(json.dumps(out))\n")
    res = subprocess.run([sys.executable, "-c", code, CFG_DIR] + sorted(SHIPPED), cwd=REPO, check=True,
                         capture_output=True, text=True)
    texts = json.loads(res.stdout.strip().splitlines()[-1])
    for name, digest in SHIPPED.items():
        assert "TILE" not in texts[name] and "write_seam" not in texts[name], name
        assert hashlib.sha256(texts[name].encode()).hexdigest() == digest, name


def test_section_prints_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    plain = Config(LOCAL_INI).asINI()
    cfg = Config(_ini_with(tmp_path, "[TILE]\ntile = 16\n"))
    t = cfg.tile
    assert t.present and (t.tile, t.overlap, t.tiles_per_forward, t.write_seam) == (16, 4, 8, False)
    assert cfg.asINI() == plain + "\n[TILE]\ntile = 16\noverlap = 4\ntiles_per_forward = 8\nwrite_seam = False\n"
    cfg = Config(_ini_with(tmp_path, "[TILE]\n; LR voxels per tile side\ntile = 9\noverlap = 0\ntiles_per_forward = 3\n"
                                     "write_seam = True\n"))
    t = cfg.tile
    assert (t.tile, t.overlap, t.tiles_per_forward, t.write_seam) == (9, 0, 3, True)
    text = cfg.asINI()
    assert text == plain + "\n[TILE]\ntile = 9\noverlap = 0\ntiles_per_forward = 3\nwrite_seam = True\n"
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.tile) == vars(t) and again.asINI() == text
    # after [ENSEMBLE], the last of the optional sections so far
    both = Config(_ini_with(tmp_path, "[TILE]\ntile = 8\noverlap = 2\n[ENSEMBLE]\nmembers = 2\n")).asINI()
    assert both.endswith("\n[ENSEMBLE]\nmembers = 2\nwrite_spread = False\n"
                         "\n[TILE]\ntile = 8\noverlap = 2\ntiles_per_forward = 8\nwrite_seam = False\n")
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.tile.present is False and back.tile.tile is None and back.asINI() == plain


@pytest.mark.parametrize("body,key", [
    ("overlap = 2\n", "tile"),                           # tile missing
    ("tile = 0\n", "tile"), ("tile = -8\n", "tile"), ("tile = sixteen\n", "tile"), ("tile = 8.0\n", "tile"),
    ("tile = 8\noverlap = 5\n", "overlap"), ("tile = 8\noverlap = -1\n", "overlap"), ("tile = 1\noverlap = 1\n", "overlap"),
    ("tile = 7\noverlap = 4\n", "overlap"), ("tile = 8\noverlap = two\n", "overlap"),
    ("tile = 8\ntiles_per_forward = 0\n", "tiles_per_forward"), ("tile = 8\ntiles_per_forward = -2\n", "tiles_per_forward"),
    ("tile = 8\ntiles_per_forward = many\n", "tiles_per_forward"),
    ("tile = 8\nwrite_seam = perhaps\n", "write_seam"),
], ids=lambda v: v.replace("\n", ";").replace(" ", "") if "=" in v else v)
def test_bad_values_are_refused_with_the_key_named(tmp_path, body, key):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        with pytest.raises(ValueError, match=rf"\[TILE\] {key} "):
            Config(_ini_with(tmp_path, "[TILE]\n" + body))
    finally:
        assert Config(LOCAL_INI).tile.present is False


def test_missing_tile_says_it_is_required(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        with pytest.raises(ValueError, match=r"\[TILE\] tile is required"):
            Config(_ini_with(tmp_path, "[TILE]\n"))
    finally:
        Config(LOCAL_INI)


# ------------------------------------------------------------------------------------------ 4. test.py and wrappers
def test_generate_without_the_section_is_the_plain_forward():
    """test.py's switch: no section (or a CPU device) -> ``gan.G`` itself, no variance, no seam"""
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.test import _generate_fields

    class Gan:
        def G(self, lr, z):
            return lr[:, :3] + 1

        def G_tiled(self, *a, **kw):
            raise AssertionError("tiles without a GPU / without the section")

        def G_ensemble(self, *a, **kw):
            raise AssertionError("the ensemble without a GPU / without the section")

    cfg = Config(LOCAL_INI)
    cfg.device = torch.device("cpu")
    lr = torch.zeros(1, 4, 2, 2, 3)
    sr, var, seam = _generate_fields(cfg, Gan(), lr, None)
    assert var is None and seam is None and torch.equal(sr, lr[:, :3] + 1)
    cfg.tile.present, cfg.tile.tile, cfg.tile.write_seam = True, 1, True  # a CPU device keeps the plain path
    try:
        sr, var, seam = _generate_fields(cfg, Gan(), lr, None)
        assert var is None and seam is None and torch.equal(sr, lr[:, :3] + 1)
        sr, var = _generate_fields(cfg, Gan(), lr, None)[:2]
        assert var is None and torch.equal(sr, lr[:, :3] + 1)
    finally:
        Config(LOCAL_INI)


def test_generate_with_the_section_on_a_gpu_asks_g_tiled_for_what_the_sections_say():
    """the switch alone, with a stub in place of the GAN and a device that is only named"""
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.test import _generate_fields

    asked = []

    class Gan:
        def G(self, lr, z):
            raise AssertionError("the plain forward with [TILE] on a GPU")

        G_ensemble = G

        def G_tiled(self, lr, z, **kw):
            asked.append(kw)
            res = ("sr",) + (("var",) if kw["with_var"] else ()) + (("seam",) if kw["with_seam"] else ())
            return res[0] if len(res) == 1 else res

    cfg = Config(LOCAL_INI)
    cfg.device = torch.device("cuda")
    try:
        cfg.tile.present, cfg.tile.tile = True, 8
        assert _generate_fields(cfg, Gan(), None, None) == ("sr", None, None)
        cfg.tile.write_seam = True
        assert _generate_fields(cfg, Gan(), None, None) == ("sr", None, "seam")
        cfg.ensemble.present, cfg.ensemble.members, cfg.ensemble.write_spread = True, 4, True
        assert _generate_fields(cfg, Gan(), None, None) == ("sr", "var", "seam")
        cfg.tile.write_seam = False
        assert _generate_fields(cfg, Gan(), None, None) == ("sr", "var", None)
        assert asked == [dict(members=1, with_var=False, with_seam=False), dict(members=1, with_var=False, with_seam=True),
                         dict(members=4, with_var=True, with_seam=True), dict(members=4, with_var=True, with_seam=False)]
    finally:
        Config(LOCAL_INI)


def test_wrappers_refuse_host_tensors():
    from gan_sr_wind_field_amd import hip_ops

    with pytest.raises(RuntimeError, match="device tensors"):
        hip_ops.tile_gather(torch.zeros(1, 3, 4, 4, 5), [0], [0], 2, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        hip_ops.tile_stitch(torch.zeros(1, 1, 3, 4, 4, 5), [0], [0], 4, 4, 0, 0)


def test_exports_are_declared_with_their_cap():
    """header, EXPORTS and the wrapper's cap agree; the ABI version stays 9"""
    from gan_sr_wind_field_amd import _lib, hip_ops

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    assert "wsr_tile_gather" in _lib.EXPORTS and "wsr_tile_stitch" in _lib.EXPORTS
    assert "int wsr_tile_gather(" in header and "int wsr_tile_stitch(" in header
    assert f"#define WSR_TILE_MAX_PER_AXIS {hip_ops.TILE_MAX_PER_AXIS}\n" in header
    assert "#define WSR_ABI_VERSION 9\n" in header
