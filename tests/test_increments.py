"""[INCREMENTS] without a GPU: the torch reference against a plain loop over the definition, the exact identities, where a
NaN goes, the columns from hand-made sums, the section, ``test()`` on a CPU device and the exports."""
import math
import os

import pytest
import torch

from conftest import REPO
from increments_cases import (LISTS, NAN, SEEDS, SHAPES, alternating_field, fields, is_nan, loop_reference, pairs_table,
                              ramp_field)
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained


# ---------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("separations", LISTS, ids=lambda s: f"{len(s)}sep")
def test_reference_against_a_plain_loop(separations):
    from gan_sr_wind_field_amd.increments import level_increments_reference, pair_counts

    B, X, Y, NZ = 2, 5, 7, 3
    HR, SR, TL = fields(B, X, Y, NZ, seed=3, channels=(4, 3, 5))
    want = loop_reference(HR, SR, TL, separations)
    got = level_increments_reference(HR, SR, TL, separations)
    assert got.dtype == torch.float64 and got.shape == (B, NZ, 3, len(separations), 2, 3, 3)
    # the same float64 terms, summed in another order: 2^-50 of the sum of their magnitudes (at most 30 terms, even orders)
    mag = want[..., [0, 0, 2]].clone()
    mag[..., 1] = (want[..., 0] * want[..., 2]).sqrt() * 1.0  # sum |d|^3 <= sqrt(sum d^2 sum d^4)
    assert bool(((got - want).abs() <= 2.0 ** -50 * mag).all())
    pairs = pairs_table(X, Y, separations)
    assert pair_counts(X, Y, separations) == [tuple(int(v) for v in row) for row in pairs.tolist()]
    none = (pairs == 0)[None, None, None, :, :, None, None].expand_as(got)
    assert bool((got[none] == 0).all()) and bool((got[~none][..., None].reshape(-1) != 0).any())
    assert bool((got[..., 0][~none[..., 0]] > 0).all())  # every S2 entry with pairs
    if len(separations) == 8:
        assert int((pairs == 0).sum()) == 9  # most of the list: r >= 5 along x, r >= 7 along y
    no_tl = level_increments_reference(HR, SR, None, separations)
    assert torch.equal(no_tl[:, :, :2], got[:, :, :2]) and float(no_tl[:, :, 2].abs().sum()) == 0
    # fp32 terms: the definition's roundings - close to the float64 value, not equal to it
    f32 = level_increments_reference(HR, SR, TL, separations, dtype=torch.float32)
    assert f32.dtype == torch.float64 and bool(((f32 - want).abs() <= 2.0 ** -20 * mag).all())


def test_gpu_seeds_leave_no_empty_comparison():
    """every S2 entry with pairs of the GPU tests' inputs is strictly positive (the small shapes here, all on the GPU)"""
    from gan_sr_wind_field_amd.increments import level_increments_reference

    for shape, seed in zip(SHAPES, SEEDS):
        if shape[1] * shape[2] * shape[3] > 20000:
            continue
        for independent in (False, True):
            ops = fields(*shape, seed=seed, independent=independent)
            s2 = level_increments_reference(*ops, LISTS[2])[..., 0]
            has = (pairs_table(shape[1], shape[2], LISTS[2]) > 0)[None, None, None, :, :, None].expand_as(s2)
            assert bool((s2[has] > 0).all()) and bool((s2[~has] == 0).all()), shape


# ---------------------------------------------------------------------------------------------------- 2. exact identities
def test_exact_identities():
    from gan_sr_wind_field_amd.increments import increments_from_sums, level_increments_reference

    B, X, Y, NZ = 2, 12, 5, 3
    sp = (1, 2, 4, 8)
    pairs = pairs_table(X, Y, sp)
    for dtype in (torch.float64, torch.float32):
        # a ramp: the x-L sums are pairs (r 2^-6)^p, everything else 0
        f = ramp_field(B, X, Y, NZ)
        got = level_increments_reference(f, f, None, sp, dtype=dtype)
        want = torch.zeros_like(got)
        for k, r in enumerate(sp):
            for o, p in enumerate((2, 3, 4)):
                want[:, :, :2, k, 0, 0, o] = pairs[k, 0] * (r * 2.0 ** -6) ** p
        assert torch.equal(got, want)
        assert torch.equal(got[:, :, 0], got[:, :, 1])  # SR = HR: equal slices
        col = increments_from_sums(got[0, 0], sp, 1, X, Y, 32.0, 100.0)
        # pooled with the y direction, whose increments are all 0: S2 = px r^2 2^-12 / (px + py), flatness (px + py) / px
        for k, r in enumerate(sp):
            px, py = pairs[k].tolist()
            assert col["flatness_L_HR"][k] == pytest.approx((px + py) / px, rel=1e-14)
            assert col["S2L_HR"][k] == pytest.approx(32.0 ** 2 * px * (r * 2.0 ** -6) ** 2 / (px + py), rel=1e-14)
            assert is_nan(col["flatness_T_HR"][k]) and is_nan(col["anisotropy_HR"][k]) and col["S2L_ratio"][k] == 1.0
        # a plane of one row of y has x pairs alone: skewness and flatness are exactly 1, S2 = (32 r 2^-6)^2
        f1 = ramp_field(1, X, 1, NZ)
        one = increments_from_sums(level_increments_reference(f1, f1, None, sp, dtype=dtype)[0, 0], sp, 1, X, 1, 32.0, 100.0)
        assert one["skewness_L_HR"] == [1.0] * 4 and one["flatness_L_HR"] == [1.0] * 4 == one["flatness_L_SR"]
        assert one["S2L_HR"] == [(0.5 * r) ** 2 for r in sp] and one["pairs"] == [float(X - r) for r in sp]
        # alternating signs: 2^-4 per pair at odd r, 0 at even r
        f = alternating_field(B, X, Y, NZ)
        got = level_increments_reference(f, f, f, sp, dtype=dtype)
        want = torch.zeros_like(got)
        want[:, :, :, 0, 0, 0, 0] = pairs[0, 0] * 2.0 ** -4
        want[:, :, :, 0, 0, 0, 2] = pairs[0, 0] * 2.0 ** -8
        assert torch.equal(got[..., [0, 2]], want[..., [0, 2]]) and float(got[:, :, :, 1:].abs().sum()) == 0
        assert float(got[:, :, :, 0, 0, 0, 1].abs().max()) <= pairs[0, 0] * 2.0 ** -6  # (the cubes alternate in sign)
        # a constant field
        f = torch.full((B, 3, X, Y, NZ), 0.7)
        assert float(level_increments_reference(f, f, f, sp, dtype=dtype).abs().sum()) == 0
        # Y = 1: the y direction has no pairs
        HR, SR, TL = fields(1, 9, 1, 2, seed=5)
        got = level_increments_reference(HR, SR, TL, sp, dtype=dtype)
        assert float(got[:, :, :, :, 1].abs().sum()) == 0 and bool((got[:, :, :, :3, 0, :, 0] > 0).all())


# ---------------------------------------------------------------------------------------------------- 3. NaN
def test_a_nan_voxel_poisons_its_pairs_only():
    from gan_sr_wind_field_amd.increments import level_increments_reference

    B, X, Y, NZ = 2, 6, 5, 3
    sp = (1, 2, 4, 8)
    HR, SR, TL = fields(B, X, Y, NZ, seed=9, channels=(3, 3, 3))
    clean = level_increments_reference(HR, SR, TL, sp)
    SR = SR.clone()
    SR[1, 1, 2, 3, 1] = NAN  # v of SR, sample 1, level 1
    got, want = level_increments_reference(SR=SR, HR=HR, TL=TL, separations=sp), loop_reference(HR, SR, TL, sp)
    bad = ~torch.isfinite(got)
    assert torch.equal(bad, ~torch.isfinite(want))
    expect = torch.zeros_like(bad)
    expect[1, 1, 1, :2, 0, 1] = True   # along x, v is T; r = 4: 2 - 4 and 2 + 4 are outside, no pair holds the voxel
    expect[1, 1, 1, :2, 1, 0] = True   # along y, v is L; r = 4: 3 - 4 and 3 + 4 are outside; r = 8 has no pairs
    assert torch.equal(bad, expect)
    assert torch.equal(got[~bad], clean[~bad])
    # a surplus channel is never read
    HR4 = torch.cat([HR, torch.full((B, 1, X, Y, NZ), NAN)], dim=1)
    assert torch.equal(level_increments_reference(HR4, HR4, None, sp)[:, :, 0], clean[:, :, 0])


# ---------------------------------------------------------------------------------------------------- 4. the columns
def test_columns_from_hand_made_sums():
    from gan_sr_wind_field_amd.increments import INCREMENT_COLUMNS, SOURCES, increments_from_sums

    assert INCREMENT_COLUMNS[:3] == ("r", "r_m", "pairs") and len(INCREMENT_COLUMNS) == 3 + 3 * 8 + 6
    assert INCREMENT_COLUMNS[3:11] == ("S2L_HR", "S2T_HR", "S2W_HR", "skewness_L_HR", "flatness_L_HR", "flatness_T_HR",
                                       "flatness_W_HR", "anisotropy_HR")
    assert INCREMENT_COLUMNS[-6:] == ("S2L_ratio", "S2L_ratio_trilinear", "S2T_ratio", "S2T_ratio_trilinear", "S2W_ratio",
                                      "S2W_ratio_trilinear")
    X, Y, sp, nf, U, d = 6, 4, (1, 5), 3, 10.0, 250.0
    # pairs per plane: r = 1: 20 along x, 18 along y; r = 5: 4 along x, none along y
    t = torch.zeros((3, 2, 2, 3, 3), dtype=torch.float64)
    t[0, 0, 0, 0] = torch.tensor([6.0, 3.0, 12.0], dtype=torch.float64)    # HR, r = 1, x, L
    t[0, 0, 1, 0] = torch.tensor([5.4, -1.0, 9.0], dtype=torch.float64)    # HR, r = 1, y, L
    t[0, 0, 0, 1] = torch.tensor([1.14, 0.0, 0.57], dtype=torch.float64)   # HR, r = 1, x, T
    t[1, 0, 0, 0] = torch.tensor([3.0, 0.0, 4.0], dtype=torch.float64)     # SR
    t[1, 0, 1, 0] = torch.tensor([2.7, 0.0, 5.0], dtype=torch.float64)
    t[0, 1, 0, 2] = torch.tensor([2.4, 0.6, 1.2], dtype=torch.float64)     # HR, r = 5, x, W
    col = increments_from_sums(t, sp, nf, X, Y, U, d)
    assert sorted(col) == sorted(INCREMENT_COLUMNS) and all(len(v) == 2 for v in col.values())
    assert col["r"] == [1, 5] and col["r_m"] == [250.0, 1250.0] and col["pairs"] == [3.0 * 38, 3.0 * 4]
    m2, m3, m4 = 11.4 / 114, 2.0 / 114, 21.0 / 114
    assert col["S2L_HR"][0] == pytest.approx(100 * m2, rel=1e-14)
    assert col["skewness_L_HR"][0] == pytest.approx(m3 / m2 ** 1.5, rel=1e-14)
    assert col["flatness_L_HR"][0] == pytest.approx(m4 / m2 ** 2, rel=1e-14)
    assert col["anisotropy_HR"][0] == pytest.approx((6.0 / 60) / (5.4 / 54), rel=1e-14)
    assert col["S2T_HR"][0] == pytest.approx(100 * 1.14 / 114, rel=1e-14)
    assert col["flatness_T_HR"][0] == pytest.approx((0.57 / 114) / (1.14 / 114) ** 2, rel=1e-14)
    assert col["S2L_ratio"][0] == pytest.approx(0.5, rel=1e-14) and col["S2L_ratio_trilinear"][0] == 0.0
    assert col["S2W_HR"] == [0.0, pytest.approx(100 * 2.4 / 12, rel=1e-14)]
    assert col["flatness_W_HR"][1] == pytest.approx((1.2 / 12) / (2.4 / 12) ** 2, rel=1e-14)
    # the nan rule: a zero denominator (S2 = 0: flatness, skewness, ratios), no pairs along y (anisotropy at r = 5)
    assert is_nan(col["flatness_W_HR"][0]) and is_nan(col["S2W_ratio"][0]) and is_nan(col["skewness_L_HR"][1])
    assert is_nan(col["anisotropy_HR"][1]) and is_nan(col["anisotropy_trilinear"][0]) and col["S2W_ratio"][1] == 0.0
    for s in SOURCES:
        assert col[f"S2T_{s}"][1] == 0.0
    # no pairs at all: every statistic is nan
    none = increments_from_sums(torch.zeros((3, 1, 2, 3, 3)), (8,), 2, 6, 4, U, d)
    assert none["pairs"] == [0.0] and all(is_nan(none[c][0]) for c in INCREMENT_COLUMNS[3:])
    for bad_table, bad_sp in ((t[:2], sp), (t, (1, 5, 9)), (t, (5, 1))):
        with pytest.raises(ValueError, match="increments_from_sums"):
            increments_from_sums(bad_table, bad_sp, nf, X, Y, U, d)


# ---------------------------------------------------------------------------------------------------- 5. config
def test_separations_refusals():
    from gan_sr_wind_field_amd.increments import check_separations, level_increments_reference, pair_counts

    assert check_separations([1, 2.0, 32], "x") == [1, 2, 32] and check_separations((7,)) == [7]
    for bad, pattern in (((), "1 .. 8 entries, not 0"), (tuple(range(1, 10)), "1 .. 8 entries, not 9"), ((0, 1), "1 .. 32"),
                         ((1, 33), "1 .. 32"), ((2, 1), "strictly ascending"), ((1, 1), "strictly ascending"),
                         ((1, 2.5), "list of integers"), ("wide", "list of integers"), (None, "list of integers"),
                         ((True, 2), "list of integers")):
        with pytest.raises(ValueError, match="who: separations must .*" + pattern):
            check_separations(bad, "who")
    f = torch.zeros((1, 3, 4, 4, 2))
    for call in (lambda: level_increments_reference(f, f, None, (2, 1)), lambda: pair_counts(4, 4, (0,)),
                 lambda: level_increments_reference(f[:, :2], f, None, (1,)), lambda: level_increments_reference(f, f[..., :1], None, (1,)),
                 lambda: level_increments_reference(f, None, None, (1,))):
        with pytest.raises(ValueError):
            call()


def test_section_parses_and_is_never_printed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        plain_cfg = Config(LOCAL_INI)
        plain, plain_str = plain_cfg.asINI(), str(plain_cfg)
        s = plain_cfg.increments
        assert s.present is False and s.on is False and "INCREMENTS" not in plain and s.separations is None
        cfg = Config(_ini_with(tmp_path, "[INCREMENTS]\nseparations = [1, 2, 4, 8, 16]\n"))
        s = cfg.increments
        assert s.present and s.on and (s.separations, s.per_level) == ([1, 2, 4, 8, 16], False)
        assert all(isinstance(r, int) for r in s.separations)
        assert cfg.asINI() == plain and str(cfg) == plain_str  # never printed
        full = Config(_ini_with(tmp_path, "[INCREMENTS]\nseparations = 3\nper_level = True\n")).increments
        assert (full.separations, full.per_level) == ([3], True)
        bad = {"": "separations must be given", "per_level = True\n": "separations must be given",
               "separations = [2, 1]\n": "separations must be strictly ascending", "separations = [1, 1]\n": "separations must be strictly",
               "separations = [0, 1]\n": "separations must lie in 1 .. 32", "separations = [1, 33]\n": "separations must lie in 1 .. 32",
               "separations = [1, 2, 3, 4, 5, 6, 7, 8, 9]\n": "separations must hold 1 .. 8 entries, not 9",
               "separations = []\n": "separations must hold", "separations = [1, 2.5]\n": "separations must be a list of integers",
               "separations = wide\n": "separations must be a list of numbers",
               "separations = [1]\nper_level = maybe\n": "per_level must be True or False"}
        for text, pattern in bad.items():
            with pytest.raises(ValueError, match=r"\[INCREMENTS\]:? " + pattern):
                Config(_ini_with(tmp_path, "[INCREMENTS]\n" + text))
        back = Config(LOCAL_INI)  # (the singleton is reset)
        assert back.increments.present is False and back.increments.separations is None and back.asINI() == plain
        assert ("increments", None) in Config._optional + Config._optional_later
    finally:
        Config(LOCAL_INI)


def test_reference_ini_files_still_parse():
    from gan_sr_wind_field_amd.config.config import Config

    folder = os.path.dirname(LOCAL_INI)
    inis = sorted(f for f in os.listdir(folder) if f.endswith(".ini"))
    assert inis
    try:
        for f in inis:
            cfg = Config(os.path.join(folder, f))
            assert cfg.increments.on is False and "[INCREMENTS]" not in cfg.asINI()
    finally:
        Config(LOCAL_INI)


# ---------------------------------------------------------------------------------------------------- 6. the loop
def _rows(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return [r.split(",") for r in f.read().strip().splitlines()]


def _snapshot(run_dir):
    """every file under test_output and the run folder: path -> bytes"""
    out = {}
    for top in ("test_output", run_dir):
        for root, _, files in os.walk(top):
            for f in files:
                with open(os.path.join(root, f), "rb") as fh:
                    out[os.path.join(root, f)] = fh.read()
    return out


def test_section_on_a_cpu_device_writes_the_files(data_root, tmp_path, monkeypatch):  # noqa: F811
    import pickle

    import numpy as np
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.config.config import IncrementsConfig
    from gan_sr_wind_field_amd.increments import (DEFAULT_SEPARATIONS, INCREMENT_COLUMNS, increments_from_sums,
                                                  level_increments_reference)
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.spectra import grid_spacing
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "increments", IncrementsConfig())
    cfg.increments.setIncrementsConfig(None)
    cfg.training.log_period = 1  # (every field is pickled)
    cfg.name = "same"
    avg_a = evaluate(cfg, ds)
    before = _snapshot(cfg.env.this_runs_folder)
    assert not any("structure_functions" in f for f in before)
    uvw = float(ds.UVW_MAX)
    ic = cfg.increments
    sp = [1, 2, 3, 32]
    ic.present, ic.separations, ic.per_level = True, sp, True
    ic.validate()
    avg_b = evaluate(cfg, ds)  # the same name: every earlier file is written again
    after = _snapshot(cfg.env.this_runs_folder)
    assert avg_a == avg_b
    for path, data in before.items():  # byte for byte, but the appended row of averages.csv (the same row twice)
        if path.endswith("averages.csv"):
            lines = after[path].decode().splitlines()
            assert after[path].startswith(data) and len(lines) == 3 and lines[1] == lines[2]
        else:
            assert after[path] == data, path
    new = sorted(os.path.basename(p) for p in set(after) - set(before))
    assert new == ["averages_structure_functions.csv", "same____structure_functions.csv",
                   "same____structure_functions_levels.csv"]

    X, Y, NZ = ds[0][1].shape[1:]
    d = grid_spacing(np.asarray(ds.x), np.asarray(ds.y))
    pooled, levels = _rows("same", "structure_functions"), _rows("same", "structure_functions_levels")
    assert pooled[0] == list(INCREMENT_COLUMNS) and len(pooled) == 1 + 4
    assert levels[0] == ["level"] + list(INCREMENT_COLUMNS) and len(levels) == 1 + NZ * 4
    with open(os.path.join("test_output", "averages_structure_functions.csv")) as f:
        av = [r.split(",") for r in f.read().strip().splitlines()]
    assert av[0] == ["Name"] + list(INCREMENT_COLUMNS) and [r[0] for r in av[1:]] == ["same"] * 4
    assert [r[1:] for r in av[1:]] == pooled[1:]

    # the files: increments_from_sums of the reference on the pickled fields
    total = torch.zeros((NZ, 3, 4, 2, 3, 3), dtype=torch.float64)
    names = [ds[i][3] for i in range(len(ds))]
    for name in names:
        with open(os.path.join(cfg.env.this_runs_folder, "fields", f"test_fields_{name}.pkl"), "rb") as f:
            p = pickle.load(f)
        HR, SR, TL = (torch.from_numpy(np.asarray(p[k]))[None] for k in ("HR", "SR", "TL"))
        total += level_increments_reference(HR, SR, TL, sp)[0]
    want = increments_from_sums(total.sum(dim=0), sp, len(ds) * NZ, X, Y, uvw, d)
    assert pooled[1:] == [[str(want[c][k]) for c in INCREMENT_COLUMNS] for k in range(4)]
    for lvl in range(NZ):
        w = increments_from_sums(total[lvl], sp, len(ds), X, Y, uvw, d)
        assert levels[1 + 4 * lvl:5 + 4 * lvl] == [[str(lvl)] + [str(w[c][k]) for c in INCREMENT_COLUMNS] for k in range(4)]
    assert want["pairs"][3] == len(ds) * NZ * ((X - 32) * Y + X * (Y - 32)) and "nan" not in pooled[4]
    assert all(v > 0 for v in want["S2L_HR"]) and all(1 < v < 100 for v in want["flatness_L_HR"])

    # the model's entry point: the same table; its defaults without the section
    gan = wind_field_GAN_3D(cfg)
    LR, HR = (ds[0][k][None] for k in (0, 1))
    TL = F.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear", align_corners=True)
    assert torch.equal(gan.level_increments(HR, HR, LR), level_increments_reference(HR, HR, TL, sp))
    ic.per_level, cfg.name = False, "two"
    evaluate(cfg, ds)
    assert sorted(f for f in os.listdir("test_output") if f.startswith("two____") and "metrics" not in f) == [
        "two____structure_functions.csv"]
    ic.setIncrementsConfig(None)
    assert torch.equal(gan.level_increments(HR, HR, LR), level_increments_reference(HR, HR, TL, DEFAULT_SEPARATIONS))


# ---------------------------------------------------------------------------------------------------- 7. the ABI
def test_exports_header_and_wrapper_limits_agree():
    import ctypes

    import gan_sr_wind_field_amd as pkg
    from gan_sr_wind_field_amd import _lib, hip_ops, increments

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_increments", "wsr_level_increments_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define WSR_INCREMENTS_MAX_SEPARATIONS {increments.MAX_SEPARATIONS}" in header
    assert f"#define WSR_INCREMENTS_MAX_SEPARATION {increments.MAX_SEPARATION}" in header
    assert "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "increments_kernels.h")) as f:
        kernels = f.read()
    assert f"constexpr int INC_TILE = {hip_ops.INCREMENTS_TILE};" in kernels and "INC_LDS_FLOATS = INC_BLOCK * INC_MAX_NR * INC_ACC" in kernels
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " increments.hip" in mk and "increments.o: increments_kernels.h" in mk
    assert callable(hip_ops.level_increments) and callable(pkg.GAN_models.wind_field_GAN_3D.wind_field_GAN_3D.level_increments)
    assert increments.DEFAULT_SEPARATIONS == (1, 2, 4, 8, 16) and increments.KINDS == ("L", "T", "W")
    # the levels a workgroup stages: what fits 12288 floats beside the forward halo, spread evenly
    assert [hip_ops.increments_level_chunk(17, sp) for sp in LISTS] == [9, 6, 3]
    assert hip_ops.increments_level_chunk(10, (1, 2, 4, 8, 16)) == 5 and hip_ops.increments_level_chunk(2, (32,)) == 2
    # the built library exports both symbols and sizes the workspace from shape and separations alone (no GPU needed)
    so = os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "libwindsr_hip.so")
    if os.path.exists(so):
        L = ctypes.CDLL(so)
        fn = L.wsr_level_increments_workspace_floats
        fn.restype = ctypes.c_int64
        sep = (ctypes.c_int32 * 5)(1, 2, 4, 8, 16)
        assert fn(1, 128, 128, 10, sep, 5) == 9 * 2 * 16 * 5 * 5 * 6 and hasattr(L, "wsr_level_increments")
        assert fn(1, 128, 128, 10, (ctypes.c_int32 * 2)(2, 1), 2) == 0 and fn(1, 128, 128, 10, None, 1) == 0
        assert fn(0, 128, 128, 10, sep, 5) == 0 and fn(1, 128, 128, 10, sep, 9) == 0 and fn(65536, 8, 8, 2, sep, 5) == 0
