"""[DISTRIBUTION] without a GPU: the tables, ``distribution.level_distribution_reference`` against an independent float64
classification (hypot, atan2, floor) and on exact cases, ``distribution_from_counts`` on hand-made tables, the section,
``test()`` on a CPU device and the exports.

The comparison with the float64 classification allows 2 counts per voxel that classification itself flags as within
1e-4 m/s of a speed edge or of ``calm`` or within 1e-5 rad of a sector boundary (a voxel that changes class leaves one
counter and enters another), and fails as vacuous when more than 0.1 % of the voxels are flagged.  Measured when the
test was written: 0 differing counts, 2 to 3 flagged voxels of 6912 per source (0.03 - 0.04 %).
"""
import math
import os

import pytest
import torch

from conftest import REPO
from distribution_cases import CALMS, INF, NAN, PARAMS, UVW, counts_f64, fields, plant, special_voxels, tables
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained


# ---------------------------------------------------------------------------------------------------- 1. the tables
def test_tables_for_the_defaults():
    from gan_sr_wind_field_amd.distribution import distribution_tables

    t = distribution_tables(32.0, 1.0, 32, 16, 0.5)
    assert t.edge2.dtype == t.bx.dtype == t.by.dtype == torch.float32
    assert t.edge2.shape == (31,) and t.bx.shape == t.by.shape == (8,)
    assert torch.equal(t.edge2, torch.tensor([(j / 32.0) ** 2 for j in range(1, 32)], dtype=torch.float64).float())
    assert float(t.edge2[0]) == 2.0 ** -10 and float(t.edge2[15]) == 0.25  # (j / 32)^2 is exact for these
    assert bool((t.edge2[1:] > t.edge2[:-1]).all())
    assert t.calm2 == (0.5 / 32.0) ** 2 == 2.0 ** -12
    for k in range(8):
        beta = -math.pi / 16 + 2 * math.pi * k / 16
        assert float(t.bx[k]) == float(torch.tensor(math.sin(beta), dtype=torch.float64).float())
        assert float(t.by[k]) == float(torch.tensor(math.cos(beta), dtype=torch.float64).float())
    assert float(t.bx[0]) < 0 < float(t.bx[1]) and float(t.by[0]) == float(t.by[1])  # +-pi / 16 about north
    for ns, nd in PARAMS:
        t = distribution_tables(12.5, 0.3, ns, nd, 0.0)
        assert t.edge2.shape == (ns - 1,) and t.bx.shape == t.by.shape == (nd // 2,) and t.calm2 == 0.0
        assert bool((t.edge2[1:] > t.edge2[:-1]).all()) and float(t.edge2[0]) > 0
    bad = [dict(bin_width=0.0), dict(bin_width=-1.0), dict(bin_width=NAN), dict(speed_bins=1), dict(speed_bins=65),
           dict(sectors=3), dict(sectors=5), dict(sectors=2), dict(sectors=38), dict(calm=-0.1), dict(calm=INF),
           dict(UVW_MAX=0.0), dict(bin_width=1e-30)]
    for kw in bad:
        args = dict(UVW_MAX=32.0, bin_width=1.0, speed_bins=32, sectors=16, calm=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=r"\d|nan|inf"):
            distribution_tables(**args)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def test_reference_against_an_independent_float64_classification():
    from gan_sr_wind_field_amd.distribution import level_distribution_reference

    B, X, Y, NZ = 2, 24, 24, 6
    HR, SR, TL = fields(B, X, Y, NZ, seed=3, channels=(3, 3, 3))
    t = tables()
    got = level_distribution_reference(HR, SR, TL, t)
    assert got.shape == (B, NZ, 3, 32, 17) and got.dtype == torch.float64
    assert bool((got.sum(dim=(3, 4)) == X * Y).all())
    nvox = B * X * Y * NZ
    for s, f in enumerate((HR, SR, TL)):
        want, flagged = counts_f64(f, 32, 16, 0.5)
        diff = float((got[:, :, s] - want).abs().sum())
        print(f"[distribution] source {s}: summed |count difference| {diff:g}, {flagged} of {nvox} voxels flagged")
        assert flagged <= 1e-3 * nvox, "vacuous: too many voxels near a class boundary"
        assert diff <= 2 * flagged
    # a wrong definition is far outside: u and v swapped moves most voxels to another sector
    swapped = level_distribution_reference(HR[:, [1, 0, 2]], SR, TL, t)
    assert float((swapped[:, :, 0] - got[:, :, 0]).abs().sum()) > 0.5 * nvox


@pytest.mark.parametrize("nd", [4, 16, 36])
def test_axis_directions(nd):
    from gan_sr_wind_field_amd.distribution import classify

    t = tables(32, nd, 0.5)
    u = torch.tensor([0.0, -0.25, 0.0, 0.25])  # from north (v < 0), east (u < 0), south, west
    v = torch.tensor([-0.25, 0.0, 0.25, 0.0])
    j, sector = classify(u, v, t)
    assert sector.tolist() == [0, nd // 4, nd // 2, 3 * nd // 4] and j.tolist() == [8, 8, 8, 8]


def test_ties_edges_zero_and_non_finite_voxels():
    from gan_sr_wind_field_amd.distribution import classify, level_distribution_reference

    # |u| = |v| at ND = 4: p = (-u, -v) on a boundary, an exact tie, goes to the clockwise sector
    t4 = tables(32, 4, 0.5)
    u = torch.tensor([-0.25, -0.25, 0.25, 0.25])  # p = NE, SE, SW, NW
    v = torch.tensor([-0.25, 0.25, 0.25, -0.25])
    assert classify(u, v, t4)[1].tolist() == [1, 2, 3, 0]
    # u = j / 32, v = 0 lands in bin j: the edge is inclusive (and the last bin is open-ended)
    t = tables()
    u = torch.arange(0, 40, dtype=torch.float32) / 32.0
    j, sector = classify(u, torch.zeros_like(u), t)
    assert j.tolist() == list(range(32)) + [31] * 8
    assert sector.tolist() == [16] + [12] * 39  # calm (0 <= 0.5), then from west
    just_below = torch.nextafter(u[1:], torch.zeros(()))
    assert classify(just_below, torch.zeros_like(just_below), t)[0].tolist() == list(range(31)) + [31] * 8
    # the zero vector at calm = 0 is calm, and so is a vector whose squared speed underflows to 0; a small one is not
    t0 = tables(32, 16, 0.0)
    z = torch.tensor([0.0, -0.0, 1e-30, 1e-18])
    assert classify(z, torch.zeros(4), t0)[1].tolist() == [16, 16, 16, 12]
    # NaN and +-Inf: classes in range, NaN calm in bin 0, every slice still sums to X * Y
    for ns, nd in PARAMS:
        for calm in CALMS:
            tt = tables(ns, nd, calm)
            vox = special_voxels(ns)
            uu, vv = (torch.tensor([p[k] for p in vox]) for k in (0, 1))
            j, sector = classify(uu, vv, tt)
            assert bool(((j >= 0) & (j < ns) & (sector >= 0) & (sector <= nd)).all())
            nan = torch.isnan(uu) | torch.isnan(vv)
            assert j[nan].tolist() == [0] * int(nan.sum()) and sector[nan].tolist() == [nd] * int(nan.sum())
            f = plant(torch.zeros((1, 3, 4, 3, 2)), vox, 0)
            out = level_distribution_reference(f, f, None, tt)
            assert bool((out[:, :, :2].sum(dim=(3, 4)) == 12).all()) and float(out[:, :, 2].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------- 3. the columns
def test_distribution_from_counts():
    from gan_sr_wind_field_amd.distribution import (ROSE_COLUMNS, SPEED_COLUMNS, SUMMARY_COLUMNS, distribution_from_counts,
                                                   level_distribution_reference)

    HR, SR, TL = fields(1, 16, 16, 3, seed=2, channels=(3, 3, 3))
    same = level_distribution_reference(HR, HR, HR, tables()).sum(dim=(0, 1))
    d = distribution_from_counts(same, 1.0)
    assert tuple(d["speed"]) == SPEED_COLUMNS and tuple(d["rose"]) == ROSE_COLUMNS and tuple(d["summary"]) == SUMMARY_COLUMNS
    s = d["summary"]
    assert (s["PSS"], s["W1"], s["rose_tv"], s["PSS_trilinear"], s["W1_trilinear"], s["rose_tv_trilinear"]) == (1, 0, 0, 1, 0, 0)
    assert len(d["speed"]["f_HR"]) == 32 and len(d["rose"]["f_HR"]) == 17
    assert sum(d["speed"]["f_HR"]) == pytest.approx(1, abs=1e-14) and sum(d["rose"]["f_HR"]) == pytest.approx(1, abs=1e-14)
    assert d["speed"]["speed_lo"][:2] == [0.0, 1.0] and d["speed"]["speed_hi"][-2:] == [31.0, math.inf]
    assert d["rose"]["dir_lo_deg"][:2] == [348.75, 11.25] and d["rose"]["dir_hi_deg"][:2] == [11.25, 33.75]
    assert math.isnan(d["rose"]["dir_lo_deg"][-1]) and math.isnan(d["rose"]["dir_hi_deg"][-1])

    # every SR voxel one bin up: W1 = bin_width, whatever the width
    c = torch.zeros((3, 6, 5), dtype=torch.float64)
    c[0, 0, 0], c[0, 1, 1], c[0, 2, 4], c[0, 3, 2] = 10, 20, 30, 40
    c[1, 1:] = c[0, :-1]
    c[2] = c[0]
    for bw in (1.0, 0.5):
        s = distribution_from_counts(c, bw)["summary"]
        assert s["W1"] == pytest.approx(bw, rel=1e-14) and s["W1_trilinear"] == 0 and s["rose_tv"] == 0
        assert s["PSS"] == 0 and s["PSS_trilinear"] == 1  # (no joint class in common)

    # hand-made: NS = 4, ND = 4, bin_width 2; HR speed marginal 0.1, 0.4, 0.3, 0.2 (the open bin)
    c = torch.zeros((3, 4, 5), dtype=torch.float64)
    c[0, 0, 4], c[0, 1, 0], c[0, 2, 1], c[0, 3, 1] = 10, 40, 30, 20
    c[1, 0, 4], c[1, 1, 0], c[1, 2, 2], c[1, 3, 1] = 20, 40, 30, 10
    c[2, 1, 0] = 100
    d = distribution_from_counts(c.tolist(), 2.0)
    s = d["summary"]
    assert d["speed"]["f_HR"] == [0.1, 0.4, 0.3, 0.2] and d["speed"]["f_trilinear"] == [0, 1, 0, 0]
    assert d["rose"]["f_HR"] == [0.4, 0.5, 0, 0, 0.1] and d["rose"]["f_SR"] == [0.4, 0.1, 0.3, 0, 0.2]
    assert s["f_overflow_HR"] == 0.2
    assert s["p50_HR"] == pytest.approx(2 * (1 + (0.5 - 0.1) / 0.4), rel=1e-14)  # linear inside bin 1: 4.0
    assert s["p90_HR"] == 6.0 and s["p99_HR"] == 6.0  # in the open bin: its lower edge
    assert s["p50_SR"] == pytest.approx(2 * (1 + (0.5 - 0.2) / 0.4), rel=1e-14) and s["p90_SR"] == pytest.approx(6.0, rel=1e-14)
    assert s["p50_trilinear"] == pytest.approx(3.0, rel=1e-14) and s["p99_trilinear"] == pytest.approx(2 + 2 * 0.99, rel=1e-14)
    assert s["PSS"] == pytest.approx((10 + 40 + 0 + 10) / 100, rel=1e-14) and s["PSS_trilinear"] == pytest.approx(0.4, rel=1e-14)
    assert s["W1"] == pytest.approx(2.0 * (0.1 + 0.1 + 0.1), rel=1e-12)  # F_SR - F_HR = 0.1 at bins 0, 1, 2
    assert s["W1_trilinear"] == pytest.approx(2.0 * (0.1 + 0.5 + 0.2), rel=1e-12)
    assert s["rose_tv"] == pytest.approx(0.5 * (0 + 0.4 + 0.3 + 0 + 0.1), rel=1e-12)
    # a launch without a baseline: frequencies 0, scores nan
    c[2] = 0
    s = distribution_from_counts(c, 2.0)
    assert s["speed"]["f_trilinear"] == [0.0] * 4 and math.isnan(s["summary"]["PSS_trilinear"]) and math.isnan(s["summary"]["p50_trilinear"])
    with pytest.raises(ValueError, match="table"):
        distribution_from_counts(torch.zeros((2, 4, 5)), 1.0)


# ---------------------------------------------------------------------------------------------------- 4. config
def test_section_parses_and_is_never_printed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        plain_cfg = Config(LOCAL_INI)
        plain, plain_str = plain_cfg.asINI(), str(plain_cfg)
        d = plain_cfg.distribution
        assert d.present is False and d.on is False and "DISTRIBUTION" not in plain and d.bin_width is None
        cfg = Config(_ini_with(tmp_path, "[DISTRIBUTION]\nbin_width = 1.0\n"))
        d = cfg.distribution
        assert d.present and d.on
        assert (d.bin_width, d.speed_bins, d.sectors, d.calm, d.per_level) == (1.0, 32, 16, 0.5, False)
        assert cfg.asINI() == plain and str(cfg) == plain_str  # never printed
        full = Config(_ini_with(tmp_path, "[DISTRIBUTION]\nbin_width = 0.5\nspeed_bins = 64\nsectors = 36\ncalm = 0\n"
                                          "per_level = True\n"))
        d = full.distribution
        assert (d.bin_width, d.speed_bins, d.sectors, d.calm, d.per_level) == (0.5, 64, 36, 0.0, True)
        assert str(d) == "[DISTRIBUTION]\nbin_width = 0.5\nspeed_bins = 64\nsectors = 36\ncalm = 0.0\nper_level = True\n"
        w = "bin_width = 1.0\n"
        bad = {"": "bin_width must be given", "speed_bins = 16\n": "bin_width must be given",
               "bin_width = 0\n": "bin_width must be .*> 0, not 0", "bin_width = -1\n": "bin_width must be .*-1",
               "bin_width = nan\n": "bin_width must be", "bin_width = wide\n": "bin_width must be a number",
               w + "speed_bins = 1\n": "speed_bins must be 2 .. 64, not 1", w + "speed_bins = 65\n": "speed_bins must be .*65",
               w + "speed_bins = 2.5\n": "speed_bins must be an integer", w + "sectors = 5\n": "sectors must be even.*5",
               w + "sectors = 2\n": "sectors must be .*4 .. 36, not 2", w + "sectors = 38\n": "sectors must be .*38",
               w + "sectors = many\n": "sectors must be an integer", w + "calm = -0.5\n": "calm must be .*>= 0, not -0.5",
               w + "calm = inf\n": "calm must be", w + "calm = still\n": "calm must be a number",
               w + "per_level = maybe\n": "per_level must be True or False"}
        for text, pattern in bad.items():
            with pytest.raises(ValueError, match=r"\[DISTRIBUTION\] " + pattern):
                Config(_ini_with(tmp_path, "[DISTRIBUTION]\n" + text))
        back = Config(LOCAL_INI)  # (the singleton is reset)
        assert back.distribution.present is False and back.distribution.bin_width is None and back.asINI() == plain
        assert ("distribution", None) in Config._optional + Config._optional_later
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
            assert cfg.distribution.on is False and "DISTRIBUTION" not in cfg.asINI()
    finally:
        Config(LOCAL_INI)


# ---------------------------------------------------------------------------------------------------- 5. the loop
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
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.config.config import DistributionConfig
    from gan_sr_wind_field_amd.distribution import (ROSE_COLUMNS, SPEED_COLUMNS, SUMMARY_COLUMNS, distribution_from_counts,
                                                   distribution_tables, level_distribution_reference)
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "distribution", DistributionConfig())
    cfg.distribution.setDistributionConfig(None)
    cfg.name = "same"
    avg_a = evaluate(cfg, ds)
    before = _snapshot(cfg.env.this_runs_folder)
    assert not any("____wind_" in f or "averages_distribution" in f for f in before)
    dc = cfg.distribution
    dc.present, dc.bin_width, dc.speed_bins, dc.sectors, dc.calm, dc.per_level = True, 0.5, 24, 12, 0.25, True
    dc.validate()
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
    assert new == ["averages_distribution.csv", "same____wind_distribution.csv", "same____wind_distribution_levels.csv",
                   "same____wind_rose.csv"]

    X, Y, NZ = ds[0][1].shape[1:]
    uvw = float(ds.UVW_MAX)
    speed, rose, levels = _rows("same", "wind_distribution"), _rows("same", "wind_rose"), _rows("same", "wind_distribution_levels")
    assert speed[0] == ["bin"] + list(SPEED_COLUMNS) and [r[0] for r in speed[1:]] == [str(k) for k in range(24)]
    assert rose[0] == ["sector"] + list(ROSE_COLUMNS) and [r[0] for r in rose[1:]] == [str(k) for k in range(12)] + ["calm"]
    assert levels[0] == ["level"] + list(SUMMARY_COLUMNS) and [r[0] for r in levels[1:]] == [str(k) for k in range(NZ)]
    assert sum(float(r[3]) for r in speed[1:]) == pytest.approx(1, abs=1e-12)  # f_HR
    assert sum(float(r[3]) for r in rose[1:]) == pytest.approx(1, abs=1e-12)
    assert speed[-1][2] == "inf" and float(speed[1][2]) == 0.5 and rose[-1][1] == "nan"

    # the averages row: distribution_from_counts of the reference on the same fields
    gan = wind_field_GAN_3D(cfg)
    gan.load_model(generator_load_path=cfg.env.generator_load_path, discriminator_load_path=None, state_load_path=None)
    gan.G.eval()
    t = distribution_tables(uvw, 0.5, 24, 12, 0.25)
    total = torch.zeros((NZ, 3, 24, 13), dtype=torch.float64)
    for i in range(len(ds)):
        LR, HR, Z = (ds[i][k][None] for k in (0, 1, 2))
        with torch.no_grad():
            SR = gan.G(LR, Z)
        TL = F.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear", align_corners=True)
        total += level_distribution_reference(HR, SR, TL, t)[0]
        if i == 0:  # the model's entry point: the same table
            assert torch.equal(gan.level_distribution(HR, SR, LR, uvw), level_distribution_reference(HR, SR, TL, t))
    assert float(total[:, 0].sum()) == len(ds) * X * Y * NZ
    want = distribution_from_counts(total.sum(dim=0), 0.5)
    av = open(os.path.join("test_output", "averages_distribution.csv")).read().strip().splitlines()
    assert av[0] == "Name," + ",".join(SUMMARY_COLUMNS) and len(av) == 2
    assert av[1] == "same," + ",".join(str(want["summary"][k]) for k in SUMMARY_COLUMNS)
    assert [r[1:] for r in speed[1:]] == [[str(want["speed"][c][k]) for c in SPEED_COLUMNS] for k in range(24)]
    assert [r[1:] for r in rose[1:]] == [[str(want["rose"][c][k]) for c in ROSE_COLUMNS] for k in range(13)]
    for lvl in range(NZ):
        s = distribution_from_counts(total[lvl], 0.5)["summary"]
        assert levels[1 + lvl][1:] == [str(s[k]) for k in SUMMARY_COLUMNS]
    s = want["summary"]
    assert 0 < s["PSS"] <= 1 and 0 < s["PSS_trilinear"] <= 1 and s["W1"] >= 0 and 0 <= s["rose_tv"] <= 1
    assert 0 < s["p50_HR"] <= s["p90_HR"] <= s["p99_HR"]

    # without per_level three new files; the gan's defaults without the section: bin_width 1.0
    dc.per_level, cfg.name = False, "three"
    evaluate(cfg, ds)
    assert sorted(f for f in os.listdir("test_output") if f.startswith("three____wind")) == [
        "three____wind_distribution.csv", "three____wind_rose.csv"]
    assert len(open(os.path.join("test_output", "averages_distribution.csv")).read().strip().splitlines()) == 3
    dc.setDistributionConfig(None)
    LR, HR, Z = (ds[0][k][None] for k in (0, 1, 2))
    TL = F.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear", align_corners=True)
    assert torch.equal(gan.level_distribution(HR, HR, LR, uvw),
                       level_distribution_reference(HR, HR, TL, distribution_tables(uvw, 1.0)))


# ---------------------------------------------------------------------------------------------------- 6. the ABI
def test_exports_header_and_wrapper_limits_agree():
    from gan_sr_wind_field_amd import _lib, distribution, hip_ops

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_distribution", "wsr_level_distribution_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define WSR_DISTRIBUTION_MAX_SPEED_BINS {hip_ops.DISTRIBUTION_MAX_SPEED_BINS}" in header
    assert f"#define WSR_DISTRIBUTION_MAX_SECTORS {hip_ops.DISTRIBUTION_MAX_SECTORS}" in header
    assert f"#define WSR_DISTRIBUTION_LDS_COUNTERS {hip_ops.DISTRIBUTION_LDS_COUNTERS}" in header
    assert hip_ops.DISTRIBUTION_MAX_SPEED_BINS == distribution.MAX_SPEED_BINS == 64
    assert hip_ops.DISTRIBUTION_MAX_SECTORS == distribution.MAX_SECTORS == 36
    assert hip_ops.distribution_level_chunk(128, 32, 16) == 28 and hip_ops.distribution_level_chunk(10, 32, 16) == 10
    assert hip_ops.distribution_level_chunk(128, 64, 36) == 6  # two workgroups per CU at the largest table
    assert "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " distribution.hip" in mk and "distribution.o: distribution_kernels.h" in mk
    # the built library exports both symbols (loading it needs no GPU)
    L = _lib.lib()
    assert hasattr(L, "wsr_level_distribution") and hasattr(L, "wsr_level_distribution_workspace_floats")
    assert L.wsr_level_distribution_workspace_floats(2, 5, 7, 3, 32, 16) == 2 * 3 * 3 * 32 * 17
    assert L.wsr_level_distribution_workspace_floats(2, 5, 7, 3, 32, 15) == 0
    assert UVW == 32.0
