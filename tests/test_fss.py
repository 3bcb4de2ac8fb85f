"""[FSS] without a GPU: the tables, ``fss.level_fss_reference`` against a plain Python loop over the definition and on
exact hand-made cases (a displaced event, the corner, a box that covers the plane, tie / NaN / Inf), ``fss_from_sums`` on
hand-made tables, the section, ``test()`` on a CPU device and the exports.  The sums are integers: every comparison of
them is exact."""
import math
import os

import pytest
import torch

from conftest import REPO
from fss_cases import DEFAULT_SCALES, INF, NAN, PARAMS, fields, is_nan, loop_reference, tables
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained


def _field(X, Y, NZ=1, B=1, events=(), value=0.5):
    """(B, 2, X, Y, NZ) zeros with u = ``value`` at the (x, y) of ``events`` on every level"""
    f = torch.zeros((B, 2, X, Y, NZ))
    for x, y in events:
        f[:, 0, x, y] = value
    return f


# ---------------------------------------------------------------------------------------------------- 1. the tables
def test_tables_round_once_and_refuse():
    from gan_sr_wind_field_amd.fss import fss_tables

    t = fss_tables(30.0, [5, 10, 15, 20])
    assert t.thr2.dtype == torch.float32 and t.thr2.shape == (4,) and t.thresholds == (5.0, 10.0, 15.0, 20.0)
    assert torch.equal(t.thr2, torch.tensor([(v / 30.0) ** 2 for v in (5, 10, 15, 20)], dtype=torch.float64).float())
    assert float(fss_tables(32.0, [8]).thr2[0]) == 2.0 ** -4  # exact
    assert bool((t.thr2[1:] > t.thr2[:-1]).all())
    bad = [dict(thresholds=[]), dict(thresholds=list(range(1, 10))), dict(thresholds=[0.0, 1.0]), dict(thresholds=[-1.0]),
           dict(thresholds=[NAN]), dict(thresholds=[INF]), dict(thresholds=[10.0, 5.0]), dict(thresholds=[5.0, 5.0]),
           dict(thresholds="fast"), dict(UVW_MAX=0.0), dict(UVW_MAX=INF),
           dict(thresholds=[1e-30]),                      # the square underflows to 0
           dict(thresholds=[1.0, 1.0 + 1e-12]),          # distinct doubles, one fp32 square
           dict(thresholds=[1e30], UVW_MAX=1e-10)]       # the square overflows
    for kw in bad:
        args = dict(UVW_MAX=30.0, thresholds=[5.0, 10.0])
        args.update(kw)
        with pytest.raises(ValueError, match="thresholds|UVW_MAX"):
            fss_tables(**args)


def test_scales_refusals():
    from gan_sr_wind_field_amd.fss import check_scales

    assert check_scales([1]) == [1] and check_scales(DEFAULT_SCALES) == list(DEFAULT_SCALES)
    for bad in ([], [3, 5], [1, 4], [1, 5, 3], [1, 3, 3], [1, 35], [1, 3, 5, 7, 9, 11, 13, 15, 17], [1, 2.5], "wide", [0, 1]):
        with pytest.raises(ValueError, match="scales"):
            check_scales(bad)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def test_reference_against_a_plain_loop():
    from gan_sr_wind_field_amd.fss import level_fss_reference

    HR, SR, TL = fields(2, 5, 7, 3, seed=1, channels=(4, 3, 2))
    TL = TL[:, :2].contiguous()  # C = 2 is enough for the reference
    for thresholds, scales in PARAMS:
        t = tables(thresholds)
        got = level_fss_reference(HR, SR, TL, t, scales)
        assert got.dtype == torch.float64 and got.shape == (2, 3, len(thresholds), len(scales), 5)
        assert torch.equal(got, loop_reference(HR, SR, TL, t.thr2, scales))
        assert torch.equal(level_fss_reference(HR, SR, None, t, scales), loop_reference(HR, SR, None, t.thr2, scales))
    assert float(got[..., 0].max()) > 0
    with pytest.raises(ValueError, match="SR"):
        level_fss_reference(HR, SR[:, :, :4], TL, t)
    with pytest.raises(ValueError, match="scales"):
        level_fss_reference(HR, SR, TL, t, (3, 5))


def test_equal_fields_score_one():
    from gan_sr_wind_field_amd.fss import fss_from_sums, level_fss_reference

    HR, _, _ = fields(2, 12, 9, 4, seed=2, channels=(3, 3, 3))
    t = tables()
    s = level_fss_reference(HR, HR.clone(), HR.clone(), t, DEFAULT_SCALES)
    assert float(s[..., 2].abs().sum()) == 0 and float(s[..., 4].abs().sum()) == 0
    assert torch.equal(s[..., 0], s[..., 1]) and torch.equal(s[..., 0], s[..., 3]) and bool((s[..., 0] > 0).all())
    col = fss_from_sums(s.sum(dim=(0, 1)), DEFAULT_SCALES, t.thresholds, 100.0, 2 * 4 * 12 * 9)
    assert col["fss"]["FSS"] == [1.0] * 24 and col["fss"]["FSS_trilinear"] == [1.0] * 24
    assert col["exceedance"]["CSI"] == [1.0] * 4 and col["exceedance"]["bias"] == [1.0] * 4
    assert col["exceedance"]["useful_scale_m"] == [100.0] * 4  # already at the grid scale


def test_displaced_event():
    """one event in HR at an interior cell, one in SR two cells along x: FSS(n) = max(0, 1 - d / n) exactly"""
    from gan_sr_wind_field_amd.fss import fss_from_sums, level_fss_reference

    X, Y, d, scales = 24, 21, 2, (1, 3, 5, 9)
    HR, SR = _field(X, Y, events=[(10, 10)]), _field(X, Y, events=[(10 + d, 10)])
    t = tables((10.0,))
    s = level_fss_reference(HR, SR, None, t, scales)[0, 0]
    for k, n in enumerate(scales):
        overlap = max(0, n - d) * n
        assert s[0, k].tolist() == [n * n, n * n, 2 * (n * n - overlap), 0, 0]
    col = fss_from_sums(s, scales, t.thresholds, 1.0, X * Y)
    assert col["fss"]["FSS"] == [max(0.0, 1 - d / n) for n in scales] == [0.0, 1 - 2 / 3, 1 - 2 / 5, 1 - 2 / 9]
    assert col["exceedance"]["CSI"] == [0.0] and col["exceedance"]["bias"] == [1.0] and col["exceedance"]["FAR"] == [1.0]
    assert col["exceedance"]["useful_scale_m"] == [5.0]  # 0.6 >= 0.5 + f_HR / 2 first at n = 5
    assert is_nan(col["exceedance"]["CSI_trilinear"][0]) and is_nan(col["fss"]["FSS_trilinear"][0])


def test_corner_event_is_zero_padded():
    from gan_sr_wind_field_amd.fss import level_fss_reference

    HR = _field(40, 37, events=[(0, 0)])
    s = level_fss_reference(HR, HR, None, tables((10.0,)), DEFAULT_SCALES)[0, 0, 0]
    for k, n in enumerate(DEFAULT_SCALES):
        r = (n - 1) // 2
        assert float(s[k, 0]) == (r + 1) ** 2, n  # the boxes that still hold the corner


def test_a_box_that_covers_the_plane():
    """n >= 2 max(X, Y) - 1: every count is the plane's number of events"""
    from gan_sr_wind_field_amd.fss import fss_from_sums, level_fss_reference

    X, Y = 7, 5
    HR, SR, TL = fields(1, X, Y, 2, seed=5, channels=(3, 3, 3))
    t = tables((5.0, 10.0, 15.0))
    scales = (1, 13, 33)
    s = level_fss_reference(HR, SR, TL, t, scales)
    ev = [((f[:, 0] ** 2 + f[:, 1] ** 2) >= t.thr2.view(-1, 1, 1, 1, 1)).sum(dim=(2, 3)).double() for f in (HR, SR, TL)]  # (NT, B, NZ)
    for k in (1, 2):
        for q in range(3):
            sh, ss, st = ev[0][q], ev[1][q], ev[2][q]
            assert torch.equal(s[:, :, q, k, 0], X * Y * sh * sh) and torch.equal(s[:, :, q, k, 1], X * Y * ss * ss)
            assert torch.equal(s[:, :, q, k, 2], X * Y * (ss - sh) ** 2) and torch.equal(s[:, :, q, k, 4], X * Y * (st - sh) ** 2)
    one = fss_from_sums(s[0, 0], scales, t.thresholds, 1.0, X * Y)
    sh, ss = float(ev[0][1, 0, 0]), float(ev[1][1, 0, 0])
    assert sh > 0 and one["fss"]["FSS"][3 + 1] == pytest.approx(2 * sh * ss / (sh * sh + ss * ss), rel=1e-15)


def test_tie_nan_and_inf():
    """hs2 == thr2 is an event (UVW_MAX 32, threshold 8, u = 0.25), a NaN is none, +Inf is one"""
    from gan_sr_wind_field_amd.fss import fss_tables, level_fss_reference

    t = fss_tables(32.0, [8.0])
    below = float(torch.nextafter(torch.tensor(0.25), torch.tensor(0.0)))
    f = torch.zeros((1, 2, 3, 3, 1))
    cases = [((0.25, 0.0), 1), ((below, 0.0), 0), ((0.0, -0.25), 1), ((NAN, 1.0), 0), ((1.0, NAN), 0), ((INF, 0.0), 1),
             ((-INF, 0.0), 1), ((INF, NAN), 0), ((0.0, 0.0), 0)]
    for (u, v), want in cases:
        f[0, 0, 1, 1, 0], f[0, 1, 1, 1, 0] = u, v
        s = level_fss_reference(f, f, None, t, (1,))
        assert float(s[0, 0, 0, 0, 0]) == want, (u, v)


def test_nobody_reaches_the_threshold():
    from gan_sr_wind_field_amd.fss import fss_from_sums, level_fss_reference

    HR, SR, TL = fields(1, 6, 6, 2, seed=3, channels=(3, 3, 3))
    t = tables((5.0, 29.0 * 2))  # 58 m/s: nobody
    s = level_fss_reference(HR, SR, TL, t, (1, 3)).sum(dim=(0, 1))
    assert float(s[1].abs().sum()) == 0 and float(s[0, :, 0].min()) > 0
    col = fss_from_sums(s, (1, 3), t.thresholds, 50.0, 72)
    assert all(is_nan(v) for v in col["fss"]["FSS"][2:]) and all(is_nan(v) for v in col["fss"]["FSS_trilinear"][2:])
    e = col["exceedance"]
    assert e["f_HR"][1] == 0.0 and all(is_nan(e[k][1]) for k in ("bias", "CSI", "POD", "FAR", "ETS", "useful_scale_m"))
    assert not is_nan(e["CSI"][0]) and col["fss"]["FSS_uniform"][2:] == [0.5, 0.5]


def test_no_baseline_gives_zero_columns():
    from gan_sr_wind_field_amd.fss import level_fss_reference

    HR, SR, TL = fields(2, 9, 6, 3, seed=4, channels=(3, 3, 3))
    t = tables()
    with_tl, without = level_fss_reference(HR, SR, TL, t, (1, 5)), level_fss_reference(HR, SR, None, t, (1, 5))
    assert torch.equal(with_tl[..., :3], without[..., :3]) and float(without[..., 3:].abs().sum()) == 0
    assert float(with_tl[..., 3].sum()) > 0


# ---------------------------------------------------------------------------------------------------- 3. the columns
def test_columns_from_hand_made_sums():
    from gan_sr_wind_field_amd.fss import EXCEEDANCE_COLUMNS, FSS_COLUMNS, fss_from_sums

    # n = 1 row: 40 events in HR, 50 in SR, 30 hits -> srd = misses + false alarms = 10 + 20; baseline 20 events, 15 hits
    npos = 100
    table = torch.zeros((2, 3, 5), dtype=torch.float64)
    table[0, 0] = torch.tensor([40, 50, 30, 20, 30])
    table[0, 1] = torch.tensor([300, 380, 170, 150, 200])   # FSS 0.75, baseline 1 - 200 / 450
    table[0, 2] = torch.tensor([900, 1000, 190, 500, 700])  # FSS 0.9, baseline 0.5
    table[1, 0] = torch.tensor([10, 0, 10, 0, 10])           # SR and the baseline never reach it
    table[1, 1] = torch.tensor([80, 0, 80, 0, 80])
    table[1, 2] = torch.tensor([200, 0, 200, 0, 200])
    col = fss_from_sums(table.tolist(), (1, 3, 5), (10.0, 20.0), 250.0, npos)
    f, e = col["fss"], col["exceedance"]
    assert tuple(f) == ("threshold", "scale") + FSS_COLUMNS and tuple(e) == ("threshold",) + EXCEEDANCE_COLUMNS
    assert f["threshold"] == [10.0] * 3 + [20.0] * 3 and f["scale"] == [1, 3, 5] * 2 and f["scale_m"] == [250.0, 750.0, 1250.0] * 2
    assert f["FSS"][:3] == [1 - 30 / 90, 1 - 170 / 680, 1 - 190 / 1900]
    assert f["FSS_trilinear"][:3] == [1 - 30 / 60, 1 - 200 / 450, 1 - 700 / 1400]
    assert f["FSS_uniform"] == [0.5 + (40 / npos) / 2] * 3 + [0.5 + (10 / npos) / 2] * 3
    assert f["FSS"][3:] == [0.0] * 3 and f["FSS_trilinear"][3:] == [0.0] * 3
    assert (e["f_HR"][0], e["f_SR"][0], e["f_trilinear"][0]) == (0.4, 0.5, 0.2)
    hits, misses, fa = 30.0, 10.0, 20.0
    chance = 40 * 50 / npos
    assert e["bias"][0] == 50 / 40 and e["CSI"][0] == hits / 60 and e["POD"][0] == hits / 40 and e["FAR"][0] == fa / 50
    assert e["ETS"][0] == (hits - chance) / (hits + misses + fa - chance)
    assert e["bias_trilinear"][0] == 0.5 and e["CSI_trilinear"][0] == 15 / 45 and e["POD_trilinear"][0] == 15 / 40
    assert e["FAR_trilinear"][0] == 5 / 20 and e["ETS_trilinear"][0] == (15 - 8) / (45 - 8)
    # useful scale: FSS_uniform is 0.7, 0.667 < 0.7 <= 0.75 at n = 3; the baseline never reaches it
    assert e["useful_scale_m"][0] == 750.0 and is_nan(e["useful_scale_m_trilinear"][0])
    # nobody but HR: bias 0, CSI 0, POD 0, FAR nan (no forecast event), useful scale absent
    assert (e["bias"][1], e["CSI"][1], e["POD"][1]) == (0.0, 0.0, 0.0) and is_nan(e["FAR"][1]) and is_nan(e["useful_scale_m"][1])
    assert e["f_trilinear"][1] == 0.0 and e["CSI_trilinear"][1] == 0.0
    # a table without baseline: its scores are nan
    table[..., 3:] = 0
    e = fss_from_sums(table, (1, 3, 5), (10.0, 20.0), 250.0, npos)["exceedance"]
    assert all(is_nan(e[k][0]) for k in EXCEEDANCE_COLUMNS if k.endswith("_trilinear")) and e["CSI"][0] == 0.5
    for bad_table, bad_scales in ((torch.zeros((2, 3, 4)), (1, 3, 5)), (torch.zeros((2, 2, 5)), (1, 3, 5)), (table, (3, 5, 9))):
        with pytest.raises(ValueError, match="table|scales"):
            fss_from_sums(bad_table, bad_scales, (10.0, 20.0), 250.0, npos)


# ---------------------------------------------------------------------------------------------------- 4. config
def test_section_parses_and_is_never_printed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        plain_cfg = Config(LOCAL_INI)
        plain, plain_str = plain_cfg.asINI(), str(plain_cfg)
        s = plain_cfg.fss
        assert s.present is False and s.on is False and "FSS" not in plain and s.thresholds is None
        cfg = Config(_ini_with(tmp_path, "[FSS]\nthresholds = [5, 10, 15, 20]\n"))
        s = cfg.fss
        assert s.present and s.on
        assert (s.thresholds, s.scales, s.per_level) == ([5.0, 10.0, 15.0, 20.0], [1, 3, 5, 9, 17, 33], False)
        assert cfg.asINI() == plain and str(cfg) == plain_str  # never printed
        full = Config(_ini_with(tmp_path, "[FSS]\nthresholds = 7.5\nscales = [1, 33]\nper_level = True\n"))
        s = full.fss
        assert (s.thresholds, s.scales, s.per_level) == ([7.5], [1, 33], True)
        w = "thresholds = [5, 10]\n"
        bad = {"": "thresholds must be given", "scales = [1, 3]\n": "thresholds must be given",
               "thresholds = [10, 5]\n": "thresholds must be strictly ascending", "thresholds = [5, 5]\n": "thresholds must be strictly",
               "thresholds = [0, 5]\n": "thresholds must be .*> 0", "thresholds = [-5]\n": "thresholds must be",
               "thresholds = [1, 2, 3, 4, 5, 6, 7, 8, 9]\n": "thresholds must hold 1 .. 8 entries, not 9",
               "thresholds = []\n": "thresholds must hold", "thresholds = fast\n": "thresholds must be a list of numbers",
               w + "scales = [1, 4]\n": "scales must be odd", w + "scales = [3, 5]\n": "scales must begin with 1",
               w + "scales = [1, 35]\n": "scales must not exceed 33, not 35", w + "scales = [1, 5, 3]\n": "scales must be strictly",
               w + "scales = [1, 3, 5, 7, 9, 11, 13, 15, 17]\n": "scales must hold 1 .. 8 entries, not 9",
               w + "scales = [1, 2.5]\n": "scales must be a list of integers", w + "scales = wide\n": "scales must be a list of numbers",
               w + "per_level = maybe\n": "per_level must be True or False"}
        for text, pattern in bad.items():
            with pytest.raises(ValueError, match=r"\[FSS\]:? " + pattern):
                Config(_ini_with(tmp_path, "[FSS]\n" + text))
        back = Config(LOCAL_INI)  # (the singleton is reset)
        assert back.fss.present is False and back.fss.thresholds is None and back.asINI() == plain
        assert tuple(back.fss.scales) == DEFAULT_SCALES
        assert ("fss", None) in Config._optional + Config._optional_later
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
            assert cfg.fss.on is False and "[FSS]" not in cfg.asINI()
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
    import numpy as np
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.config.config import FssConfig
    from gan_sr_wind_field_amd.fss import EXCEEDANCE_COLUMNS, FSS_COLUMNS, fss_from_sums, fss_tables, level_fss_reference
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.spectra import grid_spacing
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "fss", FssConfig())
    cfg.fss.setFssConfig(None)
    cfg.name = "same"
    avg_a = evaluate(cfg, ds)
    before = _snapshot(cfg.env.this_runs_folder)
    assert not any("fss" in os.path.basename(f) or "exceedance" in f for f in before)
    uvw = float(ds.UVW_MAX)
    thresholds, scales = [0.1 * uvw, 0.2 * uvw, 0.4 * uvw, 3.0 * uvw], [1, 3, 9]  # (the last one: nobody)
    fc = cfg.fss
    fc.present, fc.thresholds, fc.scales, fc.per_level = True, thresholds, scales, True
    fc.validate()
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
    assert new == ["same____exceedance.csv", "same____fss.csv", "same____fss_levels.csv"]

    X, Y, NZ = ds[0][1].shape[1:]
    d = grid_spacing(np.asarray(ds.x), np.asarray(ds.y))
    score, exc, levels = _rows("same", "fss"), _rows("same", "exceedance"), _rows("same", "fss_levels")
    assert score[0] == ["threshold", "scale"] + list(FSS_COLUMNS) and len(score) == 1 + 4 * 3
    assert exc[0] == ["threshold"] + list(EXCEEDANCE_COLUMNS) and len(exc) == 1 + 4
    assert levels[0] == ["level", "threshold", "scale"] + list(FSS_COLUMNS) and len(levels) == 1 + NZ * 4 * 3

    # the files: fss_from_sums of the reference on the same fields
    gan = wind_field_GAN_3D(cfg)
    gan.load_model(generator_load_path=cfg.env.generator_load_path, discriminator_load_path=None, state_load_path=None)
    gan.G.eval()
    t = fss_tables(uvw, thresholds)
    total = torch.zeros((NZ, 4, 3, 5), dtype=torch.float64)
    for i in range(len(ds)):
        LR, HR, Z = (ds[i][k][None] for k in (0, 1, 2))
        with torch.no_grad():
            SR = gan.G(LR, Z)
        TL = F.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear", align_corners=True)
        total += level_fss_reference(HR, SR, TL, t, scales)[0]
        if i == 0:  # the model's entry point: the same table
            assert torch.equal(gan.level_fss(HR, SR, LR, uvw), level_fss_reference(HR, SR, TL, t, scales))
    want = fss_from_sums(total.sum(dim=0), scales, thresholds, d, len(ds) * X * Y * NZ)
    assert [r for r in score[1:]] == [[str(want["fss"][c][k]) for c in ("threshold", "scale") + FSS_COLUMNS] for k in range(12)]
    assert [r for r in exc[1:]] == [[str(want["exceedance"][c][k]) for c in ("threshold",) + EXCEEDANCE_COLUMNS]
                                    for k in range(4)]
    for lvl in range(NZ):
        w = fss_from_sums(total[lvl], scales, thresholds, d, len(ds) * X * Y)["fss"]
        assert levels[1 + 12 * lvl:13 + 12 * lvl] == [[str(lvl)] + [str(w[c][k]) for c in ("threshold", "scale") + FSS_COLUMNS]
                                                      for k in range(12)]
    e = want["exceedance"]
    assert 0 < e["f_HR"][0] <= 1 and e["f_HR"][0] >= e["f_HR"][1] >= e["f_HR"][2] and e["f_HR"][3] == 0
    assert score[-1][3] == "nan" and exc[-1][4] == "nan"  # a threshold nobody reaches: nan, not an exception
    assert all(0 <= v <= 1 for v in want["fss"]["FSS"][:9])

    # without per_level two new files; the gan's defaults without the section
    fc.per_level, cfg.name = False, "two"
    evaluate(cfg, ds)
    assert sorted(f for f in os.listdir("test_output") if f.startswith("two____") and "metrics" not in f) == [
        "two____exceedance.csv", "two____fss.csv"]
    fc.setFssConfig(None)
    LR, HR, Z = (ds[0][k][None] for k in (0, 1, 2))
    TL = F.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear", align_corners=True)
    assert torch.equal(gan.level_fss(HR, HR, LR, uvw),
                       level_fss_reference(HR, HR, TL, fss_tables(uvw, [5.0, 10.0, 15.0, 20.0]), DEFAULT_SCALES))


# ---------------------------------------------------------------------------------------------------- 6. the ABI
def test_exports_header_and_wrapper_limits_agree():
    from gan_sr_wind_field_amd import _lib, fss, hip_ops

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_fss", "wsr_level_fss_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define WSR_FSS_MAX_THRESHOLDS {fss.MAX_THRESHOLDS}" in header
    assert f"#define WSR_FSS_MAX_SCALES {fss.MAX_SCALES}" in header
    assert f"#define WSR_FSS_MAX_SCALE {fss.MAX_SCALE}" in header
    assert "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "fss_kernels.h")) as f:
        kernels = f.read()
    assert f"constexpr int FS_TILE = {hip_ops.FSS_TILE};" in kernels
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " fss.hip" in mk and "fss.o: fss_kernels.h" in mk
    # the levels a workgroup stages: six with the widest halo in a launch of 512 workgroups, halved down to two below
    assert hip_ops.fss_level_chunk(64, 8, 8, 48, (1, 33)) == 6 and hip_ops.fss_level_chunk(1, 8, 8, 130, (1, 33)) == 2
    assert hip_ops.fss_level_chunk(8, 128, 128, 128, DEFAULT_SCALES) == 6 and hip_ops.fss_level_chunk(64, 128, 128, 128, (1,)) == 16
    # the built library exports both symbols (loading it needs no GPU)
    L = _lib.lib()
    assert hasattr(L, "wsr_level_fss") and hasattr(L, "wsr_level_fss_workspace_floats")
    wsf = L.wsr_level_fss_workspace_floats
    assert wsf(2, 5, 7, 3, 4, 6, 33) == 2 * 2 * 3 * 4 * 6 * 5 and wsf(1, 5, 7, 3, 1, 1, 1) == 2 * 3 * 5
    # 0 for arguments the entry refuses
    refused = [(0, 5, 7, 3, 4, 6, 33), (2, 0, 7, 3, 4, 6, 33), (2, 5, 7, -1, 4, 6, 33), (2, 5, 7, 3, 0, 6, 33),
               (2, 5, 7, 3, 9, 6, 33), (2, 5, 7, 3, 4, 0, 33), (2, 5, 7, 3, 4, 9, 33), (2, 5, 7, 3, 4, 6, 35),
               (2, 5, 7, 3, 4, 6, 32), (2, 5, 7, 3, 4, 6, 9), (2, 5, 7, 3, 4, 1, 3), (2, 5, 7, 3, 4, 2, 1),
               (65536, 5, 7, 3, 4, 6, 33), (1, 65536, 32768, 1, 4, 6, 33), (1, 32768, 32768, 2, 4, 6, 33)]
    for args in refused:
        assert wsf(*args) == 0, args
    assert math.prod((2, 3, 4, 6, 5)) * 2 == wsf(2, 5, 7, 3, 4, 6, 11)  # (six odd ascending scales fit below 11)
