"""[HUB_HEIGHT] without a GPU: the section, the tables, ``hub_height.hub_height_reference`` against an independent
per-column numpy loop built on ``np.interp`` (over h in linear mode, over ln h in log mode; the validity counts equal
count for count), ``hub_height_from_sums`` on hand-made tables, the three CSV files and the maps written from a stub
output, and the exports."""
import csv
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO
from hub_height_cases import CASES, HEIGHTS, KNOT_V, MODES, NAN, UVW, case, default_curve, make, plant_specials, tables
from test_eval import LOCAL_INI, _ini_with


def is_nan(v):
    return isinstance(v, float) and math.isnan(v)


# ---------------------------------------------------------------------------------------------------- 1. the section
def test_default_curve_from_its_formula():
    speeds, power = default_curve()
    assert speeds == [3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 25.0, 26.0]
    assert power[0] == 0.0 and power[-3:] == [1.0, 1.0, 0.0] and power[1] == (64 - 27) / 1701
    for v, p in zip(speeds[:10], power[:10]):
        assert p == (v ** 3 - 27.0) / (1728.0 - 27.0)
    assert all(b > a for a, b in zip(power[:10], power[1:10]))


def test_section_parses_and_is_never_printed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    try:
        plain_cfg = Config(LOCAL_INI)
        plain, plain_str = plain_cfg.asINI(), str(plain_cfg)
        s = plain_cfg.hub_height
        assert s.present is False and s.on is False and "HUB_HEIGHT" not in plain and s.heights is None
        cfg = Config(_ini_with(tmp_path, "[HUB_HEIGHT]\nheights = [50, 100, 150]\n"))
        s = cfg.hub_height
        assert s.present and s.on
        assert (s.heights, s.interp, s.air_density, s.per_field, s.write_maps) == ([50.0, 100.0, 150.0], "log", 1.225, False,
                                                                                  False)
        assert (s.curve_speeds, s.curve_power) == default_curve()
        assert cfg.asINI() == plain and str(cfg) == plain_str  # never printed
        full = Config(_ini_with(tmp_path, "[HUB_HEIGHT]\nheights = 80\ninterp = Linear\nair_density = 1.1\ncurve_speeds = "
                                          "[0, 10, 20]\ncurve_power = [0, 1, 0.5]\nper_field = True\nwrite_maps = True\n"))
        s = full.hub_height
        assert (s.heights, s.interp, s.air_density, s.per_field, s.write_maps) == ([80.0], "linear", 1.1, True, True)
        assert (s.curve_speeds, s.curve_power) == ([0.0, 10.0, 20.0], [0.0, 1.0, 0.5])
        h = "heights = [50, 100]\n"
        bad = {"": "heights must be given", "interp = log\n": "heights must be given",
               "heights = [100, 50]\n": "heights must be strictly ascending", "heights = [50, 50]\n": "heights must be strictly",
               "heights = [0, 50]\n": "heights must be .*> 0", "heights = [-5]\n": "heights must be",
               "heights = [1, 2, 3, 4, 5, 6, 7, 8, 9]\n": "heights must hold 1 .. 8 entries, not 9",
               "heights = []\n": "heights must hold", "heights = high\n": "heights must be a list of numbers",
               h + "interp = cubic\n": "interp must be linear or log", h + "air_density = 0\n": "air_density must be .*> 0",
               h + "air_density = -1.2\n": "air_density must be", h + "air_density = thin\n": "air_density must be a number",
               h + "curve_speeds = [0, 10]\n": "curve_speeds and curve_power must be given together",
               h + "curve_power = [0, 1]\n": "curve_speeds and curve_power must be given together",
               h + "curve_speeds = [5]\ncurve_power = [1]\n": "curve_speeds must hold 2 .. 32 knots, not 1",
               h + f"curve_speeds = {list(range(33))}\ncurve_power = {[0] * 33}\n": "curve_speeds must hold 2 .. 32 knots, not 33",
               h + "curve_speeds = [0, 10, 20]\ncurve_power = [0, 1]\n": "curve_power must hold one value per knot",
               h + "curve_speeds = [-1, 10]\ncurve_power = [0, 1]\n": "curve_speeds must be .*>= 0",
               h + "curve_speeds = [10, 10]\ncurve_power = [0, 1]\n": "curve_speeds must be strictly ascending",
               h + "curve_speeds = [0, 10]\ncurve_power = [0, 1.5]\n": "curve_power must be fractions",
               h + "curve_speeds = [0, 10]\ncurve_power = [-0.1, 1]\n": "curve_power must be fractions",
               h + "curve_speeds = fast\ncurve_power = [0, 1]\n": "curve_speeds must be a list of numbers",
               h + "per_field = maybe\n": "per_field must be True or False",
               h + "write_maps = maybe\n": "write_maps must be True or False"}
        for text, pattern in bad.items():
            with pytest.raises(ValueError, match=r"\[HUB_HEIGHT\]:? " + pattern):
                Config(_ini_with(tmp_path, "[HUB_HEIGHT]\n" + text))
        back = Config(LOCAL_INI)  # (the singleton is reset)
        assert back.hub_height.present is False and back.hub_height.heights is None and back.asINI() == plain
        assert ("hub_height", None) in Config._optional + Config._optional_later
    finally:
        Config(LOCAL_INI)


def test_reference_ini_files_still_parse():
    from gan_sr_wind_field_amd.config.config import Config

    folder = os.path.dirname(LOCAL_INI)
    try:
        for f in sorted(f for f in os.listdir(folder) if f.endswith(".ini")):
            cfg = Config(os.path.join(folder, f))
            assert cfg.hub_height.on is False and "[HUB_HEIGHT]" not in cfg.asINI()
    finally:
        Config(LOCAL_INI)


def test_tables_round_once_and_refuse():
    from gan_sr_wind_field_amd.hub_height import hub_height_tables

    t = tables()
    speeds, power = default_curve()
    assert t.heights.dtype == t.curve_v.dtype == t.curve_p.dtype == torch.float32
    assert t.heights.tolist() == list(HEIGHTS) and t.heights_m == HEIGHTS and t.UVW_MAX == UVW
    assert t.curve_v.tolist() == [float(np.float32(v / UVW)) for v in speeds]
    assert t.curve_p.tolist() == [float(np.float32(p)) for p in power]
    for kw, pattern in ((dict(UVW_MAX=0.0), "UVW_MAX"), (dict(UVW_MAX=NAN), "UVW_MAX"), (dict(heights=[]), "heights must hold"),
                        (dict(heights=[50.0, 50.0 + 1e-9]), "heights are not .* strictly ascending fp32"),
                        (dict(curve_speeds=[1.0, 1.0 + 1e-12], curve_power=[0, 1]), "curve_speeds are not .* strictly ascending fp32")):
        args = dict(UVW_MAX=UVW, heights=HEIGHTS, curve_speeds=speeds, curve_power=power)
        args.update(kw)
        with pytest.raises(ValueError, match="hub_height_tables: " + pattern):
            hub_height_tables(**args)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def loop_reference(HR, SR, TL, Z, terrain, t, interp):
    """The definition column by column with ``np.interp``: over h in linear mode, over ln h in log mode; heights above
    ground and validity in fp32, everything else in double -> sums (B, NH, 18), planes (B, NH, 7, X, Y)"""
    B, _, X, Y, NZ = HR.shape
    heights = t.heights.numpy()
    cv, cp = t.curve_v.double().numpy(), t.curve_p.double().numpy()
    f = [None if a is None else a[:, :2].numpy() for a in (HR, SR, TL)]
    z, g = Z.numpy(), terrain.numpy()
    sums = np.zeros((B, len(heights), 18))
    cols = np.zeros((B, len(heights), 7, X, Y))
    for b in range(B):
        for i in range(X):
            for j in range(Y):
                h = (z[b, 0, i, j] - g[i, j]).astype(np.float32)
                for k, q in enumerate(heights):
                    if not (h[0] <= q <= h[-1]) or np.isnan(h).any() or (interp == "log" and not h[0] > 0):
                        continue
                    hd, qd = h.astype(np.float64), np.float64(q)
                    xs, x = (np.log(hd), np.log(qd)) if interp == "log" else (hd, qd)
                    uv = [None if a is None else [np.interp(x, xs, a[b, c, i, j].astype(np.float64)) for c in (0, 1)]
                          for a in f]
                    V = [None if a is None else math.hypot(*a) for a in uv]
                    P = [None if v is None else float(np.interp(v, cv, cp)) for v in V]
                    s = sums[b, k]
                    s[0] += 1
                    cols[b, k, 6, i, j] = 1
                    for n in range(3):
                        if V[n] is None:
                            continue
                        s[1 + n] += V[n]
                        s[8 + n] += V[n] ** 3
                        s[11 + n] += P[n]
                        cols[b, k, n, i, j], cols[b, k, 3 + n, i, j] = V[n], P[n]
                        if n:
                            cross = abs(uv[0][0] * uv[n][1] - uv[0][1] * uv[n][0])
                            s[3 + n] += abs(V[n] - V[0])
                            s[5 + n] += (V[n] - V[0]) ** 2
                            s[13 + n] += abs(P[n] - P[0])
                            s[15 + n] += V[0] * math.atan2(cross, uv[0][0] * uv[n][0] + uv[0][1] * uv[n][1])
    return torch.from_numpy(sums), torch.from_numpy(cols)


def _assert_close(got, want, label):
    """double against double with another order of operations: 1e-9 of the largest entry of the row"""
    assert torch.equal(got[..., 0], want[..., 0]), f"{label}: the validity counts differ"
    tol = 1e-9 * want.abs().amax(dim=-1, keepdim=True).clamp(min=1e-30)
    assert bool(((got - want).abs() <= tol).all()), f"{label}: {float((got - want).abs().max())}"


@pytest.mark.parametrize("interp", MODES)
def test_reference_against_a_numpy_loop(interp):
    from gan_sr_wind_field_amd.hub_height import hub_height_reference
    from gan_sr_wind_field_amd.hip_ops import hub_height_columns_per_chunk

    t = tables()
    for k in (0, 1, 4):
        inputs = case(k)
        NZ = inputs[0].shape[-1]
        for label, args in ((f"case {k}", inputs), (f"case {k} with special columns",
                                                    plant_specials(inputs, hub_height_columns_per_chunk(NZ, 4))[:5])):
            sums, cols = hub_height_reference(*args, t, interp, with_columns=True)
            want, want_cols = loop_reference(*args, t, interp)
            _assert_close(sums, want, f"{label} {interp}")
            assert torch.equal(cols[:, :, 6], want_cols[:, :, 6]) and bool(((cols - want_cols).abs() <= 1e-12).all())
            assert cols.dtype == torch.float64 and sums.dtype == torch.float64
            assert torch.equal(sums, hub_height_reference(*args, t, interp))
    # without baseline: zeros in its sums and planes, the others unchanged
    HR, SR, TL, Z, terrain = case(0)
    full = hub_height_reference(HR, SR, TL, Z, terrain, t, interp)
    sums, cols = hub_height_reference(HR, SR, None, Z, terrain, t, interp, with_columns=True)
    tl = [3, 5, 7, 10, 13, 15, 17]
    rest = [k for k in range(18) if k not in tl]
    assert float(sums[..., tl].abs().sum()) == 0 and torch.equal(sums[..., rest], full[..., rest])
    assert float(cols[:, :, [2, 5]].abs().sum()) == 0
    assert not torch.isnan(full).any()  # (channel 2 and above are NaN: never read)


def test_all_cases_satisfy_their_conditions():
    for k in range(len(CASES)):
        case(k)


def test_special_columns_in_the_reference():
    """what each special column must give, height by height"""
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    t = tables()
    (B, X, Y, NZ), seed, _ = CASES[1]
    HR, SR, TL, Z, terrain, kinds = plant_specials(case(1), 25)
    assert sorted(set(kinds.flatten().tolist())) == list(range(-1, 11))
    for interp in MODES:
        _, cols = hub_height_reference(HR, SR, TL, Z, terrain, t, interp, with_columns=True)
        valid = cols[0, :, 6].reshape(4, X * Y)
        h = (Z[0, 0] - terrain[:, :, None]).reshape(X * Y, NZ)
        for c in range(X * Y):
            kind, qi = int(kinds[0, c]), c % 2
            q = HEIGHTS[qi]
            if kind == 0:  # on level NZ // 2: that level's value, bit for bit
                assert float(h[c, NZ // 2]) == q and valid[qi, c] == 1
                assert tuple(float(cols[0, qi, s].reshape(-1)[c]) for s in range(3)) == KNOT_V
            elif kind == 1:
                assert float(h[c, -1]) == q and valid[qi, c] == 1 and valid[qi + 1:, c].sum() == 0
            elif kind in (2, 5):
                assert valid[qi, c] == (0 if kind == 2 else 1)
            elif kind in (3, 4):
                assert valid[qi, c] == (1 if kind == 3 else 0)
            elif kind == 6:
                assert valid[:, c].tolist() == [0, 0, 1, 1]
            elif kind in (7, 8):
                assert valid[:, c].tolist() == ([1, 1, 1, 1] if interp == "linear" else [0, 0, 0, 0])
            elif kind in (9, 10):
                assert valid[:, c].sum() == 0


# ---------------------------------------------------------------------------------------------------- 3. the columns
def test_columns_from_hand_made_sums():
    from gan_sr_wind_field_amd.hub_height import COLUMNS, SUMS, hub_height_from_sums

    t = tables((50.0, 100.0, 200.0), 20.0)
    table = torch.zeros((3, 18), dtype=torch.float64)
    row = dict(n_valid=40, V_HR=20.0, V_SR=18.0, V_TL=16.0, absdV_SR=4.0, absdV_TL=6.0, sqdV_SR=1.6, sqdV_TL=3.6, V3_HR=5.0,
               V3_SR=4.0, V3_TL=2.5, P_HR=24.0, P_SR=20.0, P_TL=12.0, absdP_SR=6.0, absdP_TL=12.0,
               angle_SR=20.0 * math.radians(9.0), angle_TL=20.0 * math.radians(18.0))
    table[0] = torch.tensor([row[k] for k in SUMS], dtype=torch.float64)
    table[1] = table[0] * 2  # twice the columns: the same means ...
    table[1, 1:4] *= 2.0     # ... but twice the speeds
    col = hub_height_from_sums(table, t, 1.2, 100)
    assert tuple(col) == COLUMNS and all(len(v) == 3 for v in col.values())
    assert col["height_m"] == [50.0, 100.0, 200.0] and col["valid_fraction"] == [0.4, 0.8, 0.0]
    assert (col["speed_HR"][0], col["speed_SR"][0], col["speed_trilinear"][0]) == (10.0, 9.0, 8.0)
    assert col["speed_bias"][0] == -1.0 and col["speed_bias_trilinear"][0] == -2.0
    assert col["speed_mae"][0] == 2.0 and col["speed_mae_trilinear"][0] == 3.0
    assert col["speed_rmse"][0] == pytest.approx(math.sqrt(0.04) * 20.0, rel=1e-15)
    assert col["speed_rmse_trilinear"][0] == pytest.approx(math.sqrt(0.09) * 20.0, rel=1e-15)
    assert col["direction_error_deg"][0] == pytest.approx(9.0, rel=1e-14)
    assert col["direction_error_deg_trilinear"][0] == pytest.approx(18.0, rel=1e-14)
    assert col["power_density_HR"][0] == 0.5 * 1.2 * (5.0 / 40) * 8000.0
    assert col["power_density_SR"][0] == 0.5 * 1.2 * (4.0 / 40) * 8000.0
    assert col["power_density_rel_error"][0] == pytest.approx(-0.2, rel=1e-14)
    assert col["power_density_rel_error_trilinear"][0] == pytest.approx(-0.5, rel=1e-14)
    assert (col["capacity_factor_HR"][0], col["capacity_factor_SR"][0], col["capacity_factor_trilinear"][0]) == (0.6, 0.5, 0.3)
    assert col["capacity_factor_error"][0] == pytest.approx(-0.1, rel=1e-14) and col["power_mae"][0] == 0.15
    assert col["capacity_factor_error_trilinear"][0] == pytest.approx(-0.3, rel=1e-14) and col["power_mae_trilinear"][0] == 0.3
    # the shear exponent against the next lower height: the mean speed doubles from 50 to 100 m
    assert all(is_nan(col[f"shear_exponent_{s}"][0]) for s in ("HR", "SR", "trilinear"))
    assert all(col[f"shear_exponent_{s}"][1] == pytest.approx(1.0, rel=1e-14) for s in ("HR", "SR", "trilinear"))
    # no valid column: nan everywhere but the height and the fraction
    for k in COLUMNS[2:]:
        assert is_nan(col[k][2]), k
    # a table without baseline: its columns are nan, the others stay
    table[:, [3, 5, 7, 10, 13, 15, 17]] = 0
    lone = hub_height_from_sums(table, t, 1.2, 100)
    for k in COLUMNS:
        if "trilinear" in k:
            assert all(is_nan(v) for v in lone[k]), k
        else:
            assert lone[k][:2] == col[k][:2], k
    for bad in (torch.zeros((2, 18)), torch.zeros((3, 17)), torch.zeros((3,))):
        with pytest.raises(ValueError, match="table"):
            hub_height_from_sums(bad, t, 1.2, 100)


# ---------------------------------------------------------------------------------------------------- 4. the files
def test_stub_output_writes_the_files(tmp_path):
    from gan_sr_wind_field_amd.hub_height import COLUMNS, hub_height_from_sums, hub_height_reference
    from gan_sr_wind_field_amd.test import _HubHeight

    t = tables(HEIGHTS + (590.0,))  # (590 m: above most columns in both fields)
    NH = 5
    HR, SR, TL, Z, terrain = case(0)
    B, _, X, Y, NZ = HR.shape
    x, y = np.arange(X) * 200.0, np.arange(Y) * 200.0
    calls = []

    def fn(*a):
        calls.append(1)
        return hub_height_reference(*a, terrain, t, "log", True)

    folder = str(tmp_path)
    with open(os.path.join(folder, "averages_hub_height.csv"), "w") as f:  # (an earlier run's rows stay)
        f.write("Name," + ",".join(COLUMNS) + "\nearlier,row\n")
    with _HubHeight(fn, t, 1.225, True, True, (x, y), "stub", "", folder) as o:
        for b in range(B):
            o.add([f"field{b}"], SimpleNamespace(HR=HR[b:b + 1], SR=SR[b:b + 1], TL=TL[b:b + 1], Z=Z[b:b + 1]))
            o.flush()
    assert len(calls) == B

    def rows(name):
        with open(os.path.join(folder, name)) as f:
            return list(csv.reader(f))

    sums, cols = hub_height_reference(HR, SR, TL, Z, terrain, t, "log", True)
    want = hub_height_from_sums(sums.sum(dim=0), t, 1.225, B * X * Y)
    whole = rows("stub____hub_height.csv")
    assert whole[0] == list(COLUMNS) and len(whole) == 1 + NH
    assert whole[1:] == [[str(want[c][k]) for c in COLUMNS] for k in range(NH)]
    fields = rows("stub____hub_height_fields.csv")
    assert fields[0] == ["field"] + list(COLUMNS) and len(fields) == 1 + B * NH
    for b in range(B):
        w = hub_height_from_sums(sums[b], t, 1.225, X * Y)
        assert fields[1 + NH * b:1 + NH * (b + 1)] == [[f"field{b}"] + [str(w[c][k]) for c in COLUMNS] for k in range(NH)]
    av = rows("averages_hub_height.csv")
    assert av[0] == ["Name"] + list(COLUMNS) and av[1] == ["earlier", "row"] and av[2:] == [["stub"] + r for r in whole[1:]]
    m = np.load(os.path.join(folder, "stub____hub_height_maps.npz"))
    assert sorted(m.files) == ["capacity_factor", "heights", "speed", "valid_fraction", "x", "y"]
    assert m["heights"].tolist() == list(HEIGHTS) + [590.0] and m["x"].tolist() == x.tolist() and m["y"].tolist() == y.tolist()
    assert m["valid_fraction"].shape == (NH, X, Y) and m["speed"].shape == m["capacity_factor"].shape == (NH, 3, X, Y)
    n = cols[:, :, 6].sum(dim=0)
    assert np.array_equal(m["valid_fraction"], (n / B).numpy())
    assert np.array_equal(np.isnan(m["speed"][:, 0]), (n == 0).numpy()) and bool((n == 0).any()) and bool((n == B).any())
    k = 0  # 10 m: every column of every field is valid, so the map averages to the file's speed
    assert float(n[k].min()) == B
    for s, name in enumerate(("speed_HR", "speed_SR", "speed_trilinear")):
        assert float(m["speed"][k, s].mean()) == pytest.approx(want[name][k], rel=1e-12)
    assert float(m["capacity_factor"][k, 0].mean()) == pytest.approx(want["capacity_factor_HR"][k], rel=1e-12)
    # without per_field and write_maps: the two files only, the function returns the table alone; the raw suffix
    with _HubHeight(lambda *a: hub_height_reference(*a, terrain, t, "linear"), t, 1.225, False, False, (x, y), "lean",
                    "_reverse_interpolate", folder) as o:
        o.add(["a", "b"], SimpleNamespace(HR=HR, SR=SR, TL=TL, Z=Z))
    assert sorted(f for f in os.listdir(folder) if "lean" in f) == ["lean____hub_height_reverse_interpolate.csv"]
    assert rows("averages_hub_height_reverse_interpolate.csv")[1][0] == "lean"
    assert rows("lean____hub_height_reverse_interpolate.csv")[1:] != whole[1:]  # (another interpolation)


def test_gan_entry_on_a_cpu_device():
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.config.config import HubHeightConfig
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    HR, SR, _, Z, terrain = make(2, 12, 8, 5, seed=4, channels=(3, 3, 3))
    LR = 0.3 * torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
    hc = HubHeightConfig()
    hc.load(None)
    stub = SimpleNamespace(cfg=SimpleNamespace(scale=4, hub_height=hc))
    got = wind_field_GAN_3D.hub_height(stub, HR, SR, LR, Z, terrain, 20.0)  # (no section: 50, 100, 150 m, log)
    assert torch.equal(got, hub_height_reference(HR, SR, TL, Z, terrain, tables((50.0, 100.0, 150.0), 20.0), "log"))
    hc.present, hc.heights, hc.interp, hc.curve_speeds, hc.curve_power = True, [10.0, 60.0], "linear", [0.0, 12.0], [0.0, 1.0]
    got, cols = wind_field_GAN_3D.hub_height(stub, HR, SR, LR, Z, terrain, 20.0, with_columns=True)
    t = tables((10.0, 60.0), 20.0, ([0.0, 12.0], [0.0, 1.0]))
    want, want_cols = hub_height_reference(HR, SR, TL, Z, terrain, t, "linear", True)
    assert torch.equal(got, want) and torch.equal(cols, want_cols) and got.shape == (2, 2, 18)
    hc.load(None)


# ---------------------------------------------------------------------------------------------------- 5. the ABI
def test_exports_header_and_wrapper_limits_agree():
    from gan_sr_wind_field_amd import _lib, hip_ops, hub_height

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_hub_height", "wsr_hub_height_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    for macro, value in (("SUMS", hub_height.NS), ("PLANES", hub_height.PLANES), ("MAX_HEIGHTS", hub_height.MAX_HEIGHTS),
                         ("MAX_KNOTS", hub_height.MAX_KNOTS), ("MAX_NZ", hub_height.MAX_NZ)):
        assert f"#define WSR_HUB_HEIGHT_{macro} {value}\n" in header
    assert "#define WSR_ABI_VERSION 9" in header and len(hub_height.SUMS) == hub_height.NS
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "hub_height_kernels.h")) as f:
        assert f"constexpr int HH_BLOCK = {hip_ops.HUB_HEIGHT_BLOCK};" in f.read()
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " hub_height.hip" in mk and "hub_height.o: hub_height_kernels.h" in mk
    assert hip_ops.hub_height_columns_per_chunk(10, 3) == 25 and hip_ops.hub_height_columns_per_chunk(128, 8) == 2
    assert hip_ops.hub_height_columns_per_chunk(2, 8) == 32
    # the built library exports both symbols (loading it needs no GPU)
    L = _lib.lib()
    wsf = L.wsr_hub_height_workspace_floats
    assert wsf(2, 7, 6, 5, 4) == 2 * 1 * 4 * 18 and wsf(1, 16, 16, 10, 4) == 11 * 4 * 18
    assert wsf(1, 70, 60, 128, 3) == 2048 * 3 * 18  # (the cap on the partial rows)
    for args in ((0, 7, 6, 5, 4), (2, 0, 6, 5, 4), (2, 7, -1, 5, 4), (2, 7, 6, 1, 4), (2, 7, 6, 129, 4), (2, 7, 6, 5, 0),
                 (2, 7, 6, 5, 9), (65536, 7, 6, 5, 4), (1, 32769, 6, 5, 4), (1, 32768, 32768, 2, 4)):
        assert wsf(*args) == 0, args
