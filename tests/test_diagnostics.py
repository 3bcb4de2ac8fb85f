"""[DIAGNOSTICS] on the CPU: the config section, ``level_sums_reference`` against two analytic identities and a
plain-numpy loop over voxels, ``profile_from_sums`` on a hand-made table, the evaluation loop with the section on a CPU
device, and the names the C ABI carries.

Shared with test_diagnostics_gpu.py: ``ref_level_sums`` - the fifteen sums in float64 with this file's own stencil code,
and the magnitude sums ``A`` of the bound

    |got - ref| <= LAMBDA * sqrt(K) * 2^-24 * A + 2^-100,      K = X * Y, the terms of one level

(kernel_bounds.py's convention).  ``A`` is the float64 sum of: the term itself for k = 0, 1, 2, 7; ||f|| + ||HR|| for
k = 3..6; h * (theta + 1) for k = 8, 9 (the angle's error is absolute: its cross product cancels); M^2 for k = 10..12
with M the stencil applied to |coefficients| and |values|; |zc| for k = 13 and |zc - zc_0| for k = 14.
``profile_bounds`` carries bounds of the sums through the formulas of ``profile_from_sums``.
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from kernel_bounds import LAMBDA, TINY, U_FP32
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained, metric_bounds


# ------------------------------------------------------------------------------------------------- shared references
def _deriv(f, co, dim):
    """row-wise derivative of f along ``dim`` on coordinates ``co`` (broadcastable to f, full along ``dim``): three-point
    non-uniform inside, one-sided at the ends, 0 on an axis of length 1 -> (derivative, the same stencil on magnitudes)"""
    n = f.shape[dim]
    if n < 2:
        return torch.zeros_like(f), torch.zeros_like(f)

    def sl(t, a, b):
        return t.narrow(dim, a, b - a)

    hl, hr = sl(co, 1, n - 1) - sl(co, 0, n - 2), sl(co, 2, n) - sl(co, 1, n - 1)
    den = hl * hr * (hl + hr)
    a, b, c = -(hr * hr) / den, (hr * hr - hl * hl) / den, (hl * hl) / den
    lo, mid, hi = sl(f, 0, n - 2), sl(f, 1, n - 1), sl(f, 2, n)
    inner = a * lo + b * mid + c * hi
    m_inner = a.abs() * lo.abs() + b.abs() * mid.abs() + c.abs() * hi.abs()
    h0, hn = sl(co, 1, 2) - sl(co, 0, 1), sl(co, n - 1, n) - sl(co, n - 2, n - 1)
    first, m_first = (sl(f, 1, 2) - sl(f, 0, 1)) / h0, (sl(f, 1, 2).abs() + sl(f, 0, 1).abs()) / h0.abs()
    last = (sl(f, n - 1, n) - sl(f, n - 2, n - 1)) / hn
    m_last = (sl(f, n - 1, n).abs() + sl(f, n - 2, n - 1).abs()) / hn.abs()
    return torch.cat((first, inner, last), dim=dim), torch.cat((m_first, m_inner, m_last), dim=dim)


def _div(f, x, y, zc):
    """f (B, 3, X, Y, NZ) float64 -> (div, M) (B, X, Y, NZ)"""
    dx, mx = _deriv(f[:, 0], x.view(1, -1, 1, 1), 1)
    dy, my = _deriv(f[:, 1], y.view(1, 1, -1, 1), 2)
    dz, mz = _deriv(f[:, 2], zc, 3)
    return dx + dy + dz, mx + my + mz


def ref_level_sums(HR, SR, TL, x, y, Z):
    """(sums, A), both float64 (B, NZ, 15), from the fp32 (or any) values given - see the module docstring"""
    h, s, t = (f[:, :3].detach().cpu().double() for f in (HR, SR, TL))
    x, y, zc = x.detach().cpu().double(), y.detach().cpu().double(), Z.detach().cpu().double()[:, 0]

    def norm(f):
        return torch.sqrt((f ** 2).sum(dim=1))

    def angle(a, b):
        cross = (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).abs()
        dot = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
        return torch.where((cross == 0) & (dot == 0), torch.zeros_like(dot), torch.atan2(cross, dot))

    nh, ns, nt = norm(h), norm(s), norm(t)
    hs = torch.sqrt(h[:, 0] ** 2 + h[:, 1] ** 2)
    th_s, th_t = angle(h, s), angle(h, t)
    (dh, mh), (ds, ms), (dt, mt) = (_div(f, x, y, zc) for f in (h, s, t))
    z0 = zc[..., :1]
    terms = (nh, norm(h - s), norm(h - t), ns - nh, nt - nh, (ns - nh).abs(), (nt - nh).abs(), hs, hs * th_s, hs * th_t,
             dh ** 2, ds ** 2, dt ** 2, zc, zc - z0)
    mags = (nh, norm(h - s), norm(h - t), ns + nh, nt + nh, ns + nh, nt + nh, hs, hs * (th_s + 1), hs * (th_t + 1),
            mh ** 2, ms ** 2, mt ** 2, zc.abs(), (zc - z0).abs())

    def per_level(vs):
        return torch.stack([v.sum(dim=(1, 2)) for v in vs], dim=-1)

    return per_level(terms), per_level(mags)


def sum_bounds(A, K):
    return LAMBDA * math.sqrt(K) * U_FP32 * A + TINY


def profile_bounds(sums, bnd, ncols, uvw):
    """allowed |difference| of every ``PROFILE_COLUMNS`` entry per level when sum k of ``sums`` (NZ, 15) moved by at most
    ``bnd[:, k]``: linear columns by b / n (times U); a ratio s8 / s7 by (b8 + (s8 / s7) b7) / (s7 - b7); sqrt(s / n) by
    sqrt(s / n) - sqrt(max(s - b, 0) / n), the larger of its two one-sided moves"""
    from gan_sr_wind_field_amd.diagnostics import PROFILE_COLUMNS

    s, b, n, U = sums.double(), bnd.double(), float(ncols), float(uvw)

    def ratio(k):
        den = (s[:, 7] - b[:, 7]).clamp(min=0)
        return torch.where(den > 0, (b[:, k] + s[:, k] / s[:, 7] * b[:, 7]) / den, torch.full_like(den, math.inf)) * 180 / math.pi

    def rms(k):
        return (torch.sqrt(s[:, k] / n) - torch.sqrt((s[:, k] - b[:, k]).clamp(min=0) / n)) * U

    cols = (b[:, 13] / n, b[:, 14] / n, b[:, 0] / n * U, b[:, 1] / n * U, b[:, 2] / n * U, b[:, 3] / n * U, b[:, 4] / n * U,
            b[:, 5] / n * U, b[:, 6] / n * U, ratio(8), ratio(9), rms(10), rms(11), rms(12))
    return {k: v.tolist() for k, v in zip(PROFILE_COLUMNS, cols)}


def random_case(B, X, Y, NZ, seed, noise=None, c=3):
    """fp32 HR, SR, TL (B, c, X, Y, NZ), non-uniform x, y and per-column increasing raw altitudes; ``noise``: SR = HR +
    noise * N(0, 1) (the cancellation in HR - SR), None: independent random fields"""
    g = torch.Generator().manual_seed(seed)
    HR = torch.randn((B, c, X, Y, NZ), generator=g)
    SR = torch.randn((B, c, X, Y, NZ), generator=g) if noise is None else HR + noise * torch.randn((B, c, X, Y, NZ), generator=g)
    TL = HR + 0.3 * torch.randn((B, c, X, Y, NZ), generator=g)
    x = torch.cumsum(150 + 100 * torch.rand(X, generator=g), 0)
    y = torch.cumsum(150 + 100 * torch.rand(Y, generator=g), 0)
    Z = (300 * torch.rand((B, 1, X, Y, 1), generator=g) + torch.cumsum(5 + 40 * torch.rand((B, 1, X, Y, NZ), generator=g), -1))
    return HR, SR, TL, x, y, Z.contiguous()


def linear_case(X, Y, NZ, seed, abc=(0.5, -0.25, 1.5)):
    """u = a x, v = b y, w = c zc on non-uniform dyadic coordinates (every product exact in fp32): div = a + b + c"""
    g = torch.Generator().manual_seed(seed)
    a, b, c = abc
    x = torch.cumsum(torch.randint(1, 9, (X,), generator=g).float() * 0.25, 0)
    y = torch.cumsum(torch.randint(1, 9, (Y,), generator=g).float() * 0.5, 0)
    Z = (torch.randint(0, 64, (1, 1, X, Y, 1), generator=g).float()
         + torch.cumsum(torch.randint(1, 9, (1, 1, X, Y, NZ), generator=g).float() * 0.125, -1)).contiguous()
    HR = torch.stack([(a * x).view(1, X, 1, 1).expand(1, X, Y, NZ), (b * y).view(1, 1, Y, 1).expand(1, X, Y, NZ),
                      c * Z[:, 0]], dim=1).contiguous()
    return HR, x, y, Z


def rotated(HR, phi):
    """HR turned about z by phi, formed in float64 and rounded once to fp32"""
    h = HR.double()
    return torch.stack([math.cos(phi) * h[:, 0] - math.sin(phi) * h[:, 1], math.sin(phi) * h[:, 0] + math.cos(phi) * h[:, 1],
                        h[:, 2]], dim=1).float()


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    plain = Config(LOCAL_INI).asINI()
    assert Config(LOCAL_INI).diagnostics.present is False and Config(LOCAL_INI).diagnostics.on is False
    assert "DIAGNOSTICS" not in plain
    cfg = Config(_ini_with(tmp_path, "[DIAGNOSTICS]\n"))
    d = cfg.diagnostics
    assert d.present and d.on and (d.level_profile, d.per_field) == (True, False)
    assert cfg.asINI() == plain + "\n[DIAGNOSTICS]\nlevel_profile = True\nper_field = False\n"
    cfg = Config(_ini_with(tmp_path, "[DIAGNOSTICS]\nlevel_profile = True\nper_field = True\n"))
    text = cfg.asINI()
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.diagnostics) == vars(cfg.diagnostics) and again.asINI() == text and again.diagnostics.per_field
    off = Config(_ini_with(tmp_path, "[DIAGNOSTICS]\nlevel_profile = False\n"))
    assert off.diagnostics.present and not off.diagnostics.on
    for key in ("level_profile", "per_field"):
        with pytest.raises(ValueError, match=rf"\[DIAGNOSTICS\] {key}"):
            Config(_ini_with(tmp_path, f"[DIAGNOSTICS]\n{key} = maybe\n"))
    with pytest.raises(ValueError, match=r"\[DIAGNOSTICS\] per_field"):
        Config(_ini_with(tmp_path, "[DIAGNOSTICS]\nlevel_profile = False\nper_field = True\n"))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.diagnostics.present is False and back.asINI() == plain


# ---------------------------------------------------------------------------------------------------- 2. the reference
def test_reference_linear_field_has_constant_divergence():
    from gan_sr_wind_field_amd.diagnostics import SUM_NAMES, level_sums_reference

    assert len(SUM_NAMES) == 15
    for (X, Y, NZ), abc in (((7, 6, 5), (0.5, -0.25, 1.5)), ((3, 1, 4), (2.0, 0.75, -0.5)), ((5, 4, 1), (1.0, 1.0, 3.0))):
        HR, x, y, Z = linear_case(X, Y, NZ, seed=X + NZ, abc=abc)
        s = level_sums_reference(HR, HR, HR, x, y, Z)
        assert s.shape == (1, NZ, 15) and s.dtype == torch.float64
        want = sum(v for v, n in zip(abc, (X, Y, NZ)) if n > 1)  # (an axis of length 1 contributes 0)
        rms = torch.sqrt(s[0, :, 10:13] / (X * Y))
        assert float((rms - abs(want)).abs().max()) <= 1e-12 * max(1.0, abs(want)), (X, Y, NZ)
        mine, _ = ref_level_sums(HR, HR, HR, x, y, Z)
        assert float(((mine - s).abs() / (mine.abs() + 1e-300)).max()) <= 1e-11


def test_reference_rotation_gives_the_angle():
    from gan_sr_wind_field_amd.diagnostics import level_sums_reference

    HR, _, TL, x, y, Z = random_case(1, 7, 6, 5, seed=3)
    for phi in (0.3, 2.5):
        SR = rotated(HR, phi).double()  # (unrounded enough: fp32 values taken as float64 inputs)
        s = level_sums_reference(HR.double(), SR, TL, x, y, Z)[0]
        n = 7 * 6
        assert float((s[:, 8] / s[:, 7] - phi).abs().max()) <= 1e-6        # direction error = phi (fp32-rounded SR)
        assert float((s[:, 3] / n).abs().max()) <= 1e-6                     # speed bias 0
        assert float((s[:, 1] - 2 * math.sin(phi / 2) * s[:, 7]).abs().max()) <= 1e-6 * float(s[:, 7].max())
    same = level_sums_reference(HR, HR, TL, x, y, Z)[0]
    assert bool((same[:, [1, 3, 5, 8]] == 0).all()) and torch.equal(same[:, 10], same[:, 11])


def test_reference_against_a_plain_numpy_loop():
    from gan_sr_wind_field_amd.diagnostics import level_sums_reference

    X, Y, NZ = 5, 4, 3
    HR, SR, TL, x, y, Z = random_case(1, X, Y, NZ, seed=9, c=4)
    SR[0, :2, 1, 1, 1] = 0.0  # theta(HR, 0) = 0
    got = level_sums_reference(HR, SR, TL, x, y, Z)[0].numpy()
    h, s, t = (f[0, :3].double().numpy() for f in (HR, SR, TL))
    xs, ys, zc = x.double().numpy(), y.double().numpy(), Z[0, 0].double().numpy()

    def d1(vals, co, i):
        n = len(co)
        if i == 0:
            return (vals[1] - vals[0]) / (co[1] - co[0])
        if i == n - 1:
            return (vals[-1] - vals[-2]) / (co[-1] - co[-2])
        hl, hr = co[i] - co[i - 1], co[i + 1] - co[i]
        den = hl * hr * (hl + hr)
        return (-(hr * hr) * vals[i - 1] + (hr * hr - hl * hl) * vals[i] + hl * hl * vals[i + 1]) / den

    def theta(a, b):
        cr, dt = abs(a[0] * b[1] - a[1] * b[0]), a[0] * b[0] + a[1] * b[1]
        return 0.0 if cr == 0 and dt == 0 else math.atan2(cr, dt)

    want = np.zeros((NZ, 15))
    for i in range(X):
        for j in range(Y):
            for k in range(NZ):
                hv, sv, tv = h[:, i, j, k], s[:, i, j, k], t[:, i, j, k]
                nh, ns, nt = (math.sqrt(float((v ** 2).sum())) for v in (hv, sv, tv))
                hs = math.hypot(hv[0], hv[1])
                div = [d1(f[0, :, j, k], xs, i) + d1(f[1, i, :, k], ys, j) + d1(f[2, i, j, :], zc[i, j], k) for f in (h, s, t)]
                want[k] += [nh, math.sqrt(float(((hv - sv) ** 2).sum())), math.sqrt(float(((hv - tv) ** 2).sum())), ns - nh,
                            nt - nh, abs(ns - nh), abs(nt - nh), hs, hs * theta(hv, sv), hs * theta(hv, tv), div[0] ** 2,
                            div[1] ** 2, div[2] ** 2, zc[i, j, k], zc[i, j, k] - zc[i, j, 0]]
    assert np.allclose(got, want, rtol=1e-11, atol=1e-11)
    mine, A = ref_level_sums(HR, SR, TL, x, y, Z)
    assert np.allclose(mine[0].numpy(), want, rtol=1e-11, atol=1e-11) and bool((A >= mine.abs() * (1 - 1e-12)).all())
    # fp32 evaluation of the same composition sits inside the bound of the GPU tests
    f32 = level_sums_reference(HR, SR, TL, x, y, Z, dtype=torch.float32)
    assert f32.dtype == torch.float32
    assert float(((f32.double() - mine).abs() / sum_bounds(A, X * Y)).max()) <= 1.0


# ---------------------------------------------------------------------------------------------------- 3. the profile
def test_profile_from_sums_on_a_hand_made_table():
    from gan_sr_wind_field_amd.diagnostics import PROFILE_COLUMNS, profile_from_sums

    assert PROFILE_COLUMNS == ("mean_altitude", "mean_height_above_lowest_level", "average_wind_speed", "pix", "trilinear_pix",
                               "speed_bias", "speed_bias_trilinear", "speed_abs_error", "speed_abs_error_trilinear",
                               "direction_error_deg", "direction_error_deg_trilinear", "rms_div_HR", "rms_div_SR",
                               "rms_div_trilinear")
    row0 = [8.0, 2.0, 4.0, -1.0, 1.0, 1.5, 2.5, 4.0, math.pi, 2 * math.pi, 16.0, 36.0, 64.0, 400.0, 0.0]
    row1 = [6.0, 1.0, 2.0, 0.5, -0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 4.0, 1.0, 800.0, 40.0]
    for table in ([row0, row1], torch.tensor([row0, row1], dtype=torch.float64)):
        p = profile_from_sums(table, 4, 10.0)
        assert tuple(p) == PROFILE_COLUMNS and all(len(v) == 2 and all(isinstance(e, float) for e in v) for v in p.values())
        assert p["mean_altitude"] == [100.0, 200.0] and p["mean_height_above_lowest_level"] == [0.0, 10.0]
        assert p["average_wind_speed"] == [20.0, 15.0] and p["pix"] == [5.0, 2.5] and p["trilinear_pix"] == [10.0, 5.0]
        assert p["speed_bias"] == [-2.5, 1.25] and p["speed_bias_trilinear"] == [2.5, -1.25]
        assert p["speed_abs_error"] == [3.75, 1.25] and p["speed_abs_error_trilinear"] == [6.25, 1.25]
        assert p["direction_error_deg"][0] == pytest.approx(45.0, rel=1e-15) and math.isnan(p["direction_error_deg"][1])
        assert p["direction_error_deg_trilinear"][0] == pytest.approx(90.0, rel=1e-15)
        assert math.isnan(p["direction_error_deg_trilinear"][1])
        assert p["rms_div_HR"] == [20.0, 0.0] and p["rms_div_SR"] == [30.0, 10.0] and p["rms_div_trilinear"] == [40.0, 5.0]


# ---------------------------------------------------------------------------------------------------- 4. the loop
def _profile(name, suffix=""):
    with open(os.path.join("test_output", f"{name}____level_profile{suffix}.csv")) as f:
        return [r.split(",") for r in f.read().strip().splitlines()]


def test_section_on_a_cpu_device_writes_the_profile(data_root, tmp_path, monkeypatch):  # noqa: F811
    from gan_sr_wind_field_amd.config.config import DiagnosticsConfig
    from gan_sr_wind_field_amd.diagnostics import PROFILE_COLUMNS
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "diagnostics", DiagnosticsConfig())
    cfg.diagnostics.setDiagnosticsConfig(None)
    cfg.name = "plain"
    avg_a = evaluate(cfg, ds)
    assert not any("level_profile" in f for f in os.listdir("test_output"))
    cfg.diagnostics.present, cfg.diagnostics.per_field = True, True
    cfg.name = "diag"
    avg_b = evaluate(cfg, ds)
    metrics = [open(os.path.join("test_output", f"{n}____metrics.csv")).read() for n in ("plain", "diag")]
    assert metrics[0] == metrics[1] and avg_a == avg_b  # the existing files: byte for byte
    rows = _profile("diag")
    NZ = ds[0][1].shape[-1]
    nvox = math.prod(ds[0][1].shape[1:])
    assert rows[0] == ["level"] + list(PROFILE_COLUMNS) and [r[0] for r in rows[1:]] == [str(k) for k in range(NZ)]
    vals = {k: [float(r[1 + i]) for r in rows[1:]] for i, k in enumerate(PROFILE_COLUMNS)}
    assert all(math.isfinite(v) for col in vals.values() for v in col)
    assert vals["mean_height_above_lowest_level"][0] == 0.0 and min(vals["rms_div_HR"]) > 0
    # the level means reproduce averages.csv: the same voxels, summed per level in double here and per field in fp32 there
    bnd = metric_bounds(avg_b, nvox)
    for k in ("pix", "trilinear_pix", "average_wind_speed"):
        mean = sum(vals[k]) / NZ
        assert abs(mean - avg_b[k]) <= bnd[k] + 2.0 ** -22 * abs(avg_b[k]), (k, mean, avg_b[k])
    # per field: fields x NZ rows; their means (root mean squares for the divergences) are the profile
    per = _profile("diag", "_fields")
    assert per[0] == ["field", "level"] + list(PROFILE_COLUMNS) and len(per) == 1 + len(ds) * NZ
    assert [r[0] for r in per[1::NZ]] == [ds[i][3] for i in range(len(ds))]
    for i, k in enumerate(PROFILE_COLUMNS):
        for lvl in range(NZ):
            col = [float(r[2 + i]) for r in per[1:] if int(r[1]) == lvl]
            if k.startswith("rms_div"):
                want = math.sqrt(sum(v * v for v in col) / len(col))
            elif k.startswith("direction"):
                assert min(col) - 1e-9 <= vals[k][lvl] <= max(col) + 1e-9  # (a speed-weighted mean of the fields' angles)
                continue
            else:
                want = sum(col) / len(col)
            assert vals[k][lvl] == pytest.approx(want, rel=1e-12, abs=1e-12), (k, lvl)


def gan_stub(x, y, scale=4):
    """what ``wind_field_GAN_3D.level_diagnostics`` uses of its object: the coordinates and the scale"""
    from types import SimpleNamespace

    return SimpleNamespace(x=x, y=y, cfg=SimpleNamespace(scale=scale))


def test_gan_level_diagnostics_on_a_cpu_device():
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.diagnostics import level_sums_reference
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    HR, SR, _, x, y, Z = random_case(2, 12, 8, 5, seed=4)
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    got = wind_field_GAN_3D.level_diagnostics(gan_stub(x, y), HR, SR, LR, Z)
    TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
    assert got.shape == (2, 5, 15) and got.dtype == torch.float64
    assert torch.equal(got, level_sums_reference(HR, SR, TL, x, y, Z))
    with pytest.raises(ValueError, match="feed_xy_niter"):
        wind_field_GAN_3D.level_diagnostics(gan_stub(None, None), HR, SR, LR, Z)


# ---------------------------------------------------------------------------------------------------- 5. the ABI
def test_exports_and_header_carry_the_new_names():
    from gan_sr_wind_field_amd import _lib

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_diagnostics", "wsr_level_diagnostics_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert "#define WSR_LEVEL_DIAG_SUMS 15" in header and "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        assert "diagnostics.hip" in f.read()
