"""[SSIM] without a GPU: the section, the tap table, ``ssim.level_ssim_reference`` against a plain Python loop over the
positions and against closed forms, ``ssim_from_sums`` on a hand-made table, ``test()`` and a validation epoch on a CPU
device, the exports - and the bound of tests/test_ssim_gpu.py (derived in tests/ssim_bounds.py) evaluated on the CPU:

* sound: the same formulas composed in torch fp32 (``level_ssim_reference(..., dtype=torch.float32)``) stay within it at
  every shape of the GPU list, for both kinds of input of the GPU tests;
* with teeth: at seven probe shapes (windows 3 to 11; independent uniform fields, and smooth fields with 2 % noise) the
  float64 table of a wrong evaluation - SR and TL shifted by one voxel in x, and separately in y, before the moments -
  differs from the right one by at least 10 times the bound in every (sample, level, component) sum.  The seeds are fixed
  ones for which both conditions hold (``TEETH_CASES``).

Measured when the tests were written: worst fp32 |err| / bound 1.6e-2 over all sums (one position, 3 x 3 x 4), 1.0e-2 on the
probe inputs; mutation / bound between 20 (35 x 35, uniform fields) and 12 700.
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from kernel_bounds import assert_within
from ssim_bounds import GPU_CASES, NS, TEETH_CASES, _windowed, case_data, case_id, constant_planes, fields, ref_ssim
from test_data_and_train import data_root  # noqa: F401  (a fixture)
from test_eval import LOCAL_INI, _ini_with, _trained


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_and_is_never_printed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    plain_cfg = Config(LOCAL_INI)
    plain, plain_str = plain_cfg.asINI(), str(plain_cfg)
    assert plain_cfg.ssim.present is False and plain_cfg.ssim.on is False and "SSIM" not in plain
    cfg = Config(_ini_with(tmp_path, "[SSIM]\n"))
    s = cfg.ssim
    assert s.present and s.on
    assert (s.window_size, s.sigma, s.data_range, s.per_level, s.validation) == (11, 1.5, 2.0, False, True)
    assert cfg.asINI() == plain and str(cfg) == plain_str  # never printed
    full = Config(_ini_with(tmp_path, "[SSIM]\nwindow_size = 7\nsigma = 1.0\ndata_range = 1.5\nper_level = True\n"
                                      "validation = False\n"))
    s = full.ssim
    assert (s.window_size, s.sigma, s.data_range, s.per_level, s.validation) == (7, 1.0, 1.5, True, False)
    assert str(s) == "[SSIM]\nwindow_size = 7\nsigma = 1.0\ndata_range = 1.5\nper_level = True\nvalidation = False\n"
    bad = {"window_size = 4": "window_size.*4", "window_size = 1": "window_size.*1", "window_size = 17": "window_size.*17",
           "window_size = wide": "window_size.*integer", "sigma = 0": "sigma.*0", "sigma = -1.5": "sigma.*-1.5",
           "sigma = nan": "sigma", "data_range = 0": "data_range.*0", "data_range = big": "data_range.*number",
           "per_level = maybe": "per_level.*True or False", "validation = 2": "validation.*True or False"}
    for line, pattern in bad.items():
        with pytest.raises(ValueError, match=r"\[SSIM\] " + pattern):
            Config(_ini_with(tmp_path, f"[SSIM]\n{line}\n"))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.ssim.present is False and back.ssim.window_size == 11 and back.asINI() == plain


# ---------------------------------------------------------------------------------------------------- 2. the definition
def test_taps_are_the_normalised_gaussian_rounded_once():
    from gan_sr_wind_field_amd.ssim import taps

    for win, sigma in ((3, 0.8), (5, 1.2), (11, 1.5), (15, 2.0)):
        g = taps(win, sigma)
        assert g.dtype == torch.float32 and g.shape == (win,)
        w = [math.exp(-((k - (win - 1) / 2) ** 2) / (2 * sigma * sigma)) for k in range(win)]
        want = torch.tensor([v / math.fsum(w) for v in w], dtype=torch.float64)
        assert float((g.double() - want).abs().max()) <= 2.0 ** -24 * float(want.max())
        assert torch.equal(g, g.flip(0)) and abs(float(g.double().sum()) - 1) < win * 2.0 ** -25
    for win, sigma in ((4, 1.0), (1, 1.0), (17, 1.0), (5, 0.0), (5, -1.0)):
        with pytest.raises(ValueError, match=r"\d"):
            taps(win, sigma)


def _loop_reference(HR, SR, TL, win, sigma, L):
    """the definition, position by position, in Python floats"""
    from gan_sr_wind_field_amd.ssim import taps

    g = [float(v) for v in taps(win, sigma)]
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    B, _, X, Y, NZ = HR.shape
    out = torch.zeros((B, NZ, 3, NS), dtype=torch.float64)
    for b in range(B):
        for z in range(NZ):
            for c in range(3):
                a = HR[b, c, :, :, z].tolist()
                for pair, F in enumerate((SR, TL)):
                    s = F[b, c, :, :, z].tolist()
                    for x in range(X - win + 1):
                        for y in range(Y - win + 1):
                            m = [0.0] * 5
                            for i in range(win):
                                for j in range(win):
                                    w, p, q = g[i] * g[j], a[x + i][y + j], s[x + i][y + j]
                                    for n, v in enumerate((p, q, p * p, q * q, p * q)):
                                        m[n] += w * v
                            mua, mus = m[0], m[1]
                            va, vs, cov = m[2] - mua * mua, m[3] - mus * mus, m[4] - mua * mus
                            l = (2 * mua * mus + C1) / (mua * mua + mus * mus + C1)
                            cs = (2 * cov + C2) / (va + vs + C2)
                            out[b, z, c, 2 * pair] += l * cs
                            out[b, z, c, 2 * pair + 1] += cs
    return out


def test_reference_against_a_plain_python_loop():
    from gan_sr_wind_field_amd.ssim import level_ssim_reference

    HR, SR, TL = (t.double() for t in fields(2, 5, 4, 3, seed=11, kind="uniform", c=4))
    got = level_ssim_reference(HR, SR, TL, 3, 1.0, 2.0)
    assert got.shape == (2, 3, 3, NS) and got.dtype == torch.float64
    want = _loop_reference(HR, SR, TL, 3, 1.0, 2.0)
    assert float((got - want).abs().max()) < 1e-13 * 6
    other = level_ssim_reference(HR, SR, TL, 3, 1.0, 1.0)  # (the data range enters)
    assert float((other - _loop_reference(HR, SR, TL, 3, 1.0, 1.0)).abs().max()) < 1e-13 * 6 and not torch.allclose(other, got)
    # the float64 evaluation of the tests is a third implementation
    ref, _ = ref_ssim(HR.float(), SR.float(), TL.float(), 3, 1.0)
    assert float((level_ssim_reference(HR.float(), SR.float(), TL.float(), 3, 1.0) - ref).abs().max()) < 1e-12


def test_analytic_cases():
    from gan_sr_wind_field_amd.ssim import constants, level_ssim_reference, n_positions, taps

    B, X, Y, NZ, win, sigma = 1, 9, 8, 2, 5, 1.2
    npos = n_positions(X, Y, win)
    C1, C2 = constants(2.0)
    assert (C1, C2) == (0.02 ** 2, 0.06 ** 2) and npos == 5 * 4
    ones = torch.ones((B, 3, X, Y, NZ), dtype=torch.float64)
    p, q = 0.5, -0.25
    for w, sg in ((win, sigma), (3, 1.0), (7, 1.0)):  # (the closed form takes the sum of the fp32 taps along)
        got = level_ssim_reference(p * ones, q * ones, p * ones, w, sg) / n_positions(X, Y, w)
        l, cs = constant_planes(p, q, w, sg)
        assert abs(l - (2 * p * q + C1) / (p * p + q * q + C1)) < 1e-6 and abs(cs - 1) < 1e-3
        assert torch.allclose(got[..., 0], torch.full_like(got[..., 0], l * cs), rtol=0, atol=1e-12)
        assert torch.allclose(got[..., 1], torch.full_like(got[..., 1], cs), rtol=0, atol=1e-12)
        assert torch.allclose(got[..., 2:], torch.ones_like(got[..., 2:]), rtol=0, atol=1e-12)  # the pair (p, p): 1
    # SR = alpha HR: mu_s = alpha mu_a, var_s = alpha^2 var_a, cov = alpha var_a
    HR = fields(B, X, Y, NZ, seed=5, kind="uniform")[0].double()
    alpha = 0.5
    got = level_ssim_reference(HR, alpha * HR, HR, win, sigma)
    g = taps(win, sigma).double().numpy()
    a = np.ascontiguousarray(HR.numpy().transpose(0, 4, 1, 2, 3))
    mu = _windowed(a, g)
    var = _windowed(a * a, g) - mu * mu
    l = (2 * alpha * mu * mu + C1) / ((1 + alpha * alpha) * mu * mu + C1)
    cs = (2 * alpha * var + C2) / ((1 + alpha * alpha) * var + C2)
    assert torch.allclose(got[..., 0], torch.from_numpy((l * cs).sum(axis=(-2, -1))), rtol=1e-12, atol=0)
    assert torch.allclose(got[..., 1], torch.from_numpy(cs.sum(axis=(-2, -1))), rtol=1e-12, atol=0)
    assert float(got[..., 1].max()) < npos  # (a damped field loses contrast)
    assert torch.allclose(got[..., 2:], torch.full_like(got[..., 2:], float(npos)), rtol=0, atol=1e-11)  # TL = HR: 1
    for bad in ((HR[:, :, :4], 5), (HR, 4), (HR, 17)):
        with pytest.raises(ValueError, match=r"\d"):
            level_ssim_reference(bad[0], bad[0], bad[0], bad[1], sigma)


def test_ssim_from_sums_on_a_hand_made_table():
    from gan_sr_wind_field_amd.ssim import SSIM_COLUMNS, SSIM_SUMS, columns_from_sums, ssim_from_sums

    assert SSIM_SUMS == ("ssim_sr", "cs_sr", "ssim_tl", "cs_tl")
    # NZ = 2, npos = 10: level 0 holds (component c, sum j) -> c + j, level 1 twice that
    t = torch.tensor([[[c + j for j in range(4)] for c in range(3)], [[2 * (c + j) for j in range(4)] for c in range(3)]],
                     dtype=torch.float64)
    m = ssim_from_sums(t, 10)
    assert m["levels"] == [[(3 + 3 * j) / 30 for j in range(4)], [(6 + 6 * j) / 30 for j in range(4)]]
    assert m["mean"] == pytest.approx([(9 + 9 * j) / 60 for j in range(4)], rel=1e-15)
    assert m["components"] == [[pytest.approx(3 * (c + j) / 20, rel=1e-15) for j in range(4)] for c in range(3)]
    assert ssim_from_sums(t.tolist(), 10) == m
    # a sum of tables over 3 fields, and a stack of them, count as more planes
    assert ssim_from_sums(3 * t, 30)["mean"] == pytest.approx(m["mean"], rel=1e-15)
    assert ssim_from_sums(torch.stack([t, t, t]), 30)["mean"] == pytest.approx(m["mean"], rel=1e-15)
    row = columns_from_sums(t, 10)
    assert len(row) == len(SSIM_COLUMNS) == 7
    assert row == [m["mean"][0], m["mean"][2], m["mean"][1], m["mean"][3]] + [m["components"][c][0] for c in range(3)]
    with pytest.raises(ValueError, match="table"):
        ssim_from_sums(torch.zeros((2, 3, 5)), 10)


# ---------------------------------------------------------------------------------------------------- 3. the bound
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_the_bound_holds_for_fp32_on_the_cpu(case, kind):
    from gan_sr_wind_field_amd.ssim import level_ssim_reference

    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, TL, ref, bnd = case_data(case, kind)
    assert ref.shape == bnd.shape == (B, NZ, 3, NS) and bool((bnd > 0).all())
    got = level_ssim_reference(HR, SR, TL, win, sigma, 2.0, dtype=torch.float32)
    assert_within(got, ref, bnd, f"ssim fp32 on the CPU vs float64[{case_id(case)} {kind}]", kind="sums")


@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("case", TEETH_CASES, ids=case_id)
def test_the_bound_has_teeth(case, kind):
    from gan_sr_wind_field_amd.ssim import level_ssim_reference

    (B, X, Y, NZ), (win, sigma), seed = case
    HR, SR, TL = fields(B, X, Y, NZ, seed=seed, kind=kind, noise=2e-2)
    ref, bnd = ref_ssim(HR, SR, TL, win, sigma)
    got = level_ssim_reference(HR, SR, TL, win, sigma, 2.0, dtype=torch.float32)
    worst = assert_within(got, ref, bnd, f"ssim fp32 on the CPU vs float64, teeth inputs[{case_id(case)} {kind}]", kind="sums")
    least = math.inf
    for axis in (2, 3):  # the wrong evaluation: SR and TL one voxel off along x, then along y
        wrong, _ = ref_ssim(HR, torch.roll(SR, 1, dims=axis), torch.roll(TL, 1, dims=axis), win, sigma)
        ratio = (wrong - ref).abs() / bnd
        least = min(least, float(ratio.min()))
        assert bool((ratio >= 10).all()), (case, kind, axis, float(ratio.min()))
    print(f"[bound] {case_id(case)} {kind}: fp32 |err| / bound {worst:.3g}, mutation / bound >= {least:.3g}")


# ---------------------------------------------------------------------------------------------------- 4. the loops
def _rows(name, what):
    with open(os.path.join("test_output", f"{name}____{what}.csv")) as f:
        return [r.split(",") for r in f.read().strip().splitlines()]


def test_section_on_a_cpu_device_writes_the_files(data_root, tmp_path, monkeypatch):  # noqa: F811
    from gan_sr_wind_field_amd.config.config import SsimConfig
    from gan_sr_wind_field_amd.ssim import SSIM_COLUMNS, level_ssim_reference, n_positions
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "ssim", SsimConfig())
    cfg.ssim.setSsimConfig(None)
    cfg.name = "plain"
    avg_a = evaluate(cfg, ds)
    assert not any("ssim" in f for f in os.listdir("test_output"))
    cfg.ssim.present, cfg.ssim.per_level, cfg.ssim.window_size, cfg.ssim.sigma = True, True, 7, 1.0
    cfg.name = "ssim"
    avg_b = evaluate(cfg, ds)
    metrics = [open(os.path.join("test_output", f"{n}____metrics.csv")).read() for n in ("plain", "ssim")]
    assert metrics[0] == metrics[1] and avg_a == avg_b  # the existing files: byte for byte
    X, Y, NZ = ds[0][1].shape[1:]
    rows = _rows("ssim", "ssim")
    assert rows[0] == ["field"] + list(SSIM_COLUMNS) and len(rows) == 1 + len(ds)
    assert [r[0] for r in rows[1:]] == [r[0] for r in _rows("ssim", "metrics")[1:]]
    vals = [[float(v) for v in r[1:]] for r in rows[1:]]
    for v in vals:
        assert all(-1 <= x <= 1 for x in v) and v[0] == pytest.approx(sum(v[4:]) / 3, rel=1e-12)
    # the truth against itself: 1; and the per-field rows reproduce the averages
    HR = ds[0][1][None]
    same = level_ssim_reference(HR, HR, HR, 7, 1.0) / n_positions(X, Y, 7)
    assert torch.allclose(same, torch.ones_like(same), rtol=0, atol=1e-9)
    av = open(os.path.join("test_output", "averages_ssim.csv")).read().strip().splitlines()
    assert av[0] == "Name,Average SSIM,Average SSIM_trilinear,Average CS,Average CS_trilinear" and len(av) == 2
    name, *means = av[1].split(",")
    assert name == "ssim"
    for k, m in enumerate(means):
        assert float(m) == pytest.approx(sum(v[k] for v in vals) / len(vals), rel=1e-12)
    per = _rows("ssim", "ssim_levels")
    assert per[0] == ["level"] + list(SSIM_COLUMNS) and [r[0] for r in per[1:]] == [str(k) for k in range(NZ)]
    for k in range(len(SSIM_COLUMNS)):  # the mean over the levels of the per-level file is the mean over the fields
        assert sum(float(r[1 + k]) for r in per[1:]) / NZ == pytest.approx(sum(v[k] for v in vals) / len(vals), rel=1e-12)
    # a window larger than the domain: refused at the first batch, with the numbers
    cfg.ssim.window_size, cfg.name = 15, "wide"
    if min(X, Y) < 15:
        with pytest.raises(ValueError, match=rf"{X} x {Y}.*15 x 15"):
            evaluate(cfg, ds)


def gan_stub(scale=4, **ssim):
    """what ``wind_field_GAN_3D.level_ssim`` uses of its object: the scale and the section"""
    from types import SimpleNamespace

    from gan_sr_wind_field_amd.config.config import SsimConfig

    sc = SsimConfig()
    sc.setSsimConfig(None)
    for k, v in ssim.items():
        setattr(sc, k, v)
    return SimpleNamespace(cfg=SimpleNamespace(scale=scale, ssim=sc))


def test_gan_level_ssim_on_a_cpu_device():
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.ssim import level_ssim_reference

    HR, SR, _ = fields(2, 12, 8, 5, seed=4, kind="uniform")
    LR = torch.randn((2, 4, 3, 2, 5), generator=torch.Generator().manual_seed(5))
    TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
    got = wind_field_GAN_3D.level_ssim(gan_stub(window_size=5, sigma=1.2), HR, SR, LR)
    assert got.shape == (2, 5, 3, NS) and got.dtype == torch.float64
    assert torch.equal(got, level_ssim_reference(HR, SR, TL, 5, 1.2, 2.0))
    with pytest.raises(ValueError, match="12 x 8.*11 x 11"):
        wind_field_GAN_3D.level_ssim(gan_stub(), HR, SR, LR)  # (the default window does not fit)


def test_a_validation_batch_on_a_cpu_device_adds_the_two_metrics(monkeypatch):
    import torch.nn.functional as F

    from gan_sr_wind_field_amd.config.config import Config, SsimConfig
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.ssim import level_ssim_reference, n_positions

    def make(section, validation=True):
        cfg = Config(LOCAL_INI)
        cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
        cfg.gpu_id, cfg.device = None, torch.device("cpu")
        cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 8, 1, 4
        cfg.generator.terrain_number_of_features = 4
        cfg.discriminator.num_features = 4
        cfg.gan_config.number_of_z_layers = 4
        monkeypatch.setattr(cfg, "ssim", SsimConfig())
        cfg.ssim.setSsimConfig(None)
        if section:
            cfg.ssim.present, cfg.ssim.window_size, cfg.ssim.sigma, cfg.ssim.validation = True, 5, 1.2, validation
        torch.manual_seed(3)
        return wind_field_GAN_3D(cfg)

    plain = make(False)
    assert list(plain.get_metrics_dict_ref()) == ["val_PSNR", "Trilinear_PSNR", "pix_loss_unscaled", "trilinear_pix_loss"]
    gan = make(True)
    assert list(gan.get_metrics_dict_ref())[4:] == ["val_SSIM", "Trilinear_SSIM"]
    HR, SR, _ = fields(2, 16, 16, 4, seed=8, kind="smooth")
    LR = HR[:, :, ::4, ::4].contiguous()
    LR = torch.cat([LR, torch.zeros_like(LR[:, :1])], dim=1)
    gan._val_ssim(LR, HR, SR)
    TL = F.interpolate(LR[:, :3], scale_factor=(4, 4, 1), mode="trilinear", align_corners=True)
    want = level_ssim_reference(HR, SR, TL, 5, 1.2).sum(dim=(0, 1, 2)) / (3 * 2 * 4 * n_positions(16, 16, 5))
    m = gan.get_metrics_dict_ref()
    assert float(m["val_SSIM"]) == pytest.approx(float(want[0]), rel=1e-12)
    assert float(m["Trilinear_SSIM"]) == pytest.approx(float(want[2]), rel=1e-12)
    assert list(make(True, validation=False).get_metrics_dict_ref()) == list(plain.get_metrics_dict_ref())


# ---------------------------------------------------------------------------------------------------- 5. the ABI
def test_exports_header_and_wrapper_limits_agree():
    from gan_sr_wind_field_amd import _lib, hip_ops, ssim

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for name in ("wsr_level_ssim", "wsr_level_ssim_workspace_floats"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define WSR_SSIM_SUMS {hip_ops.SSIM_SUMS}" in header and hip_ops.SSIM_SUMS == len(ssim.SSIM_SUMS) == NS
    assert f"#define WSR_SSIM_MAX_WIN {hip_ops.SSIM_MAX_WIN}" in header and hip_ops.SSIM_MAX_WIN == ssim.MAX_WIN == 15
    assert hip_ops.SSIM_MAX_NZ == ssim.MAX_NZ == 256
    assert "#define WSR_ABI_VERSION 9" in header
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert " ssim.hip" in mk and "ssim.o: ssim_kernels.h" in mk
