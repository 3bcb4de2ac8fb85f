"""[SSIM_LOSS] on the CPU: the config section, the closed-form vector-Jacobian product of tests/ssim_loss_bounds.py against
float64 autograd of ``ssim.ssim_maps`` (the truth test_ssim_loss_gpu.py leans on), its error bound shown to be sound (a torch
fp32 evaluation lies inside it), not vacuous (``MEAN_CAP``) and to have teeth (two wrong evaluations are far outside it),
the analytic properties of the loss, a generator iteration with the section on a CPU device, and the names the C ABI
carries.

Measured when the file was written: the closed form agrees with float64 autograd to 1.1e-14 of the largest gradient
element; fp32 autograd stays at or below 0.0069 of the bound; the mean bound is at most 7.2e-3 of the gradient's rms (smooth,
17 x 15 x 4, window 15); the wrong evaluations are at least 61 bounds off.
"""
import math
import os
import re

import pytest
import torch

from conftest import REPO
from ssim_bounds import fields, ref_ssim
from ssim_loss_bounds import (CASES, MEAN_CAP, TEETH_CASES, autograd_vjp, case_data, case_id, random_gout, ref_vjp,
                              tightness)
from test_eval import LOCAL_INI, _ini_with

KINDS = ("uniform", "smooth")
G_KEYS = {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}


class Section:
    """the attributes ``ssim_loss`` reads from a config section"""

    def __init__(self, **kw):
        self.__dict__.update(dict(dict(window_size=11, sigma=1.5, data_range=2.0), **kw))


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config, SsimConfig
    from gan_sr_wind_field_amd.ssim_loss import SSIM_LOSS

    plain = Config(LOCAL_INI).asINI()
    off = Config(LOCAL_INI).ssim_loss
    assert off.present is False and off.on is False and "SSIM_LOSS" not in plain
    assert SSIM_LOSS == dict(weight=None, window_size=11, sigma=1.5, data_range=2.0)
    assert all(SSIM_LOSS[k] == getattr(SsimConfig, k) for k in ("window_size", "sigma", "data_range"))
    cfg = Config(_ini_with(tmp_path, "[SSIM_LOSS]\nweight = 0.1\n"))
    s = cfg.ssim_loss
    assert s.present and s.on and {k: getattr(s, k) for k in SSIM_LOSS} == dict(SSIM_LOSS, weight=0.1)
    assert cfg.ssim.present is False  # (independent of [SSIM])
    assert cfg.asINI() == plain + "\n[SSIM_LOSS]\nweight = 0.1\nwindow_size = 11\nsigma = 1.5\ndata_range = 2.0\n"
    both = Config(_ini_with(tmp_path, "[SPECTRAL_LOSS]\nweight = 1\n[SSIM]\nwindow_size = 5\n[SSIM_LOSS]\n; the weight\n"
                                      "weight = 2\nwindow_size = 7\nsigma = 1\ndata_range = 1.5\n"))
    assert both.ssim.window_size == 5 and both.ssim_loss.window_size == 7
    text = both.asINI()
    assert text.endswith("weight = 2.0\nwindow_size = 7\nsigma = 1.0\ndata_range = 1.5\n")
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.ssim_loss) == vars(both.ssim_loss) and again.asINI() == text
    refusals = [("", r"weight is required"), ("weight = 0\n", r"weight.*0"), ("weight = -1\n", r"weight.*-1"),
                ("weight = nan\n", r"weight.*nan"), ("weight = 1\nwindow_size = 4\n", r"window_size.*4"),
                ("weight = 1\nwindow_size = 17\n", r"window_size.*17"), ("weight = 1\nwindow_size = 1\n", r"window_size.*1"),
                ("weight = 1\nsigma = 0\n", r"sigma.*0"), ("weight = 1\nsigma = inf\n", r"sigma.*inf"),
                ("weight = 1\ndata_range = -2\n", r"data_range.*-2")]
    for body, pattern in refusals:
        with pytest.raises(ValueError, match=r"\[SSIM_LOSS\] " + pattern):
            Config(_ini_with(tmp_path, "[SSIM_LOSS]\n" + body))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.ssim_loss.present is False and back.ssim_loss.weight is None and back.asINI() == plain


def test_a_patch_smaller_than_the_window_is_refused_with_the_key():
    from gan_sr_wind_field_amd.ssim_loss import ssim_loss

    HR, SR, _ = fields(1, 6, 5, 2, seed=1, kind="uniform")
    with pytest.raises(ValueError, match=r"\[SSIM_LOSS\] window_size.*6 x 5.*7 x 7"):
        ssim_loss(HR, SR, Section(window_size=7))


# ---------------------------------------------------------------------------------------------------- 2. the VJP
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_closed_form_vjp_against_float64_autograd_and_the_bound_is_sound(case, kind):
    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, gout, grad, bound = case_data(case, kind)
    g64 = autograd_vjp(HR, SR, gout, win, sigma, torch.float64)
    scale = float(grad.abs().max())
    agree = float((g64 - grad).abs().max()) / scale
    assert agree <= 1e-12, (case, kind, agree)
    g32 = autograd_vjp(HR, SR, gout, win, sigma, torch.float32)
    ratio = float(((g32 - grad).abs() / bound).max())
    tight = tightness(grad, bound)
    print(f"[ssim_loss] {case_id(case)} {kind}: closed form vs float64 autograd {agree:.2e}; fp32 autograd |err| / bound "
          f"{ratio:.4f}; mean bound / rms gradient {tight:.2e}")
    assert bool((bound > 0).all()) and ratio <= 1.0, (case, kind, ratio)
    assert tight <= MEAN_CAP, (case, kind, tight)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", TEETH_CASES, ids=case_id)
def test_the_bound_has_teeth(case, kind):
    (B, X, Y, NZ), (win, sigma), seed = case
    HR, SR, _ = fields(B, X, Y, NZ, seed=seed, kind=kind)
    gout = random_gout(B, NZ, seed + 1)
    grad, bound = ref_vjp(HR, SR, gout, win, sigma)
    for wrong in (dict(drop_alpha=True), dict(crop=True)):
        off, _ = ref_vjp(HR, SR, gout, win, sigma, **wrong)
        worst = float(((off - grad).abs() / bound).max())
        assert worst >= 10.0, (case, kind, wrong, worst)


def test_surplus_channels_are_never_read_and_get_no_gradient():
    from ssim_bounds import poisoned

    from gan_sr_wind_field_amd.ssim_loss import pair_sums

    HR, SR, _ = fields(1, 7, 6, 2, seed=3, kind="uniform")
    x = poisoned(SR, 5).requires_grad_(True)
    P = pair_sums(poisoned(HR, 4), x, 3, 1.0)
    want, _ = ref_ssim(HR, SR, SR, 3, 1.0)
    assert P.dtype == torch.float64 and P.shape == (1, 2, 3, 2) and float((P.detach() - want[..., :2]).abs().max()) < 1e-10
    P.sum().backward()
    assert bool((x.grad[:, 3:] == 0).all()) and bool(torch.isfinite(x.grad[:, :3]).all())


# ---------------------------------------------------------------------------------------------------- 3. the loss
def test_the_loss_is_zero_for_equal_fields_lies_in_0_2_and_falls_along_its_gradient():
    from gan_sr_wind_field_amd.ssim_loss import ssim_loss

    for (B, X, Y, NZ), (win, sigma) in (CASES[0], CASES[2]):
        sec = Section(window_size=win, sigma=sigma)
        HR, SR, _ = fields(B, X, Y, NZ, seed=9, kind="smooth", noise=0.2)
        zero = ssim_loss(HR, HR.clone(), sec)
        assert zero.dtype == torch.float32 and zero.dim() == 0 and float(zero) == 0.0
        for other in (SR, -HR, fields(B, X, Y, NZ, seed=10, kind="uniform")[0]):
            assert 0.0 < float(ssim_loss(HR, other, sec)) < 2.0
        x = SR.clone().requires_grad_(True)
        L0 = ssim_loss(HR, x, sec)
        L0.backward()
        step = 1e-2 / float(x.grad.abs().max())
        L1 = ssim_loss(HR, (x - step * x.grad).detach(), sec)
        assert float(L1) < float(L0), (float(L0), float(L1))
        # the value: 1 - the mean of the float64 sums
        ref, _ = ref_ssim(HR, SR, SR, win, sigma)
        want = 1.0 - float(ref[..., 0].sum()) / (3 * B * NZ * (X - win + 1) * (Y - win + 1))
        assert abs(float(L0) - want) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 4. the model
def _cpu_gan(section, spectral=None):
    from test_dist_gloo import _build_gan

    gan, cfg = _build_gan()
    for sec, keys in ((cfg.ssim_loss, section), (cfg.spectral_loss, spectral)):
        sec.present = keys is not None
        for k, v in (keys or {}).items():
            setattr(sec, k, v)
    return gan, cfg


def test_update_G_on_a_cpu_device_with_and_without_the_section(monkeypatch):
    from gan_sr_wind_field_amd import ssim_loss as mod
    from gan_sr_wind_field_amd.config.config import SpectralLossConfig, SsimLossConfig
    from oracle.gan import synthetic_batch
    from test_dist_gloo import _g_iteration

    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    X, Y, NZ = HR.shape[2:]
    WIN, SIGMA, W = 7, 1.0, 0.1
    seen = []
    orig = mod.pair_sums

    def recorded(hr, sr, win=11, sigma=1.5, data_range=2.0):
        seen.append((hr.detach().clone(), sr.detach().clone(), win, sigma, data_range))
        return orig(hr, sr, win, sigma, data_range)

    monkeypatch.setattr(mod, "pair_sums", recorded)
    try:
        gan0, cfg0 = _cpu_gan(None)
        w0, l0 = _g_iteration(gan0, cfg0, LR, HR, Z, x, y)
        assert not seen and set(l0) == G_KEYS  # never called, exactly the old keys
        assert set(gan0.get_G_val_loss_dict_ref()) == G_KEYS

        gan1, cfg1 = _cpu_gan(dict(weight=W, window_size=WIN, sigma=SIGMA, data_range=2.0))
        before = {k: v.clone() for k, v in gan1.G.state_dict().items()}
        w1, l1 = _g_iteration(gan1, cfg1, LR, HR, Z, x, y)
        assert len(seen) == 1 and seen[0][2:] == (WIN, SIGMA, 2.0) and torch.equal(seen[0][0], HR)
        ref, _ = ref_ssim(seen[0][0], seen[0][1], seen[0][1], WIN, SIGMA)
        want = W * (1.0 - float(ref[..., 0].sum()) / (3 * HR.shape[0] * NZ * (X - WIN + 1) * (Y - WIN + 1)))
        assert want > 0 and abs(l1["ssim"] - want) <= 1e-5 * want
        # one more entry of the core vector: the total moves by it, the other terms do not, the step differs
        assert abs((l1["total"] - l0["total"]) - l1["ssim"]) <= 1e-5 * abs(l1["total"])
        assert set(l1) == G_KEYS | {"ssim"} and all(l1[k] == l0[k] for k in l0 if k != "total")
        assert any(not torch.equal(w1[k], w0[k]) for k in w0)

        # with [SPECTRAL_LOSS] too: ``ssim`` behind ``spectral``, each weighted by its own weight
        gan3, cfg3 = _cpu_gan(dict(weight=W, window_size=WIN, sigma=SIGMA, data_range=2.0), spectral=dict(weight=0.05))
        _, l3 = _g_iteration(gan3, cfg3, LR, HR, Z, x, y)
        assert list(l3)[-2:] == ["spectral", "ssim"] and l3["ssim"] == l1["ssim"] and l3["spectral"] > 0
        assert abs((l3["total"] - l0["total"]) - l3["ssim"] - l3["spectral"]) <= 1e-5 * abs(l3["total"])
        cfg3.spectral_loss.present = False

        # a NaN in the term: the total is not finite, the Adam step is skipped, the weights stay bit-equal
        gan2, cfg2 = _cpu_gan(dict(weight=W, window_size=WIN, sigma=SIGMA))
        monkeypatch.setattr(mod, "pair_sums", lambda *a, **kw: orig(*a, **kw) * float("nan"))
        _, l2 = _g_iteration(gan2, cfg2, LR, HR, Z, x, y)
        assert math.isnan(l2["ssim"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, before[k]), k
        # validation logs it too
        monkeypatch.setattr(mod, "pair_sums", orig)
        gan1.update_G(LR, HR, Z, 0, False)
        assert float(gan1.get_G_val_loss_dict_ref()["ssim"]) > 0
    finally:
        for cls, sec in ((SsimLossConfig, cfg0.ssim_loss), (SpectralLossConfig, cfg0.spectral_loss)):  # (the singletons)
            for k in ["present"] + [k for k, _ in cls._schema]:
                setattr(sec, k, getattr(cls, k))


# ---------------------------------------------------------------------------------------------------- 5. the C ABI
def test_exports_are_in_the_header_and_in_EXPORTS():
    from gan_sr_wind_field_amd._lib import EXPORTS

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for n in ("wsr_ssim_pair_sums_workspace_floats", "wsr_ssim_pair_sums", "wsr_ssim_pair_sums_bwd",
              "wsr_ssim_pair_sums_bwd_tile"):
        assert n in EXPORTS and re.search(rf"\b{n}\s*\(", header), n
    assert int(re.search(r"#define\s+WSR_ABI_VERSION\s+(\d+)", header).group(1)) == 9
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        assert "ssim_loss.hip" in f.read()
