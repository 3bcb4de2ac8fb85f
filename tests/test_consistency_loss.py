"""[CONSISTENCY_LOSS] on the CPU: the config section, ``coarse_residual_reference`` against a plain double loop over the
definition and against the bits of ``degradation.degrade_lr``, the analytic properties of ``L_cons`` (zero with a zero
gradient for SR = HR, |c| and c^2 for a constant shift), the closed-form vector-Jacobian product against autograd and a
central difference of the float64 reference, adjointness, a generator iteration with the section on a CPU device, and
the names the C ABI carries.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from consistency_loss_bounds import random_upstream, tables_for, wind_fields
from test_eval import LOCAL_INI, _ini_with

G_KEYS = {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}
EXPORTS_NEW = ("wsr_coarse_residual", "wsr_coarse_residual_bwd", "wsr_coarse_residual_geometry")


class Section:
    """the attributes ``consistency_loss`` reads from a config section"""

    def __init__(self, **kw):
        self.__dict__.update(dict(dict(kernel="box", sigma=None, factor=0, norm="l1"), **kw))


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.consistency_loss import CONSISTENCY_LOSS

    plain = Config(LOCAL_INI).asINI()
    off = Config(LOCAL_INI).consistency_loss
    assert off.present is False and off.on is False and "CONSISTENCY_LOSS" not in plain
    assert CONSISTENCY_LOSS == dict(weight=None, kernel=None, sigma=None, factor=0, norm="l1")
    order = [a for a, _ in Config._optional + Config._optional_later + Config._optional_last]
    assert order[-1] == "consistency_loss"  # loads and prints behind every other section
    cfg = Config(_ini_with(tmp_path, "[CONSISTENCY_LOSS]\nweight = 1.0\nkernel = box\n"))
    s = cfg.consistency_loss
    assert s.present and s.on and s.resolved_factor(cfg.scale) == cfg.scale
    assert {k: getattr(s, k) for k in CONSISTENCY_LOSS} == dict(CONSISTENCY_LOSS, weight=1.0, kernel="box")
    assert cfg.degradation.present is False  # (independent of [DEGRADATION])
    # (a box has no sigma: the key is not printed, so that the text loads again)
    assert cfg.asINI() == plain + "\n[CONSISTENCY_LOSS]\nweight = 1.0\nkernel = box\nfactor = 0\nnorm = l1\n"
    with open(str(tmp_path / "box.ini"), "w") as f:
        f.write(cfg.asINI())
    assert Config(str(tmp_path / "box.ini")).asINI() == plain + "\n[CONSISTENCY_LOSS]\nweight = 1.0\nkernel = box\nfactor = 0\nnorm = l1\n"
    both = Config(_ini_with(tmp_path, "[DISTRIBUTION_LOSS]\nweight = 1\nbin_width = 1\n[DEGRADATION]\nkernel = box\n"
                                      "[CONSISTENCY_LOSS]\n; the weight\nweight = 2\nkernel = Gaussian\nsigma = 2.0\n"
                                      "factor = 8\nnorm = L2\n"))
    assert both.degradation.kernel == "box" and both.consistency_loss.kernel == "gaussian"
    assert both.consistency_loss.resolved_factor(both.scale) == 8
    text = both.asINI()
    assert text.endswith("[CONSISTENCY_LOSS]\nweight = 2.0\nkernel = gaussian\nsigma = 2.0\nfactor = 8\nnorm = l2\n")
    assert text.index("[DISTRIBUTION_LOSS]") < text.index("[CONSISTENCY_LOSS]")
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.consistency_loss) == vars(both.consistency_loss) and again.asINI() == text
    ok = "weight = 1\nkernel = box\n"
    refusals = [("kernel = box\n", r"weight is required"), ("weight = 0\nkernel = box\n", r"weight.*0"),
                ("weight = -1\nkernel = box\n", r"weight.*-1"), ("weight = nan\nkernel = box\n", r"weight.*nan"),
                ("weight = 1\n", r"kernel is required"), ("weight = 1\nkernel = lanczos\n", r"kernel.*lanczos"),
                ("weight = 1\nkernel = gaussian\n", r"sigma is required"),
                ("weight = 1\nkernel = gaussian\nsigma = 0\n", r"sigma.*0"),
                ("weight = 1\nkernel = gaussian\nsigma = 10.5\n", r"sigma.*10\.5"),
                (ok + "factor = 1\n", r"factor.*1"), (ok + "factor = 33\n", r"factor.*33"), (ok + "factor = -4\n", r"factor.*-4"),
                (ok + "norm = huber\n", r"norm.*huber"), (ok + "factor = many\n", r"factor must be an integer")]
    for body, pattern in refusals:
        with pytest.raises(ValueError, match=r"\[CONSISTENCY_LOSS\] " + pattern):
            Config(_ini_with(tmp_path, "[CONSISTENCY_LOSS]\n" + body))
    for factor in (2, 32):
        assert Config(_ini_with(tmp_path, f"[CONSISTENCY_LOSS]\n{ok}factor = {factor}\n")).consistency_loss.factor == factor
    # a tap radius above 32 cannot be reached inside the ranges (box: 16, gaussian: 30): the check is the one of
    # [DEGRADATION], shown here on the section object with a radius forced past it
    from gan_sr_wind_field_amd import degradation
    from gan_sr_wind_field_amd.config.config import ConsistencyLossConfig

    sec = ConsistencyLossConfig()
    sec.present, sec.weight, sec.kernel, sec.sigma, sec.factor, sec.norm = True, 1.0, "gaussian", 10.0, 4, "l1"
    sec.validate(4)
    old = degradation.MAX_RADIUS
    degradation.MAX_RADIUS = 29
    try:
        with pytest.raises(ValueError, match=r"\[CONSISTENCY_LOSS\] kernel = gaussian at factor 4 needs a tap radius above 29"):
            sec.validate(4)
    finally:
        degradation.MAX_RADIUS = old
    for scale in (None, 1, 64):  # factor = 0 stands for [DEFAULT] scale, which must itself be 2 .. 32
        sec.factor = 0
        with pytest.raises(ValueError, match=r"\[CONSISTENCY_LOSS\] factor = 0 needs \[DEFAULT\] scale"):
            sec.validate(scale)
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.consistency_loss.present is False and back.consistency_loss.weight is None and back.asINI() == plain


def test_parameters_and_tables_are_refused_with_the_number():
    from gan_sr_wind_field_amd import degradation
    from gan_sr_wind_field_amd.consistency_loss import check_parameters, coarse_tables, consistency_loss

    t = coarse_tables("box", None, 4, 16, 12)
    wx, wy, R = degradation.tables(degradation.DegradationSpec("box", None), 4, 16, 12)
    assert t.R == R == 2 and t.s == 4 and np.array_equal(t.wx.numpy(), wx) and np.array_equal(t.wy.numpy(), wy)
    assert coarse_tables("box", 3.0, 4, 16, 12) is t  # (sigma is not a key of a box; cached per shape and device)
    for args, pattern in ((("lanczos", None, 4), "kernel.*lanczos"), (("gaussian", None, 4), "sigma"),
                          (("gaussian", 11.0, 4), "sigma.*11"), (("box", None, 1), "factor.*1"), (("box", None, 33), "33"),
                          (("box", None, 2.5), "2.5")):
        with pytest.raises(ValueError, match=pattern):
            check_parameters(*args)
    HR = torch.zeros((1, 3, 6, 5, 2))
    with pytest.raises(ValueError, match=r"factor 8 is larger than the 6 x 5 patch"):
        consistency_loss(HR, HR, Section(factor=8), 4)
    with pytest.raises(ValueError, match=r"factor 6 is larger than the 6 x 5 patch"):
        consistency_loss(HR, HR, Section(), 6)
    with pytest.raises(ValueError, match=r"C >= 3"):
        consistency_loss(HR[:, :2], HR[:, :2], Section(), 2)
    with pytest.raises(ValueError, match=r"does not match"):
        consistency_loss(HR, HR[..., :1], Section(), 2)
    with pytest.raises(ValueError, match=r"norm.*huber"):
        consistency_loss(HR, HR, Section(norm="huber"), 2)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def _loop_residual(HR, SR, tables):
    """the definition, cell by cell in Python doubles -> (B, 3, XL, YL, NZ)"""
    B, _, X, Y, NZ = HR.shape
    s, R = tables.s, tables.R
    wx, wy = tables.wx.double().tolist(), tables.wy.double().tolist()
    XL, YL = len(wx), len(wy)
    e = (SR[:, :3].double() - HR[:, :3].double()).tolist()
    out = torch.zeros((B, 3, XL, YL, NZ), dtype=torch.float64)
    for b in range(B):
        for c in range(3):
            for i in range(XL):
                for j in range(YL):
                    for z in range(NZ):
                        acc = 0.0
                        for dy in range(2 * R + 1):
                            y = s * j + dy - R
                            if not 0 <= y < Y:
                                continue
                            g = 0.0
                            for dx in range(2 * R + 1):
                                x = s * i + dx - R
                                if 0 <= x < X:
                                    g += wx[i][dx] * e[b][c][x][y][z]
                            acc += wy[j][dy] * g
                        out[b, c, i, j, z] = acc
    return out


@pytest.mark.parametrize("kernel,sigma,s,shape", [("box", None, 2, (2, 3, 5, 7, 2)), ("box", None, 3, (1, 4, 6, 5, 2)),
                                                  ("gaussian", 1.0, 4, (1, 3, 9, 6, 1))])
def test_the_reference_against_a_plain_loop_over_the_definition(kernel, sigma, s, shape):
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_reference

    B, C, X, Y, NZ = shape
    tables = tables_for(kernel, sigma, s, X, Y)
    HR, SR = wind_fields(B, C, X, Y, NZ, seed=3)
    r = coarse_residual_reference(HR, SR, tables)
    assert r.dtype == torch.float64 and r.shape == (B, 3, -(-X // s), -(-Y // s), NZ)
    want = _loop_residual(HR, SR, tables)
    assert float((r - want).abs().max()) <= 1e-15 and float(want.abs().max()) > 1e-3
    # every weight row sums to 1 (to fp32 rounding), every in-range weight is positive, every out-of-range one zero
    for w, n in ((tables.wx, X), (tables.wy, Y)):
        assert float((w.double().sum(dim=1) - 1.0).abs().max()) <= (2 * tables.R + 1) * 2.0 ** -24
        pos = s * torch.arange(w.shape[0]).view(-1, 1) + torch.arange(-tables.R, tables.R + 1).view(1, -1)
        inside = (pos >= 0) & (pos < n)
        assert bool((w[inside] > 0).all()) and bool((w[~inside] == 0).all())


@pytest.mark.parametrize("kernel,sigma,s,shape", [("box", None, 2, (2, 3, 8, 6, 3)), ("box", None, 3, (1, 3, 9, 6, 2)),
                                                  ("box", None, 4, (1, 4, 16, 16, 10)), ("gaussian", 2.0, 4, (1, 3, 16, 12, 2)),
                                                  ("box", None, 2, (1, 3, 5, 7, 3)), ("box", None, 3, (1, 3, 7, 5, 2)),
                                                  ("box", None, 4, (1, 3, 10, 13, 2)), ("gaussian", 2.0, 4, (1, 3, 9, 11, 2))])
def test_the_residual_of_a_zero_truth_carries_the_bits_of_degrade_lr(kernel, sigma, s, shape):
    """``coarse_residual(0, F)`` is ``D(F)``: the fp32 reference gives the bits of the CPU loader's ``degrade_lr`` for the
    same kernel, also at extents that ``s`` does not divide"""
    from gan_sr_wind_field_amd import degradation
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_reference

    B, C, X, Y, NZ = shape
    tables = tables_for(kernel, sigma, s, X, Y)
    _, F = wind_fields(B, C, X, Y, NZ, seed=4)
    r = coarse_residual_reference(torch.zeros_like(F), F, tables, torch.float32)
    assert r.dtype == torch.float32
    spec = degradation.DegradationSpec(kernel, sigma)
    want = np.stack([degradation.degrade_lr(F[b, :3].numpy(), s, spec) for b in range(B)])
    assert np.array_equal(r.numpy().view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------- 3. the loss
def test_the_loss_is_zero_with_a_zero_gradient_for_equal_fields_and_not_finite_for_a_nan():
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_reference, consistency_loss

    HR, SR = wind_fields(2, 4, 9, 8, 3, seed=5)
    for norm in ("l1", "l2"):
        for sec in (Section(norm=norm), Section(norm=norm, kernel="gaussian", sigma=1.5, factor=3)):
            x = HR.clone().requires_grad_(True)
            zero = consistency_loss(HR, x, sec, 2)
            assert zero.dtype == torch.float32 and zero.dim() == 0 and float(zero.detach()) == 0.0
            zero.backward()
            assert bool((x.grad == 0).all())
            x = SR.clone().requires_grad_(True)
            L = consistency_loss(HR, x, sec, 2)
            L.backward()
            assert float(L.detach()) > 0 and bool(torch.isfinite(x.grad).all()) and bool((x.grad[:, 3:] == 0).all())
            assert float(x.grad[:, :3].abs().max()) > 0
            bad = SR.clone()
            bad[1, 0, 2, 3, 1] = float("nan")
            assert math.isnan(float(consistency_loss(HR, bad, sec, 2)))
            inf = SR.clone()
            inf[0, 1, 0, 0, 0] = float("inf")
            assert not math.isfinite(float(consistency_loss(HR, inf, sec, 2)))
    # SR = HR gives r exactly 0, every element +0.0
    r = coarse_residual_reference(HR, HR.clone(), tables_for("box", None, 2, 9, 8), torch.float32)
    assert bool((r.view(torch.int32) == 0).all())
    # a NaN shows up in exactly the coarse cells whose footprint holds it: box, s = 2, R = 1, x = 2 and y = 3 -> i = 1,
    # j in {1, 2}; the same level, sample and component only
    tables = tables_for("box", None, 2, 9, 8)
    r = coarse_residual_reference(HR, bad, tables, torch.float32)
    want = torch.zeros_like(r, dtype=torch.bool)
    want[1, 0, 1, 1:3, 1] = True
    assert torch.equal(torch.isnan(r), want)


@pytest.mark.parametrize("norm", ["l1", "l2"])
@pytest.mark.parametrize("c", [0.25, -0.003])
def test_a_constant_shift_costs_its_magnitude(norm, c):
    """SR = HR + c: every weight row sums to 1 to fp32 rounding, so r = c in every cell, L_cons = |c| (l1), c^2 (l2)"""
    from gan_sr_wind_field_amd.consistency_loss import consistency_loss

    HR, _ = wind_fields(2, 3, 10, 7, 3, seed=6)
    HR = HR.double()
    for sec in (Section(norm=norm), Section(norm=norm, factor=3), Section(norm=norm, kernel="gaussian", sigma=2.0)):
        L = float(consistency_loss(HR, HR + c, sec, 2))
        want = abs(c) if norm == "l1" else c * c
        # (every fp32 weight is rounded once, a relative u: a row sums to 1 within u, r = c (1 + 2 u), its square twice
        # that; the sums themselves are float64 here and the scalar is rounded to fp32 once more)
        assert abs(L - want) <= 40 * 2.0 ** -24 * want, (L, want)


# ---------------------------------------------------------------------------------------------------- 4. the VJP
@pytest.mark.parametrize("kernel,sigma,s,shape", [("box", None, 2, (2, 3, 5, 7, 3)), ("box", None, 3, (1, 4, 6, 5, 2)),
                                                  ("gaussian", 2.0, 4, (1, 3, 8, 9, 2)), ("gaussian", 10.0, 8, (1, 3, 16, 12, 1))])
def test_the_closed_form_vjp_against_autograd_a_central_difference_and_adjointness(kernel, sigma, s, shape):
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_reference, coarse_residual_vjp

    B, C, X, Y, NZ = shape
    tables = tables_for(kernel, sigma, s, X, Y)
    HR, SR = wind_fields(B, C, X, Y, NZ, seed=7)
    SR = torch.nan_to_num(SR)  # (surplus channels: finite, so that a difference quotient may move them)
    G = random_upstream(B, tables.wx.shape[0], tables.wy.shape[0], NZ, 8).double()
    x = SR.double().requires_grad_(True)
    h64 = HR.double().requires_grad_(True)
    r = coarse_residual_reference(h64, x, tables)
    assert r.requires_grad
    (r * G).sum().backward()
    assert h64.grad is None  # HR is detached
    closed = coarse_residual_vjp(G, tables, shape)
    assert closed.dtype == torch.float64 and closed.shape == x.grad.shape
    assert bool((x.grad[:, 3:] == 0).all()) and bool((closed[:, 3:] == 0).all())
    scale = float(closed.abs().max())
    assert scale > 0 and float((x.grad - closed).abs().max()) <= 1e-14 * scale
    # a central difference of the float64 reference: the operator is linear, so the quotient is exact to rounding
    h = 2.0 ** -10
    f = lambda t: float((coarse_residual_reference(HR, t, tables) * G).sum())  # noqa: E731
    gen = torch.Generator().manual_seed(9)
    for _ in range(6):
        idx = tuple(int(torch.randint(0, n, (1,), generator=gen)) for n in shape)
        e = torch.zeros(shape, dtype=torch.float64)
        e[idx] = h
        num = (f(SR.double() + e) - f(SR.double() - e)) / (2 * h)
        assert abs(num - float(closed[idx])) <= 1e-10 * scale, idx
    # adjointness <D e, G> = <e, D^T G> in float64
    e = torch.randn((B, 3, X, Y, NZ), generator=gen, dtype=torch.float64)
    lhs = float((coarse_residual_reference(torch.zeros_like(e), e, tables) * G).sum())
    rhs = float((e * closed[:, :3]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)) and abs(lhs) > 0
    with pytest.raises(ValueError, match="does not belong"):
        coarse_residual_vjp(G[..., :-1] if NZ > 1 else G[:, :2], tables, shape)


def test_the_fp32_vjp_sums_in_ascending_order_of_the_coarse_index():
    """the closed form in fp32 is the backward kernel's arithmetic: per element, the terms enter in ascending i, then j"""
    from gan_sr_wind_field_amd.consistency_loss import coarse_residual_vjp

    B, C, X, Y, NZ, s = 1, 3, 9, 7, 2, 2
    tables = tables_for("gaussian", 1.5, s, X, Y)
    R = tables.R
    G = random_upstream(B, tables.wx.shape[0], tables.wy.shape[0], NZ, 10)
    got = coarse_residual_vjp(G, tables, (B, C, X, Y, NZ), torch.float32)
    wx, wy = tables.wx.numpy(), tables.wy.numpy()
    g = G.numpy()
    want = np.zeros((B, C, X, Y, NZ), dtype=np.float32)
    for c in range(3):
        for x in range(X):
            t = np.zeros((wy.shape[0], NZ), dtype=np.float32)
            for i in range(wx.shape[0]):
                d = x - s * i + R
                if 0 <= d <= 2 * R:
                    t = t + wx[i, d] * g[0, c, i]
            for y in range(Y):
                acc = np.zeros(NZ, dtype=np.float32)
                for j in range(wy.shape[0]):
                    d = y - s * j + R
                    if 0 <= d <= 2 * R:
                        acc = acc + wy[j, d] * t[j]
                want[0, c, x, y] = acc
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------- 5. the model
LOSS_SECTIONS = ("consistency_loss", "distribution_loss", "ssim_loss", "spectral_loss")


def _cpu_gan(**sections):
    from test_dist_gloo import _build_gan

    gan, cfg = _build_gan()
    for name in LOSS_SECTIONS:
        sec, keys = getattr(cfg, name), sections.get(name)
        sec.present = keys is not None
        for k, v in (keys or {}).items():
            setattr(sec, k, v)
    return gan, cfg


def _reset_sections(cfg):
    for name in LOSS_SECTIONS:  # (singletons)
        sec = getattr(cfg, name)
        for k in ["present"] + [k for k, _ in type(sec)._schema]:
            setattr(sec, k, getattr(type(sec), k))


def test_update_G_on_a_cpu_device_with_and_without_the_section(monkeypatch):
    from gan_sr_wind_field_amd import consistency_loss as mod
    from oracle.gan import synthetic_batch
    from test_dist_gloo import _g_iteration

    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    W = 0.5
    seen = []
    orig = mod.coarse_residual

    def recorded(hr, sr, tables):
        seen.append((hr.detach().clone(), sr.detach().clone(), tables))
        return orig(hr, sr, tables)

    monkeypatch.setattr(mod, "coarse_residual", recorded)
    section = dict(weight=W, kernel="box", sigma=None, factor=0, norm="l1")
    gan0, cfg0 = _cpu_gan()
    try:
        w0, l0 = _g_iteration(gan0, cfg0, LR, HR, Z, x, y)
        assert not seen and set(l0) == G_KEYS  # never called, exactly the old keys
        assert set(gan0.get_G_val_loss_dict_ref()) == G_KEYS
        with pytest.raises(ValueError, match=r"\[CONSISTENCY_LOSS\]"):
            gan0.coarse_residual(HR, HR)

        gan1, cfg1 = _cpu_gan(consistency_loss=section)
        before = {k: v.clone() for k, v in gan1.G.state_dict().items()}
        w1, l1 = _g_iteration(gan1, cfg1, LR, HR, Z, x, y)
        assert len(seen) == 1 and torch.equal(seen[0][0], HR)
        tables = seen[0][2]
        assert (tables.s, tables.R) == (cfg1.scale, cfg1.scale // 2) == (4, 2) and tuple(tables.wx.shape) == (16, 5)
        r = mod.coarse_residual_reference(seen[0][0], seen[0][1], tables)
        want = W * float(mod.loss_from_residual(r, "l1"))
        assert want > 0 and abs(l1["consistency"] - want) <= 1e-5 * want
        # one more entry of the core vector: the total moves by it, the other terms do not, the step differs
        assert abs((l1["total"] - l0["total"]) - l1["consistency"]) <= 1e-5 * abs(l1["total"])
        assert set(l1) == G_KEYS | {"consistency"} and all(l1[k] == l0[k] for k in l0 if k != "total")
        assert any(not torch.equal(w1[k], w0[k]) for k in w0)
        # from code: the residual of a batch under the section's keys
        got = gan1.coarse_residual(seen[0][0], seen[0][1])
        assert len(seen) == 2 and torch.equal(got, r)

        # with the three other loss sections too: ``consistency`` last, each weighted by its own weight
        gan3, cfg3 = _cpu_gan(consistency_loss=dict(section, norm="l2", kernel="gaussian", sigma=1.0, factor=2),
                              distribution_loss=dict(weight=0.1, bin_width=1.0, speed_bins=32, pool="level"),
                              ssim_loss=dict(weight=0.05, window_size=7, sigma=1.0),
                              spectral_loss=dict(weight=0.05))
        gan3.set_wind_scale(20.0)
        _, l3 = _g_iteration(gan3, cfg3, LR, HR, Z, x, y)
        assert list(l3)[-4:] == ["spectral", "ssim", "distribution", "consistency"]
        assert all(l3[k] > 0 for k in list(l3)[-4:])
        extras = sum(l3[k] for k in list(l3)[-4:])
        assert abs((l3["total"] - l0["total"]) - extras) <= 1e-5 * abs(l3["total"])
        r3 = mod.coarse_residual_reference(seen[-1][0], seen[-1][1], seen[-1][2])
        assert seen[-1][2].s == 2 and abs(l3["consistency"] - W * float(mod.loss_from_residual(r3, "l2"))) <= 1e-5 * l3["consistency"]
        _reset_sections(cfg3)

        # a NaN planted in SR: the residual is non-finite in its footprint, the term and the total are NaN, the Adam step
        # is skipped and the weights stay
        gan2, cfg2 = _cpu_gan(consistency_loss=section)

        def poisoned(hr, sr, tables):
            bump = torch.zeros_like(sr)
            bump[0, 1, 5, 6, 2] = float("nan")
            return orig(hr, sr + bump, tables)

        monkeypatch.setattr(mod, "coarse_residual", poisoned)
        _, l2 = _g_iteration(gan2, cfg2, LR, HR, Z, x, y)
        assert math.isnan(l2["consistency"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, before[k]), k
        # validation logs it too
        monkeypatch.setattr(mod, "coarse_residual", orig)
        gan1.update_G(LR, HR, Z, 0, False)
        assert float(gan1.get_G_val_loss_dict_ref()["consistency"]) > 0

        # a factor larger than the patch: refused at the first batch with the numbers
        gan4, cfg4 = _cpu_gan(consistency_loss=dict(section, factor=32))
        with pytest.raises(ValueError, match=r"factor 32 is larger than the 16 x 16 patch"):
            gan4.coarse_residual(HR[:, :, :16, :16], HR[:, :, :16, :16])
    finally:
        _reset_sections(cfg0)


# ---------------------------------------------------------------------------------------------------- 6. the C ABI
def test_exports_are_in_the_header_in_EXPORTS_and_in_the_library():
    from gan_sr_wind_field_amd import _lib
    from gan_sr_wind_field_amd._lib import EXPORTS

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for n in EXPORTS_NEW:
        assert n in EXPORTS and re.search(rf"\b{n}\s*\(", header), n
    assert "wsr_coarse_residual_workspace_floats" not in header  # (neither launch uses a workspace)
    assert int(re.search(r"#define\s+WSR_ABI_VERSION\s+(\d+)", header).group(1)) == 9
    lds = int(re.search(r"#define\s+WSR_CONSISTENCY_LOSS_LDS_FLOATS\s+(\d+)", header).group(1))
    assert (2 * 32 + 32) * 128 <= lds and 2 * 4 * lds <= 160 * 1024  # R = 32, s = 32, NZ = 128 fits; two per CU
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "consistency_loss.hip" in make and "consistency_loss.o: consistency_loss_kernels.h" in make
    so = os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "libwindsr_hip.so")
    if os.path.isfile(so):  # (the library loads without a device: the symbols are there and the ABI is still 9)
        L = _lib.lib()
        assert L.wsr_abi_version() == 9
        for n in EXPORTS_NEW:
            assert hasattr(L, n), n
        import ctypes as C

        geom = (C.c_int32 * 8)()
        assert L.wsr_coarse_residual_geometry(4, 2, 1, 64, 64, 10, geom) == 0 and tuple(geom)[:2] == (16, 16)
        assert L.wsr_coarse_residual_geometry(4, 32, 1, 64, 64, 128, geom) == 0  # R = 32 with NZ = 128 fits
        assert max(tuple(geom)[6:]) <= lds
        assert L.wsr_coarse_residual_geometry(4, 32, 1, 64, 64, 512, geom) == -2
        assert L.wsr_coarse_residual_geometry(1, 2, 1, 64, 64, 10, geom) == -1
        assert L.wsr_coarse_residual_geometry(4, 33, 1, 64, 64, 10, geom) == -1
