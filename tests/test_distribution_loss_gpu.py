"""[DISTRIBUTION_LOSS] on the GPU: ``wsr_speed_soft_counts`` and ``wsr_speed_soft_counts_bwd`` (csrc/distribution_loss.hip)
against float64 at the same fp32 inputs - the tables entry by entry within ``forward_bound``, the gradient element by
element within the bound of ``ref_backward`` - then what is exact (row sums, the same bits twice, SR = HR, the NaN column),
the launch geometry, refusals, the loss through autograd on both paths, a generator iteration and ``run.py --train
--test``.  The tables, the workspace and the gradient of the kernels live in ``Guarded`` buffers.

The bounds are derived in tests/distribution_loss_bounds.py; nothing here is fitted.

Measured on an MI355X when the kernels were written: worst |err| / bound 0.14 for the tables (two bins; 0.004 to 0.04 at the
other shapes) and 0.66 for the gradient (64 x 64 x 10, where 5e-5 of the voxels are left out; none elsewhere); the loss through
autograd 3.9e-4 (value) and 0.38 (gradient) of its bounds on both paths.  The whole file ran in 17 s.
"""
import math
import os
import re
import time

import pytest
import torch

from distribution_loss_bounds import (forward_bound, loss_bound, random_upstream, ref_backward, reference_tables,
                                      signs_are_safe, tables_for, wind_fields)
from kernel_bounds import U_FP32, Guarded, assert_guards_intact, assert_within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()

#: (B, C, X, Y, NZ), NS: odd sizes; the reference's patch with a surplus channel; the largest LDS table; two bins; several
#: workgroups on one (sample, source) table, forward and backward
CASES = [((2, 3, 5, 7, 3), 32), ((1, 4, 16, 16, 10), 32), ((1, 3, 8, 8, 128), 64), ((2, 3, 6, 5, 4), 2),
         ((1, 3, 64, 64, 10), 32)]
MULTI = CASES[4]


def case_id(case):
    return "x".join(str(v) for v in case[0]) + f"-ns{case[1]}"


_data: dict = {}


def case_data(case):
    """(tables, HR, SR, float64 reference tables, upstream fp32 table, float64 gradient, its bound, the compared voxels):
    computed once per case, never modified"""
    if case not in _data:
        (B, C, X, Y, NZ), ns = case
        tables = tables_for(ns)
        HR, SR = wind_fields(B, C, X, Y, NZ, tables, seed=11 + CASES.index(case))
        G = random_upstream(B, NZ, ns, 31)
        _data[case] = (tables, HR, SR, reference_tables(HR, SR, tables), G) + ref_backward(SR, G, tables)
    return _data[case]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _forward(hip, HR, SR, tables, label=""):
    """the C entry on device copies, tables and workspace in guarded buffers -> (2, B, NZ, NS + 1) float64 on the host; a
    second launch must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    ns = tables.speed_bins
    hr, sr = HR.to(DEV).contiguous(), SR.to(DEV).contiguous()
    n_ws = int(hip.wsr_speed_soft_counts_workspace_floats(B, X, Y, NZ, ns))
    assert n_ws == 2 * 2 * B * NZ * (ns + 1)
    got = []
    for _ in range(2):
        out = Guarded((2, B, NZ, 2 * (ns + 1)), torch.float32, DEV)  # (2, B, NZ, NS + 1) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_speed_soft_counts(hip_ops._p(hr), HR.shape[1], hip_ops._p(sr), SR.shape[1], tables.c, ns, B, X, Y, NZ,
                                        hip_ops._p(ws.t), hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"speed_soft_counts {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (2, B, NZ, ns + 1) and torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    return got[0]


def _backward(hip, SR, G, tables, label=""):
    """the C entry on device copies, dsr in a guarded buffer pre-filled with NaN -> (B, C, X, Y, NZ) fp32 on the host; every
    element must be overwritten, and a second launch must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, C, X, Y, NZ = SR.shape
    sr, g = SR.to(DEV).contiguous(), G.to(DEV).contiguous()
    got = []
    for _ in range(2):
        dsr = Guarded((B, C, X, Y, NZ), torch.float32, DEV, fill=float("nan"))
        check(hip.wsr_speed_soft_counts_bwd(hip_ops._p(sr), C, hip_ops._p(g), tables.c, tables.speed_bins, B, X, Y, NZ,
                                            hip_ops._p(dsr.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(dsr, label=f"speed_soft_counts_bwd {label}")
        got.append(dsr.t.cpu())
    assert not bool(torch.isnan(got[0]).any()), f"{label}: an element of dsr was not written"
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    return got[0]


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_against_float64_and_what_is_exact(hip, case):
    from gan_sr_wind_field_amd import hip_ops

    (B, C, X, Y, NZ), ns = case
    tables, HR, SR, ref, *_ = case_data(case)
    n = X * Y
    u, v = HR[:, 0].double(), HR[:, 1].double()
    t = torch.sqrt(u * u + v * v) * tables.c - 0.5
    assert float(t.min()) < 0 and float(t.max()) > ns - 1 and int((u == 0).sum()) >= 3  # both clamps, planted zeros
    got = _forward(hip, HR, SR, tables, case_id(case))
    bnd = torch.full_like(ref, forward_bound(n, ns))
    worst = assert_within(got, ref, bnd, f"speed_soft_counts vs float64[{case_id(case)}]", kind="sums")
    assert bool((got.sum(dim=-1) == float(n)).all())  # every row sums to X * Y exactly
    assert bool((got[..., ns] == 0).all())
    assert bool((got * 65536.0 == torch.round(got * 65536.0)).all())  # fixed point
    wrapped = hip_ops.speed_soft_counts(HR.to(DEV), SR.to(DEV), tables)
    assert wrapped.dtype == torch.float64 and torch.equal(_bits(wrapped.cpu()), _bits(got))
    # SR = HR bit for bit: the two tables are identical
    same = _forward(hip, HR, HR.clone(), tables, "SR = HR")
    assert torch.equal(_bits(same[0]), _bits(same[1])) and torch.equal(_bits(same[0]), _bits(got[0]))
    print(f"[fwd] {case_id(case)}: worst |err| / bound {worst:.3g}")


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=case_id)
def test_planted_nans_are_counted_in_their_column_and_get_no_gradient(hip, case):
    (B, C, X, Y, NZ), ns = case
    tables = tables_for(ns)
    HR, SR = wind_fields(B, C, X, Y, NZ, tables, seed=41, nans=4)
    bad = torch.isnan(SR[:, 0]) | torch.isnan(SR[:, 1])
    assert int(bad.sum()) == 4 * B
    SR[0, 1, 0, 0, 0] = float("inf")  # (and an infinite speed)
    bad[0, 0, 0, 0] = True
    got = _forward(hip, HR, SR, tables, "nan")
    assert torch.equal(got[1][..., ns], bad.double().sum(dim=(1, 2))) and bool((got[0][..., ns] == 0).all())
    assert bool((got.sum(dim=-1) == float(X * Y)).all())
    ref = reference_tables(HR, SR, tables)
    assert_within(got, ref, torch.full_like(ref, forward_bound(X * Y, ns)), f"speed_soft_counts with NaNs[{case_id(case)}]",
                  kind="sums")
    G = random_upstream(B, NZ, ns, 42)
    dsr = _backward(hip, SR, G, tables, "nan")
    assert bool((dsr[:, 0][bad] == 0).all()) and bool((dsr[:, 1][bad] == 0).all()) and bool((dsr[:, 2:] == 0).all())
    grad, bound, keep = ref_backward(SR, G, tables)
    mask = keep.unsqueeze(1).expand_as(grad)
    assert_within(torch.where(mask, dsr.double(), grad), grad, bound, f"speed_soft_counts_bwd with NaNs[{case_id(case)}]")


# ---------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_against_the_float64_vjp(hip, case):
    (B, C, X, Y, NZ), ns = case
    tables, HR, SR, _, G, grad, bound, keep = case_data(case)
    left_out = 1.0 - float(keep.double().mean())
    assert left_out <= 0.01, (case, left_out)
    got = _backward(hip, SR, G, tables, case_id(case))
    assert bool((got[:, 2:] == 0).all())
    mask = keep.unsqueeze(1).expand_as(grad)
    worst = assert_within(torch.where(mask, got.double(), grad), grad, bound,
                          f"speed_soft_counts_bwd vs float64[{case_id(case)}]")
    # the voxels left out still hold the derivative of one of the two neighbouring pieces: nothing wild
    assert bool((got.double().abs() <= 2 * G.abs().max().double() * tables.c * (1 + 1e-6)).all())
    dead = ((torch.sqrt(SR[:, 0].double() ** 2 + SR[:, 1].double() ** 2) * tables.c - 0.5) < -1e-3)
    assert int(dead.sum()) >= 3 and bool((got[:, 0][dead] == 0).all()) and bool((got[:, 1][dead] == 0).all())
    zero = _backward(hip, SR, torch.zeros_like(G), tables, "G = 0")
    assert bool((zero == 0).all())
    print(f"[bwd] {case_id(case)}: left out {left_out:.2e}, worst |err| / bound {worst:.3g}")


def test_the_launch_geometry_puts_several_workgroups_on_one_table(hip):
    from gan_sr_wind_field_amd import hip_ops

    (B, C, X, Y, NZ), ns = MULTI
    cb, ncb, eb, nbwd = hip_ops.speed_soft_counts_geometry(B, X, Y, NZ, ns)
    assert ncb > 1 and (ncb - 1) * cb < X * Y <= ncb * cb and (X * Y) % cb != 0  # several ranges, the last one partial
    assert nbwd > 1 and (nbwd - 1) * eb < X * Y * NZ <= nbwd * eb
    assert cb * 65536 < 2 ** 32
    (B, C, X, Y, NZ), ns = CASES[0]
    assert hip_ops.speed_soft_counts_geometry(B, X, Y, NZ, ns)[:2] == (X * Y, 1)  # ... and one
    # the column range never reaches 2^16: a 32-bit LDS counter cannot overflow
    assert hip_ops.speed_soft_counts_geometry(1, 1024, 1024, 1, 2)[0] <= 65535
    with pytest.raises(RuntimeError):
        hip_ops.speed_soft_counts_geometry(1, 8, 8, 129, 64)


# ---------------------------------------------------------------------------------------------------- 3. structure
def test_the_wrapper_through_autograd(hip):
    from gan_sr_wind_field_amd import hip_ops

    case = CASES[1]  # (a surplus channel holding NaN)
    (B, C, X, Y, NZ), ns = case
    tables, HR, SR, _, G, *_ = case_data(case)
    sr = SR.to(DEV).requires_grad_(True)
    hr = HR.to(DEV).requires_grad_(True)
    H = hip_ops.speed_soft_counts(hr, sr, tables)
    up = torch.zeros_like(H)
    up[1, :, :, :ns] = G.to(DEV).double()
    up[0] = 7.0          # (no gradient towards HR, whatever arrives there)
    up[1, :, :, ns] = 3.0  # (the NaN column carries none)
    (H * up).sum().backward()
    assert hr.grad is None and sr.grad.shape == sr.shape and bool((sr.grad[:, 2:] == 0).all())
    assert torch.equal(_bits(sr.grad.cpu()), _bits(_backward(hip, SR, G, tables)))
    # the forward does not depend on whether SR requires grad; non-contiguous and float64 inputs pass through
    plain = hip_ops.speed_soft_counts(HR.to(DEV), SR.to(DEV), tables)
    assert torch.equal(_bits(plain), _bits(H.detach()))
    wide = torch.cat([SR, SR], dim=4).to(DEV)[..., :NZ]
    assert not wide.is_contiguous()
    assert torch.equal(_bits(hip_ops.speed_soft_counts(HR.to(DEV).double(), wide, tables)), _bits(plain))


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_every_buffer_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, C, X, Y, NZ, NS = 1, 3, 6, 5, 3, 8
    tables = tables_for(NS)
    HR, SR = (t.to(DEV) for t in wind_fields(B, C, X, Y, NZ, tables, seed=1))
    G = random_upstream(B, NZ, NS, 2).to(DEV)
    n_ws = int(hip.wsr_speed_soft_counts_workspace_floats(B, X, Y, NZ, NS))
    assert n_ws > 0
    out = Guarded((2, B, NZ, 2 * (NS + 1)), torch.float32, DEV)
    ws = Guarded((n_ws + 2,), torch.float32, DEV)
    dsr = Guarded((B, C, X, Y, NZ), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws, dsr)]
    p = hip_ops._p

    def fwd(hr=HR, hr_c=C, sr=SR, sr_c=C, c=tables.c, ns=NS, b=B, nx=X, ny=Y, nz=NZ, w=ws.t, o=out.t):
        return hip.wsr_speed_soft_counts(p(hr), hr_c, p(sr), sr_c, c, ns, b, nx, ny, nz, p(w), p(o), hip_ops._stream())

    def bwd(sr=SR, sr_c=C, g=G, c=tables.c, ns=NS, b=B, nx=X, ny=Y, nz=NZ, o=dsr.t):
        return hip.wsr_speed_soft_counts_bwd(p(sr), sr_c, p(g), c, ns, b, nx, ny, nz, p(o), hip_ops._stream())

    shared = [dict(sr=None), dict(o=None), dict(sr_c=1), dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(ns=1),
              dict(ns=65), dict(ns=-4), dict(c=0.0), dict(c=-1.0), dict(c=float("inf")), dict(c=float("nan"))]
    for kw in shared + [dict(hr=None), dict(hr_c=1), dict(w=None), dict(w=ws.t[1:])]:  # (... not 8-byte aligned)
        assert fwd(**kw) == -1, kw
    for kw in shared + [dict(g=None)]:
        assert bwd(**kw) == -1, kw
    for kw in (dict(nz=129, ns=64), dict(nz=4161, ns=2), dict(b=65536), dict(nx=65536, ny=32768, nz=1),
               dict(nx=32768, ny=32768, nz=2)):
        assert fwd(**kw) == -2 and bwd(**kw) == -2, kw
    wsf = hip.wsr_speed_soft_counts_workspace_floats
    assert wsf(0, X, Y, NZ, NS) == wsf(1, X, Y, 129, 64) == wsf(1, X, Y, NZ, 1) == wsf(1, X, Y, NZ, 65) == 0
    assert wsf(1, 8, 8, 128, 64) == 2 * 2 * 128 * 65
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws, dsr), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers, a CPU tensor a RuntimeError
    ok = hip_ops.speed_soft_counts(HR, SR, tables)
    assert ok.shape == (2, B, NZ, NS + 1) and bool(torch.isfinite(ok).all())
    for args in ((HR[:, :1], SR), (HR.long(), SR), (HR, SR[..., :2]), (HR, torch.cat([SR, SR])), (HR[0], SR[0])):
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.speed_soft_counts(*args, tables)
    with pytest.raises(ValueError, match="65"):
        hip_ops.speed_soft_counts(HR, SR, tables._replace(speed_bins=65))
    with pytest.raises(ValueError, match="speed_bins.*1"):
        hip_ops.speed_soft_counts(HR, SR, tables._replace(speed_bins=1))
    deep = torch.zeros((1, 2, 2, 2, 129), device=DEV)
    with pytest.raises(ValueError, match="129"):
        hip_ops.speed_soft_counts(deep, deep, tables_for(64))
    with pytest.raises(RuntimeError):
        hip_ops.speed_soft_counts(HR.cpu(), SR, tables)
    with pytest.raises(RuntimeError):
        hip_ops.speed_soft_counts(HR, SR.cpu(), tables)


# ---------------------------------------------------------------------------------------------------- 5. the loss
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("pool", ["level", "sample"])
def test_the_loss_through_autograd(hip, monkeypatch, pool, fused):
    """value and SR.grad of ``distribution_loss`` on the device against float64, on both paths (each held to the truth,
    not to the other): the value within ``loss_bound`` widened by 4 u for the float32 scalar, the gradient within the
    backward bound with one more rounding on the upstream table (gamma_7; the module docstring of the bounds), at the
    voxels away from a bin switch."""
    from test_distribution_loss import Section

    from gan_sr_wind_field_amd import distribution_loss as mod
    from gan_sr_wind_field_amd import hip_ops

    monkeypatch.setenv("WSR_FUSED_DISTRIBUTION_LOSS", fused)
    calls = []
    orig = hip_ops.speed_soft_counts
    monkeypatch.setattr(hip_ops, "speed_soft_counts", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    # (the seeds: inputs whose float64 running sums are nowhere within 2 eps of each other, checked below)
    for ((B, C, X, Y, NZ), ns), seed in ((((2, 4, 12, 9, 3), 16), 55), (MULTI, 51)):
        tables = tables_for(ns)
        HR, SR = wind_fields(B, C, X, Y, NZ, tables, seed=seed)
        ref = reference_tables(HR, SR, tables).requires_grad_(True)
        assert signs_are_safe(ref.detach(), ns, pool), "choose inputs whose running sums differ by more than 2 eps"
        want = mod.loss_from_counts(ref[0], ref[1], tables.bin_width, pool)
        (G64,) = torch.autograd.grad(want, ref)
        sr = SR.to(DEV).requires_grad_(True)
        n0 = len(calls)
        L = mod.distribution_loss(HR.to(DEV), sr, Section(pool=pool), tables)
        assert L.dtype == torch.float32 and L.dim() == 0 and len(calls) - n0 == (1 if fused == "1" else 0)
        L.backward()
        lim = loss_bound(ns, tables.bin_width) + 4 * U_FP32 * max(abs(float(want.detach())), 1.0)
        assert float(want.detach()) > 0 and abs(float(L.detach()) - float(want.detach())) <= lim, (pool, fused, float(L.detach()), lim)
        grad, bound, keep = ref_backward(SR, G64[1, :, :, :ns].float(), tables, roundings=7)
        assert float(keep.double().mean()) >= 0.99
        mask = keep.unsqueeze(1).expand_as(grad)
        got = sr.grad.cpu()
        assert bool((got[:, 2:] == 0).all()) and bool(torch.isfinite(got).all())
        worst = assert_within(torch.where(mask, got.double(), grad), grad, bound + 4 * U_FP32 * grad.abs(),
                              f"distribution_loss grad vs float64[{B}x{X}x{Y}x{NZ} {pool} fused={fused}]")
        print(f"[loss] {B}x{X}x{Y}x{NZ} {pool} fused={fused}: value |err| / bound "
              f"{abs(float(L.detach()) - float(want.detach())) / lim:.3g}, grad worst |err| / bound {worst:.3g}")
    # SR = HR: exactly zero, with an exactly zero gradient; a NaN in SR: NaN, without a host read in between
    x = HR.to(DEV).clone().requires_grad_(True)
    zero = mod.distribution_loss(HR.to(DEV), x, Section(pool=pool), tables)
    zero.backward()
    assert float(zero.detach()) == 0.0 and bool((x.grad == 0).all())
    bad = SR.clone()
    bad[0, 1, 1, 1, 1] = float("nan")
    assert math.isnan(float(mod.distribution_loss(HR.to(DEV), bad.to(DEV), Section(pool=pool), tables)))


# ---------------------------------------------------------------------------------------------------- 6. the model
UVW = 20.0


def _small_gan(section, ssim=None):
    """the small GAN of tests/test_grad_clip_gpu.py on the device, ``[DISTRIBUTION_LOSS]`` (and ``[SSIM_LOSS]``) switched
    as the arguments say"""
    from test_grad_clip_gpu import _build_gan

    gan, cfg = _build_gan(clip=False)
    for sec, keys in ((cfg.distribution_loss, section), (cfg.ssim_loss, ssim)):
        sec.present = keys is not None
        for k, v in (keys or {}).items():
            setattr(sec, k, v)
    return gan, cfg


def _reset_sections(cfg):
    from gan_sr_wind_field_amd.config.config import DistributionLossConfig, SsimLossConfig

    for cls, sec in ((DistributionLossConfig, cfg.distribution_loss), (SsimLossConfig, cfg.ssim_loss)):  # (singletons)
        for k in ["present"] + [k for k, _ in cls._schema]:
            setattr(sec, k, getattr(cls, k))


def test_update_G_with_and_without_the_section(hip, monkeypatch):
    from gan_sr_wind_field_amd import distribution_loss as mod
    from gan_sr_wind_field_amd import hip_ops
    from oracle.gan import synthetic_batch

    LR, HR, Z, x, y = (t.to(DEV) for t in synthetic_batch(2, 16, 4, 4, seed=2001))
    W, BW, NS = 0.1, 1.0, 32
    seen = []
    orig = hip_ops.speed_soft_counts

    def recorded(hr, sr, tables):
        seen.append((hr.detach().cpu(), sr.detach().cpu(), tables))
        return orig(hr, sr, tables)

    monkeypatch.setattr(hip_ops, "speed_soft_counts", recorded)
    keys = {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}

    def g_iteration(gan, cfg):
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 1)
        gan.optimize_parameters(LR, HR, Z, 0)
        torch.cuda.synchronize()
        weights = {k: v.detach().cpu().clone() for k, v in gan.G.state_dict().items()}
        return weights, {k: float(v.detach()) for k, v in gan.get_G_train_loss_dict_ref().items()}

    gan0, cfg0 = _small_gan(None)
    try:
        w0, l0 = g_iteration(gan0, cfg0)
        assert not seen and set(l0) == keys and set(gan0.get_G_val_loss_dict_ref()) == keys  # never called, today's keys
        # a configuration that never mentions the section (the attribute is not there at all): the same bits
        gan00, cfg00 = _small_gan(None)
        missing = type("NoSection", (), {"__getattr__": lambda self, k: getattr(cfg00, k) if k != "distribution_loss" else
                                         (_ for _ in ()).throw(AttributeError(k))})()
        gan00.cfg = missing
        gan00.set_wind_scale(UVW)
        w00, l00 = g_iteration(gan00, cfg00)
        assert l00 == l0 and all(torch.equal(w00[k], w0[k]) for k in w0)

        section = dict(weight=W, bin_width=BW, speed_bins=NS, pool="level")
        gan1, cfg1 = _small_gan(section)
        with pytest.raises(ValueError, match=r"set_wind_scale\(dataset_train\.UVW_MAX\)"):
            g_iteration(gan1, cfg1)
        gan1, cfg1 = _small_gan(section)
        gan1.set_wind_scale(UVW)
        w1, l1 = g_iteration(gan1, cfg1)
        assert len(seen) == 1 and torch.equal(seen[0][0], HR.cpu())  # once per pass
        tables = seen[0][2]
        assert (tables.speed_bins, tables.bin_width, tables.UVW_MAX) == (NS, BW, UVW)
        ref = reference_tables(seen[0][0], seen[0][1], tables)
        want = float(mod.loss_from_counts(ref[0], ref[1], BW, "level"))
        assert set(l1) == keys | {"distribution"} and want > 0
        assert abs(l1["distribution"] - W * want) <= W * (loss_bound(NS, BW) + 8 * U_FP32 * max(want, 1.0)), (l1, want)
        assert all(l1[k] == l0[k] for k in keys - {"total"})
        assert abs((l1["total"] - l0["total"]) - l1["distribution"]) <= 4 * U_FP32 * abs(l1["total"])
        assert any(not torch.equal(w1[k], w0[k]) for k in w0) and all(bool(torch.isfinite(v).all()) for v in w1.values())

        # with [SSIM_LOSS] too: ``distribution`` behind ``ssim``, the same value
        gan3, cfg3 = _small_gan(section, ssim=dict(weight=0.05, window_size=7, sigma=1.0))
        gan3.set_wind_scale(UVW)
        _, l3 = g_iteration(gan3, cfg3)
        assert list(l3)[-2:] == ["ssim", "distribution"] and l3["distribution"] == l1["distribution"] and l3["ssim"] > 0
        cfg3.ssim_loss.present = False

        # a non-finite voxel counted in a table: the term is NaN, the Adam step is skipped, the weights stay bit-equal
        gan2, cfg2 = _small_gan(section)
        gan2.set_wind_scale(UVW)
        w_before = {k: v.detach().clone() for k, v in gan2.G.state_dict().items()}

        def poisoned(hr, sr, tables):
            H = orig(hr, sr, tables)
            bump = torch.zeros_like(H)
            bump[1, 0, 0, 0], bump[1, 0, 0, tables.speed_bins] = -1.0, 1.0
            return H + bump

        monkeypatch.setattr(hip_ops, "speed_soft_counts", poisoned)
        _, l2 = g_iteration(gan2, cfg2)
        assert math.isnan(l2["distribution"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, w_before[k]), k
        monkeypatch.setattr(hip_ops, "speed_soft_counts", recorded)
        m = len(seen)
        gan1.update_G(LR, HR, Z, 0, False)  # validation: once more, logged in the validation dict
        assert len(seen) == m + 1 and float(gan1.get_G_val_loss_dict_ref()["distribution"]) > 0
    finally:
        _reset_sections(cfg0)


def _test_files(name, run_dir):
    """what ``--test`` wrote: path relative to the run -> bytes"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____"):
            with open(os.path.join("test_output", f), "rb") as fh:
                out[f[len(name):]] = fh.read()
    for f in sorted(os.listdir(os.path.join(run_dir, "fields"))):
        with open(os.path.join(run_dir, "fields", f), "rb") as fh:
            out["fields/" + f] = fh.read()
    return out


def test_run_train_and_test_with_the_section(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.speed_soft_counts

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "speed_soft_counts", counted)
    val_dicts = []
    orig_val = wind_field_GAN_3D.get_G_val_loss_dict_ref
    monkeypatch.setattr(wind_field_GAN_3D, "get_G_val_loss_dict_ref",
                        lambda self: val_dicts.append(dict(orig_val(self))) or orig_val(self))
    section = "\n[DISTRIBUTION_LOSS]\nweight = 0.1\nbin_width = 1.0\nspeed_bins = 32\npool = level\n"
    ssim = "\n[SSIM_LOSS]\nweight = 0.1\nwindow_size = 11\nsigma = 1.5\ndata_range = 2.0\n"
    spectral = "\n[SPECTRAL_LOSS]\nweight = 0.05\nwindow = hann\nk_min = 1\nk_max = 0\nrel_floor = 1e-06\n"
    extras = "\n[GRAD_CLIP]\nclip_generator = True\n\n[EMA]\n"

    def run(name, flags, extra, **env):
        ini = str(tmp_path / f"{name}.ini")
        cfg = _write_ini(ini)
        cfg.name = name
        if "GRAD_CLIP" in extra:
            cfg.generator.max_norm = 0.5
        for k, v in env.items():
            setattr(cfg.env, k, v)
        plain_text = cfg.asINI()
        assert "DISTRIBUTION_LOSS" not in plain_text  # today's text
        with open(ini, "w") as f:
            f.write(plain_text + extra)
        runmod.main(flags + ["--cfg", ini])
        return os.path.join(str(tmp_path), "runs", name)

    try:
        for name, extra, on in (("plain", "", False), ("dist", section, True),
                                ("dist_all", extras + spectral + ssim + section, True)):
            before, n_val = calls["n"], len(val_dicts)
            run_dir = run(name, ["--train", "--test"], extra)
            with open(os.path.join(run_dir, f"{name}.train")) as f:
                log = f.read()
            with open(os.path.join(run_dir, "config.ini")) as f:
                snapshot = f.read()
            values = [float(v) for v in re.findall(r"\bdistribution: (\S+)", log)]
            seen_val = val_dicts[n_val:]
            if on:
                assert calls["n"] > before and snapshot.endswith(section)
                # (weight 0.1 times a distance of at most 31 bins of 1 m/s; the first line holds the dict's initial zero)
                assert len(values) >= 6 and all(math.isfinite(v) and 0 <= v <= 3.1 for v in values) and max(values) > 0, values
                assert seen_val and all("distribution" in d for d in seen_val)
                assert any(float(d["distribution"]) > 0 for d in seen_val)
                if spectral in extra:
                    assert len(re.findall(r"\bspectral: (\S+)", log)) == len(values) == len(re.findall(r"\bssim: (\S+)", log))
            else:
                assert calls["n"] == before and not values and "DISTRIBUTION_LOSS" not in snapshot
                assert all("distribution" not in d for d in seen_val)
            assert os.path.isfile(os.path.join(run_dir, "G_6.pth"))
        # --test on the same weights without and with the section: every file byte for byte
        dir_t = os.path.join(str(tmp_path), "runs", "dist")
        load = dict(generator_load_path=os.path.join(dir_t, "G_6.pth"), discriminator_load_path=os.path.join(dir_t, "D_6.pth"),
                    state_load_path=os.path.join(dir_t, "state_6.pth"))
        before = calls["n"]
        a = _test_files("t_plain", run("t_plain", ["--test"], "", **load))
        b = _test_files("t_dist", run("t_dist", ["--test"], section, **load))
        assert calls["n"] == before  # (--test never evaluates the generator loss)
        assert sorted(a) == sorted(b) and len(a) >= 2
        for k in a:
            assert a[k] == b[k], k
    finally:
        _reset_sections(Config)
    print(f"[time] tests/test_distribution_loss_gpu.py up to here: {time.time() - T0:.1f} s")
