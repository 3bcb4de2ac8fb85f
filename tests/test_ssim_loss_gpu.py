"""[SSIM_LOSS] on the GPU: ``wsr_ssim_pair_sums`` and ``wsr_ssim_pair_sums_bwd`` (csrc/ssim_loss.hip) against float64 - the
forward against ``ref_ssim`` of tests/ssim_bounds.py and, bit for bit, against ``hip_ops.level_ssim``; the backward,
element-wise, against the closed-form vector-Jacobian product of tests/ssim_loss_bounds.py with its bound - then an
identity that needs no reference, structure (the same bits twice, surplus channels, every element written, guards),
refusals, the loss through autograd on both paths, a generator iteration and ``run.py --train --test``.  The sums, the
workspace and the gradient of the kernels live in ``Guarded`` buffers.

The bounds are derived in tests/ssim_bounds.py and tests/ssim_loss_bounds.py (LAMBDA = 16 of kernel_bounds.py, untouched)
and shown on the CPU to hold for a torch fp32 evaluation and to reject two wrong evaluations (tests/test_ssim_loss.py).
The shapes are the six of ssim_loss_bounds.CASES, four more of the forward's tests (one position, one level, 128 and 256
levels) and three across the boundaries of the backward's own tile geometry (``BOUNDARY``).

Measured on an MI355X when the kernels were written: worst |err| / bound 0.014 for the forward sums (one position, 3 x 3 x 4)
and 0.012 for the backward (smooth, 35 x 34 x 3; 0.0080 at 2 x 7 x 6 x 5 and 13 x 12 x 128, 0.0029 at 70 x 66 x 6 and
17 x 15 x 256); the identity's difference at most 0.036 of what the bounds allow; the loss through autograd 7.1e-4 (value) and 3.8e-3
(gradient) of its bounds on both paths.  The whole file ran in 15 s.
"""
import ctypes
import math
import os
import re
import time

import pytest
import torch

from kernel_bounds import U_FP32, Guarded, assert_guards_intact, assert_within
from ssim_bounds import fields, poisoned, ref_ssim
from ssim_loss_bounds import CASES, MEAN_CAP, case_data, case_id, random_gout, ref_vjp, tightness

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()
C1, C2 = 0.02 ** 2, 0.06 ** 2  # data_range 2
KINDS = ("uniform", "smooth")

#: across the boundaries of ssl_bwd_geom: a partial last z chunk under a tile that is the plane; 2 x 2 tiles, the last
#: ones clipped; the 32-pixel cap of a tile side, with a last tile one pixel wide
BOUNDARY = [((1, 13, 12, 19), (5, 1.2)), ((1, 35, 34, 3), (3, 1.0)), ((1, 33, 5, 2), (3, 1.0))]
GPU_CASES = CASES + [((1, 3, 3, 4), (3, 0.8)), ((1, 5, 4, 1), (3, 1.0)), ((1, 13, 12, 128), (5, 1.2)),
                     ((1, 17, 15, 256), (15, 2.0))] + BOUNDARY


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _forward(hip, HR, SR, win, sigma, label=""):
    """the C entry on device copies, sums and workspace in guarded buffers -> (B, NZ, 3, 2) float64 on the host; a second
    launch must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops, ssim
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    hr, sr = HR.to(DEV).contiguous(), SR.to(DEV).contiguous()
    taps = ssim.taps(win, sigma).to(DEV)
    n_ws = int(hip.wsr_ssim_pair_sums_workspace_floats(B, X, Y, NZ, win))
    assert n_ws >= B * NZ * 3 * 2
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, 3, 4), torch.float32, DEV)  # (B, NZ, 3, 2) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_ssim_pair_sums(hip_ops._p(hr), HR.shape[1], hip_ops._p(sr), SR.shape[1], hip_ops._p(taps), win, C1, C2,
                                     B, X, Y, NZ, hip_ops._p(ws.t), hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, ws, label=f"ssim_pair_sums {label}")
        got.append(out.t.view(torch.float64).cpu())
    assert got[0].shape == (B, NZ, 3, 2) and torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    return got[0]


def _backward(hip, HR, SR, gout, win, sigma, label=""):
    """the C entry on device copies, dsr in a guarded buffer pre-filled with NaN -> (B, 3, X, Y, NZ) fp32 on the host; every
    element must be overwritten, and a second launch must give the same bits"""
    from gan_sr_wind_field_amd import hip_ops, ssim
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    hr, sr = HR.to(DEV).contiguous(), SR.to(DEV).contiguous()
    g = gout.to(DEV).contiguous()
    taps = ssim.taps(win, sigma).to(DEV)
    got = []
    for _ in range(2):
        dsr = Guarded((B, 3, X, Y, NZ), torch.float32, DEV, fill=float("nan"))
        check(hip.wsr_ssim_pair_sums_bwd(hip_ops._p(hr), HR.shape[1], hip_ops._p(sr), SR.shape[1], hip_ops._p(g),
                                         hip_ops._p(taps), win, C1, C2, B, X, Y, NZ, hip_ops._p(dsr.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(dsr, label=f"ssim_pair_sums_bwd {label}")
        got.append(dsr.t.cpu())
    assert not bool(torch.isnan(got[0]).any()), f"{label}: an element of dsr was not written"
    assert torch.equal(_bits(got[0]), _bits(got[1])), f"{label}: two calls differ"
    return got[0]


def _tile(hip, X, Y, NZ, win):
    t = (ctypes.c_int32 * 3)()
    assert hip.wsr_ssim_pair_sums_bwd_tile(X, Y, NZ, win, t) == 0
    return tuple(t)


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_forward_against_float64_and_bit_equal_to_level_ssim(hip, case, kind):
    from gan_sr_wind_field_amd import hip_ops

    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, _, _, _ = case_data(case, kind)
    ref, bnd = ref_ssim(HR, SR, SR, win, sigma)
    worst = 0.0
    for c in (3, 5):
        got = _forward(hip, poisoned(HR, c), poisoned(SR, 8 - c), win, sigma, f"{case_id(case)} c={c}")
        worst = max(worst, assert_within(got, ref[..., :2], bnd[..., :2],
                                         f"ssim_pair_sums vs float64[{case_id(case)} {kind} c={c}]", kind="sums"))
    hr, sr = HR.to(DEV), SR.to(DEV)
    logged = hip_ops.level_ssim(hr, sr, sr, win, sigma)[..., :2].cpu()
    assert torch.equal(_bits(got), _bits(logged)), "the trained quantity is not the logged quantity, bit for bit"
    wrapped = hip_ops.ssim_pair_sums(hr, sr, win, sigma)
    assert wrapped.dtype == torch.float64 and torch.equal(_bits(wrapped.cpu()), _bits(got))
    print(f"[fwd] {case_id(case)} {kind}: worst |err| / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_backward_against_the_float64_vjp(hip, case, kind):
    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, gout, grad, bound = case_data(case, kind)
    assert tightness(grad, bound) <= MEAN_CAP, (case, kind, tightness(grad, bound))
    worst = 0.0
    for c in (3, 5):
        got = _backward(hip, poisoned(HR, c), poisoned(SR, 8 - c), gout, win, sigma, f"{case_id(case)} c={c}")
        worst = max(worst, assert_within(got, grad, bound, f"ssim_pair_sums_bwd vs float64[{case_id(case)} {kind} c={c}]"))
    print(f"[bwd] {case_id(case)} {kind}: tile {_tile(hip, X, Y, NZ, win)}, worst |err| / bound {worst:.3g}")


def test_the_boundary_shapes_cross_the_boundaries_of_the_tile_geometry(hip):
    (_, X, Y, NZ), (win, _) = BOUNDARY[0]
    TX, TY, ZC = _tile(hip, X, Y, NZ, win)
    assert (TX, TY) == (X, Y) and ZC < NZ and NZ % ZC != 0  # one tile per plane, a partial last z chunk
    (_, X, Y, NZ), (win, _) = BOUNDARY[1]
    TX, TY, ZC = _tile(hip, X, Y, NZ, win)
    assert TX < X < 2 * TX and TY < Y < 2 * TY and ZC == NZ  # 2 x 2 tiles, the last ones clipped
    (_, X, Y, NZ), (win, _) = BOUNDARY[2]
    assert _tile(hip, X, Y, NZ, win) == (32, Y, NZ) and X == 33  # the cap of a tile side; a last tile of one pixel
    seen = {_tile(hip, X, Y, NZ, win)[2] == NZ for (_, X, Y, NZ), (win, _) in GPU_CASES}
    assert seen == {True, False}  # chunks that are all of NZ, and chunks that are not
    # a function of (X, Y, NZ, win) alone, and refused like the launch
    t = (ctypes.c_int32 * 3)()
    assert hip.wsr_ssim_pair_sums_bwd_tile(6, 5, 3, 7, t) == -1 and hip.wsr_ssim_pair_sums_bwd_tile(6, 5, 257, 3, t) == -2
    assert hip.wsr_ssim_pair_sums_bwd_tile(6, 5, 3, 3, None) == -1


# ---------------------------------------------------------------------------------------------------- 3. an identity
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], BOUNDARY[1]], ids=case_id)
def test_the_directional_derivative_on_the_device(hip, case):
    """sum gout (P(SR + d) - P(SR - d)) = 2 <dsr, d> + O(|d|^3): no reference but the bounds.  SR is a multiple of 2^-12 and
    d = +-2^-6, so SR + d, SR - d and the half steps are exact in fp32; the step is that large because the difference of
    the two sums has to stand clear of their own rounding bounds, which do not shrink with it.  The third-order remainder
    of a central difference is bounded from a second evaluation at half the step: with D(t) the left side for the step t d, D(1) - 2 D(1/2) = (3/4) r + O(t^5),
    r the remainder of D(1); a factor 2 covers the higher orders."""
    (B, X, Y, NZ), (win, sigma) = case
    HR, SR, _ = (torch.round(t * 4096) / 4096 for t in fields(B, X, Y, NZ, seed=21, kind="smooth", noise=0.1))
    gen = torch.Generator().manual_seed(22)
    d = (torch.randint(0, 2, SR.shape, generator=gen).float() * 2 - 1) * 2.0 ** -6
    assert torch.equal((SR + d).double(), SR.double() + d.double())
    assert torch.equal((SR - d / 2).double(), SR.double() - d.double() / 2)
    gout = random_gout(B, NZ, 23)
    dsr = _backward(hip, HR, SR, gout, win, sigma, "identity")
    _, vb = ref_vjp(HR, SR, gout, win, sigma)  # (only the bound is used)

    def D(step):
        pp, pm = _forward(hip, HR, SR + step, win, sigma), _forward(hip, HR, SR - step, win, sigma)
        bp, bm = (ref_ssim(HR, s, s, win, sigma)[1][..., :2] for s in (SR + step, SR - step))
        return float((gout * (pp - pm)).sum()), float((gout.abs() * (bp + bm)).sum())

    lhs, b1 = D(d)
    half, b2 = D(d / 2)
    rhs = 2 * float((dsr.double() * d.double()).sum())
    third = 2 * (4.0 / 3.0) * (abs(lhs - 2 * half) + b1 + 2 * b2)
    allowed = b1 + 2 * float((vb * d.abs().double()).sum()) + third
    size = 2 * float(dsr.double().norm()) * float(d.double().norm())  # (the size of the terms of <dsr, d>)
    print(f"[identity] {case_id(case)}: |lhs - rhs| / allowed {abs(lhs - rhs) / allowed:.3g}, allowed / size {allowed / size:.3g}")
    assert abs(lhs - rhs) <= allowed and allowed <= 5e-2 * size, (case, lhs, rhs, allowed, size)


# ---------------------------------------------------------------------------------------------------- 4. structure
@pytest.mark.parametrize("case", [CASES[0], CASES[3], BOUNDARY[0]], ids=case_id)
def test_structure(hip, case):
    from gan_sr_wind_field_amd import hip_ops

    (B, X, Y, NZ), (win, sigma) = case
    npos = float((X - win + 1) * (Y - win + 1))
    for kind in KINDS:
        HR, SR, gout, grad, bound = case_data(case, kind)
        # SR = HR bit for bit: every sum is the number of positions; the backward is finite and inside its bound
        same = _forward(hip, HR, HR.clone(), win, sigma, f"SR = HR {case_id(case)}")
        assert bool((same == npos).all()), (case, kind, same.flatten()[:8])
        ref, bnd = ref_vjp(HR, HR, gout, win, sigma)
        got = _backward(hip, HR, HR.clone(), gout, win, sigma, f"SR = HR {case_id(case)}")
        assert bool(torch.isfinite(got).all())
        assert_within(got, ref, bnd, f"ssim_pair_sums_bwd at SR = HR[{case_id(case)} {kind}]")
        # a zero upstream gradient: a zero gradient
        zero = _backward(hip, HR, SR, torch.zeros_like(gout), win, sigma, "gout = 0")
        assert bool((zero == 0).all())
        # the wrapper: NaN-poisoned surplus channels are never read and get a zero gradient; the rest is the C entry's
        sr5 = poisoned(SR, 5).to(DEV).requires_grad_(True)
        P = hip_ops.ssim_pair_sums(poisoned(HR, 4).to(DEV), sr5, win, sigma)
        assert torch.equal(_bits(P.detach().cpu()), _bits(_forward(hip, HR, SR, win, sigma)))
        (P * gout.to(DEV)).sum().backward()
        assert bool((sr5.grad[:, 3:] == 0).all())
        assert torch.equal(_bits(sr5.grad[:, :3].cpu()), _bits(_backward(hip, HR, SR, gout, win, sigma)))
        # HR is detached: no gradient towards it, and a double backward is refused
        hr = HR.to(DEV).requires_grad_(True)
        sr = SR.to(DEV).requires_grad_(True)
        hip_ops.ssim_pair_sums(hr, sr, win, sigma).sum().backward()
        assert hr.grad is None and sr.grad is not None
        # ... and the forward does not depend on whether SR requires grad
        assert torch.equal(_bits(hip_ops.ssim_pair_sums(HR.to(DEV), SR.to(DEV), win, sigma).cpu()), _bits(P[..., :].detach().cpu()))


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_buffer_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops, ssim

    B, X, Y, NZ, WIN = 1, 6, 5, 3, 3
    HR, SR, _ = (t.to(DEV) for t in fields(B, X, Y, NZ, seed=1, kind="uniform"))
    TAPS = ssim.taps(15, 2.0).to(DEV)  # (long enough for every window the calls below name)
    GOUT = random_gout(B, NZ, 2).to(DEV)
    n_ws = int(hip.wsr_ssim_pair_sums_workspace_floats(B, X, Y, NZ, WIN))
    assert n_ws > 0
    out = Guarded((B, NZ, 3, 4), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    dsr = Guarded((B, 3, X, Y, NZ), torch.float32, DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws, dsr)]
    p = hip_ops._p

    def fwd(hr=HR, hr_c=3, sr=SR, sr_c=3, taps=TAPS, win=WIN, c1=C1, c2=C2, b=B, nx=X, ny=Y, nz=NZ, w=ws.t, o=out.t):
        return hip.wsr_ssim_pair_sums(p(hr), hr_c, p(sr), sr_c, p(taps), win, c1, c2, b, nx, ny, nz, p(w), p(o),
                                      hip_ops._stream())

    def bwd(hr=HR, hr_c=3, sr=SR, sr_c=3, g=GOUT, taps=TAPS, win=WIN, c1=C1, c2=C2, b=B, nx=X, ny=Y, nz=NZ, o=dsr.t):
        return hip.wsr_ssim_pair_sums_bwd(p(hr), hr_c, p(sr), sr_c, p(g), p(taps), win, c1, c2, b, nx, ny, nz, p(o),
                                          hip_ops._stream())

    shared = [dict(hr=None), dict(sr=None), dict(taps=None), dict(o=None), dict(hr_c=2), dict(sr_c=2), dict(b=0), dict(nx=0),
              dict(ny=-1), dict(nz=0), dict(win=4), dict(win=1), dict(win=17), dict(win=-3), dict(win=7), dict(nx=2),
              dict(win=5, ny=4), dict(c1=0.0), dict(c2=-1.0)]
    for kw in shared + [dict(w=None)]:
        assert fwd(**kw) == -1, kw
    for kw in shared + [dict(g=None)]:
        assert bwd(**kw) == -1, kw
    for kw in (dict(nz=257), dict(b=65536), dict(nx=32769), dict(ny=32769), dict(nx=32768, ny=32768, nz=2)):
        assert fwd(**kw) == -2 and bwd(**kw) == -2, kw
    wsf = hip.wsr_ssim_pair_sums_workspace_floats
    assert wsf(0, X, Y, NZ, 3) == wsf(1, X, Y, 257, 3) == wsf(1, X, Y, NZ, 4) == wsf(1, X, 2, NZ, 3) == wsf(1, X, Y, NZ, 7) == 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws, dsr), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    ok = hip_ops.ssim_pair_sums(HR, SR, 3, 1.0)
    assert ok.shape == (B, NZ, 3, 2) and bool(torch.isfinite(ok).all())
    for args in ((HR[:, :2], SR), (HR.long(), SR), (HR, SR[..., :2]), (HR, torch.cat([SR, SR]))):
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.ssim_pair_sums(*args, 3, 1.0)
    for win, sigma, rng, pattern in ((4, 1.0, 2.0, "window.*4"), (17, 1.0, 2.0, "17"), (3, 0.0, 2.0, "sigma"),
                                     (3, 1.0, 0.0, "data_range"), (7, 1.0, 2.0, "6 x 5.*7 x 7")):
        with pytest.raises(ValueError, match=pattern):
            hip_ops.ssim_pair_sums(HR, SR, win, sigma, rng)
    deep = torch.zeros((1, 3, 3, 3, 257), device=DEV)
    with pytest.raises(ValueError, match="257"):
        hip_ops.ssim_pair_sums(deep, deep, 3, 1.0)
    with pytest.raises(RuntimeError):
        hip_ops.ssim_pair_sums(HR.cpu(), SR, 3, 1.0)
    # non-contiguous and float64 inputs pass through .contiguous().float()
    wide = torch.cat([SR, SR], dim=4)[..., :NZ]
    assert not wide.is_contiguous() and torch.equal(_bits(hip_ops.ssim_pair_sums(HR.double(), wide, 3, 1.0)), _bits(ok))


# ---------------------------------------------------------------------------------------------------- 6. the loss
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("case", [((2, 12, 8, 3), (5, 1.2)), ((1, 16, 16, 2), (11, 1.5))], ids=case_id)
def test_the_loss_through_autograd(hip, monkeypatch, case, fused):
    """value and SR.grad of ``ssim_loss`` on the device against float64, on both paths (each held to the truth, not to the
    other).  L = 1 - sum P0 / n is linear in the sums: its bound is the sum of their bounds over n, and its gradient is
    the VJP with G0 = -1 / n, G1 = 0 with that VJP's bound; both widened by 4 u for the float32 scalar."""
    from test_ssim_loss import Section

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import ssim_loss as mod

    monkeypatch.setenv("WSR_FUSED_SSIM_LOSS", fused)
    calls = []
    orig = hip_ops.ssim_pair_sums
    monkeypatch.setattr(hip_ops, "ssim_pair_sums", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    (B, X, Y, NZ), (win, sigma) = case
    n = 3 * B * NZ * (X - win + 1) * (Y - win + 1)
    for kind in KINDS:
        HR, SR, _ = fields(B, X, Y, NZ, seed=5, kind=kind, noise=0.05, c=4)
        sr = SR.to(DEV).requires_grad_(True)
        n0 = len(calls)
        L = mod.ssim_loss(HR.to(DEV), sr, Section(window_size=win, sigma=sigma))
        assert L.dtype == torch.float32 and L.dim() == 0 and len(calls) - n0 == (1 if fused == "1" else 0)
        L.backward()
        ref, bnd = ref_ssim(HR, SR, SR, win, sigma)
        want, dL = 1.0 - float(ref[..., 0].sum()) / n, float(bnd[..., 0].sum()) / n
        lim = dL + 4 * U_FP32 * max(abs(want), 1.0)
        assert abs(float(L) - want) <= lim, (case, kind, float(L), want, lim)
        gout = torch.zeros((B, NZ, 3, 2), dtype=torch.float64)
        gout[..., 0] = -1.0 / n
        grad, bound = ref_vjp(HR, SR, gout, win, sigma)
        assert tightness(grad, bound) <= MEAN_CAP
        worst = assert_within(sr.grad[:, :3].cpu(), grad, bound + 4 * U_FP32 * grad.abs(),
                              f"ssim_loss grad vs float64[{case_id(case)} {kind} fused={fused}]")
        assert bool((sr.grad[:, 3:] == 0).all())
        print(f"[loss] {case_id(case)} {kind} fused={fused}: value |err| / bound {abs(float(L) - want) / lim:.3g}, grad worst "
              f"|err| / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- 7. the model
def _small_gan(section, spectral=None):
    """the small GAN of tests/test_grad_clip_gpu.py on the device, ``[SSIM_LOSS]`` (and ``[SPECTRAL_LOSS]``) switched as
    the arguments say"""
    from test_grad_clip_gpu import _build_gan

    gan, cfg = _build_gan(clip=False)
    for sec, keys in ((cfg.ssim_loss, section), (cfg.spectral_loss, spectral)):
        sec.present = keys is not None
        for k, v in (keys or {}).items():
            setattr(sec, k, v)
    return gan, cfg


def _reset_sections(cfg):
    from gan_sr_wind_field_amd.config.config import SpectralLossConfig, SsimLossConfig

    for cls, sec in ((SsimLossConfig, cfg.ssim_loss), (SpectralLossConfig, cfg.spectral_loss)):  # (class-level singletons)
        for k in ["present"] + [k for k, _ in cls._schema]:
            setattr(sec, k, getattr(cls, k))


def test_update_G_with_and_without_the_section(hip, monkeypatch):
    from gan_sr_wind_field_amd import hip_ops
    from oracle.gan import synthetic_batch

    LR, HR, Z, x, y = (t.to(DEV) for t in synthetic_batch(2, 16, 4, 4, seed=2001))
    B, _, X, Y, NZ = HR.shape
    WIN, SIGMA, W = 7, 1.0, 0.1
    n = 3 * B * NZ * (X - WIN + 1) * (Y - WIN + 1)
    seen = []
    orig = hip_ops.ssim_pair_sums

    def recorded(hr, sr, win=11, sigma=1.5, data_range=2.0):
        seen.append((hr.detach().cpu(), sr.detach().cpu(), win, sigma, data_range))
        return orig(hr, sr, win, sigma, data_range)

    monkeypatch.setattr(hip_ops, "ssim_pair_sums", recorded)
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
        missing = type("NoSection", (), {"__getattr__": lambda self, k: getattr(cfg00, k) if k != "ssim_loss" else
                                         (_ for _ in ()).throw(AttributeError(k))})()
        gan00.cfg = missing
        w00, l00 = g_iteration(gan00, cfg00)
        assert l00 == l0 and all(torch.equal(w00[k], w0[k]) for k in w0)

        section = dict(weight=W, window_size=WIN, sigma=SIGMA, data_range=2.0)
        gan1, cfg1 = _small_gan(section)
        w1, l1 = g_iteration(gan1, cfg1)
        assert len(seen) == 1 and seen[0][2:] == (WIN, SIGMA, 2.0) and torch.equal(seen[0][0], HR.cpu())  # once per pass
        ref, bnd = ref_ssim(seen[0][0], seen[0][1], seen[0][1], WIN, SIGMA)
        want, dL = 1.0 - float(ref[..., 0].sum()) / n, float(bnd[..., 0].sum()) / n
        assert set(l1) == keys | {"ssim"} and want > 0
        assert abs(l1["ssim"] - W * want) <= W * (dL + 8 * U_FP32 * max(want, 1.0)), (l1["ssim"], W * want, dL)
        assert all(l1[k] == l0[k] for k in keys - {"total"})
        assert abs((l1["total"] - l0["total"]) - l1["ssim"]) <= 4 * U_FP32 * abs(l1["total"])
        assert any(not torch.equal(w1[k], w0[k]) for k in w0) and all(bool(torch.isfinite(v).all()) for v in w1.values())

        # with [SPECTRAL_LOSS] too: ``ssim`` behind ``spectral``, the same value
        gan3, cfg3 = _small_gan(section, spectral=dict(weight=0.05))
        _, l3 = g_iteration(gan3, cfg3)
        assert list(l3)[-2:] == ["spectral", "ssim"] and l3["ssim"] == l1["ssim"] and l3["spectral"] > 0
        cfg3.spectral_loss.present = False

        # a NaN planted in the term: the Adam step is skipped, the weights stay bit-equal
        gan2, cfg2 = _small_gan(section)
        w_before = {k: v.detach().clone() for k, v in gan2.G.state_dict().items()}
        monkeypatch.setattr(hip_ops, "ssim_pair_sums", lambda *a, **kw: orig(*a, **kw) * float("nan"))
        _, l2 = g_iteration(gan2, cfg2)
        assert math.isnan(l2["ssim"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, w_before[k]), k
        monkeypatch.setattr(hip_ops, "ssim_pair_sums", recorded)
        m = len(seen)
        gan1.update_G(LR, HR, Z, 0, False)  # validation: once more, logged in the validation dict
        assert len(seen) == m + 1 and float(gan1.get_G_val_loss_dict_ref()["ssim"]) > 0
    finally:
        _reset_sections(cfg0)


def test_run_train_and_test_with_the_section(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.config.config import Config

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.ssim_pair_sums

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "ssim_pair_sums", counted)
    section = "\n[SSIM_LOSS]\nweight = 0.1\nwindow_size = 11\nsigma = 1.5\ndata_range = 2.0\n"
    spectral = "\n[SPECTRAL_LOSS]\nweight = 0.05\nwindow = hann\nk_min = 1\nk_max = 0\nrel_floor = 1e-06\n"
    extras = "\n[GRAD_CLIP]\nclip_generator = True\n\n[EMA]\n\n[SSIM]\n"
    try:
        for name, extra, on in (("plain", "", False), ("ssim", section, True), ("ssim_all", extras + spectral + section, True)):
            ini = str(tmp_path / f"{name}.ini")
            cfg = _write_ini(ini)
            cfg.name = name
            if "GRAD_CLIP" in extra:
                cfg.generator.max_norm = 0.5
            plain_text = cfg.asINI()
            assert "SSIM_LOSS" not in plain_text  # today's text
            with open(ini, "w") as f:
                f.write(plain_text + extra)
            before = calls["n"]
            runmod.main(["--train", "--test", "--cfg", ini])
            run_dir = os.path.join(str(tmp_path), "runs", name)
            with open(os.path.join(run_dir, f"{name}.train")) as f:
                log = f.read()
            with open(os.path.join(run_dir, "config.ini")) as f:
                snapshot = f.read()
            values = [float(v) for v in re.findall(r"\bssim: (\S+)", log)]
            if on:
                assert calls["n"] > before and snapshot.endswith(section)
                # (weight 0.1 times a loss in [0, 2); the first line holds the dict's initial zero)
                assert len(values) >= 6 and all(math.isfinite(v) and 0 <= v < 0.2 for v in values) and max(values) > 0, values
                if spectral in extra:
                    assert len(re.findall(r"\bspectral: (\S+)", log)) == len(values)
            else:
                assert calls["n"] == before and not values and "SSIM_LOSS" not in snapshot
            assert os.path.isfile(os.path.join(run_dir, "G_6.pth"))
    finally:
        _reset_sections(Config)
    print(f"[time] tests/test_ssim_loss_gpu.py up to here: {time.time() - T0:.1f} s")
