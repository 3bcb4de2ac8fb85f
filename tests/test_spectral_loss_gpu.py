"""[SPECTRAL_LOSS] on the GPU: ``wsr_spectral_energy`` and ``wsr_spectral_energy_bwd`` (csrc/spectral_loss.hip) against the
float64 evaluation of the definitions (``ref_spectra`` of tests/test_spectra.py for the energies, ``ref_vjp`` of
tests/test_spectral_loss.py - explicit DFT matrices - for the vector-Jacobian product; nothing of spectral_loss.py or of
the kernels), the quadratic identity evaluated on the device, structure, refusals, the loss through autograd on both
paths, and the model: a generator iteration and ``run.py --train --test`` with and without the section.  Every buffer a
kernel writes lives in a ``Guarded`` allocation.

Bounds (kernel_bounds.py's convention, LAMBDA = 16 untouched).  Energies: the per-bin bound of test_spectra_gpu.py
(``delta_a``).  The VJP, per element of dsr: the sum of the forward's error in the saved F_sr propagated
(2 scale w delta_sr sum_modes h |G|), the inverse transform's own rounding (LAMBDA 2^-24 sqrt(X KY) 2 scale w ||h G F||_2),
2^-24 relative for rounding gbin, and the plane average of those for the mean term.  The inputs are such that this bound
is at most 1e-2 of the rms of the float64 gradient (asserted), so a dropped or misplaced mode fails; no element is exempt.
The loss: those bounds carried through the formula (``loss_bounds``).

Measured worst |err| / bound on the MI355X, per shape (B, X, Y, NZ), the larger of the two windows (every test prints its
figure: run with ``-s``; DESIGN.md section 20 has the same table):

    shape            energy    VJP       VJP bound / rms of the float64 gradient (asserted <= 1e-2)
    (2, 7, 6, 5)     0.038     0.017     4.5e-4
    (1, 16, 16, 10)  0.015     0.0057    1.7e-3
    (1, 1, 8, 3)     0.056     0.015     7.8e-5
    (1, 5, 1, 4)     0.039     0.029     4.4e-5
    (1, 33, 20, 3)   0.026     0.0038    4.1e-3
    (1, 9, 5, 130)   0.032     0.017     5.0e-4
    (1, 70, 6, 17)   0.038     0.0086    2.5e-3
    (1, 3, 130, 2)   0.023     0.011     1.7e-3
    (1, 7, 129, 20)  0.016     0.0074    5.0e-3

The quadratic identity, |lhs - rhs| / allowed: 8.1e-5 (hann) and 1.4e-6 (none) at (2, 7, 6, 5), 9.3e-7 and 9.1e-6 at
(1, 33, 20, 3).  The loss through autograd, value / worst element of SR.grad: the kernels 4.4e-4 / 3.1e-3 at (2, 12, 8, 5)
and 1.3e-4 / 5.5e-4 at (1, 16, 16, 10); the composed path (``WSR_FUSED_SPECTRAL=0``) 1.5e-3 / 1.9e-3 and 3.6e-4 / 5.5e-4.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from kernel_bounds import Guarded, U_FP32, assert_guards_intact, assert_within
from test_spectra import np_bins, random_fields, ref_spectra
from test_spectral_loss import Section, loss_bounds, np_bin_set, ref_energy, ref_vjp, truth_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
WINDOW_CODES = {"none": 0, "hann": 1}
# (B, X, Y, NZ): the issue's six, and one shape across each chunk boundary of the new kernels' geometry:
#   (1, 70, 6, 17)  kx chunks - 32 modes per workgroup pass of the forward column kernel at 16 levels, 64 rows per slab and
#                   64 values of x per pass of the inverse column kernel - and z chunks: 17 levels, 16 per workgroup of
#                   both column passes
#   (1, 7, 129, 20) row-pass lines: a workgroup of the forward row pass stages at most 8192 / Y = 63 -> 60 lines (x, z)
#                   instead of 64, one of the inverse row pass 8192 / (2 KY) = 63 -> 60; with 20 levels that is 3 values of
#                   x per workgroup, so X = 7 takes three line blocks of each pass, the last one with 1 of its 3 values of
#                   x.  ((1, 33, 20, 3): 63 lines padded to 64, two blocks; (1, 9, 5, 130): 130 levels, 64 per workgroup
#                   of the row passes; (1, 3, 130, 2): the same limit of 60 lines with a single block of 6.)
CASES = [(2, 7, 6, 5), (1, 16, 16, 10), (1, 1, 8, 3), (1, 5, 1, 4), (1, 33, 20, 3), (1, 9, 5, 130), (1, 70, 6, 17),
         (1, 3, 130, 2), (1, 7, 129, 20)]
IDS = ["x".join(map(str, d)) for d in CASES]


def _poisoned(t, c):
    """``c`` channels: the first three of t, the surplus ones NaN (they must never be read)"""
    if c == 3:
        return t[:, :3].contiguous()
    return torch.cat([t[:, :3], torch.full((t.shape[0], c - 3) + tuple(t.shape[2:]), float("nan"))], dim=1).contiguous()


def _forward(hip, HR, SR, window, save=True, label=""):
    """the C entry on device copies, out / workspace / saved in guarded buffers, twice: the same bits ->
    (e (B, NZ, NK, 2) float64 on the host, saved on the device or None)"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, _, X, Y, NZ = HR.shape
    hr, sr = HR.to(DEV).contiguous(), SR.to(DEV).contiguous()
    NK = int(hip.wsr_level_spectra_bins(X, Y))
    assert NK == np_bins(X, Y)[1]
    n_ws = int(hip.wsr_spectral_energy_workspace_floats(B, X, Y, NZ))
    n_sv = int(hip.wsr_spectral_energy_saved_floats(B, X, Y, NZ))
    assert n_sv == 2 * B * 3 * X * (Y // 2 + 1) * NZ and n_ws > 2 * n_sv
    got = []
    for _ in range(2):
        out = Guarded((B, NZ, NK, 4), torch.float32, DEV)  # (B, NZ, NK, 2) doubles
        ws = Guarded((n_ws,), torch.float32, DEV)
        sv = Guarded((n_sv,), torch.float32, DEV) if save else None
        check(hip.wsr_spectral_energy(hip_ops._p(hr), HR.shape[1], hip_ops._p(sr), SR.shape[1], B, X, Y, NZ,
                                      WINDOW_CODES[window], hip_ops._p(ws.t), hip_ops._p(sv.t if save else None),
                                      hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(*([out, ws] + ([sv] if save else [])), label=f"spectral_energy {label}")
        got.append((out.t.view(torch.float64).cpu(), sv.t.clone() if save else None))
    assert torch.equal(got[0][0].view(torch.int64), got[1][0].view(torch.int64)), f"{label}: two calls differ"
    if save:
        assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32)), f"{label}: two saved spectra differ"
        assert bool(torch.isfinite(got[0][1]).all()), f"{label}: an element of saved was not written"
    return got[0]


def _backward(hip, saved, gbin, dims, window, label=""):
    """``wsr_spectral_energy_bwd`` with dsr and the workspace in guarded buffers, twice: the same bits -> dsr on the host"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, X, Y, NZ = dims
    g = torch.as_tensor(gbin, dtype=torch.float64).contiguous().to(DEV)
    n_ws = int(hip.wsr_spectral_energy_workspace_floats(B, X, Y, NZ))
    got = []
    for _ in range(2):
        dsr = Guarded((B, 3, X, Y, NZ), torch.float32, DEV)
        ws = Guarded((n_ws,), torch.float32, DEV)
        check(hip.wsr_spectral_energy_bwd(hip_ops._p(saved), hip_ops._p(g), B, X, Y, NZ, WINDOW_CODES[window], hip_ops._p(ws.t),
                                          hip_ops._p(dsr.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(dsr, ws, label=f"spectral_energy_bwd {label}")
        got.append(dsr.t.cpu())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), f"{label}: two calls differ"
    return got[0]


# ---------------------------------------------------------------------------------------------------- 1. energy
@pytest.mark.parametrize("window", ["hann", "none"])
@pytest.mark.parametrize("dims", CASES, ids=IDS)
def test_energy_against_float64(hip, dims, window):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = dims
    worst = 0.0
    for mean in (0.0, 8.0):
        HR, SR, _ = random_fields(B, X, Y, NZ, seed=X * 7 + NZ + int(mean), mean=mean)
        ref, bnd = (torch.from_numpy(v[..., :2].copy()) for v in ref_spectra(HR, SR, HR, window))
        for c in (3, 5):
            hr, sr = _poisoned(HR, c), _poisoned(SR, 8 - c)
            got, _ = _forward(hip, hr, sr, window, save=(c == 5), label=f"{dims} c={c}")
            worst = max(worst, assert_within(got, ref, bnd, f"spectral_energy vs float64[{dims} {window} mean={mean} c={c}]",
                                             kind="sums"))
            wrapped = hip_ops.spectral_energy(hr.to(DEV), sr.to(DEV), window)  # the wrapper: the same launch
            assert wrapped.dtype == torch.float64 and torch.equal(wrapped.cpu().view(torch.int64), got.view(torch.int64))
    print(f"[energy] {dims} {window}: worst |err| / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- 2. the VJP
def _gbins(B, NZ, X, Y, seed):
    """a random gbin and one that is zero in all but one (non-empty, middle) bin"""
    NK = np_bins(X, Y)[1]
    g = torch.randn((B, NZ, NK), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()
    K = np_bin_set(X, Y)
    one = np.zeros_like(g)
    one[:, :, K[len(K) // 2]] = g[:, :, K[len(K) // 2]]
    return {"random": g, "one bin": one}


@pytest.mark.parametrize("window", ["hann", "none"])
@pytest.mark.parametrize("dims", CASES, ids=IDS)
def test_vjp_against_float64(hip, dims, window):
    B, X, Y, NZ = dims
    worst = tight = 0.0
    for mean in (0.0, 1.0):
        HR, SR, _ = random_fields(B, X, Y, NZ, seed=X * 5 + NZ + int(mean), mean=mean)
        _, saved = _forward(hip, HR, SR, window, label=f"{dims}")
        for name, gbin in _gbins(B, NZ, X, Y, seed=X + Y + NZ).items():
            ref, bnd = ref_vjp(SR, gbin, window)
            rms = np.sqrt((ref ** 2).mean(axis=(1, 2, 3, 4)))
            assert (bnd.max(axis=(1, 2, 3, 4)) <= 1e-2 * rms).all(), (dims, window, name, bnd.max(), rms)
            tight = max(tight, float((bnd.max(axis=(1, 2, 3, 4)) / rms).max()))
            got = _backward(hip, saved, gbin, dims, window, label=f"{dims} {name}")
            worst = max(worst, assert_within(got, torch.from_numpy(ref), torch.from_numpy(bnd),
                                             f"spectral_energy_bwd vs float64[{dims} {window} mean={mean} {name}]"))
            plane = got.double().sum(dim=(2, 3))  # every plane sums to zero: the truth's does, within the summed bounds
            assert bool((plane.abs() <= torch.from_numpy(bnd.sum(axis=(2, 3)))).all()), (dims, window, name)
    print(f"[vjp] {dims} {window}: worst |err| / bound {worst:.3g} (bound at most {tight:.2g} of the gradient's rms)")


# ---------------------------------------------------------------------------------------------------- 3. the identity
@pytest.mark.parametrize("dims", [(2, 7, 6, 5), (1, 33, 20, 3)], ids=str)
def test_the_quadratic_identity_on_the_device(hip, dims):
    """sum gbin (e_sr(SR + d) - e_sr(SR - d)) = 2 <dsr, d> exactly for any d (e_sr is quadratic in SR): no reference but the
    bounds.  SR and d are multiples of 2^-10 below 8 in size, so SR + d and SR - d are exact in fp32."""
    B, X, Y, NZ = dims
    NK = np_bins(X, Y)[1]
    gen = torch.Generator().manual_seed(17)
    HR = torch.randn((B, 3, X, Y, NZ), generator=gen)
    SR, d = (torch.round(torch.randn((B, 3, X, Y, NZ), generator=gen).clamp(-7, 7) * 1024) / 1024 for _ in range(2))
    assert torch.equal((SR + d).double(), SR.double() + d.double())
    gbin = torch.randn((B, NZ, NK), generator=gen, dtype=torch.float64)
    for window in ("hann", "none"):
        _, saved = _forward(hip, HR, SR, window)
        dsr = _backward(hip, saved, gbin, dims, window)
        _, vb = ref_vjp(SR, gbin.numpy(), window)  # (only the bound is used)
        ep, _ = _forward(hip, HR, SR + d, window, save=False)
        em, _ = _forward(hip, HR, SR - d, window, save=False)
        bp, bm = (ref_energy(HR, s, window)[1][..., 1] for s in (SR + d, SR - d))
        lhs = float((gbin * (ep[..., 1] - em[..., 1])).sum())
        rhs = 2 * float((dsr.double() * d.double()).sum())
        allowed = float((gbin.abs().numpy() * (bp + bm)).sum()) + 2 * float((vb * d.abs().double().numpy()).sum())
        print(f"[identity] {dims} {window}: |lhs - rhs| / allowed {abs(lhs - rhs) / allowed:.3g}")
        size = 2 * float(dsr.double().norm()) * float(d.double().norm())  # (the size of the terms of <dsr, d>)
        assert abs(lhs - rhs) <= allowed and allowed <= 1e-2 * size, (dims, window, lhs, rhs, allowed, size)


# ---------------------------------------------------------------------------------------------------- 4. structure
def test_structure(hip):
    from gan_sr_wind_field_amd import hip_ops

    for dims in ((2, 7, 6, 5), (1, 9, 5, 130), (1, 70, 6, 17)):
        B, X, Y, NZ = dims
        NK = np_bins(X, Y)[1]
        HR, SR, _ = random_fields(*dims, seed=33, mean=1.0)
        same, saved = _forward(hip, HR, HR.clone(), "hann", label=f"SR = HR {dims}")  # (two calls: the same bits, inside)
        i64 = same.view(torch.int64)
        assert torch.equal(i64[..., 1], i64[..., 0]) and bool((same[..., 0].sum(dim=-1) > 0).all()), dims
        zero = _backward(hip, saved, np.zeros((B, NZ, NK)), dims, "hann", label=f"gbin = 0 {dims}")
        assert bool((zero == 0).all()), dims
        # surplus channels of a 5-channel SR: never read, zero gradient through the wrapper; the rest is the C entry's
        sr5 = _poisoned(SR, 5).to(DEV).requires_grad_(True)
        e = hip_ops.spectral_energy(_poisoned(HR, 4).to(DEV), sr5, "hann")
        gbin = torch.randn((B, NZ, NK), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (e[..., 1] * gbin.to(DEV)).sum().backward()
        assert sr5.grad.shape == sr5.shape and bool((sr5.grad[:, 3:] == 0).all()) and bool(torch.isfinite(sr5.grad).all())
        e_c, sv = _forward(hip, HR, SR, "hann")
        # the six-plane forward repeats the arithmetic of csrc/spectra.hip: the bits of wsr_level_spectra's first two sums
        ls = hip_ops.level_spectra(HR.to(DEV), SR.to(DEV), HR.to(DEV), "hann")[..., :2].contiguous().cpu()
        assert torch.equal(e_c.view(torch.int64), ls.view(torch.int64)), dims
        direct = _backward(hip, sv, gbin, dims, "hann")
        assert torch.equal(sr5.grad[:, :3].cpu().view(torch.int32), direct.view(torch.int32)), dims
        g_hr = hip_ops.spectral_energy(HR.to(DEV).requires_grad_(True), SR.to(DEV), "hann")
        assert not g_hr.requires_grad  # only e_sr carries gradient, and only towards SR: nothing is saved without it
        bf = hip_ops.spectral_energy(HR.to(DEV).bfloat16(), SR.to(DEV).bfloat16(), "none")  # (made contiguous().float())
        assert bf.dtype == torch.float64 and bool(torch.isfinite(bf).all())


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_buffer_untouched(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = 1, 4, 4, 3
    HR, SR, _ = (t.to(DEV) for t in random_fields(B, X, Y, NZ, seed=1))
    NK = int(hip.wsr_level_spectra_bins(X, Y))
    n_ws = int(hip.wsr_spectral_energy_workspace_floats(B, X, Y, NZ))
    n_sv = int(hip.wsr_spectral_energy_saved_floats(B, X, Y, NZ))
    out = Guarded((B, NZ, NK, 4), torch.float32, DEV)
    ws = Guarded((n_ws,), torch.float32, DEV)
    sv = Guarded((n_sv,), torch.float32, DEV)
    dsr = Guarded((B, 3, X, Y, NZ), torch.float32, DEV)
    gbin = torch.ones((B, NZ, NK), dtype=torch.float64, device=DEV)
    before = [g.base.view(torch.int32).clone() for g in (out, ws, sv, dsr)]
    p = hip_ops._p

    def fwd(hr=HR, hr_c=3, sr=SR, sr_c=3, b=B, nx=X, ny=Y, nz=NZ, win=1, w=ws.t, s=sv.t, o=out.t):
        return hip.wsr_spectral_energy(p(hr), hr_c, p(sr), sr_c, b, nx, ny, nz, win, p(w), p(s), p(o), hip_ops._stream())

    def bwd(s=sv.t, g=gbin, b=B, nx=X, ny=Y, nz=NZ, win=1, w=ws.t, d=dsr.t):
        return hip.wsr_spectral_energy_bwd(p(s), p(g), b, nx, ny, nz, win, p(w), p(d), hip_ops._stream())

    sizes_bad = [dict(b=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(win=2), dict(win=-1)]
    sizes_big = [dict(nx=1025), dict(ny=1025), dict(b=65536), dict(nz=65536), dict(nx=1024, ny=1024, nz=2048)]
    for kw in [dict(hr=None), dict(sr=None), dict(w=None), dict(o=None), dict(hr_c=2), dict(sr_c=0)] + sizes_bad:
        assert fwd(**kw) == -1, kw
    for kw in [dict(s=None), dict(g=None), dict(w=None), dict(d=None)] + sizes_bad:
        assert bwd(**kw) == -1, kw
    for kw in sizes_big:
        assert fwd(**kw) == -2 and bwd(**kw) == -2, kw
    for fn in (hip.wsr_spectral_energy_workspace_floats, hip.wsr_spectral_energy_saved_floats):
        assert fn(1, 1025, 4, 3) == 0 == fn(0, 4, 4, 3) and fn(1, 4, 4, 65536) == 0 and fn(1, 4, 4, 3) > 0
    torch.cuda.synchronize()
    for g, b4 in zip((out, ws, sv, dsr), before):
        assert torch.equal(g.base.view(torch.int32), b4)

    # the wrapper: every refusal a ValueError with the numbers
    ok = hip_ops.spectral_energy(HR, SR)
    assert ok.shape == (B, NZ, NK, 2) and bool(torch.isfinite(ok).all())
    bad = [(HR[:, :2], SR), (HR, SR[:, :2]), (HR[0], SR), (HR, SR[..., :2]), (HR, torch.cat([SR, SR])), (HR.long(), SR)]
    for args in bad:
        with pytest.raises(ValueError, match=r"\d"):
            hip_ops.spectral_energy(*args)
    with pytest.raises(ValueError, match="window.*hamming"):
        hip_ops.spectral_energy(HR, SR, "hamming")
    wide = torch.zeros((1, 3, 1025, 1, 1), device=DEV)
    with pytest.raises(ValueError, match="1025"):
        hip_ops.spectral_energy(wide, wide)
    with pytest.raises(RuntimeError):
        hip_ops.spectral_energy(HR.cpu(), SR)


# ---------------------------------------------------------------------------------------------------- 6. the loss
@pytest.mark.parametrize("fused", ["1", "0"], ids=["kernels", "composed"])
@pytest.mark.parametrize("dims,ks", [((2, 12, 8, 5), (1, 0)), ((1, 16, 16, 10), (2, -2))], ids=str)
def test_the_loss_through_autograd(hip, monkeypatch, dims, ks, fused):
    """value and SR.grad of ``spectral_loss`` on the device against float64, on both paths (each held to the truth, not to
    the other): the bounds of the energies and of the VJP carried through the formula"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import spectral_loss as slmod

    monkeypatch.setenv("WSR_FUSED_SPECTRAL", fused)
    calls = []
    orig = hip_ops.spectral_energy
    monkeypatch.setattr(hip_ops, "spectral_energy", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    B, X, Y, NZ = dims
    NK = np_bins(X, Y)[1]
    k_min, k_max = ks[0], (NK + ks[1] if ks[1] < 0 else ks[1])
    HR, SR, _ = random_fields(B, X, Y, NZ, seed=5, noise=0.5, c=4)
    for window in ("hann", "none"):
        sec = Section(window=window, k_min=k_min, k_max=k_max, rel_floor=1e-6)
        sr = SR.to(DEV).requires_grad_(True)
        n0 = len(calls)
        L = slmod.spectral_loss(HR.to(DEV), sr, sec)
        assert L.dtype == torch.float32 and L.dim() == 0 and len(calls) - n0 == (1 if fused == "1" else 0)
        L.backward()
        e, be = ref_energy(HR, SR, window)
        want, dL, gbin, dg = loss_bounds(e, be, X, Y, k_min, k_max, 1e-6)
        assert abs(float(L) - want) <= dL + 2 * U_FP32 * want, (dims, window, float(L), want, dL)
        ref, bnd = ref_vjp(SR, gbin, window, dgbin=dg)
        assert bnd.max() <= 1e-2 * math.sqrt((ref ** 2).mean()), (dims, window)
        worst = assert_within(sr.grad[:, :3].cpu(), torch.from_numpy(ref), torch.from_numpy(bnd),
                              f"spectral_loss grad vs float64[{dims} {window} fused={fused}]")
        assert bool((sr.grad[:, 3:] == 0).all())
        print(f"[loss] {dims} {window} fused={fused}: value |err| / bound {abs(float(L) - want) / (dL + 2 * U_FP32 * want):.3g}, "
              f"grad worst |err| / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- 7. the model
def _small_gan(section):
    """the small GAN of tests/test_grad_clip_gpu.py on the device, ``[SPECTRAL_LOSS]`` switched as ``section`` says"""
    from test_grad_clip_gpu import _build_gan

    gan, cfg = _build_gan(clip=False)
    sl = cfg.spectral_loss
    sl.present = section is not None
    for k, v in (section or {}).items():
        setattr(sl, k, v)
    return gan, cfg


def _reset_section(cfg):
    from gan_sr_wind_field_amd.config.config import SpectralLossConfig

    for k in ("present", "weight", "window", "k_min", "k_max", "rel_floor"):  # (the class-level singleton)
        setattr(cfg.spectral_loss, k, getattr(SpectralLossConfig, k))


def test_update_G_with_and_without_the_section(hip, monkeypatch):
    from gan_sr_wind_field_amd import hip_ops
    from oracle.gan import synthetic_batch

    LR, HR, Z, x, y = (t.to(DEV) for t in synthetic_batch(2, 16, 4, 4, seed=2001))
    X, Y = HR.shape[2:4]
    seen = []
    orig = hip_ops.spectral_energy

    def recorded(hr, sr, window="hann"):
        seen.append((hr.detach().cpu(), sr.detach().cpu(), window))
        return orig(hr, sr, window)

    monkeypatch.setattr(hip_ops, "spectral_energy", recorded)
    keys = {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}

    def g_iteration(gan, cfg):
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 1)
        gan.optimize_parameters(LR, HR, Z, 0)
        torch.cuda.synchronize()
        grad = gan.G.hr_convs[2].weight.grad.detach().cpu().clone()
        return grad, {k: float(v.detach()) for k, v in gan.get_G_train_loss_dict_ref().items()}

    gan0, cfg0 = _small_gan(None)
    try:
        g0, l0 = g_iteration(gan0, cfg0)
        assert not seen and set(l0) == keys and set(gan0.get_G_val_loss_dict_ref()) == keys  # never called, today's keys

        gan1, cfg1 = _small_gan(dict(weight=0.05, window="hann", k_min=1, k_max=0, rel_floor=1e-6))
        g1, l1 = g_iteration(gan1, cfg1)
        assert len(seen) == 1 and torch.equal(seen[0][0], HR.cpu())  # once per generator pass
        e, be = ref_energy(seen[0][0], seen[0][1], "hann")
        want, dL, _, _ = loss_bounds(e, be, X, Y)
        assert set(l1) == keys | {"spectral"} and want > 0
        assert abs(l1["spectral"] - 0.05 * want) <= 0.05 * (dL + 4 * U_FP32 * want), (l1["spectral"], 0.05 * want, dL)
        assert all(l1[k] == l0[k] for k in keys - {"total"})
        assert abs((l1["total"] - l0["total"]) - l1["spectral"]) <= 4 * U_FP32 * abs(l1["total"])
        assert not torch.equal(g1, g0) and bool(torch.isfinite(g1).all())

        # a NaN planted in the spectral term: the Adam step is skipped, the weights stay bit-equal
        gan2, cfg2 = _small_gan(dict(weight=0.05))
        w_before = {k: v.detach().clone() for k, v in gan2.G.state_dict().items()}
        monkeypatch.setattr(hip_ops, "spectral_energy", lambda hr, sr, window="hann": orig(hr, sr, window) * float("nan"))
        _, l2 = g_iteration(gan2, cfg2)
        assert math.isnan(l2["spectral"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, w_before[k]), k
        monkeypatch.setattr(hip_ops, "spectral_energy", recorded)
        n = len(seen)
        gan1.update_G(LR, HR, Z, 0, False)  # validation: once more, logged in the validation dict
        assert len(seen) == n + 1 and float(gan1.get_G_val_loss_dict_ref()["spectral"]) > 0
    finally:
        _reset_section(cfg0)


def test_run_train_and_test_with_the_section(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.config.config import Config

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    calls = {"n": 0}
    orig = hip_ops.spectral_energy

    def counted(*a, **kw):
        calls["n"] += 1
        return orig(*a, **kw)

    monkeypatch.setattr(hip_ops, "spectral_energy", counted)
    section = "\n[SPECTRAL_LOSS]\nweight = 0.05\nwindow = hann\nk_min = 1\nk_max = 0\nrel_floor = 1e-06\n"
    extras = "\n[GRAD_CLIP]\nclip_generator = True\n\n[EMA]\n"
    try:
        for name, extra, want_calls in (("plain", "", False), ("spec", section, True), ("spec_ema_clip", extras + section, True)):
            ini = str(tmp_path / f"{name}.ini")
            cfg = _write_ini(ini)
            cfg.name = name
            if "GRAD_CLIP" in extra:
                cfg.generator.max_norm = 0.5
            plain_text = cfg.asINI()
            assert "SPECTRAL_LOSS" not in plain_text  # today's text
            with open(ini, "w") as f:
                f.write(plain_text + extra)
            before = calls["n"]
            runmod.main(["--train", "--test", "--cfg", ini])
            run_dir = os.path.join(str(tmp_path), "runs", name)
            with open(os.path.join(run_dir, f"{name}.train")) as f:
                log = f.read()
            with open(os.path.join(run_dir, "config.ini")) as f:
                snapshot = f.read()
            values = [float(v) for v in re.findall(r"\bspectral: (\S+)", log)]
            if want_calls:
                assert calls["n"] > before and snapshot.endswith(section)
                assert len(values) >= 6 and all(math.isfinite(v) for v in values) and max(values) > 0, values
            else:
                assert calls["n"] == before and not values and "SPECTRAL_LOSS" not in snapshot
            assert os.path.isfile(os.path.join(run_dir, "G_6.pth"))
    finally:
        _reset_section(Config)
