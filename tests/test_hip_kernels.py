"""Parity of the individual HIP kernels (through the C-ABI) against the golden
fixtures produced by the reference and against fp64 CPU restatements.

Tolerances (rel-L2 over the whole tensor):
  fp32 path : 1e-5 outputs / input grads, 2e-5 filter grads (float atomics)
  bf16 path : 1e-2 against the fp32 goldens (operands rounded to 8 bits);
              4e-3 against an fp32 CPU conv of the *same* bf16-rounded operands.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import reload_wsr_env, rel_l2
from cases import CONV_CASES
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

T = torch.from_numpy
DEV = "cuda:0"
TOL = {torch.float32: (1e-5, 2e-5), torch.bfloat16: (1e-2, 1e-2)}


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def to_ndhwc(x, ctot, off, dt):
    """logical (B,C,X,Y,Z) cpu -> NDHWC window of a (B,X,Y,Z,ctot) device buffer (rest = NaN canary... zeros for pads)."""
    B, C_, X, Y, Z = x.shape
    buf = torch.zeros((B, X, Y, Z, ctot), dtype=dt, device=DEV)
    buf[..., off:off + C_] = x.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    return buf


def from_ndhwc(buf, off, C_):
    return buf[..., off:off + C_].permute(0, 4, 1, 2, 3).float().cpu()


def _slabs(xo, macs):
    """x-plane ranges of the output the float64 reference covers: all planes, or - where a full reference would take
    seconds on the host - the first four and the last four (the first and the ragged last x tile)"""
    return [None] if macs < 4e9 or xo <= 8 else [(0, 4), (xo - 4, xo)]


def _xs(t, xs):
    return t if xs is None else t[:, :, xs[0]:xs[1]]


def packed_master(w):
    """master weights stay in nn.Conv3d's logical layout; just move to the device."""
    return w.contiguous().to(DEV)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_fwd_dgrad_wgrad(golden, hip, dt, case):
    o = ops()
    name, cin, cout, k, s, p, bias, act, xyz, B = case
    g = golden("conv_cases.npz")
    x, w, y_ref, gy, dx_ref, dw_ref = (T(g[f"{name}.{n}"]) for n in ("x", "w", "y", "gy", "dx", "dw"))
    b = T(g[f"{name}.b"]).to(DEV) if bias else None
    tol_out, tol_w = TOL[dt]
    e = o.piece_elems(dt)
    cin_p, cout_p = o.pad_channels(cin, dt), o.pad_channels(cout, dt)
    in_off, out_off = e, 2 * e  # exercise channel windows
    in_ctot, out_ctot = cin_p + 2 * e, cout_p + 3 * e
    geom = o.ConvGeom(cin_p, cout, k, s, p)
    xb = to_ndhwc(x, in_ctot, in_off, dt)
    wm = packed_master(w)
    wp = o.pack_filter(wm, dt, kpad=cin_p)
    d = o.make_desc(geom, dt, B, xyz, in_ctot, in_off, out_ctot, out_off)
    yb = torch.full((B, d.Xo, d.Yo, d.Zo, out_ctot), 7.0, dtype=dt, device=DEV)
    o.conv_fwd(d, xb, wp, yb, bias=b, act=act, slope=0.2)
    torch.cuda.synchronize()
    y = from_ndhwc(yb, out_off, cout)
    assert rel_l2(y, y_ref) < tol_out
    # nothing outside the window was touched
    assert float((yb[..., :out_off].float() - 7.0).abs().max()) == 0.0
    assert float((yb[..., out_off + cout:].float() - 7.0).abs().max()) == 0.0
    if dt == torch.bfloat16:  # tight check against the same rounded operands
        xr, wr = x.bfloat16().float(), w.bfloat16().float()
        y2 = F.conv3d(xr, wr, b.cpu() if bias else None, s, p)
        y2 = F.leaky_relu(y2, 0.2) if act else y2
        assert rel_l2(y, y2) < 4e-3

    # ---- backward: g = gy * lrelu'(y) in place, then dgrad / wgrad ---------------
    gb = to_ndhwc(gy, out_ctot, out_off, dt)
    if act:
        # bf16: take the mask from the golden y - rounding flips the sign of ~0.2 % of
        # the near-zero activations, which is a 5x change of those gradient elements
        ymask = yb if dt == torch.float32 else to_ndhwc(y_ref, out_ctot, out_off, dt)
        o.lrelu_bwd_(gb, out_off, ymask, out_off, cout_p, 0.2)
    wt = o.pack_filter(wm, dt, transpose=True, kpad=cout_p)
    dgeom = o.ConvGeom(cin, cout_p, k, s, p)
    dd = o.make_desc(dgeom, dt, B, xyz, in_ctot, in_off, out_ctot, out_off)
    dxb = torch.full((B,) + tuple(xyz) + (in_ctot,), 3.0, dtype=dt, device=DEV)
    o.conv_dgrad(dd, gb, wt, dxb)
    dx = from_ndhwc(dxb, in_off, cin)
    assert rel_l2(dx, dx_ref) < tol_out
    assert float((dxb[..., :in_off].float() - 3.0).abs().max()) == 0.0
    # accumulate mode: dx += result
    o.conv_dgrad(dd, gb, wt, dxb, accumulate=True)
    assert rel_l2(from_ndhwc(dxb, in_off, cin), 2 * dx_ref) < tol_out
    # planar fp32 gradient (used for network inputs)
    dxp = torch.zeros((B, cin) + tuple(xyz), dtype=torch.float32, device=DEV)
    dd2 = o.make_desc(o.ConvGeom(cin, cout_p, k, s, p), dt, B, xyz, cin, 0, out_ctot, out_off)
    o.conv_dgrad(dd2, gb, wt, dxp, dx_planar=True)
    assert rel_l2(dxp.cpu(), dx_ref) < tol_out

    dwp = torch.zeros((cout, geom.taps, cin_p), dtype=torch.float32, device=DEV)
    o.conv_wgrad(d, xb, gb, dwp)
    dw = torch.ones((cout, cin) + tuple(k), dtype=torch.float32, device=DEV)
    o.unpack_wgrad(dwp, dw, scale=0.5)
    assert rel_l2((dw.cpu() - 1.0) * 2.0, dw_ref) < tol_w
    if bias:
        db = gb[..., out_off:out_off + cout].float().sum(dim=(0, 1, 2, 3)).cpu()
        assert rel_l2(db, T(g[f"{name}.db"])) < tol_out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_upconv_fused_upsample(golden, hip, dt):
    """nearest x(2,2,1) folded into the conv gather; backward = dgrad at fine res + 2x2 fold."""
    o = ops()
    g = golden("blocks.npz")
    x, w, y_ref, gy, dx_ref, dw_ref = (T(g[f"up.{n}"]) for n in ("x", "w", "y", "gy", "dx", "dw"))
    tol_out, tol_w = TOL[dt]
    B, C_, X, Y, Z = x.shape
    geom = o.ConvGeom(8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1), upsample=True)
    xb = to_ndhwc(x, 8, 0, dt)
    wm = packed_master(w)
    d = o.make_desc(geom, dt, B, (X, Y, Z), 8, 0, 8, 0)
    yb = torch.empty((B, 2 * X, 2 * Y, Z, 8), dtype=dt, device=DEV)
    o.conv_fwd(d, xb, o.pack_filter(wm, dt), yb, act=True, slope=0.2)
    assert rel_l2(from_ndhwc(yb, 0, 8), y_ref) < tol_out
    gb = to_ndhwc(gy, 8, 0, dt)
    o.lrelu_bwd_(gb, 0, yb if dt == torch.float32 else to_ndhwc(y_ref, 8, 0, dt), 0, 8, 0.2)
    fine = torch.empty((B, 2 * X, 2 * Y, Z, 8), dtype=dt, device=DEV)
    o.conv_dgrad(d, gb, o.pack_filter(wm, dt, transpose=True), fine)
    dxb = torch.empty((B, X, Y, Z, 8), dtype=dt, device=DEV)
    o.upsample2_bwd(fine, dxb)
    assert rel_l2(from_ndhwc(dxb, 0, 8), dx_ref) < (tol_out if dt == torch.float32 else 1.5e-2)
    dwp = torch.zeros((8, 27, 8), dtype=torch.float32, device=DEV)
    o.conv_wgrad(d, xb, gb, dwp)
    dw = torch.zeros((8, 8, 3, 3, 3), dtype=torch.float32, device=DEV)
    o.unpack_wgrad(dwp, dw)
    assert rel_l2(dw.cpu(), dw_ref) < tol_w


@pytest.mark.parametrize("case", [
    # (cin, cout, kernel, stride, pad, xyz, bias, act): the discriminator's deep layers at the benchmark's size
    (256, 256, (4, 4, 3), (2, 2, 2), (1, 1, 1), (8, 8, 64), False, False),   # features.4.1.0 -> 4x4x32
    (256, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1), (8, 8, 64), False, False),   # features.4.0.0
    (256, 256, (4, 4, 3), (2, 2, 1), (1, 1, 1), (16, 16, 64), True, True),   # features.3.1.0 -> 8x8x64 (+bias, act)
    (128, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), (6, 5, 7), True, True),
])
def test_split_reduction_matches_single_pass(hip, case):
    """Launches with few workgroups and long reductions split the reduction channels over more workgroups when the
    caller passes a workspace with the call (wsr_epilogue_t.ws / wsr_dgrad_opts_t.ws, ABI 6): same result as the single-pass launch up to the fp32
    summation order (both sides round the same sums to bf16 once: 2e-3), forward and input gradient, and as the fp32
    CPU conv of the same bf16-rounded operands (4e-3); two split launches are bit-identical."""
    o = ops()
    cin, cout, k, st, pad, xyz, has_bias, act = case
    dt = torch.bfloat16
    torch.manual_seed(3)
    B = 1
    x = torch.randn(B, cin, *xyz).to(dt).float()
    w = (torch.randn(cout, cin, *k) / math.sqrt(cin * k[0] * k[1] * k[2])).to(dt).float()
    bias = torch.randn(cout) * 0.1 if has_bias else None
    geom = o.ConvGeom(cin, cout, k, st, pad)
    d = o.make_desc(geom, dt, B, xyz, cin, 0, cout, 0)
    oxyz = (d.Xo, d.Yo, d.Zo)
    xb = to_ndhwc(x, cin, 0, dt)
    wf = o.pack_filter_frag(w.to(DEV))
    bd = bias.to(DEV) if has_bias else None
    ys = []
    for ws in (False, True, True):
        yb = torch.full((B,) + oxyz + (cout,), float("nan"), dtype=dt, device=DEV)
        assert o.conv_fwd_tile(d, xb, wf, yb, bias=bd, act=act, slope=0.2, use_ws=ws)
        ys.append(from_ndhwc(yb, 0, cout))
    y_ref = F.conv3d(x, w, bias, stride=st, padding=pad)
    if act:
        y_ref = F.leaky_relu(y_ref, 0.2)
    assert rel_l2(ys[0], y_ref) < 4e-3 and rel_l2(ys[1], y_ref) < 4e-3
    assert rel_l2(ys[1], ys[0]) < 2e-3
    assert torch.equal(ys[1], ys[2])
    if st == (1, 1, 1):  # input gradient on the tile kernel (stride 1)
        gy = torch.randn(B, cout, *oxyz).to(dt).float()
        gb = to_ndhwc(gy, cout, 0, dt)
        wft = o.pack_filter_frag(w.to(DEV), transpose=True)
        dxs = []
        for ws in (False, True):
            dxb = torch.full((B,) + xyz + (cin,), float("nan"), dtype=dt, device=DEV)
            assert o.conv_dgrad_tile(d, gb, wft, dxb, alpha=0.5, use_ws=ws)
            dxs.append(from_ndhwc(dxb, 0, cin))
        xr = x.clone().requires_grad_(True)
        (dx_ref,) = torch.autograd.grad(F.conv3d(xr, w, None, stride=st, padding=pad), xr, gy)
        assert rel_l2(dxs[0], 0.5 * dx_ref) < 4e-3 and rel_l2(dxs[1], 0.5 * dx_ref) < 4e-3


def test_split_reduction_is_reentrant_across_streams(hip):
    """ABI 6: the split-reduction workspace travels with the call (the library keeps no state between calls), so two
    split launches may be in flight on two streams at once - each with its own workspace - and give exactly what each
    gives alone.  (ABI 5 registered ONE process-wide workspace: concurrent launches would have mixed their partial
    sums.)  Many rounds, alternating issue order."""
    o = ops()
    dt = torch.bfloat16
    torch.manual_seed(11)
    cases = [(256, 256, (3, 3, 3), (8, 8, 16)), (512, 256, (3, 3, 3), (4, 4, 8))]
    jobs = []
    for cin, cout, k, xyz in cases:
        x = torch.randn(1, cin, *xyz).to(dt).float()
        w = (torch.randn(cout, cin, *k) / math.sqrt(cin * 27)).to(dt).float()
        d = o.make_desc(o.ConvGeom(cin, cout, k, (1, 1, 1), (1, 1, 1)), dt, 1, xyz, cin, 0, cout, 0)
        xb, wf = to_ndhwc(x, cin, 0, dt), o.pack_filter_frag(w.to(DEV))
        alone = torch.empty((1,) + xyz + (cout,), dtype=dt, device=DEV)
        assert o.conv_fwd_tile(d, xb, wf, alone)
        jobs.append((d, xb, wf, alone, xyz, cout))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ptrs = set()
    for rnd in range(12):
        outs = []
        order = (0, 1) if rnd % 2 == 0 else (1, 0)
        for i in order:
            d, xb, wf, alone, xyz, cout = jobs[i]
            with torch.cuda.stream(streams[i]):
                ptrs.add(o.tile_workspace()[0])
                y = torch.full((1,) + xyz + (cout,), float("nan"), dtype=dt, device=DEV)
                assert o.conv_fwd_tile(d, xb, wf, y)
                outs.append((i, y))
        torch.cuda.synchronize()
        for i, y in outs:
            assert torch.equal(y, jobs[i][3]), (rnd, i)
    assert len(ptrs) == 2  # one workspace per stream


def test_dgrad_accumulates_from_another_buffer(hip):
    """ABI 6 ``wsr_dgrad_opts_t.acc_src``: dx = alpha * conv^T(dy) + acc_src on the first n channels, everything else
    freshly written - the same numbers as accumulating in place on a copy of acc_src.  3x3x3 on the halo-tile kernel
    and the in-place-capable streaming 1x1x1 kernel (LFF input gradient, 128 -> 256 with the identity shortcut)."""
    o = ops()
    dt = torch.bfloat16
    torch.manual_seed(5)
    for (cin, cout, k, pad, xyz, n_acc) in [(64, 32, (3, 3, 3), (1, 1, 1), (8, 8, 16), 32),
                                            (256, 128, (1, 1, 1), (0, 0, 0), (8, 16, 16), 128)]:
        gy = torch.randn(1, cout, *xyz).to(dt).float()
        w = (torch.randn(cout, cin, *k) / math.sqrt(cout)).to(dt).float()
        d = o.make_desc(o.ConvGeom(cin, cout, k, (1, 1, 1), pad), dt, 1, xyz, cin, 0, cout, 0)
        gb = to_ndhwc(gy, cout, 0, dt)
        wft = o.pack_filter_frag(w.to(DEV), transpose=True)
        src = torch.randn((1,) + xyz + (cin,), device=DEV).to(dt)
        inplace = src.clone()
        assert o.conv_dgrad_tile(d, gb, wft, inplace, alpha=0.7, accumulate=n_acc)
        moved = torch.full_like(src, float("nan"))
        assert o.conv_dgrad_tile(d, gb, wft, moved, alpha=0.7, accumulate=n_acc, acc_src=src)
        assert torch.equal(moved, inplace)


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("case", [(32, 32, 2, (16, 16, 16)), (64, 64, 1, (8, 16, 16)), (128, 256, 2, (8, 8, 8)),
                                  (32, 64, 1, (4, 6, 5))])
def test_strided_input_gradient_in_parity_form(hip, case, batched):
    """Input gradient of the discriminator's down-sampling convs (4x4x3, stride (2,2,1|2), padding 1; reference
    torch_blocks.py:372-521) as 2x2xKZ' parity convs over dy on the tile kernels, each writing its own lattice of dx:
    against autograd of the fp32 CPU conv on the same bf16-rounded operands (4e-3: output rounding only - the parity
    filters are selections of the master taps, nothing is summed before the rounding)."""
    o = ops()
    cin, cout, sz, oxyz = case
    dt = torch.bfloat16
    torch.manual_seed(17)
    B = 2
    ixyz = (2 * oxyz[0], 2 * oxyz[1], sz * oxyz[2])
    w = (torch.randn(cout, cin, 4, 4, 3) / math.sqrt(cin * 48)).to(dt).float()
    gy = torch.randn(B, cout, *oxyz).to(dt).float()
    x = torch.zeros(B, cin, *ixyz, requires_grad=True)
    y = F.conv3d(x, w, None, stride=(2, 2, sz), padding=1)
    assert tuple(y.shape[2:]) == oxyz
    (dx_ref,) = torch.autograd.grad(y, x, gy)
    gb = to_ndhwc(gy, cout, 0, dt)
    dxg = kb.Guarded((B,) + ixyz + (cin,), dt, DEV, fill=float("nan"))
    dxb = dxg.t
    for zc in range(sz):
        kzp = 3 if sz == 1 else (1 if zc == 0 else 2)
        wp = torch.empty(4, cin, cout, 2, 2, kzp, device=DEV)
        o.strided_parity_filters(w.to(DEV), wp, sz, zc)
        n = o.frag_filter_elems(wp[0], False)
        frag = torch.empty(4 * n, dtype=dt, device=DEV)
        for ph in range(4):
            o.pack_filter_frag(wp[ph], out=frag[ph * n:(ph + 1) * n])
        pz = 1 if sz == 1 else 0
        if batched:
            d = o.make_desc(o.ConvGeom(cout, cin, (2, 2, kzp), (1, 1, 1), (1, 1, pz)), dt, B, oxyz, cout, 0, cin, 0,
                            lat=(0, 0, 4, sz, zc))
            assert o.conv_fwd_tile(d, gb, frag, dxb)
        else:
            for ph in range(4):
                a, b = ph >> 1, ph & 1
                d = o.make_desc(o.ConvGeom(cout, cin, (2, 2, kzp), (1, 1, 1), (1 - a, 1 - b, pz)), dt, B, oxyz, cout, 0,
                                cin, 0, lat=(a, b, 0, sz, zc))
                assert o.conv_fwd_tile(d, gb, frag[ph * n:(ph + 1) * n], dxb)
    dx = from_ndhwc(dxb, 0, cin)
    assert not torch.isnan(dx).any()  # every lattice was written
    assert rel_l2(dx, dx_ref) < 4e-3
    kb.assert_guards_intact(dxg, label=str(case))
    x64 = torch.zeros((B, cin) + ixyz, dtype=torch.float64, requires_grad=True)
    (r64,) = torch.autograd.grad(F.conv3d(x64, w.double(), None, (2, 2, sz), 1), x64, gy.double())
    xa = torch.zeros((B, cin) + ixyz, dtype=torch.float64, requires_grad=True)
    (A,) = torch.autograd.grad(F.conv3d(xa, w.double().abs(), None, (2, 2, sz), 1), xa, gy.double().abs())
    kb.assert_within(dx, r64, kb.bound(r64, A, 12 * cout, kb.RHO_BF16), f"strided dgrad[{case} {batched}]")


@pytest.mark.parametrize("B,N,K", [(1, 100, 131072), (2, 100, 20480), (5, 7, 8192)])
def test_linear_rows_matches_torch(hip, B, N, K):
    """``wsr_linear_rows`` (first classifier layer of the discriminator, Discriminator_3D.py:171-175) against
    ``F.linear`` in fp64 - fp32 accumulation over up to 131 072 terms: 1e-5 - forward and the three gradients."""
    o = ops()
    torch.manual_seed(21)
    x = torch.randn(B, K, device=DEV, requires_grad=True)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).requires_grad_(True)
    b = torch.randn(N, device=DEV, requires_grad=True)
    y = o.linear_rows(x, w, b)
    assert y is not None
    g = torch.randn(B, N, device=DEV)
    y.backward(g)
    xr, wr, br = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    yr = F.linear(xr, wr, br)
    yr.backward(g.double())
    assert rel_l2(y, yr.float()) < 1e-5
    assert rel_l2(x.grad, xr.grad.float()) < 1e-5 and rel_l2(w.grad, wr.grad.float()) < 1e-5
    assert rel_l2(b.grad, br.grad.float()) < 1e-5
    y2 = o.linear_rows(x, w, b)
    assert torch.equal(y, y2)  # bit-reproducible


def _subpixel_sets(a, i):
    """taps of the 3-wide filter that read un-sampled offset i of output parity a (wsr_subpixel_fold)"""
    return ([0], [1, 2])[i] if a == 0 else ([0, 1], [2])[i]


def test_subpixel_fold_and_adjoint(hip):
    """wsr_subpixel_fold against its definition; wsr_subpixel_unfold is its adjoint (and exact on fold outputs)."""
    o = ops()
    torch.manual_seed(5)
    w = torch.randn(6, 5, 3, 3, 3)
    ref = torch.zeros(4, 6, 5, 2, 2, 3)
    for a in range(2):
        for b in range(2):
            for i in range(2):
                for j in range(2):
                    for kx in _subpixel_sets(a, i):
                        for ky in _subpixel_sets(b, j):
                            ref[2 * a + b, :, :, i, j] += w[:, :, kx, ky]
    wp = torch.empty(4, 6, 5, 2, 2, 3, device=DEV)
    o.subpixel_fold(w.to(DEV), wp)
    assert rel_l2(wp.cpu(), ref) < 1e-6
    g = torch.randn(4, 6, 5, 2, 2, 3)
    dw = torch.empty(6, 5, 3, 3, 3, device=DEV)
    o.subpixel_unfold(g.to(DEV), dw)
    lhs, rhs = float((ref * g).sum()), float((w * dw.cpu()).sum())
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs)


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("shape", [(2, 32, 48, 8, 16, 16), (1, 16, 16, 5, 7, 10), (1, 128, 128, 8, 8, 32)])
def test_subpixel_upconv_forward_and_dgrad(hip, shape, batched):
    """Sub-pixel form of nearest x(2,2,1) + 3x3x3 conv (+bias, LeakyReLU) on the tile kernels: four 2x2x3 parity
    convs on the un-sampled input (reference torch_blocks.py:345-347).  Against the fp32 CPU conv of the up-sampled
    bf16-rounded input with the master filter (1e-2: the parity filters are bf16 roundings of tap SUMS) and against
    the same parity convs evaluated in fp32 on the CPU with the same rounded filters (4e-3: output rounding only);
    the input gradient (four accumulating launches on the output-gradient lattices) against autograd."""
    o = ops()
    B, cin, cout, X, Y, Z = shape
    dt = torch.bfloat16
    torch.manual_seed(11)
    x = torch.randn(B, cin, X, Y, Z).to(dt).float()
    w = torch.randn(cout, cin, 3, 3, 3) / math.sqrt(27 * cin)
    bias = torch.randn(cout) * 0.1
    xb = to_ndhwc(x, cin, 0, dt)
    wp = torch.empty(4, cout, cin, 2, 2, 3, device=DEV)
    o.subpixel_fold(w.to(DEV), wp)
    n = o.frag_filter_elems(wp[0], False)
    frag = torch.empty(4 * n, dtype=dt, device=DEV)
    for ph in range(4):
        o.pack_filter_frag(wp[ph], out=frag[ph * n:(ph + 1) * n])
    ctot = cout + 8  # the last up-conv writes a window of the wider concat buffer
    yg = kb.Guarded((B, 2 * X, 2 * Y, Z, ctot), dt, DEV, window=(0, cout), outside=float("nan"), fill=float("nan"))
    yb = yg.t
    bd = bias.to(DEV)
    if batched:
        d = o.make_desc(o.ConvGeom(cin, cout, (2, 2, 3), (1, 1, 1), (1, 1, 1)), dt, B, (X, Y, Z), cin, 0, ctot, 0,
                        lat=(0, 0, 4))
        assert o.conv_fwd_tile(d, xb, frag, yb, bias=bd, act=True, slope=0.2)
    else:
        for ph in range(4):
            a, b = ph >> 1, ph & 1
            d = o.make_desc(o.ConvGeom(cin, cout, (2, 2, 3), (1, 1, 1), (1 - a, 1 - b, 1)), dt, B, (X, Y, Z), cin, 0,
                            ctot, 0, lat=(a, b, 0))
            assert o.conv_fwd_tile(d, xb, frag[ph * n:(ph + 1) * n], yb, bias=bd, act=True, slope=0.2)
    y = from_ndhwc(yb, 0, cout)
    assert torch.isnan(yb[..., cout:].float()).all()  # nothing outside the window was written
    kb.assert_guards_intact(yg, label=str(shape))
    xr = x.clone().requires_grad_(True)
    up = F.interpolate(xr, scale_factor=(2, 2, 1), mode="nearest")
    y_ref = F.leaky_relu(F.conv3d(up, w, bias, padding=1), 0.2)
    assert rel_l2(y, y_ref.detach()) < 1e-2
    wpr = wp.cpu().to(dt).float()
    y_par = torch.empty_like(y_ref)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        xp = F.pad(x, (1, 1, 1 - b, b, 1 - a, a))
        y_par[:, :, a::2, b::2] = F.leaky_relu(F.conv3d(xp, wpr[ph], bias), 0.2)
    assert rel_l2(y, y_par.detach()) < 4e-3
    r64 = torch.empty(y_ref.shape, dtype=torch.float64)
    A = torch.empty_like(r64)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        xp = F.pad(x, (1, 1, 1 - b, b, 1 - a, a))
        r64[:, :, a::2, b::2], A[:, :, a::2, b::2] = kb.ref_fwd(xp, wpr[ph], (0, 0, 0), bias=bias, act=True)
    kb.assert_within(y, r64, kb.bound(r64, A, 12 * cin, kb.RHO_BF16), f"subpixel fwd[{shape} {batched}]")
    # input gradient
    gy = torch.randn_like(y_ref).to(dt).float()
    (dx_ref,) = torch.autograd.grad(F.conv3d(up, w, None, padding=1), xr, gy)
    gb = to_ndhwc(gy, ctot, 0, dt)
    dxg = kb.Guarded((B, X, Y, Z, cin), dt, DEV, fill=float("nan"))
    dxb = dxg.t
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        d = o.make_desc(o.ConvGeom(cin, cout, (2, 2, 3), (1, 1, 1), (1 - a, 1 - b, 1)), dt, B, (X, Y, Z), cin, 0,
                        ctot, 0, lat=(a, b, 0))
        assert o.conv_dgrad_tile(d, gb, o.pack_filter_frag(wp[ph].contiguous(), transpose=True), dxb, accumulate=ph > 0)
    got = from_ndhwc(dxb, 0, cin)
    assert rel_l2(got, dx_ref) < 1.5e-2
    kb.assert_guards_intact(dxg, label=f"subpixel dgrad {shape}")
    # float64 of the four parity launches with the rounded parity filters; every launch stores its running sum in
    # bf16 and the next one reads it back: rho is paid on each of the four stored partial sums
    r64 = torch.zeros((B, cin, X, Y, Z), dtype=torch.float64)
    A = torch.zeros_like(r64)
    mag = torch.zeros_like(r64)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        wv, gv = wpr[ph].double(), gy[:, :, a::2, b::2].double()
        for total, wt, gt in ((r64, wv, gv), (A, wv.abs(), gv.abs())):
            xv = torch.zeros((B, cin, X, Y, Z), dtype=torch.float64, requires_grad=True)
            (dph,) = torch.autograd.grad(F.conv3d(F.pad(xv, (1, 1, 1 - b, b, 1 - a, a)), wt), xv, gt)
            total += dph
        mag += r64.abs()  # the running sum this launch stores
    kb.assert_within(got, r64, kb.bound(r64, A, 4 * 12 * cout + 4, kb.RHO_BF16, rho_mag=mag),
                     f"subpixel dgrad[{shape}]")


@pytest.mark.parametrize("shape", [(2, 32, 48, 8, 16, 16), (1, 128, 128, 8, 8, 32), (1, 64, 64, 5, 6, 10)])
def test_subpixel_upconv_filter_gradient(hip, shape):
    """Filter gradient of nearest x(2,2,1) + 3x3x3 conv in parity form: four 2x2x3 gradients, each over the un-sampled
    input and ITS lattice of the output gradient (deterministic split copies + ordered reduce), folded back by
    wsr_subpixel_unfold - against autograd of the fp32 CPU conv on the same bf16-rounded operands (1e-3: fp32
    accumulation, only the summation order differs)."""
    o = ops()
    B, cin, cout, X, Y, Z = shape
    dt = torch.bfloat16
    torch.manual_seed(13)
    x = torch.randn(B, cin, X, Y, Z).to(dt).float()
    gy = torch.randn(B, cout, 2 * X, 2 * Y, Z).to(dt).float()
    w = torch.zeros(cout, cin, 3, 3, 3, requires_grad=True)
    up = F.interpolate(x, scale_factor=(2, 2, 1), mode="nearest")
    (dw_ref,) = torch.autograd.grad(F.conv3d(up, w, None, padding=1), w, gy)
    xb = to_ndhwc(x, cin, 0, dt)
    gb = to_ndhwc(gy, cout + 16, 0, dt)  # (the last up-conv's output gradient is a window of the concat buffer)
    dwp = torch.empty(4, cout, cin, 2, 2, 3, device=DEV)
    jobs = []
    keep = []
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        d = o.make_desc(o.ConvGeom(cin, cout, (2, 2, 3), (1, 1, 1), (1 - a, 1 - b, 1)), dt, B, (X, Y, Z), cin, 0,
                        cout + 16, 0, lat=(a, b, 0))
        n = o.conv_wgrad_nparts(d)
        pg = kb.Guarded((n, cout, 12, cin), torch.float32, DEV)
        parts = pg.t
        o.conv_wgrad_parts(d, xb, gb, parts, n)
        jobs.append((parts[0], dwp[ph], 1.0, n, parts[0].numel()))
        keep.append(pg)
    o.unpack_wgrad_reduce_multi(o.unpack_job_table(jobs))
    dwg = kb.Guarded((cout, cin, 3, 3, 3), torch.float32, DEV)
    dw = dwg.t
    o.subpixel_unfold(dwp, dw)
    assert rel_l2(dw.cpu(), dw_ref) < 1e-3
    kb.assert_guards_intact(dwg, *keep, label=str(shape))
    r64, A = kb.ref_wgrad(x, gy, (3, 3, 3), (1, 1, 1), ups=True)
    K = 4 * B * X * Y * Z + 4 * max(p.shape[0] for p in keep) + 4
    kb.assert_within(dw.cpu(), r64, kb.bound(r64, A, K, 0.0), f"subpixel wgrad[{shape}]", kind="filter")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_epilogue_residual_dropout_planar(hip, dt):
    """bias + LReLU + channel scale + alpha*v + beta*res, NDHWC and planar outputs."""
    o = ops()
    gen = torch.Generator().manual_seed(5)
    B, cin, cout, xyz = 2, 16, 24, (5, 4, 6)
    x = torch.randn((B, cin) + xyz, generator=gen)
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen) * 0.1
    b = torch.randn(cout, generator=gen)
    res = torch.randn((B, cout) + xyz, generator=gen)
    cs = torch.rand((B, cout), generator=gen)
    if dt == torch.bfloat16:
        x, w, res = x.bfloat16().float(), w.bfloat16().float(), res.bfloat16().float()
    ref = F.leaky_relu(F.conv3d(x, w, b, 1, 1), 0.2) * cs.view(B, cout, 1, 1, 1) * 0.2 + 0.5 * res
    geom = o.ConvGeom(cin, cout, (3, 3, 3))
    d = o.make_desc(geom, dt, B, xyz, cin, 0, cout, 0)
    xb, rb = to_ndhwc(x, cin, 0, dt), to_ndhwc(res, cout, 0, dt)
    yb = torch.empty((B,) + xyz + (cout,), dtype=dt, device=DEV)
    wp = o.pack_filter(packed_master(w), dt)
    o.conv_fwd(d, xb, wp, yb, bias=b.to(DEV), chan_scale=cs.to(DEV).contiguous(), res=rb, alpha=0.2, beta=0.5,
               act=True, slope=0.2)
    assert rel_l2(from_ndhwc(yb, 0, cout), ref) < (1e-5 if dt == torch.float32 else 6e-3)
    yp = torch.empty((B, cout) + xyz, dtype=torch.float32, device=DEV)
    o.conv_fwd(d, xb, wp, yp, bias=b.to(DEV), act=False, out_planar=True)
    assert rel_l2(yp.cpu(), F.conv3d(x, w, b, 1, 1)) < (1e-5 if dt == torch.float32 else 4e-3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_layout_and_window_helpers(hip, dt):
    o = ops()
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((2, 3, 4, 5, 6), generator=gen)
    buf = torch.full((2, 4, 5, 6, 16), 9.0, dtype=dt, device=DEV)
    o.planar_to_ndhwc(x.to(DEV), buf, d_off=4, c_fill=8)
    got = buf[..., 4:7].permute(0, 4, 1, 2, 3).float().cpu()
    assert rel_l2(got, x) < (1e-7 if dt == torch.float32 else 4e-3)
    assert float(buf[..., 7:12].float().abs().max()) == 0.0 and float((buf[..., :4].float() - 9).abs().max()) == 0.0
    back = o.ndhwc_to_planar(buf, 3, 4).cpu()
    assert rel_l2(back, got) == 0.0
    # axpby on windows
    a = torch.randn((2, 4, 5, 6, 16), generator=gen).to(DEV).to(dt)
    bsrc = torch.randn((2, 4, 5, 6, 8), generator=gen).to(DEV).to(dt)
    exp = a.float().clone()
    exp[..., 8:16] = 0.5 * bsrc.float() + 2.0 * exp[..., 8:16]
    o.chan_axpby(a, 8, bsrc, 0, 8, alpha=0.5, beta=2.0)
    assert rel_l2(a.float().cpu(), exp.cpu()) < (1e-6 if dt == torch.float32 else 4e-3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C_", [4, 32, 256])
def test_batchnorm_kernels(hip, dt, C_):
    """bn_stats / apply / backward vs torch's CPU batch_norm autograd (training mode)."""
    o = ops()
    gen = torch.Generator().manual_seed(C_)
    shape = (2, 6, 5, 7, C_)
    x = (torch.randn(shape, generator=gen) * 1.5 + 0.3)
    gamma = 1 + 0.1 * torch.randn(C_, generator=gen)
    beta = 0.1 * torch.randn(C_, generator=gen)
    gy = torch.randn(shape, generator=gen)
    if dt == torch.bfloat16:
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
    xl = x.permute(0, 4, 1, 2, 3).double().requires_grad_(True)
    gl, bl = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yl = F.leaky_relu(F.batch_norm(xl, None, None, gl, bl, True, 0.1, 1e-5), 0.2)
    (yl * gy.permute(0, 4, 1, 2, 3).double()).sum().backward()
    n = x.numel() // C_
    xb = x.to(DEV).to(dt)
    sums = torch.full((2 * C_,), float("nan"), device=DEV)  # overwritten, not accumulated into
    o.bn_stats(xb, sums)
    mean = sums[:C_] / n
    s2 = torch.full((2 * C_,), float("nan"), device=DEV)
    o.bn_stats(xb, s2, shift=mean)
    var = s2[C_:] / n - (s2[:C_] / n) ** 2
    assert rel_l2(mean.cpu(), xl.detach().mean(dim=(0, 2, 3, 4)).float()) < 1e-4
    invstd = torch.rsqrt(var + 1e-5)
    yb = torch.empty_like(xb)
    g_d, b_d = gamma.to(DEV), beta.to(DEV)
    o.bn_apply_lrelu(xb, yb, mean, invstd, g_d, b_d, True, 0.2)
    tol = 2e-5 if dt == torch.float32 else 6e-3
    assert rel_l2(yb.float().cpu(), yl.detach().permute(0, 2, 3, 4, 1).float()) < tol
    gb = gy.to(DEV).to(dt)
    s2 = torch.full((2 * C_,), float("nan"), device=DEV)
    o.bn_bwd_reduce(gb, yb, xb, mean, invstd, True, 0.2, s2)
    assert rel_l2(s2[:C_].cpu(), bl.grad.float()) < (1e-4 if dt == torch.float32 else 1e-2)
    assert rel_l2(s2[C_:].cpu(), gl.grad.float()) < (1e-4 if dt == torch.float32 else 1e-2)
    dxb = torch.empty_like(xb)
    o.bn_bwd_apply(gb, xb, dxb, mean, invstd, g_d, s2, 1.0 / n)
    assert rel_l2(dxb.float().cpu(), xl.grad.permute(0, 2, 3, 4, 1).float()) < (1e-4 if dt == torch.float32 else 1.5e-2)
    # eval mode, no parameter gradients (D inside a generator iteration): the LeakyReLU derivative of the layer's output
    # rides on the BatchNorm pass (ABI 6) - equal to lrelu_bwd followed by the plain eval-mode pass
    g0 = gy.to(DEV).to(dt)
    want = g0.clone()
    o.lrelu_bwd_(want, 0, yb, 0, C_, 0.2)
    ref = torch.empty_like(xb)
    assert o.bn_bwd_apply(want, xb, ref, mean, invstd, g_d, None, 0.0)
    got = torch.full_like(xb, float("nan"))
    assert o.bn_bwd_apply(g0, xb, got, mean, invstd, g_d, None, 0.0, act_y=yb, slope=0.2)
    assert rel_l2(got.float().cpu(), ref.float().cpu()) < (6e-3 if dt == torch.bfloat16 else 1e-6)  # (one rounding instead of two)


def test_adam_matches_torch(hip):
    o = ops()
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(10007, generator=gen)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=8e-5, betas=(0.9, 0.999), weight_decay=0.01)
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 6):
        gr = torch.randn(10007, generator=gen)
        ref.grad = gr.clone()
        opt.step()
        o.adam_step(p, gr.to(DEV), m, v, 8e-5, 0.9, 0.999, 1e-8, 0.01, step)
    assert rel_l2(p.cpu(), ref.detach()) < 1e-6
    assert float((p.cpu() - p0).abs().max()) > 1e-5


def test_big_shapes_properties(hip):
    """Full-size layer shapes: linearity of the conv in x and agreement of the
    bf16 and fp32 paths (no CPU reference at these sizes)."""
    o = ops()
    gen = torch.Generator(device=DEV).manual_seed(3)
    B, xyz, cin, cout = 1, (32, 32, 16), 224, 32
    geom = o.ConvGeom(cin, cout, (3, 3, 3))
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen, device=DEV) * 0.02
    x1 = torch.randn((B,) + xyz + (256,), generator=gen, device=DEV)
    x2 = torch.randn((B,) + xyz + (256,), generator=gen, device=DEV)
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        d = o.make_desc(geom, dt, B, xyz, 256, 0, 256, 224)
        wp = o.pack_filter(w, dt)
        ys = []
        for xin in (x1, x2, x1 + x2):
            buf = xin.to(dt).clone()
            o.conv_fwd(d, buf, wp, buf, act=False)  # writes channels 224..255 of the same dense buffer
            ys.append(buf[..., 224:].float())
        outs[dt] = ys
    f = outs[torch.float32]
    assert rel_l2(f[0] + f[1], f[2]) < 1e-5
    assert rel_l2(outs[torch.bfloat16][0], f[0]) < 1e-2


def _cpu_wgrad(x, gy, k, p):
    """fp32 CPU filter gradient of a stride-1 conv: x (B,Cin,X,Y,Z), gy (B,Cout,X,Y,Z)."""
    w = torch.zeros((gy.shape[1], x.shape[1]) + tuple(k), requires_grad=True)
    F.conv3d(x, w, None, 1, p).backward(gy)
    return w.grad


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", [
    ("hr0_like", 48, 48, (5, 5, 5), (9, 10, 10), 1, False),   # TN=3 config, ragged tiles, nz = 10 (one z tile)
    ("hr0_z17", 16, 96, (5, 5, 5), (8, 8, 17), 1, False),      # z tiled by 8 with a ragged last tile
    ("hr1_like", 144, 3, (5, 5, 5), (8, 9, 6), 2, False),      # 3 real output channels in an 8-wide window
    ("k3_128", 40, 128, (3, 3, 3), (6, 9, 13), 1, False),      # TN=4 config, two n-chunks, ragged c-chunk
    ("k3_gc", 64, 32, (3, 3, 3), (5, 8, 9), 2, False),         # TN=2 config
    ("k3_up", 16, 64, (3, 3, 3), (4, 5, 6), 1, True),          # nearest x(2,2,1) folded into the x tile load
    ("lff_1x1", 256, 128, (1, 1, 1), (5, 6, 19), 1, False),    # 1x1x1: <8,1,8>, two c-chunks of 128 channels
    # the geometry every launch of the benchmarked 128-level workloads takes: z extent a multiple of 16 ->
    # 16-level tiles, the Z16 voxel<->k mapping (second transposing read at a constant offset), several z tiles
    ("hr0_z32", 144, 144, (5, 5, 5), (8, 12, 32), 1, False),   # <3,16,1,Z16>: 4x4x16 tiles, 2 z tiles
    ("k3_z16", 128, 128, (3, 3, 3), (8, 8, 16), 2, False),     # <4,7,2,Z16>: 4x8x16 tiles
    ("k3_up_z16", 32, 64, (3, 3, 3), (4, 4, 16), 1, True),     # Z16 with the up-sampled x tile
    ("lff_z48", 256, 128, (1, 1, 1), (4, 8, 48), 1, False),    # <8,1,8,Z16>, 3 z tiles
    ("hr1z_z16", 144, 15, (5, 5, 1), (8, 8, 16), 1, False),    # z-folded last conv: (5,5,1) taps, 15 outputs
    # the same gradient with the operands' roles exchanged (engine.SWAP_THIN_WGRAD): 16 -> 144, <3,4,1>: one c-tile,
    # three n-chunks of 48, flat 8x8x4 tiles; and the instantiation on 3x3x3 taps with a ragged volume
    ("hr1z_T", 16, 144, (5, 5, 1), (16, 8, 16), 1, False),
    ("thin_T_k3", 8, 48, (3, 3, 3), (5, 9, 10), 2, False),
    # one c-tile, few output channels: <1,4,1> (terrain 16 -> 16), <2,4,1> (discriminator 3 -> 32, channels padded to 8)
    ("terrain1_like", 16, 16, (3, 3, 3), (8, 8, 16), 1, False),
    ("d0_like", 8, 32, (3, 3, 3), (6, 10, 16), 2, False),
    ("d0_ragged", 8, 24, (3, 3, 3), (5, 7, 9), 1, False),
])
def test_wgrad_tile_kernel_bf16(hip, name, cin, cout, k, xyz, B, ups):
    """LDS-tile filter-gradient kernel (bf16) vs an fp32 CPU wgrad of the same rounded operands."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(len(name) + cin)
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    oxyz = (xyz[0] * 2, xyz[1] * 2, xyz[2]) if ups else xyz
    gy = torch.randn((B, cout) + tuple(oxyz), generator=gen).bfloat16().float()
    p = tuple(kk // 2 for kk in k)
    cout_p = o.pad_channels(cout, dt)
    geom = o.ConvGeom(cin, cout, k, (1, 1, 1), p, upsample=ups)
    xb = to_ndhwc(x, cin + 16, 8, dt)
    gb = to_ndhwc(gy, cout_p + 8, 8, dt)
    d = o.make_desc(geom, dt, B, xyz, cin + 16, 8, cout_p + 8, 8)
    dwg = kb.Guarded((cout, geom.taps, cin), torch.float32, DEV, fill=0.0)
    dwp = dwg.t
    o.conv_wgrad(d, xb, gb, dwp)
    dw = torch.zeros((cout, cin) + tuple(k), dtype=torch.float32, device=DEV)
    o.unpack_wgrad(dwp, dw)
    xr = x
    if ups:
        xr = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ref = _cpu_wgrad(xr, gy, k, p)
    assert rel_l2(dw.cpu(), ref) < 2e-5, name  # fp32 accumulation of exact bf16 products
    kb.assert_guards_intact(dwg, label=name)
    r64, A = kb.ref_wgrad(x, gy, k, p, ups=ups)
    K = B * math.prod(oxyz) + o.conv_wgrad_nparts(d)
    kb.assert_within(dw.cpu(), r64, kb.bound(r64, A, K, 0.0), f"wgrad bf16 atomic[{name}]", kind="filter")


@pytest.mark.parametrize("nf,gc,B,xyz", [(16, 8, 2, (6, 7, 9)), (128, 32, 1, (8, 8, 32))],
                         ids=["small", "full_width_z32"])
def test_wgrad_dense_block_fused(hip, nf, gc, B, xyz):
    """One launch for the four growth convs of an RDB: conv i reads channels [0, nf + i*gc) of the
    dense buffer; block-triangular (n, c) structure (reference torch_blocks.py:256-267).  The second case is
    the shipped block width on 16-level tiles (the launch the benchmark issues 48 times per backward)."""
    o = ops()
    dt = torch.bfloat16
    nconv = 4
    gen = torch.Generator().manual_seed(77)
    dense = nf + nconv * gc
    x = torch.randn((B, dense) + xyz, generator=gen).bfloat16().float()
    g = torch.randn((B, dense) + xyz, generator=gen).bfloat16().float()
    xb = to_ndhwc(x, dense, 0, dt)
    gb = to_ndhwc(g, dense, 0, dt)
    cin_w = nf + (nconv - 1) * gc
    geom = o.ConvGeom(cin_w, nconv * gc, (3, 3, 3))
    d = o.make_desc(geom, dt, B, xyz, dense, 0, dense, nf)
    dwg = kb.Guarded((nconv * gc, 27, cin_w), torch.float32, DEV, fill=0.0)
    dwp = dwg.t
    o.conv_wgrad_tri(d, xb, gb, dwp, nf, gc)
    K = B * math.prod(xyz) + o.conv_wgrad_nparts(d, nf, gc)
    for i in range(nconv):
        ci = nf + i * gc
        dw = torch.zeros((gc, ci, 3, 3, 3), dtype=torch.float32, device=DEV)
        o.unpack_wgrad(dwp[i * gc:(i + 1) * gc], dw)
        ref = _cpu_wgrad(x[:, :ci], g[:, nf + i * gc:nf + (i + 1) * gc], (3, 3, 3), (1, 1, 1))
        assert rel_l2(dw.cpu(), ref) < 2e-5, i
        r64, A = kb.ref_wgrad(x[:, :ci], g[:, nf + i * gc:nf + (i + 1) * gc], (3, 3, 3), (1, 1, 1))
        kb.assert_within(dw.cpu(), r64, kb.bound(r64, A, K, 0.0), f"tri[{nf} {gc} conv {i}]", kind="filter")
    kb.assert_guards_intact(dwg, label="tri")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[4] == (1, 1, 1)], ids=lambda c: c[0])
def test_conv_tile_kernels_vs_golden(golden, hip, case, dt):
    """LDS halo-tile forward / input-gradient kernels (stride 1; bf16, and fp32 = the reference's own arithmetic, ABI 6)
    on the reference's conv fixtures: channel windows, bias, activation, accumulation, planar gradient."""
    o = ops()
    f32 = dt == torch.float32
    name, cin, cout, k, s, p, bias, act, xyz, B = case
    g = golden("conv_cases.npz")
    x, w, y_ref, gy, dx_ref = (T(g[f"{name}.{n}"]) for n in ("x", "w", "y", "gy", "dx"))
    b = T(g[f"{name}.b"]).to(DEV) if bias else None
    cin_p, cout_p = o.pad_channels(cin, dt), o.pad_channels(cout, dt)
    in_off, out_off = 8, 16
    in_ctot, out_ctot = cin_p + 16, cout_p + 24
    xb = to_ndhwc(x, in_ctot, in_off, dt)
    wm = packed_master(w)
    d = o.make_desc(o.ConvGeom(cin_p, cout, k, s, p), dt, B, xyz, in_ctot, in_off, out_ctot, out_off)
    yg = kb.Guarded((B, d.Xo, d.Yo, d.Zo, out_ctot), dt, DEV, window=(out_off, cout), outside=7.0, fill=7.0)
    yb = yg.t
    tol_ref, tol_same = (1e-5, 1e-5) if f32 else (1e-2, 4e-3)
    if f32 and k == (1, 1, 1):  # (1x1x1 in fp32 stays on the generic kernel)
        assert not o.conv_fwd_tile(d, xb, o.pack_filter_frag(wm, dtype=dt), yb, bias=b, act=act, slope=0.2)
        return
    assert o.conv_fwd_tile(d, xb, o.pack_filter_frag(wm, dtype=dt), yb, bias=b, act=act, slope=0.2)
    y = from_ndhwc(yb, out_off, cout)
    assert rel_l2(y, y_ref) < tol_ref
    assert float((yb[..., :out_off].float() - 7.0).abs().max()) == 0.0
    assert float((yb[..., out_off + cout:].float() - 7.0).abs().max()) == 0.0
    kb.assert_guards_intact(yg, label=name)
    # element-wise against float64 of the operands the kernel multiplies (bf16: the rounded fixtures)
    xo, wo = (x, w) if f32 else (x.bfloat16().float(), w.bfloat16().float())
    taps = k[0] * k[1] * k[2]
    r64, A = kb.ref_fwd(xo, wo, p, bias=b, act=act)
    kb.assert_within(y, r64, kb.bound(r64, A, taps * cin, kb.rho_for(dt)), f"tile fwd {dt_name(dt)}[golden {name}]")
    if not f32:
        y2 = F.conv3d(x.bfloat16().float(), w.bfloat16().float(), b.cpu() if bias else None, s, p)
        y2 = F.leaky_relu(y2, 0.2) if act else y2
        assert rel_l2(y, y2) < tol_same  # same rounded operands, fp32 accumulation, bf16 store
    # the generic implicit-GEMM kernel computes the same thing
    yb2 = torch.full_like(yb, 7.0)
    o.conv_fwd(d, xb, o.pack_filter(wm, dt, kpad=cin_p), yb2, bias=b, act=act, slope=0.2)
    assert rel_l2(yb.float(), yb2.float()) < tol_same

    gb = to_ndhwc(gy, out_ctot, out_off, dt)
    if act:
        o.lrelu_bwd_(gb, out_off, to_ndhwc(y_ref, out_ctot, out_off, dt), out_off, cout_p, 0.2)
    wft = o.pack_filter_frag(wm, transpose=True, dtype=dt)
    dd = o.make_desc(o.ConvGeom(cin, cout_p, k, s, p), dt, B, xyz, in_ctot, in_off, out_ctot, out_off)
    dxg = kb.Guarded((B,) + tuple(xyz) + (in_ctot,), dt, DEV, window=(in_off, cin), outside=3.0, fill=3.0)
    dxb = dxg.t
    assert o.conv_dgrad_tile(dd, gb, wft, dxb)
    assert rel_l2(from_ndhwc(dxb, in_off, cin), dx_ref) < tol_ref
    assert float((dxb[..., :in_off].float() - 3.0).abs().max()) == 0.0
    kb.assert_guards_intact(dxg, label=name)
    g_in = from_ndhwc(gb, out_off, cout)  # the (masked, stored) output gradient the kernel reads
    r64, A = kb.ref_dgrad(g_in, wo, p)
    kb.assert_within(from_ndhwc(dxb, in_off, cin), r64, kb.bound(r64, A, taps * cout, kb.rho_for(dt)),
                     f"tile dgrad {dt_name(dt)}[golden {name}]")
    assert o.conv_dgrad_tile(dd, gb, wft, dxb, accumulate=True)
    assert rel_l2(from_ndhwc(dxb, in_off, cin), 2 * dx_ref) < tol_ref
    kb.assert_guards_intact(dxg, label=f"{name} accumulate")
    # dx = stored(d) + d: one stored value |d| read back, then |2d| stored; fresh sums of A twice
    kb.assert_within(from_ndhwc(dxb, in_off, cin), 2 * r64,
                     kb.bound(2 * r64, 2 * A, taps * cout, kb.rho_for(dt), rho_mag=3 * r64.abs()),
                     f"tile dgrad {dt_name(dt)}[golden {name} accumulate]")
    dxpg = kb.Guarded((B, cin) + tuple(xyz), torch.float32, DEV, fill=0.0)
    dxp = dxpg.t
    dd2 = o.make_desc(o.ConvGeom(cin, cout_p, k, s, p), dt, B, xyz, cin, 0, out_ctot, out_off)
    assert o.conv_dgrad_tile(dd2, gb, wft, dxp, dx_planar=True)
    assert rel_l2(dxp.cpu(), dx_ref) < tol_ref
    kb.assert_guards_intact(dxpg, label=f"{name} planar")
    kb.assert_within(dxp.cpu(), r64, kb.bound(r64, A, taps * cout, 0.0), f"tile dgrad planar[golden {name} {dt_name(dt)}]")


# Which launch_ct<WM, WN, TM, TN, TPK, MASK, F32, WK, SIMPLE> serves the forward / the input gradient of each case below
# (asserted through hip_ops.last_tile_instantiation(); None: another kernel).  These volumes are small, so with nothing
# forced they take the 128-voxel tiles of conv_tile_small.hip; the SIMPLE forms step aside wherever the call's workspace
# might split the reduction (<= 128 workgroups and >= 4 chunks, conv_tile_impl.h launch_ct).
SHAPES_WITNESS = {
    "rdb_n32": ((2, 1, 4, 2, 2, 0, 0, 4, 0), (2, 2, 4, 2, 2, 0, 0, 2, 1)),
    "hr0_n144": ((2, 2, 4, 2, 2, 0, 0, 2, 0), (2, 2, 4, 2, 2, 0, 0, 2, 0)),
    "up_n128": ((2, 2, 4, 2, 2, 0, 0, 2, 0), (2, 2, 4, 2, 2, 0, 0, 2, 0)),
    "lff_1x1": (None, None),
    "dg_n224": ((2, 2, 4, 2, 2, 0, 0, 2, 1), (2, 1, 4, 2, 2, 0, 0, 4, 0)),
    "n64_c24": ((4, 1, 4, 4, 4, 0, 0, 1, 0), (2, 1, 4, 2, 2, 0, 0, 4, 0)),
    "n3_k5": ((2, 1, 4, 2, 2, 0, 0, 4, 0), (4, 2, 4, 5, 4, 0, 0, 1, 0)),
}


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", [
    ("rdb_n32", 160, 32, (3, 3, 3), (9, 10, 19), 1, False),    # <2,1,4,2> with four K-step shares; dgrad <2,2,4,2>, two
    ("hr0_n144", 144, 144, (5, 5, 5), (9, 7, 10), 1, False),   # <2,2,4,2>, two shares: TPK=2 with an odd tap count (125)
    ("up_n128", 128, 128, (3, 3, 3), (5, 6, 8), 1, True),      # nearest x(2,2,1) folded into the halo load, <2,2,4,2>
    ("lff_1x1", 256, 128, (1, 1, 1), (7, 9, 11), 2, False),    # 256 <-> 128: the streaming 1x1x1 kernel, not the tile one
    ("dg_n224", 32, 224, (3, 3, 3), (6, 9, 17), 1, False),     # <2,2,4,2>: 224 outputs as four 64-channel groups
    ("n64_c24", 24, 64, (3, 3, 3), (8, 5, 6), 2, False),       # TPK=4 (24 channels), N=64: <4,1,4,4,4>
    ("n3_k5", 144, 3, (5, 5, 5), (8, 8, 10), 1, False),        # N=3 (one 16-tile); dgrad <4,2,4,5> with TPK=4 (8 channels)
])
def test_conv_tile_shapes_vs_cpu(hip, name, cin, cout, k, xyz, B, ups):
    """Tile-kernel configurations at small volumes against an fp32 CPU conv of the same bf16-rounded operands,
    forward and input gradient (with residual epilogue on the forward pass).  (Every instantiation, the 512- and
    256-voxel ones included: test_conv_tile_matrix.py.)"""
    _check_tile_conv(name, cin, cout, k, xyz, B, ups, want=SHAPES_WITNESS[name])


SHAPES_FP32_WITNESS = {  # (as SHAPES_WITNESS: forward, input gradient)
    "rdb_n32": ((8, 1, 4, 2, 2, 0, 1, 1, 0), (4, 2, 4, 6, 2, 0, 1, 1, 0)),
    "hr0_n144": ((8, 1, 4, 9, 2, 0, 1, 1, 0), (8, 1, 4, 9, 2, 0, 1, 1, 0)),
    "up_n128": ((8, 1, 4, 8, 2, 0, 1, 1, 0), (8, 1, 4, 8, 2, 0, 1, 1, 0)),
    "pre_n128": ((8, 1, 4, 8, 2, 0, 1, 1, 0), (8, 1, 4, 8, 2, 0, 1, 1, 0)),
    "dg_n224": ((4, 2, 4, 8, 2, 0, 1, 1, 0), (8, 1, 4, 2, 2, 0, 1, 1, 0)),
    "n64_c20": ((4, 1, 4, 4, 4, 0, 1, 1, 0), (8, 1, 4, 2, 2, 0, 1, 1, 0)),
    "n15_k551": ((8, 1, 4, 1, 2, 0, 1, 1, 0), (8, 1, 4, 9, 2, 0, 1, 1, 0)),
    "t0_c4": ((8, 1, 4, 1, 4, 0, 1, 1, 0), (8, 1, 4, 1, 2, 0, 1, 1, 0)),
}


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", [
    ("rdb_n32", 160, 32, (3, 3, 3), (9, 10, 19), 1, False),    # <8,1,4,2,2,F32>: 20 chunks of 8 channels; dgrad <4,2,4,6>
    ("hr0_n144", 144, 144, (5, 5, 5), (9, 7, 10), 1, False),   # <8,1,4,9,2,F32>, odd tap count
    ("up_n128", 128, 128, (3, 3, 3), (5, 6, 8), 1, True),      # nearest x(2,2,1) folded into the halo load, <8,1,4,8>
    ("pre_n128", 128, 128, (3, 3, 3), (8, 16, 16), 1, False),  # production tile 4x8x16, <8,1,4,8,2,F32>
    ("dg_n224", 32, 224, (3, 3, 3), (6, 9, 17), 1, False),     # <4,2,4,8,2,F32>: two n-tile wave columns; dgrad <8,1,4,2>
    ("n64_c20", 20, 64, (3, 3, 3), (8, 5, 6), 2, False),       # TPK=4 (20 channels = 5 pieces), N=64: <4,1,4,4,4>
    ("n15_k551", 144, 15, (5, 5, 1), (8, 8, 10), 1, False),    # the z-folded last conv: one n-tile, flat tiles; dgrad <8,1,4,9>
    ("t0_c4", 4, 16, (3, 3, 3), (8, 8, 16), 1, False),         # 1 / 3 / 4-channel inputs padded to one piece: <8,1,4,1,4>
])
def test_conv_tile_shapes_fp32_vs_cpu(hip, name, cin, cout, k, xyz, B, ups):
    """the fp32 instantiations of the halo-tile kernel (ABI 6; the reference's own arithmetic, AMP is commented out in
    Generator_3D_Resnet_ESRGAN.py:65): exact fp32 products and sums - 2e-5 against the fp32 CPU conv."""
    _check_tile_conv(name, cin, cout, k, xyz, B, ups, dt=torch.float32, want=SHAPES_FP32_WITNESS[name])


THIN_WITNESS = {  # (forward, input gradient)
    "needle_x": ((8, 1, 3, 2, 2, 0, 0, 1, 1), (8, 1, 3, 2, 2, 0, 0, 1, 1)),
    "needle_y": ((8, 1, 3, 2, 2, 0, 0, 1, 1), (8, 1, 3, 2, 2, 0, 0, 1, 1)),
    "thin_slab": ((8, 1, 3, 8, 2, 0, 0, 1, 0), (8, 1, 3, 8, 2, 0, 0, 1, 0)),
    "k5_needle": ((8, 1, 4, 9, 2, 0, 0, 1, 0), (8, 1, 4, 9, 2, 0, 0, 1, 0)),
}


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", [
    # z extents that leave the x-y tile budget no power of two (512 / 10 = 51) on volumes no square tile suits: the picker
    # takes the split with the fewest tiles among candidates INSIDE the 8-bit coordinate fields of the tile tables, no wider
    # than the volume and with a halo at most 1.3 x the most nearly square tile's (conv_tile_impl.h pick_tile, round 6)
    ("needle_x", 32, 32, (3, 3, 3), (300, 3, 10), 1, False),    # long along x: a 51 x 1 tile would be the "fewest tiles"
    ("needle_y", 32, 32, (3, 3, 3), (2, 290, 10), 1, False),    # long along y, beyond 255 voxels
    ("thin_slab", 128, 128, (3, 3, 3), (70, 5, 10), 1, False),  # the 128-wide tile on a 5-voxel-wide slab
    ("k5_needle", 144, 144, (5, 5, 5), (40, 3, 10), 1, False),  # 5x5x5 halo on a 3-voxel-wide volume
])
def test_conv_tile_long_thin_volumes(hip, monkeypatch, name, cin, cout, k, xyz, B, ups):
    """the halo-tile kernels on long thin 10-level volumes (tile coordinates are packed in 8 bits per axis: a needle-shaped
    tile through such a volume must not wrap them), against the CPU conv; WSR_CT_NOSMALL keeps them off the 128-voxel
    tiles.  With so few tiles the 32- and 128-wide launches take the 384-voxel forms (dispatch_ct: one round of
    workgroups either way), the 144-wide one the 512-voxel tile."""
    monkeypatch.setenv("WSR_CT_NOSMALL", "1")
    reload_wsr_env()
    _check_tile_conv(name, cin, cout, k, xyz, B, ups, want=THIN_WITNESS[name])


PROD_CASES = [
    # z extents of several 16-level tiles, as in the benchmarked 128-level workloads; WSR_CT_NOSMALL keeps these small
    # volumes off the 128-voxel tiles.  A handful of tiles is one round of workgroups on 512- and on 384-voxel tiles alike,
    # so dispatch_ct moves the 32- and 128-wide launches to the 384-voxel forms (3 < 4), and the workspace the call carries
    # makes the SIMPLE forms step aside wherever the reduction has >= 4 chunks: the comments name what the witness shows
    ("hr0_prod", 144, 144, (5, 5, 5), (12, 16, 32), 1, False),   # <8,1,4,9>: one activation buffer, 9 chunks
    ("n128_prod", 128, 128, (3, 3, 3), (8, 16, 32), 1, False),   # <8,1,3,8>: 384-voxel tile, 128 outputs
    ("pre_prod", 128, 128, (3, 3, 3), (4, 8, 48), 2, False),     # same, batch 2, 3 z tiles
    ("up_prod", 128, 128, (3, 3, 3), (4, 8, 32), 1, True),       # up-sampling gather on the 512-voxel tile <8,1,4,8>
    ("grow_prod", 96, 32, (3, 3, 3), (8, 8, 32), 1, False),      # <8,1,3,2>: growth conv over 96 channels
    ("rdb_prod", 224, 32, (3, 3, 3), (8, 8, 16), 1, False),      # <8,1,3,2>: last growth conv (per-conv form); dgrad <4,2,4,7>
    ("dwin_prod", 32, 128, (3, 3, 3), (8, 8, 32), 1, False),     # input gradient of a growth window: 128 -> 32, <8,1,3,2>
    ("hr1z_prod", 144, 15, (5, 5, 1), (8, 16, 32), 1, False),    # z-folded last conv, <8,1,4,1>; dgrad <4,2,4,5>
    ("t1_prod", 16, 16, (3, 3, 3), (8, 16, 32), 1, False),       # terrain conv 16 -> 16; dgrad: the sliding-window kernel
]
PROD_WITNESS = {  # (forward, input gradient) with WSR_CT_NOSMALL and the call's workspace
    "hr0_prod": ((8, 1, 4, 9, 2, 0, 0, 1, 0), (8, 1, 4, 9, 2, 0, 0, 1, 0)),
    "n128_prod": ((8, 1, 3, 8, 2, 0, 0, 1, 0), (8, 1, 3, 8, 2, 0, 0, 1, 0)),
    "pre_prod": ((8, 1, 3, 8, 2, 0, 0, 1, 0), (8, 1, 3, 8, 2, 0, 0, 1, 0)),
    "up_prod": ((8, 1, 4, 8, 2, 0, 0, 1, 0), (8, 1, 3, 8, 2, 0, 0, 1, 0)),
    "grow_prod": ((8, 1, 3, 2, 2, 0, 0, 1, 0), (8, 1, 3, 8, 2, 0, 0, 1, 1)),
    "rdb_prod": ((8, 1, 3, 2, 2, 0, 0, 1, 0), (4, 2, 4, 7, 2, 0, 0, 1, 0)),
    "dwin_prod": ((8, 1, 3, 8, 2, 0, 0, 1, 1), (8, 1, 3, 2, 2, 0, 0, 1, 0)),
    "hr1z_prod": ((8, 1, 4, 1, 2, 0, 0, 1, 0), (4, 2, 4, 5, 2, 0, 0, 1, 0)),
    "t1_prod": ((8, 1, 4, 1, 2, 0, 0, 1, 0), None),
}
PROD_WITNESS_512 = {  # ... with WSR_CT_NO_TM3 as well and no workspace: the forms the full-size volumes take
    "hr0_prod": ((8, 1, 4, 9, 2, 0, 0, 1, 0), (8, 1, 4, 9, 2, 0, 0, 1, 0)),
    "n128_prod": ((8, 1, 4, 8, 2, 0, 0, 1, 1), (8, 1, 4, 8, 2, 0, 0, 1, 1)),
    "pre_prod": ((8, 1, 4, 8, 2, 0, 0, 1, 1), (8, 1, 4, 8, 2, 0, 0, 1, 1)),
    "up_prod": ((8, 1, 4, 8, 2, 0, 0, 1, 0), (8, 1, 4, 8, 2, 0, 0, 1, 1)),
    "grow_prod": ((8, 1, 4, 2, 2, 0, 0, 1, 1), (8, 1, 4, 8, 2, 0, 0, 1, 1)),
    "rdb_prod": ((8, 1, 4, 2, 2, 0, 0, 1, 1), (4, 2, 4, 7, 2, 0, 0, 1, 0)),
    "dwin_prod": ((8, 1, 4, 8, 2, 0, 0, 1, 1), (8, 1, 4, 2, 2, 0, 0, 1, 1)),
    "hr1z_prod": ((8, 1, 4, 1, 2, 0, 0, 1, 0), (4, 2, 4, 5, 2, 0, 0, 1, 0)),
    "t1_prod": ((8, 1, 4, 1, 2, 0, 0, 1, 0), None),
}


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", PROD_CASES)
def test_conv_tile_production_geometry(hip, monkeypatch, name, cin, cout, k, xyz, B, ups):
    monkeypatch.setenv("WSR_CT_NOSMALL", "1")
    reload_wsr_env()
    _check_tile_conv(name, cin, cout, k, xyz, B, ups, want=PROD_WITNESS[name])


@pytest.mark.parametrize("name,cin,cout,k,xyz,B,ups", PROD_CASES)
def test_conv_tile_production_geometry_on_512_voxel_tiles(hip, monkeypatch, name, cin, cout, k, xyz, B, ups):
    """the same cases kept off the 384-voxel tiles too (WSR_CT_NO_TM3) and without a workspace: the 512-voxel SIMPLE forms
    of conv_tile_simple_narrow.hip / conv_tile_simple_n128.hip, which the full-size volumes take"""
    monkeypatch.setenv("WSR_CT_NOSMALL", "1")
    monkeypatch.setenv("WSR_CT_NO_TM3", "1")
    reload_wsr_env()
    _check_tile_conv(name, cin, cout, k, xyz, B, ups, want=PROD_WITNESS_512[name], use_ws=False)


def dt_name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


def _witnessed(want, label, call):
    """run ``call`` (one tile entry point) and hold ``hip_ops.last_tile_instantiation()`` to ``want``: the nine template
    parameters of the launch_ct that served it, with the thread's launch count advanced by one - or, ``want`` None, a
    count that stood still: the streaming 1x1x1 or sliding-window kernel served the call"""
    o = ops()
    seq0 = o.last_tile_instantiation()["seq"]
    ok = call()
    w = o.last_tile_instantiation()
    got = tuple(w[f] for f in o.TILE_INST_FIELDS[:9])
    print(f"[witness] {label}: {got if w['seq'] != seq0 else None} seq +{w['seq'] - seq0} plan {o.last_tile_plan()}")
    if want is None:
        assert w["seq"] == seq0, f"{label}: expected another kernel, the halo-tile kernel ran {got}"
    else:
        assert w["seq"] == seq0 + 1, f"{label}: {w['seq'] - seq0} halo-tile launches"
        assert got == tuple(want), f"{label}: instantiation {got}, expected {tuple(want)}"
    return ok


def _check_tile_conv(name, cin, cout, k, xyz, B, ups, dt=torch.bfloat16, want=None, use_ws=True):
    """``want`` = (forward, input gradient): the launch_ct<WM, WN, TM, TN, TPK, MASK, F32, WK, SIMPLE> each launch must be
    served by (None: not the halo-tile kernel)"""
    o = ops()
    tol = 4e-3 if dt == torch.bfloat16 else 2e-5  # (operands are bf16-exact in both: fp32 products are exact)
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    w = (torch.randn((cout, cin) + tuple(k), generator=gen) / math.sqrt(cin * k[0] * k[1] * k[2])).bfloat16().float()
    p = tuple(kk // 2 for kk in k)
    geom = o.ConvGeom(cin, cout, k, (1, 1, 1), p, upsample=ups)
    cout_p = o.pad_channels(cout, dt)
    xb = to_ndhwc(x, cin + 8, 8, dt)
    d = o.make_desc(geom, dt, B, xyz, cin + 8, 8, cout_p + 8, 0)
    oxyz = (d.Xo, d.Yo, d.Zo)
    res = torch.randn((B, cout) + oxyz, generator=gen).bfloat16().float()
    rb = to_ndhwc(res, cout_p, 0, dt)
    yg = kb.Guarded((B,) + oxyz + (cout_p + 8,), dt, DEV, window=(0, cout), fill=0.0)
    yb = yg.t
    wm = packed_master(w)
    wfr = o.pack_filter_frag(wm, dtype=dt)
    assert want is not None, name
    assert _witnessed(want[0], f"{name} forward", lambda: o.conv_fwd_tile(d, xb, wfr, yb, res=rb, res_off=0, alpha=0.2,
                                                                         beta=1.0, use_ws=use_ws))
    xr = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if ups else x
    ref = 0.2 * F.conv3d(xr, w, None, 1, p) + res
    assert rel_l2(from_ndhwc(yb, 0, cout), ref) < tol, name
    taps = k[0] * k[1] * k[2]
    slabs = _slabs(oxyz[0], B * math.prod(oxyz) * cin * cout * taps)
    fam = "bf16" if dt == torch.bfloat16 else "fp32"
    for xs in slabs:
        r64, A = kb.ref_fwd(x, w, p, ups=ups, alpha=0.2, res=_xs(res, xs), beta=1.0, xs=xs)
        kb.assert_within(_xs(from_ndhwc(yb, 0, cout), xs), r64, kb.bound(r64, A, taps * cin, kb.rho_for(dt)),
                         f"tile fwd {fam}[{name} x {xs}]")
    kb.assert_guards_intact(yg, label=name)
    # input gradient (at the fine resolution when up-sampled; the 2x2 fold is a separate kernel)
    gy = torch.randn((B, cout) + oxyz, generator=gen).bfloat16().float()
    gb = to_ndhwc(gy, cout_p + 8, 0, dt)
    dd = o.make_desc(o.ConvGeom(cin, cout_p, k, (1, 1, 1), p, upsample=ups), dt, B, xyz, cin + 8, 8, cout_p + 8, 0)
    dxg = kb.Guarded((B,) + tuple(xr.shape[2:]) + (cin + 8,), dt, DEV, window=(8, cin), fill=0.0)
    dxb = dxg.t
    wft = o.pack_filter_frag(wm, transpose=True, dtype=dt)
    assert _witnessed(want[1], f"{name} input gradient", lambda: o.conv_dgrad_tile(dd, gb, wft, dxb, use_ws=use_ws))
    xg = xr.clone().requires_grad_(True)
    F.conv3d(xg, w, None, 1, p).backward(gy)
    assert rel_l2(from_ndhwc(dxb, 8, cin), xg.grad) < tol, name
    for xs in slabs:
        r64, A = kb.ref_dgrad(gy, w, p, xs=xs)
        kb.assert_within(_xs(from_ndhwc(dxb, 8, cin), xs), r64, kb.bound(r64, A, taps * cout, kb.rho_for(dt)),
                         f"tile dgrad {fam}[{name} x {xs}]")
    kb.assert_guards_intact(dxg, label=name)


@pytest.mark.parametrize("dt,C,ctot,off,nvox", [(torch.bfloat16, 128, 128, 0, 32 * 32 * 16), (torch.bfloat16, 32, 256, 96, 1000),
                                               (torch.float32, 48, 64, 8, 777), (torch.float32, 4, 8, 4, 5)])
def test_chan_sum_bias_gradient(hip, dt, C, ctot, off, nvox):
    """LFF bias gradient (torch_blocks.py:278 backward): scaled per-channel sum of an NDHWC window, fp32 out"""
    from gan_sr_wind_field_amd import hip_ops as o

    g = torch.Generator(device="cuda:0").manual_seed(5)
    x = torch.randn((1, nvox, 1, 1, ctot), device="cuda:0", generator=g).to(dt)
    out = torch.full((C,), float("nan"), device="cuda:0")
    assert o.chan_sum(x, off, C, out, scale=0.2)
    want = 0.2 * x[..., off:off + C].double().sum(dim=(0, 1, 2, 3))
    assert rel_l2(out, want.float()) < 1e-5
    assert not o.chan_sum(x[..., :6].contiguous(), 0, 6, torch.empty(6, device="cuda:0"))  # C % 4: caller falls back


def test_zfold_and_its_adjoint(hip):
    """z-folded last conv: fold sums the KZ z-taps kept as channels, unfold is its adjoint (windsr_hip.h)"""
    from gan_sr_wind_field_amd import hip_ops as o

    B, C, KZ, pz, X, Y, Z = 2, 3, 5, 2, 4, 3, 7
    g = torch.Generator(device="cuda:0").manual_seed(11)
    t = torch.randn((B, C * KZ, X, Y, Z), device="cuda:0", generator=g)
    bias = torch.randn(C, device="cuda:0", generator=g)
    y = torch.empty((B, C, X, Y, Z), device="cuda:0")
    o.zfold(t, y, bias, KZ, pz)
    want = bias.view(1, C, 1, 1, 1).expand(B, C, X, Y, Z).clone()
    tp = F.pad(t, (pz, KZ - 1 - pz))
    for c in range(C):
        for k in range(KZ):
            want[:, c] += tp[:, c * KZ + k, :, :, k:k + Z]
    assert rel_l2(y, want) < 1e-6
    # adjoint: <fold(t) - bias, gy> == <t, unfold(gy)>
    gy = torch.randn((B, C, X, Y, Z), device="cuda:0", generator=g)
    d = torch.full((B, X, Y, Z, 16), float("nan"), device="cuda:0")
    o.zunfold(gy, d, KZ, pz, 0, 16)
    assert torch.equal(d[..., 15], torch.zeros_like(d[..., 15]))
    lhs = ((y - bias.view(1, C, 1, 1, 1)) * gy).sum()
    rhs = (t.permute(0, 2, 3, 4, 1) * d[..., :15]).sum()
    assert abs(float(lhs - rhs)) < 1e-3 * abs(float(lhs))
    db = torch.empty((B, X, Y, Z, 16), device="cuda:0", dtype=torch.bfloat16)
    o.zunfold(gy, db, KZ, pz, 0, 16)
    assert rel_l2(db.float(), d) < 4e-3


def test_wind_gradient_forward_and_adjoint(hip):
    """fused wind-field derivatives == torch.gradient (x, y, coordinate spacing) + the non-uniform z stencil of
    the reference (process_data.py:273-313), and its backward == autograd of that expression"""
    from gan_sr_wind_field_amd import hip_ops as o
    from gan_sr_wind_field_amd import process_data as pd

    B, X, Y, Z = 2, 7, 6, 9
    g = torch.Generator().manual_seed(17)
    f = torch.randn((B, 3, X, Y, Z), generator=g, dtype=torch.float64)
    xs = torch.cumsum(torch.rand(X, generator=g, dtype=torch.float64) + 0.5, 0) * 100.0
    ys = torch.cumsum(torch.rand(Y, generator=g, dtype=torch.float64) + 0.5, 0) * 100.0
    zc = torch.cumsum(torch.rand((B, 1, X, Y, Z), generator=g, dtype=torch.float64) + 0.2, -1) * 30.0
    fr = f.clone().requires_grad_(True)
    want = pd.calculate_gradient_of_wind_field(fr, xs, ys, zc)  # host tensors: the torch expression
    gy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (want * gy).sum().backward()
    fd = f.float().to("cuda:0").requires_grad_(True)
    got = o.wind_gradient(fd, xs.float().to("cuda:0"), ys.float().to("cuda:0"), zc.float().to("cuda:0"))
    assert got.shape == (B, 9, X, Y, Z)
    assert rel_l2(got.detach(), want.detach().float()) < 2e-5
    (got * gy.float().to("cuda:0")).sum().backward()
    assert rel_l2(fd.grad, fr.grad.float()) < 2e-5
    # degenerate extents: a single level has no z derivative
    one = o.wind_gradient(fd.detach()[..., :1].contiguous(), xs.float().to("cuda:0"), ys.float().to("cuda:0"),
                          zc.float().to("cuda:0")[..., :1].contiguous())
    assert torch.equal(one[:, 6:], torch.zeros_like(one[:, 6:]))


def test_wind_gradient_vs_reference_fixture_and_oracle(golden, hip):
    """``wsr_wind_gradient`` against the Jacobian stacks the REFERENCE's calculate_gradient_of_wind_field produced
    (tests/golden/physics.npz, recorded by make_golden.py), and ``wsr_wind_gradient_bwd`` against autograd of the
    oracle restatement (oracle/physics.py) in fp64 - neither side involves the product's own torch expression."""
    from gan_sr_wind_field_amd import hip_ops as o
    from oracle import physics as ophys

    g = golden("physics.npz")
    xs, ys, zc = (T(g[k]).to(DEV) for k in ("x", "y", "Z"))
    for src, want in (("HR", "grad_hr"), ("SR", "grad_sr")):
        got = o.wind_gradient(T(g[src]).to(DEV), xs, ys, zc)
        assert rel_l2(got, T(g[want])) < 2e-6, src
    # adjoint: d/df of sum(J * gy), oracle in fp64
    gen = torch.Generator().manual_seed(23)
    f = T(g["SR"]).double().requires_grad_(True)
    J = ophys.wind_gradient(f, T(g["x"]).double(), T(g["y"]).double(), T(g["Z"]).double())
    gy = torch.randn(J.shape, generator=gen, dtype=torch.float64)
    (J * gy).sum().backward()
    fd = T(g["SR"]).to(DEV).requires_grad_(True)
    (o.wind_gradient(fd, xs, ys, zc) * gy.float().to(DEV)).sum().backward()
    assert rel_l2(fd.grad, f.grad) < 2e-6
    # the four normalisers of the loss (reference get_norm_factors_of_gradients) from the HIP Jacobians
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import get_norm_factors_of_gradients
    n = get_norm_factors_of_gradients(o.wind_gradient(T(g["HR"]).to(DEV), xs, ys, zc),
                                      o.wind_gradient(T(g["SR"]).to(DEV), xs, ys, zc))
    np.testing.assert_allclose([float(v) for v in n], g["norms"], rtol=1e-5)


def test_fused_content_losses_vs_reference_fixture_and_oracle(golden, hip):
    """``wsr_physics_loss_stats`` / ``_bwd``: the 6 sums and 8 maxima against the same quantities formed from the
    Jacobian stacks the REFERENCE produced (physics.npz), the four normalised MSE terms + L1 against the oracle's
    composed expressions (oracle/gan.py G_loss_terms arithmetic) and d loss / d SR against fp64 autograd of them."""
    from gan_sr_wind_field_amd import hip_ops as o
    from oracle import physics as ophys

    g = golden("physics.npz")
    HR, SR, Z, x, y = (T(g[k]) for k in ("HR", "SR", "Z", "x", "y"))
    jh, js = T(g["grad_hr"]).double(), T(g["grad_sr"]).double()
    srd = SR.to(DEV).requires_grad_(True)
    sums, mx = o.physics_loss_stats(HR.to(DEV), srd, x.to(DEV), y.to(DEV), Z.to(DEV))
    d3 = lambda j: j[:, 0] + j[:, 4] + j[:, 8]  # noqa: E731
    d2 = lambda j: j[:, 0] + j[:, 4]  # noqa: E731
    want = [((js[:, :6] - jh[:, :6]) ** 2).sum(), ((js[:, 6:] - jh[:, 6:]) ** 2).sum(), ((d3(jh) - d3(js)) ** 2).sum(),
            ((d2(jh) - d2(js)) ** 2).sum(), (HR.double() - SR.double()).abs().sum(), ((HR.double() - SR.double()) ** 2).sum()]
    np.testing.assert_allclose(sums.detach().cpu().numpy(), [float(v) for v in want], rtol=2e-5)
    wmax = [f(j) for j in (jh, js) for f in (lambda j: j[:, :6].abs().max(), lambda j: j[:, 6:].max(),
                                             lambda j: d3(j).abs().max(), lambda j: d2(j).abs().max())]
    np.testing.assert_allclose(mx.cpu().numpy(), [float(v) for v in wmax], rtol=1e-5)
    # determinism of the two-pass reduction
    s2, m2 = o.physics_loss_stats(HR.to(DEV), srd, x.to(DEV), y.to(DEV), Z.to(DEV))
    assert torch.equal(s2, sums) and torch.equal(m2, mx)
    # loss terms and gradient: weights of the shipped ini
    w = dict(pix=0.136, xy=3.064, z=0.2, div=0.366, div2=0.721)
    n = torch.max(mx[:4], mx[4:] / 100)
    nv = float(HR.shape[0] * HR[0, 0].numel())
    loss = (w["xy"] * sums[0] / (n[0] ** 2 * 6 * nv) + w["z"] * sums[1] / (n[1] ** 2 * 3 * nv)
            + w["div"] * sums[2] / (n[2] ** 2 * nv) + w["div2"] * sums[3] / (n[3] ** 2 * nv) + w["pix"] * sums[4] / (3 * nv))
    loss.backward()
    srr = SR.double().requires_grad_(True)
    gh = ophys.wind_gradient(HR.double(), x.double(), y.double(), Z.double())
    gs = ophys.wind_gradient(srr, x.double(), y.double(), Z.double())
    nn_ = ophys.gradient_norm_factors(gh, gs)
    F_ = torch.nn.functional
    ref = (w["xy"] * F_.mse_loss(gs[:, :6] / nn_[0], gh[:, :6] / nn_[0]) + w["z"] * F_.mse_loss(gs[:, 6:] / nn_[1], gh[:, 6:] / nn_[1])
           + w["div"] * F_.mse_loss(d3(gh) / nn_[2], d3(gs) / nn_[2]) + w["div2"] * F_.mse_loss(d2(gh) / nn_[3], d2(gs) / nn_[3])
           + w["pix"] * F_.l1_loss(HR.double(), srr))
    assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref))
    ref.backward()
    assert rel_l2(srd.grad, srr.grad) < 1e-5
    # the l2 pixel criterion's sum carries its gradient too
    srd.grad = None
    sums, _ = o.physics_loss_stats(HR.to(DEV), srd, x.to(DEV), y.to(DEV), Z.to(DEV))
    (sums[5] / (3 * nv)).backward()
    assert rel_l2(srd.grad, 2 * (SR - HR) / (3 * nv)) < 1e-6


# (TX, TY, TZ, NTW, ngroups, ksplit) of the launches below: all four run the first tile shape in 32-wide groups (few
# tiles), and the two with Cin >= 64 split their reduction (the wrapper always passes a workspace)
STRIDED_PLANS = {"d_down_s221": (4, 4, 9, 2, 2, 2), "d_down_s222": (4, 4, 11, 2, 1, 1),
                 "d_down_n256": (4, 4, 6, 2, 8, 8), "d_down_k5": (4, 4, 6, 2, 1, 1)}


@pytest.mark.parametrize("name,cin,cout,k,s,p,xyz,B", [
    ("d_down_s221", 64, 64, (4, 4, 3), (2, 2, 1), (1, 1, 1), (12, 10, 9), 1),     # blocks 1-3 of D
    ("d_down_s222", 32, 32, (4, 4, 3), (2, 2, 2), (1, 1, 1), (16, 12, 22), 2),    # first / last block (halved z)
    ("d_down_n256", 256, 256, (4, 4, 3), (2, 2, 1), (1, 1, 1), (8, 8, 6), 1),     # eight 32-channel groups
    ("d_down_k5", 32, 32, (4, 4, 5), (2, 2, 2), (1, 1, 2), (10, 12, 11), 1),      # feat_kern_size 5
])
def test_conv_tile_strided_forward_vs_cpu(hip, name, cin, cout, k, s, p, xyz, B):
    """Stride-2 down-sampling convs of the discriminator (torch_blocks.py:138-142) through the halo-tile kernel:
    forward with bias + LeakyReLU against an fp32 CPU conv of the same bf16-rounded operands, and element-wise against
    float64 (K = taps * Cin + the split count the launch reports); the output is guarded.  The instantiation matrix of
    this path is test_conv_strided_matrix.py."""
    o = ops()
    dt = torch.bfloat16
    plan = STRIDED_PLANS[name]
    gen = torch.Generator().manual_seed(cin + 3 * cout + sum(s))
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    w = (torch.randn((cout, cin) + tuple(k), generator=gen) / math.sqrt(cin * k[0] * k[1] * k[2])).bfloat16().float()
    bias = torch.randn(cout, generator=gen)
    geom = o.ConvGeom(cin, cout, k, s, p)
    xb = to_ndhwc(x, cin, 0, dt)
    d = o.make_desc(geom, dt, B, xyz, cin, 0, cout, 0)
    oxyz = (d.Xo, d.Yo, d.Zo)
    yg = kb.Guarded((B,) + oxyz + (cout,), dt, DEV, fill=float("nan"))
    yb = yg.t
    assert o.conv_fwd_tile(d, xb, o.pack_filter_frag(packed_master(w)), yb, bias=bias.to(DEV), act=True, slope=0.2)
    got_plan = o.last_tile_plan()
    assert tuple(got_plan[f] for f in ("TX", "TY", "TZ", "NTW", "ngroups", "ksplit")) == plan, (name, got_plan)
    ref = F.leaky_relu(F.conv3d(x, w, bias, s, p), 0.2)
    assert tuple(ref.shape[2:]) == oxyz
    assert rel_l2(from_ndhwc(yb, 0, cout), ref) < 4e-3, name
    kb.assert_guards_intact(yg, label=name)
    r64, A = kb.ref_fwd(x, w, p, stride=s, bias=bias, act=True, slope=kb._f32(0.2))
    kb.assert_within(from_ndhwc(yb, 0, cout), r64, kb.bound(r64, A, cin * k[0] * k[1] * k[2] + plan[5], kb.RHO_BF16),
                     f"strided fwd[{name}]")


@pytest.mark.parametrize("name,k,xyz,B,ctot,off,bias", [
    ("prod_5x5", (5, 5, 1), (12, 32, 16), 1, 144, 0, False),     # whole tiles, blocked workgroup order off (nty = 2)
    ("blocked", (5, 5, 1), (8, 64, 32), 1, 144, 0, False),       # nty = 4, ntz = 8: 4 x 8 tile blocks per XCD share
    ("ragged", (5, 5, 1), (9, 24, 10), 2, 152, 8, True),         # partial y tile, z = 10 (reference patches), window, bias
    ("segments", (5, 5, 1), (40, 16, 4), 1, 144, 0, False),      # one column: the x axis is cut into segments
    ("k3", (3, 3, 1), (8, 16, 8), 1, 144, 0, False),
])
def test_conv_slide_forward_vs_cpu(hip, name, k, xyz, B, ctot, off, bias):
    """sliding-window kernel of the z-folded last conv (conv_slide.hip; reference Generator_3D_Resnet_ESRGAN.py:105-110
    in the (KX, KY, 1) x 15-output form of DESIGN 4.4): planar fp32 result against an fp32 CPU conv of the same
    bf16-rounded operands, bit-identical between two launches."""
    o = ops()
    dt = torch.bfloat16
    cin, cout = 144, 15
    gen = torch.Generator().manual_seed(77 + xyz[0])
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    w = (torch.randn((cout, cin) + tuple(k), generator=gen) / math.sqrt(cin * k[0] * k[1])).bfloat16().float()
    bv = torch.randn(cout, generator=gen) if bias else None
    p = (k[0] // 2, k[1] // 2, 0)
    xb = to_ndhwc(x, ctot, off, dt)
    if off:  # canary: channels outside the window must not be read
        xb[..., :off] = float("nan")
    d = o.make_desc(o.ConvGeom(cin, cout, k, (1, 1, 1), p), dt, B, xyz, ctot, off, cout, 0)
    wf = o.pack_filter_frag(packed_master(w))
    ref = F.conv3d(x, w, bv, 1, p)
    outs = []
    for _ in range(2):
        yg = kb.Guarded((B, cout) + tuple(xyz), torch.float32, DEV)
        assert o.conv_fwd_tile(d, xb, wf, yg.t, bias=bv.to(DEV) if bias else None, out_planar=True)
        outs.append(yg.t.cpu())
        kb.assert_guards_intact(yg, label=name)
    assert torch.isfinite(outs[0]).all(), name
    assert rel_l2(outs[0], ref) < 2e-5, name  # fp32 accumulation of exactly representable products
    assert torch.equal(outs[0], outs[1]), name
    r64, A = kb.ref_fwd(x, w, p, bias=bv)
    kb.assert_within(outs[0], r64, kb.bound(r64, A, k[0] * k[1] * cin, 0.0), f"slide fwd[{name}]")


@pytest.mark.parametrize("name,k,xyz,B,ctot,off,drop", [
    ("prod_5x5", (5, 5, 1), (12, 32, 16), 1, 144, 0, True),
    ("blocked", (5, 5, 1), (8, 64, 32), 1, 144, 0, False),
    ("ragged", (5, 5, 1), (9, 24, 10), 2, 152, 8, True),
    ("segments", (5, 5, 1), (40, 16, 4), 1, 144, 0, True),
    ("k3", (3, 3, 1), (8, 16, 8), 1, 144, 0, False),
])
def test_conv_slide_input_gradient_vs_cpu(hip, name, k, xyz, B, ctot, off, drop):
    """input gradient of the z-folded last conv on the sliding-window kernel (conv_slide.hip): 16 -> 144 channels with
    the LeakyReLU + Dropout3d backward of hr_convs[0] (reference Generator_3D_Resnet_ESRGAN.py:95-104) in the epilogue,
    against fp32 CPU autograd of the same bf16-rounded operands; channels outside the written window stay untouched."""
    o = ops()
    dt = torch.bfloat16
    cin, cout, slope = 144, 15, 0.2
    gen = torch.Generator().manual_seed(91 + xyz[0])
    w = (torch.randn((cout, cin) + tuple(k), generator=gen) / math.sqrt(cout * k[0] * k[1])).bfloat16().float()
    gy = torch.randn((B, cout) + tuple(xyz), generator=gen).bfloat16().float()
    h = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()   # saved output of the layer below
    keep = (torch.bernoulli(torch.full((B, cin), 0.9), generator=gen) / 0.9) if drop else None
    p = (k[0] // 2, k[1] // 2, 0)
    gb = to_ndhwc(gy, 16, 0, dt)
    hb = to_ndhwc(h, ctot, off, dt)
    dxg = kb.Guarded((B,) + tuple(xyz) + (ctot,), dt, DEV, window=(off, cin), outside=7.0, fill=7.0)
    dxb = dxg.t
    d = o.make_desc(o.ConvGeom(cin, 16, k, (1, 1, 1), p), dt, B, xyz, ctot, off, 16, 0)
    wpad = torch.cat([w, torch.zeros((1,) + tuple(w.shape[1:]))])
    wft = o.pack_filter_frag(packed_master(wpad), transpose=True)
    m = (hb, off, 0, cin, slope) + ((keep.to(DEV),) if drop else ())
    assert o.conv_dgrad_tile(d, gb, wft, dxb, mask=m)
    xg = torch.zeros((B, cin) + tuple(xyz), requires_grad=True)
    F.conv3d(xg, w, None, 1, p).backward(gy)
    ref = xg.grad * torch.where(h > 0, 1.0, slope)
    if drop:
        ref = ref * keep[:, :, None, None, None]
    got = from_ndhwc(dxb, off, cin)
    assert torch.isfinite(got).all(), name
    assert rel_l2(got, ref) < 4e-3, name  # bf16 rounding of the result
    if off:
        assert bool((dxb[..., :off] == 7.0).all()), name
    kb.assert_guards_intact(dxg, label=name)
    r64, A = kb.ref_dgrad(gy, w, p, mask_y=h, slope=slope, keep=keep)
    kb.assert_within(got, r64, kb.bound(r64, A, k[0] * k[1] * cout, kb.RHO_BF16), f"slide dgrad[{name}]")


def test_conv_tile_beyond_32_bit_element_offsets(hip):
    """A 144-channel tensor of 512 x 512 x 128 voxels holds 4.8e9 elements (BASELINE.json configs[2] read literally):
    the halo-tile kernel addresses it with 32-bit offsets relative to a 64-bit per-workgroup base.  The last x-planes of
    a 3x3x3 144 -> 144 conv over the WHOLE tensor (19 GB of operands) equal, bit for bit, the same conv on a crop of
    those planes + halo - which sits entirely below 2^32 and is pinned to the CPU conv by the other tests - and so do
    the planes on both sides of the 2^32-element boundary; forward and input gradient."""
    o = ops()
    dt = torch.bfloat16
    C_, X, Y, Z = 144, 512, 512, 128
    assert X * Y * Z * C_ > 2 ** 32
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = torch.empty((1, X, Y, Z, C_), dtype=dt, device=DEV)
    for x0 in range(0, X, 32):  # (fill in slabs: randn makes an fp32 temporary)
        x[:, x0:x0 + 32] = torch.randn((1, 32, Y, Z, C_), generator=gen, device=DEV).to(dt)
    w = (torch.randn((C_, C_, 3, 3, 3), generator=gen, device=DEV) / math.sqrt(C_ * 27))
    geom = o.ConvGeom(C_, C_, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    plane = Y * Z * C_
    xb = 2 ** 32 // plane  # the x-plane that holds element 2^32
    for transpose in (False, True):
        wf = o.pack_filter_frag(w, transpose=transpose)
        run = (lambda d, a, b: o.conv_dgrad_tile(d, a, wf, b)) if transpose else (lambda d, a, b: o.conv_fwd_tile(d, a, wf, b))
        y = torch.empty_like(x)
        assert run(o.make_desc(geom, dt, 1, (X, Y, Z), C_, 0, C_, 0), x, y)
        for lo, hi in ((X - 10, X), (xb - 4, xb + 5)):
            clo, chi = max(lo - 1, 0), min(hi + 1, X)
            crop = x[:, clo:chi].contiguous()
            yc = torch.empty_like(crop)
            assert run(o.make_desc(geom, dt, 1, (chi - clo, Y, Z), C_, 0, C_, 0), crop, yc)
            assert torch.isfinite(y[:, lo:hi].float()).all()
            assert torch.equal(y[:, lo:hi], yc[:, lo - clo:hi - clo]), (transpose, lo, hi)
        del y
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,cin,cout,xyz,B,in_ctot,in_off,out_ctot,out_off,bias,act", [
    ("terrain1", 16, 16, (12, 16, 32), 1, 16, 0, 144, 128, False, False),   # 16 -> 16 into the concat window, TZ = 32
    ("terrain0", 1, 16, (9, 24, 32), 1, 8, 0, 16, 0, False, True),          # 1 channel padded to 8, LeakyReLU
    ("d_first", 3, 32, (10, 20, 48), 2, 8, 0, 32, 0, True, True),           # two samples, Z = 48 (16-level tiles), bias
    ("feature", 4, 128, (16, 12, 16), 1, 8, 0, 256, 0, False, False),       # n-tiles over the waves, 4-row tiles
    ("ragged", 16, 16, (5, 13, 16), 2, 24, 8, 40, 16, True, False),         # partial y tile, input window, x < 8
    ("segments", 8, 32, (70, 8, 16), 1, 8, 0, 32, 0, False, True),          # one column: the x axis is cut into segments
    ("narrow_out", 16, 12, (8, 16, 16), 1, 16, 0, 16, 4, False, False),     # 12 outputs: the tail channels of the n-tile are dropped
])
def test_conv_thin_forward_vs_cpu(hip, name, cin, cout, xyz, B, in_ctot, in_off, out_ctot, out_off, bias, act):
    """sliding-window kernel of the 3x3x3 convs with <= 16 stored reduction channels (conv_thin.hip; reference
    Generator_3D_Resnet_ESRGAN.py:78-85, 111-119, Discriminator_3D.py:67-75): against an fp32 CPU conv of the same
    bf16-rounded operands (the result is rounded to bf16 once: 4e-3), bit-identical between two launches, channels
    outside the written window untouched, and equal - up to that one rounding - to the halo-tile kernel it replaces."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(5 + xyz[0])
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / math.sqrt(cin * 27)).bfloat16().float()
    bv = torch.randn(cout, generator=gen) * 0.3 if bias else None
    cp = (cin + 7) // 8 * 8
    xb = to_ndhwc(x, in_ctot, in_off, dt)
    if in_off:
        xb[..., :in_off] = float("nan")  # canary: channels outside the window must not be read
    d = o.make_desc(o.ConvGeom(cin, cout, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, B, xyz, in_ctot, in_off, out_ctot, out_off,
                    cin=cp)
    wf = o.pack_filter_frag(packed_master(w))
    ref = F.conv3d(x, w, bv, 1, 1)
    if act:
        ref = F.leaky_relu(ref, 0.2)
    outs = []
    for _ in range(2):
        yg = kb.Guarded((B,) + tuple(xyz) + (out_ctot,), dt, DEV, window=(out_off, cout), outside=7.0, fill=7.0)
        assert o.conv_fwd_tile(d, xb, wf, yg.t, bias=bv.to(DEV) if bias else None, act=act, slope=0.2)
        kb.assert_guards_intact(yg, label=name)
        outs.append(yg.t)
    got = from_ndhwc(outs[0], out_off, cout)
    r64, A = kb.ref_fwd(x, w, (1, 1, 1), bias=bv, act=act)
    kb.assert_within(got, r64, kb.bound(r64, A, 27 * cin, kb.RHO_BF16), f"thin fwd[{name}]")
    assert torch.isfinite(got).all(), name
    assert rel_l2(got, ref) < 4e-3, name
    assert torch.equal(outs[0], outs[1]), name
    keep = torch.ones(out_ctot, dtype=torch.bool)
    keep[out_off:out_off + cout] = False
    assert bool((outs[0][..., keep.to(DEV)] == 7.0).all()), name
    import os
    os.environ["WSR_NO_THIN"] = "1"
    reload_wsr_env()
    try:
        y2 = torch.full((B,) + tuple(xyz) + (out_ctot,), 7.0, dtype=dt, device=DEV)
        assert o.conv_fwd_tile(d, xb, wf, y2, bias=bv.to(DEV) if bias else None, act=act, slope=0.2)
    finally:
        del os.environ["WSR_NO_THIN"]
        reload_wsr_env()
    assert rel_l2(got, from_ndhwc(y2, out_off, cout)) < 4e-3, name


@pytest.mark.parametrize("name,cin,cout,xyz,B,alpha", [("terrain1", 16, 16, (12, 16, 32), 1, 1.0),
                                                       ("wide_in", 64, 16, (6, 9, 16), 2, 0.5),
                                                       ("thin8", 16, 8, (8, 8, 48), 1, 1.0)])
def test_conv_thin_input_gradient_vs_cpu(hip, name, cin, cout, xyz, B, alpha):
    """input gradient of a 3x3x3 conv with <= 16 OUTPUT channels (terrain_convs.1, reference
    Generator_3D_Resnet_ESRGAN.py:111-119) on the same sliding-window kernel: fp32 CPU autograd of the same
    bf16-rounded operands."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(31 + xyz[0])
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / math.sqrt(cout * 27)).bfloat16().float()
    gy = torch.randn((B, cout) + tuple(xyz), generator=gen).bfloat16().float()
    cop = (cout + 7) // 8 * 8
    gb = to_ndhwc(gy, cop, 0, dt)
    d = o.make_desc(o.ConvGeom(cin, cout, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, B, xyz, cin, 0, cop, 0, cout=cop)
    wpad = torch.cat([w, torch.zeros((cop - cout,) + tuple(w.shape[1:]))]) if cop != cout else w
    wft = o.pack_filter_frag(packed_master(wpad), transpose=True)
    dxg = kb.Guarded((B,) + tuple(xyz) + (cin,), dt, DEV, fill=float("nan"))
    dxb = dxg.t
    assert o.conv_dgrad_tile(d, gb, wft, dxb, alpha=alpha)
    xg = torch.zeros((B, cin) + tuple(xyz), requires_grad=True)
    F.conv3d(xg, w, None, 1, 1).backward(gy)
    got = from_ndhwc(dxb, 0, cin)
    assert torch.isfinite(got).all(), name
    assert rel_l2(got, alpha * xg.grad) < 4e-3, name
    kb.assert_guards_intact(dxg, label=name)
    r64, A = kb.ref_dgrad(gy, w, (1, 1, 1), alpha=alpha)
    kb.assert_within(got, r64, kb.bound(r64, A, 27 * cout, kb.RHO_BF16), f"thin dgrad[{name}]")


@pytest.mark.parametrize("sz,cin,cout,xyz,B", [(1, 32, 32, (16, 16, 8), 2), (2, 64, 128, (8, 16, 12), 1),
                                                (2, 32, 64, (12, 8, 6), 1)])
def test_strided_filter_gradient_in_parity_form(hip, sz, cin, cout, xyz, B):
    """filter gradient of the discriminator's down-sampling convs (reference torch_blocks.py:372-521: kernel (4,4,3),
    stride (2,2,1|2), padding 1) as stride-1 2x2xKZ' gradients over parity sub-lattices of the input
    (``wsr_conv_t.lat = 3`` + ``wsr_strided_parity_unfold``) against fp32 CPU autograd of the same bf16-rounded
    operands; two runs are bit-identical (ordered reduction of the split copies)."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(3 * cin + cout + sz)
    x = torch.randn((B, cin) + tuple(xyz), generator=gen).bfloat16().float()
    w = torch.zeros((cout, cin, 4, 4, 3), requires_grad=True)
    y = F.conv3d(x, w, None, (2, 2, sz), 1)
    gy = torch.randn(y.shape, generator=gen).bfloat16().float()
    y.backward(gy)
    oxyz = tuple(y.shape[2:])
    assert (2 * oxyz[0], 2 * oxyz[1], sz * oxyz[2]) == tuple(xyz)
    xb, gb = to_ndhwc(x, cin, 0, dt), to_ndhwc(gy, cout, 0, dt)
    outs, guards, n_max = [], [], 0
    for _ in range(2):
        dwg = kb.Guarded((cout, cin, 4, 4, 3), torch.float32, DEV)
        dw = dwg.t
        guards.append(dwg)
        for zc in range(sz):
            kzp = 3 if sz == 1 else (1 if zc == 0 else 2)
            pz, mz, oz = (1, 1, 0) if sz == 1 else ((0, 2, 0) if zc == 0 else (1, 2, 1))
            tw = torch.full((4, cout, cin, 2, 2, kzp), float("nan"), dtype=torch.float32, device=DEV)
            jobs, keep = [], []
            for ph in range(4):
                a_, b_ = ph >> 1, ph & 1
                g = o.ConvGeom(cin, cout, (2, 2, kzp), (1, 1, 1), (1 - a_, 1 - b_, pz))
                d = o.make_desc(g, dt, B, oxyz, cin, 0, cout, 0, lat=(1 - a_, 1 - b_, 0, mz, oz, True))
                n = o.conv_wgrad_nparts(d)
                n_max = max(n_max, n)
                pg = kb.Guarded((n, cout, g.taps, cin), torch.float32, DEV)
                parts = pg.t
                o.conv_wgrad_parts(d, xb, gb, parts, n)
                guards.append(pg)
                jobs.append((parts[0], tw[ph], 1.0, n, parts[0].numel()))
                keep.append(parts)
            o.unpack_wgrad_reduce_multi(o.unpack_job_table(jobs))
            o.strided_parity_unfold(tw, dw, sz, zc)
        outs.append(dw.cpu())
    assert torch.isfinite(outs[0]).all()
    assert rel_l2(outs[0], w.grad) < 2e-5  # fp32 accumulation of exactly representable products
    assert torch.equal(outs[0], outs[1])
    kb.assert_guards_intact(*guards, label="strided wgrad")
    w64 = torch.zeros((cout, cin, 4, 4, 3), dtype=torch.float64, requires_grad=True)
    (r64,) = torch.autograd.grad(F.conv3d(x.double(), w64, None, (2, 2, sz), 1), w64, gy.double())
    (A,) = torch.autograd.grad(F.conv3d(x.double().abs(), w64, None, (2, 2, sz), 1), w64, gy.double().abs())
    kb.assert_within(outs[0], r64, kb.bound(r64, A, B * math.prod(oxyz) + n_max, 0.0),
                     f"strided wgrad[{sz} {cin} {cout}]", kind="filter")


@pytest.mark.parametrize("shape", [(32, 128, 3, 3, 3), (128, 256, 1, 1, 1), (256, 128, 1, 1, 1), (144, 144, 5, 5, 5),
                                   (3, 144, 5, 5, 1), (32, 3, 3, 3, 3), (64, 40, 4, 4, 3), (20, 24, 3, 3, 1)])
def test_filter_fragments_of_a_job_table_equal_the_single_filter_pack(hip, shape):
    """wsr_pack_filter_frag_multi (LDS-staged, one launch per network) writes bit for bit what wsr_pack_filter_frag
    (one gather kernel per filter) writes - forward and transposed (input-gradient) fragment order."""
    o = ops()
    gen = torch.Generator().manual_seed(sum(shape))
    w = torch.randn(shape, generator=gen).to(DEV)
    jobs, want = [], []
    for tr in (False, True):
        want.append(o.pack_filter_frag(w, transpose=tr))
        out = torch.full_like(want[-1], float("nan"))
        jobs.append((w, out, tr))
    o.pack_filter_frag_multi(o.pack_job_table(jobs))
    torch.cuda.synchronize()
    for (_, out, tr), ref in zip(jobs, want):
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), f"transpose={tr}"


@pytest.mark.parametrize("transpose", [False, True])
def test_stacked_filter_parts_equal_the_pack_of_the_stacked_filter(hip, transpose):
    """The stacked filter of a dense block (reference torch_blocks.py:256-267: conv i reads channels [0, nf + i*gc))
    assembled from its source convs by red_total > 0 jobs == the plain pack of the concatenated virtual filter."""
    o = ops()
    gen = torch.Generator().manual_seed(77 + int(transpose))
    c_lo, c_n = 32, 48
    srcs = [torch.randn((co, ci, 3, 3, 3), generator=gen).to(DEV) for co, ci in ((32, 96), (16, 128), (32, 160))]
    virt = torch.cat([w[:, c_lo:c_lo + c_n] for w in srcs], 0).contiguous()  # (80, 48, 3, 3, 3)
    ref = o.pack_filter_frag(virt, transpose=transpose)
    out = torch.full_like(ref, float("nan"))
    jobs, off, tot = [], 0, virt.shape[0]
    for w in srcs:
        jobs.append((w, out, transpose, c_lo, c_n, off, tot, 0, c_n) if transpose else
                    (w, out, transpose, c_lo, c_n, 0, c_n, off, tot))
        off += w.shape[0]
    o.pack_filter_frag_multi(o.pack_job_table(jobs))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("world,G,C_", [(1, 2, 32), (2, 2, 64), (8, 1, 256), (3, 2, 8)])
def test_syncbn_shard_algebra_vs_float64(hip, world, G, C_):
    """wsr_bn_shard_stats / wsr_bn_combine_shards (the per-channel algebra around SyncBN's one collective per layer)
    against the pairwise combination of equal shards in float64: the combined mean / M2 equal the statistics of the
    concatenated data."""
    o = ops()
    gen = torch.Generator().manual_seed(100 * world + C_)
    n = 40  # values per rank, group and channel
    data = torch.randn((world, G, n, C_), generator=gen, dtype=torch.float64) * 2.0 + 0.7
    recs = []
    for r in range(world):
        x = data[r]                                         # (G, n, C)
        mean = x.mean(dim=1)                                # local mean
        d = x - mean[:, None, :].float().double()           # shifted by the fp32 mean the kernels hold
        work = torch.zeros((G, 2 * C_), dtype=torch.float32, device=DEV)
        work[:, :C_] = mean.float().to(DEV)
        st = torch.zeros((G, 4 * C_), dtype=torch.float32, device=DEV)
        st[:, 2 * C_:3 * C_] = d.sum(dim=1).float().to(DEV)         # sum d (~0)
        st[:, 3 * C_:] = (d * d).sum(dim=1).float().to(DEV)         # sum d^2
        send = torch.empty((G, 2 * C_), dtype=torch.float32, device=DEV)
        o.bn_shard_stats(work, st[:, 2 * C_:], float(n), send)
        recs.append(send)
    gathered = torch.stack(recs)                            # (world, G, 2C)
    work = torch.full((G, 2 * C_), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.full((G, 4 * C_), float("nan"), dtype=torch.float32, device=DEV)
    o.bn_combine_shards(gathered, float(n), work, st[:, 2 * C_:])
    torch.cuda.synchronize()
    allx = data.permute(1, 0, 2, 3).reshape(G, world * n, C_)
    gmean = allx.mean(dim=1)
    m2 = ((allx - gmean[:, None, :]) ** 2).sum(dim=1)
    np.testing.assert_allclose(work[:, :C_].cpu().double().numpy(), gmean.numpy(), rtol=2e-6, atol=2e-6)
    assert torch.equal(st[:, 2 * C_:3 * C_].cpu(), torch.zeros((G, C_)))
    np.testing.assert_allclose(st[:, 3 * C_:].cpu().double().numpy(), m2.numpy(), rtol=2e-5)
    assert torch.isnan(work[:, C_:]).all() and torch.isnan(st[:, :2 * C_]).all()  # nothing else is written


@pytest.mark.gpu
def test_ordered_reduce_row_form_is_bit_identical(hip, monkeypatch):
    """wsr_unpack_wgrad_reduce_multi: the row form (one workgroup per output channel, whole packed rows of every
    split copy) against the chunk form (64 input channels per workgroup, WSR_UNPACK_ROWS=0) - the same additions in
    the same order, so the master-layout gradients are bit-identical, and equal to the plain ordered sum."""
    from conftest import reload_wsr_env

    o = ops()
    gen = torch.Generator().manual_seed(11)
    shapes = [  # (n_parts, Cout, taps, kpad, Cin, scale)
        (21, 32, 27, 224, 160, 1.0),    # a growth conv of a stacked dense-block gradient (its window of the row)
        (21, 32, 27, 224, 224, 1.0),
        (32, 128, 1, 256, 256, 0.2),    # LFF
        (85, 144, 25, 16, 16, 1.0),     # the z-folded last conv, roles exchanged
        (9, 48, 125, 144, 144, 1.0),    # 5x5x5: the [Cin][taps] image does not fit the row form's LDS -> chunk form
        (5, 8, 27, 8, 3, 1.0),          # 3 of 8 stored channels
        (3, 16, 12, 20, 18, 0.5),       # channel tail inside a float4
        (1, 1, 1, 128, 128, 1.0),       # the bias form (a (1, 1, nf) packed row -> (1, nf, 1)): a single copy
        (12, 1, 1, 128, 128, 0.2),      # ur_sum_parts: the 8 + 4 tails
        (31, 1, 1, 128, 128, 1.0),      # 16 + 8 + 4 + 3
        (512, 1, 1, 128, 128, 0.2),     # every partial row of a capped channel sum
    ]
    jobs, refs = [], []
    for n, cout, taps, kpad, cin, scale in shapes:
        parts = torch.randn((n, cout, taps, kpad), generator=gen).to(DEV)
        dst = torch.full((cout, cin, taps), float("nan"), device=DEV)
        jobs.append((parts[0], dst, scale, n, parts[0].numel()))
        acc = torch.zeros((cout, taps, kpad), device=DEV)
        for s_ in range(n):  # the kernel's order: ((0 + p0) + p1) + ...
            acc = acc + parts[s_]
        refs.append((scale * acc[:, :, :cin]).permute(0, 2, 1).contiguous())
        jobs[-1] += (parts,)  # (keeps the copies alive)
    outs = {}
    for rows in ("0", "1"):
        monkeypatch.setenv("WSR_UNPACK_ROWS", rows)
        reload_wsr_env()
        for j in jobs:
            j[1].fill_(float("nan"))
        o.unpack_wgrad_reduce_multi(o.unpack_job_table([j[:5] for j in jobs]))
        outs[rows] = [j[1].clone() for j in jobs]
    for a, b, r, sh in zip(outs["0"], outs["1"], refs, shapes):
        assert torch.equal(a, b), sh
        assert torch.equal(b, r), sh


@pytest.mark.gpu
def test_table_adam_equals_torch_adam(hip):
    """tools/table_adam.TableAdam (one wsr_adam_multi launch over a device table of tensor chunks, ABI 7) against
    torch.optim.Adam on the CPU: the same parameters after six steps with weight decay and a learning-rate change, the
    same state layout, and a state_dict round trip in the middle that continues the step count."""
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(5)
    shapes = [(70001,), (33, 7, 3, 3, 3), (128,), (5,), (32768,), (32769,)]
    ref_p = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    dev_p = [p.detach().clone().to(DEV).requires_grad_(True) for p in ref_p]
    kw = dict(lr=8e-5, betas=(0.5, 0.999), weight_decay=0.01)
    ref = torch.optim.Adam(ref_p, **kw)
    opt = TableAdam(dev_p, **kw)
    calls = []
    opt.register_step_post_hook(lambda *_: calls.append(1))
    for it in range(6):
        if it == 3:  # checkpoint round trip + a scheduler-style learning-rate change
            sd = opt.state_dict()
            assert float(sd["state"][0]["step"]) == 3.0 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
            opt = TableAdam(dev_p, **kw)
            opt.load_state_dict(sd)
            opt.register_step_post_hook(lambda *_: calls.append(1))
            for o_ in (ref, opt):
                o_.param_groups[0]["lr"] = 4e-5
        for rp, dp in zip(ref_p, dev_p):
            g = torch.randn(rp.shape, generator=gen)
            rp.grad, dp.grad = g.clone(), g.to(DEV)
        ref.step()
        opt.step()
    assert len(calls) == 6
    for rp, dp in zip(ref_p, dev_p):
        assert rel_l2(dp.detach().cpu(), rp.detach()) < 1e-6
    sd = opt.state_dict()
    assert float(sd["state"][5]["step"]) == 6.0
    assert rel_l2(sd["state"][0]["exp_avg_sq"].cpu(), ref.state_dict()["state"][0]["exp_avg_sq"]) < 1e-6
    # a parameter without a gradient: torch's own (fused) step takes over, counts stay consistent
    dev_p[2].grad = None
    opt.step()
    opt.step()
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 8.0 and float(sd["state"][2]["step"]) == 6.0
    # ... and with the gradient back the group is at two different step counts: torch's per-tensor form keeps running
    dev_p[2].grad = torch.zeros_like(dev_p[2])
    opt.step()
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 9.0 and float(sd["state"][2]["step"]) == 7.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_concat_as_two_tensors_equals_the_concatenated_conv(hip, dt):
    """ABI 8 - the generator's concat in front of its 5x5x5 conv (reference Generator_3D_Resnet_ESRGAN.py:228,
    torch.cat((x, Zf), 1): 128 up-conv channels + 16 terrain channels) as TWO tensors: forward (wsr_epilogue_t.in2),
    input gradient (wsr_dgrad_opts_t.dx2) and filter gradient (wsr_conv3d_wgrad_parts_x2) must equal the same kernels
    on the concatenated buffer BIT FOR BIT (same products, same order - only the addresses differ), at the tile
    geometry of the benchmark (512-voxel tiles, 9 n-tiles); shapes the two-tensor kernels do not serve say so
    (wsr_conv_split_ok) instead of computing something else."""
    o = ops()
    nf, tf, k, p = 128, 16, (5, 5, 5), (2, 2, 2)
    B, xyz = 1, (16, 32, 128)   # 65 536 voxels: the smallest volume dispatch_ct keeps on the 512-voxel tiles
    cin = cout = nf + tf
    gen = torch.Generator().manual_seed(11)
    xa = torch.randn((B,) + xyz + (nf,), generator=gen).to(DEV).to(dt)
    xt = torch.randn((B,) + xyz + (tf,), generator=gen).to(DEV).to(dt)
    xcat = torch.cat([xa, xt], dim=-1).contiguous()
    w = (torch.randn((cout, cin) + k, generator=gen) / math.sqrt(cin * 125)).to(DEV)
    geom = o.ConvGeom(cin, cout, k, (1, 1, 1), p)
    d_cat = o.make_desc(geom, dt, B, xyz, cin, 0, cout, 0)
    d_two = o.make_desc(geom, dt, B, xyz, nf, 0, cout, 0, cin=cin)      # the first tensor's window holds nf channels
    assert o.conv_split_ok(d_two, nf)
    d_small = o.make_desc(geom, dt, B, (8, 8, 16), nf, 0, cout, 0, cin=cin)
    assert not o.conv_split_ok(d_small, nf) or dt == torch.float32      # small bf16 volumes run the 128-voxel tiles
    assert not o.conv_split_ok(o.make_desc(o.ConvGeom(80, 80, k, (1, 1, 1), p), dt, B, xyz, 64, 0, 80, 0, cin=80), 64)
    wf = o.pack_filter_frag(w, dtype=dt)
    bias = torch.randn(cout, generator=gen).to(DEV)
    y_cat = torch.zeros((B,) + xyz + (cout,), dtype=dt, device=DEV)
    y_two = torch.zeros_like(y_cat)
    assert o.conv_fwd_tile(d_cat, xcat, wf, y_cat, bias=bias, act=True, slope=0.2)
    assert o.conv_fwd_tile(d_two, xa, wf, y_two, bias=bias, act=True, slope=0.2, in2=xt, in2_c0=nf)
    assert torch.equal(y_cat, y_two) and float(y_cat.float().abs().sum()) > 0
    # against the CPU conv of the same operands on a slab (the whole volume would take minutes on the host)
    sl = slice(4, 10)
    ref = F.leaky_relu(F.conv3d(xcat[:, 2:12].permute(0, 4, 1, 2, 3).float().cpu(), w.to(dt).float().cpu(),
                                bias.cpu(), 1, p), 0.2)[:, :, 2:8]
    assert rel_l2(y_two[:, sl].permute(0, 4, 1, 2, 3).float().cpu(), ref) < (4e-3 if dt == torch.bfloat16 else 2e-5)
    # input gradient: channels [0, nf) to one tensor, [nf, nf + tf) to the other
    gy = torch.randn((B,) + xyz + (cout,), generator=gen).to(DEV).to(dt)
    wt = o.pack_filter_frag(w, transpose=True, dtype=dt)
    dx_cat = torch.zeros((B,) + xyz + (cin,), dtype=dt, device=DEV)
    dxa = torch.full((B,) + xyz + (nf,), float("nan"), dtype=dt, device=DEV)
    dxt = torch.full((B,) + xyz + (tf,), float("nan"), dtype=dt, device=DEV)
    assert o.conv_dgrad_tile(d_cat, gy, wt, dx_cat)
    assert o.conv_dgrad_tile(d_two, gy, wt, dxa, dx2=dxt, dx2_c0=nf)
    assert torch.equal(dx_cat[..., :nf], dxa) and torch.equal(dx_cat[..., nf:], dxt)
    # filter gradient: same split copies, same ordered sum
    n = o.conv_wgrad_nparts(d_cat)
    parts_cat = torch.empty((n, cout, 125, cin), dtype=torch.float32, device=DEV)
    parts_two = torch.full_like(parts_cat, float("nan"))
    o.conv_wgrad_parts(d_cat, xcat, gy, parts_cat, n)
    o.conv_wgrad_parts(d_two, xa, gy, parts_two, n, x2=xt, x2_c0=nf)
    assert torch.equal(parts_cat, parts_two)
    del parts_cat, parts_two
    torch.cuda.empty_cache()


def test_plane_sum_uses_the_batch(hip):
    """bias gradient of the last conv (planar fp32 (B, 3, V) -> 3 sums): every (sample, voxel slice) is a row of the
    two-pass sum - a batch of 32 small patches is 96+ workgroups, not 9 - and the result does not depend on the launch
    (fixed summation order)."""
    o = ops()
    gen = torch.Generator().manual_seed(4)
    for B, V in ((32, 64 * 64 * 10), (1, 128 * 128 * 16), (5, 1000), (600, 64)):
        src = torch.randn((B, 3, V), generator=gen).to(DEV)
        out = torch.empty(3, device=DEV)
        o.plane_sum(src, out)
        ref = src.double().sum(dim=(0, 2))
        assert rel_l2(out, ref) < 1e-6, (B, V)
        out2 = torch.empty(3, device=DEV)
        o.plane_sum(src, out2)
        assert torch.equal(out, out2)


def test_lff_filter_gradient_on_ten_level_patches(hip):
    """the 1x1x1 (LFF) filter gradient at the cluster configuration's trunk shape - batch 32 of 16 x 16 x 10 voxels: the
    tile kernel takes the voxels as a flat index (no halo, no geometry), same sums as the fp32 CPU evaluation."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(21)
    B, xyz, cin, cout = 4, (16, 16, 10), 256, 128
    x = torch.randn((B, cin) + xyz, generator=gen).bfloat16().float()
    gy = torch.randn((B, cout) + xyz, generator=gen).bfloat16().float()
    geom = o.ConvGeom(cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    xb, gb = to_ndhwc(x, cin, 0, dt), to_ndhwc(gy, cout, 0, dt)
    d = o.make_desc(geom, dt, B, xyz, cin, 0, cout, 0)
    n = o.conv_wgrad_nparts(d)
    parts = torch.full((n, cout, 1, cin), float("nan"), dtype=torch.float32, device=DEV)
    o.conv_wgrad_parts(d, xb, gb, parts, n)
    dw = parts.sum(0)[:, 0, :].cpu()
    ref = torch.einsum("bnxyz,bcxyz->nc", gy, x)
    assert rel_l2(dw, ref) < 2e-5


@pytest.mark.parametrize("name,cin,cout,k,xyz,B", [
    # the cluster configuration's trunk (config/wind_field_GAN_3D_config_cluster.ini:42-47: batch 32 of 16 x 16 x 10 LR
    # patches): 6 tiles of 512 rows per sample leave a quarter of the CUs idle in the single round - 8 tiles of 384
    ("tm3_n128", 128, 128, (3, 3, 3), (16, 16, 10), 32),   # <8,1,3,8>: first stage of a dense block, lr_conv; its dgrad too
    ("tm3_grow", 96, 32, (3, 3, 3), (16, 16, 10), 32),     # <8,1,3,2>: growth conv over 96 channels
])
def test_conv_tile_384_voxel_tiles(hip, name, cin, cout, k, xyz, B):
    """conv_tile_tm3.hip: the launches dispatch_ct moves to 384-voxel tiles (fewer rounds x rows than on 512-voxel
    ones) against the fp32 CPU conv of the same bf16 operands - forward with a residual, input gradient."""
    want = {"tm3_n128": ((8, 1, 3, 8, 2, 0, 0, 1, 1), (8, 1, 3, 8, 2, 0, 0, 1, 1)),
            "tm3_grow": ((8, 1, 3, 2, 2, 0, 0, 1, 1), (8, 1, 3, 8, 2, 0, 0, 1, 1))}[name]
    _check_tile_conv(name, cin, cout, k, xyz, B, False, want=want)


def test_conv_tile_384_voxel_tiles_masked_window(hip):
    """... and the masked growth-window input gradient of the stacked dense-block backward on those tiles: 96 reduction
    channels -> 32 produced channels, accumulated onto the buffer, times the LeakyReLU derivative of the saved output"""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(77)
    B, xyz, red, n = 32, (16, 16, 10), 96, 32
    gy = torch.randn((B, red) + xyz, generator=gen).bfloat16().float()        # output gradients of the later convs
    w = (torch.randn((red, n, 3, 3, 3), generator=gen) / math.sqrt(red * 27)).bfloat16().float()  # (Cout = red, Cin = n)
    acc = torch.randn((B, n) + xyz, generator=gen).bfloat16().float()         # what the window already holds
    ysaved = torch.randn((B, n) + xyz, generator=gen).bfloat16().float()      # saved forward output (sign = mask)
    bufg = kb.Guarded((B,) + xyz + (256,), dt, DEV, window=(128, n), fill=acc.permute(0, 2, 3, 4, 1).to(DEV).to(dt), outside=0.0)
    buf = bufg.t
    buf[..., 160:160 + red] = gy.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    bufg.snap = bufg.base.view(kb._INT_VIEW[dt])[bufg.mask].clone()  # (the gradients it reads are guard elements from here on)
    yb = to_ndhwc(ysaved, 256, 128, dt)
    d = o.make_desc(o.ConvGeom(n, red, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, B, xyz, 256, 128, 256, 160)
    wt = o.pack_filter_frag(packed_master(w), transpose=True, dtype=dt)
    assert _witnessed((8, 1, 3, 2, 2, 1, 0, 1, 1), "tm3 masked window",
                      lambda: o.conv_dgrad_tile(d, buf, wt, buf, alpha=1.0, accumulate=True, mask=(yb, 128, 0, n, 0.2)))
    xg = torch.zeros((B, n) + xyz, requires_grad=True)
    F.conv3d(xg, w, None, 1, 1).backward(gy)
    ref = (xg.grad + acc) * torch.where(ysaved > 0, torch.ones_like(ysaved), torch.full_like(ysaved, 0.2))
    assert rel_l2(from_ndhwc(buf, 128, n), ref) < 4e-3
    assert torch.equal(buf[..., 160:160 + red].cpu(), gy.permute(0, 2, 3, 4, 1).to(dt))  # the gradients it read are intact
    kb.assert_guards_intact(bufg, label="tm3 masked window")
    # element-wise: the accumulated value is an exact bf16 operand, so rho is paid on the stored result only
    r64, A = kb.ref_dgrad(gy, w, (1, 1, 1), acc=acc, mask_y=ysaved, slope=kb._f32(0.2), mask_win=(0, n))
    kb.assert_within(from_ndhwc(buf, 128, n), r64, kb.bound(r64, A, 27 * red, kb.RHO_BF16), "tile dgrad bf16[tm3 masked window]")


def test_conv_thin_paired_stores_equal_the_plain_form(hip, monkeypatch):
    """conv_thin.hip, paired 16-byte stores (one v_permlane32_swap per dword between the results of an m-tile pair, the
    n-tile's rows dealt to the lane groups as channel blocks 0, 2, 1, 3): forced on for the one-n-tile convs (default: only
    where several waves share a voxel row - the feature conv), bit-identical to the 8-byte form, windows and tails included."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(3)
    for cin, cout, xyz, in_ctot, in_off, out_ctot, out_off in ((16, 16, (8, 16, 32), 16, 0, 16, 0), (8, 16, (9, 11, 32), 24, 8, 40, 16),
                                                            (8, 128, (8, 8, 32), 8, 0, 128, 0), (16, 16, (5, 9, 16), 16, 0, 144, 128)):
        x = torch.randn((1, cin) + xyz, generator=gen)
        w = torch.randn((cout, cin, 3, 3, 3), generator=gen) / math.sqrt(cin * 27)
        bias = torch.randn(cout, generator=gen).to(DEV)
        xb = to_ndhwc(x, in_ctot, in_off, dt)
        d = o.make_desc(o.ConvGeom(cin, cout, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, 1, xyz, in_ctot, in_off, out_ctot, out_off)
        wf = o.pack_filter_frag(packed_master(w), dtype=dt)
        outs = []
        for pair in ("0", "1"):
            monkeypatch.setenv("WSR_CT3_PAIR", pair)
            reload_wsr_env()
            y = torch.full((1,) + xyz + (out_ctot,), 7.0, dtype=dt, device=DEV)
            assert o.conv_fwd_tile(d, xb, wf, y, bias=bias, act=True, slope=0.2)
            outs.append(y)
        assert torch.equal(outs[0], outs[1]), (cin, cout, xyz)
        assert float(outs[1][..., out_off:out_off + cout].float().abs().sum()) > 0
        if out_ctot > cout:  # the rest of the voxel rows is untouched
            rest = torch.cat([outs[1][..., :out_off], outs[1][..., out_off + cout:]], dim=-1)
            assert bool((rest == 7.0).all())
    monkeypatch.delenv("WSR_CT3_PAIR")
    reload_wsr_env()


@pytest.mark.gpu
def test_conv_tile_simple_instantiations_equal_the_general_ones(hip, monkeypatch):
    """conv_tile_simple_*.hip: the trunk's plain stride-1 launches run instantiations whose stride / lattice / parity /
    split-reduction / planar-output switches are compile-time constants (fewer spilled SGPRs, half the code).  Same
    arithmetic in the same order: bit-identical to the general instantiations (WSR_CT_SIMPLE=0) on the split dense-block
    forward (128-wide block-input part with bias + LeakyReLU on the first window only, 32-wide second stage with the
    partial sums joining before the activation), on the stacked input gradient's windows (128-wide accumulate, 32-wide
    with the LeakyReLU-backward mask) - at the trunk's tile sizes and on a small volume (128-voxel tiles, K-step shares)."""
    o = ops()
    dt = torch.bfloat16
    gen = torch.Generator().manual_seed(11)
    nf, gc, ctot = 128, 32, 256
    for xyz in ((32, 32, 64), (16, 16, 10), (16, 24, 40)):
        buf0 = (torch.randn((1,) + xyz + (ctot,), generator=gen) * 0.5).to(dt).to(DEV)
        gd0 = (torch.randn((1,) + xyz + (ctot,), generator=gen) * 0.5).to(dt).to(DEV)
        w_pre = torch.randn((4 * gc, nf, 3, 3, 3), generator=gen) / math.sqrt(nf * 27)
        w_grow = torch.randn((gc, 2 * gc, 3, 3, 3), generator=gen) / math.sqrt(2 * gc * 27)
        b_pre = torch.randn(4 * gc, generator=gen).to(DEV)
        b_grow = torch.randn(gc, generator=gen).to(DEV)
        f_pre = o.pack_filter_frag(packed_master(w_pre), dtype=dt)
        f_grow = o.pack_filter_frag(packed_master(w_grow), dtype=dt)
        ft_pre = o.pack_filter_frag(packed_master(w_pre), transpose=True, dtype=dt)
        ft_grow = o.pack_filter_frag(packed_master(w_grow), transpose=True, dtype=dt)
        d_pre = o.make_desc(o.ConvGeom(nf, 4 * gc, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, 1, xyz, ctot, 0, ctot, nf)
        d_grow = o.make_desc(o.ConvGeom(2 * gc, gc, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, 1, xyz, ctot, nf, ctot, nf + 2 * gc)
        # input gradients: 128 produced channels from the 4*gc growth gradients; 32 produced from 2*gc of them, masked
        g_pre = o.make_desc(o.ConvGeom(nf, 4 * gc, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, 1, xyz, ctot, 0, ctot, nf)
        g_grow = o.make_desc(o.ConvGeom(gc, 2 * gc, (3, 3, 3), (1, 1, 1), (1, 1, 1)), dt, 1, xyz, ctot, nf, ctot, nf + gc)
        ft_win = o.pack_filter_frag(packed_master(torch.randn((2 * gc, gc, 3, 3, 3), generator=gen) / math.sqrt(gc * 27)),
                                    transpose=True, dtype=dt)
        outs = []
        for simple in ("0", "1"):
            monkeypatch.setenv("WSR_CT_SIMPLE", simple)
            reload_wsr_env()
            buf, gd = buf0.clone(), gd0.clone()
            assert o.conv_fwd_tile(d_pre, buf, f_pre, buf, bias=b_pre, act=True, slope=0.2, act_c1=gc)
            assert o.conv_fwd_tile(d_grow, buf, f_grow, buf, bias=b_grow, res=buf, res_off=nf + 2 * gc, beta=1.0, act=2,
                                   slope=0.2)
            assert o.conv_dgrad_tile(g_grow, gd, ft_win, gd, alpha=1.0, accumulate=True, mask=(buf, nf, 0, gc, 0.2))
            assert o.conv_dgrad_tile(g_pre, gd, ft_pre, gd, alpha=1.0, accumulate=True)
            outs.append((buf, gd))
        assert torch.equal(outs[0][0], outs[1][0]), xyz
        assert torch.equal(outs[0][1], outs[1][1]), xyz
        assert not torch.equal(outs[1][0], buf0) and not torch.equal(outs[1][1], gd0)
        assert bool(torch.isfinite(outs[1][0].float()).all()) and bool(torch.isfinite(outs[1][1].float()).all())
    monkeypatch.delenv("WSR_CT_SIMPLE")
    reload_wsr_env()


@pytest.mark.parametrize("B", [1, 2, 5, 32, 300])
@pytest.mark.parametrize("ext_means", [False, True], ids=["own_means", "given_means"])
def test_ragan_loss_vs_torch(hip, B, ext_means):
    """``wsr_ragan_loss`` (ABI 9): the relativistic-average GAN loss of the reference (wind_field_GAN_3D.py:360-364 generator
    term, :552-556 discriminator loss) and all its partial derivatives from one launch, against torch's composed ops
    (``nn.BCEWithLogitsLoss`` on ``u - mean(v)`` / ``v - mean(u)``) and their autograd - with the means taken inside, and
    with batch-global means handed in as differentiable scalars (the data-parallel form)."""
    o = ops()
    g = torch.Generator().manual_seed(B)
    u0, v0 = torch.randn(B, generator=g) * 3, torch.randn(B, generator=g) * 3 + 0.5
    lu = (torch.full((B,), 0.9) + 0.05 * torch.randn(B, generator=g)).clamp(0, 1)
    lv = (0.05 * torch.randn(B, generator=g)).clamp(0, 1)
    crit = torch.nn.BCEWithLogitsLoss()
    w = 1.7  # upstream gradient
    res = {}
    for which in ("torch", "hip"):
        u, v = u0.clone().to(DEV).requires_grad_(True), v0.clone().to(DEV).requires_grad_(True)
        mu_l, mv_l = (u * 1.0).mean() + 0.1, (v * 1.0).mean() - 0.2  # "global" means: functions of the inputs, not THE means
        if which == "torch":
            mu, mv = (mu_l, mv_l) if ext_means else (u.mean(), v.mean())
            loss = (crit(u - mv, lu.to(DEV)) + crit(v - mu, lv.to(DEV))) / 2.0
        else:
            loss = o.ragan_loss(u, v, lu.to(DEV), lv.to(DEV), *((mu_l, mv_l) if ext_means else ()))
        (loss * w).backward()
        res[which] = (float(loss), u.grad.cpu(), v.grad.cpu())
    assert res["hip"][0] == pytest.approx(res["torch"][0], rel=2e-6, abs=1e-7)
    assert rel_l2(res["hip"][1], res["torch"][1]) < 3e-6 and rel_l2(res["hip"][2], res["torch"][2]) < 3e-6
    # 0-d logits (batch 1 squeezed, as the train step has them) and a detached real side
    if B == 1:
        u, v = u0[0].clone().to(DEV).requires_grad_(True), v0[0].clone().to(DEV)
        loss = o.ragan_loss(u, v, lu[0].to(DEV), lv[0].to(DEV))
        loss.backward()
        assert loss.shape == () and u.grad.shape == () and float(loss) == pytest.approx(res["torch"][0], rel=2e-6) or ext_means
