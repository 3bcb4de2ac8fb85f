"""CPU checks of tests/kernel_bounds.py: the float64 references equal float64 autograd, the element-wise bound holds
for CPU emulations of the kernels' arithmetic (not too tight), it rejects small local errors that the whole-tensor
rel-L2 tolerances of the kernel tests accept (not too loose), and guarded buffers report a single stray write."""
import math
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
import kernel_bounds as kb

f64 = torch.float64


def _bf(t):
    return t.bfloat16().float()


# ---- references ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,ups,B", [((3, 3, 3), False, 2), ((5, 5, 5), False, 1), ((3, 3, 3), True, 2),
                                     ((5, 5, 1), False, 2), ((1, 1, 1), False, 2)])
def test_references_equal_float64_autograd(k, ups, B):
    gen = torch.Generator().manual_seed(sum(k) + B + ups)
    cin, cout, ctot, off, xyz = 5, 7, 9, 3, (4, 5, 6)
    pad = tuple(kk // 2 for kk in k)
    xbuf = torch.randn((B, ctot) + xyz, generator=gen, dtype=f64)
    x = xbuf[:, off:off + cin].clone().requires_grad_(True)
    w = torch.randn((cout, cin) + k, generator=gen, dtype=f64).requires_grad_(True)
    bias = torch.randn(cout, generator=gen, dtype=f64)
    xin = kb.up2(x) if ups else x
    y = F.conv3d(xin, w, None, 1, pad)
    res = torch.randn(y.shape, generator=gen, dtype=f64)
    cs = torch.rand((B, cout), generator=gen, dtype=f64)
    # forward with the full epilogue, on windows
    want = 0.3 * F.leaky_relu(y + bias.view(1, -1, 1, 1, 1), 0.2) * cs.view(B, cout, 1, 1, 1) - 0.7 * res
    got, A = kb.ref_fwd(xbuf, w, pad, ups=ups, bias=bias, act=True, chan_scale=cs, alpha=0.3, res=res, beta=-0.7,
                        in_win=(off, cin))
    torch.testing.assert_close(got, want.detach(), rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    # ... on an x slab
    got_s, _ = kb.ref_fwd(x, w, pad, ups=ups, xs=(1, 3))
    torch.testing.assert_close(got_s, y.detach()[:, :, 1:3], rtol=1e-12, atol=1e-12)
    # input gradient, with the LeakyReLU / Dropout3d mask and an accumulated value
    gy = torch.randn(y.shape, generator=gen, dtype=f64)
    (dx,) = torch.autograd.grad(y, x, gy, retain_graph=True)
    h = torch.randn(x.shape, generator=gen, dtype=f64)
    keep = torch.rand((B, cin), generator=gen, dtype=f64)
    acc = torch.randn(x.shape, generator=gen, dtype=f64)
    want = (0.5 * dx + acc) * torch.where(h > 0, 1.0, 0.2) * keep.view(B, cin, 1, 1, 1)
    got, A = kb.ref_dgrad(gy, w, pad, ups=ups, alpha=0.5, mask_y=h, keep=keep, acc=acc)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    if not ups:
        got_s, _ = kb.ref_dgrad(gy, w, pad, xs=(2, 4))
        torch.testing.assert_close(got_s, dx[:, :, 2:4], rtol=1e-12, atol=1e-12)
    # filter gradient
    (dw,) = torch.autograd.grad(y, w, gy)
    got, A = kb.ref_wgrad(xbuf, gy, k, pad, ups=ups, in_win=(off, cin))
    torch.testing.assert_close(got, dw, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())


@pytest.mark.parametrize("k,s,pad,xyz", [((4, 4, 3), (2, 2, 1), (1, 1, 1), (9, 8, 5)),
                                         ((4, 4, 5), (2, 2, 2), (1, 1, 2), (8, 7, 9)),
                                         ((3, 3, 3), (1, 1, 2), (1, 1, 1), (5, 4, 7)),
                                         ((3, 4, 3), (1, 2, 1), (0, 0, 0), (6, 9, 4))])
def test_strided_forward_reference_equals_a_direct_sum(k, s, pad, xyz):
    """``ref_fwd(stride=...)``: every output voxel is the explicit sum over taps at input voxel o * s - pad + tap
    (written out here, without conv3d), A the same over magnitudes, and an x slab is the slab of the whole"""
    gen = torch.Generator().manual_seed(sum(k) + 7 * sum(s))
    B, cin, cout = 2, 3, 4
    x = torch.randn((B, cin) + xyz, generator=gen, dtype=f64)
    w = torch.randn((cout, cin) + k, generator=gen, dtype=f64)
    bias = torch.randn(cout, generator=gen, dtype=f64)
    out = tuple((xyz[i] + 2 * pad[i] - k[i]) // s[i] + 1 for i in range(3))
    xp = F.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    want, mag = torch.zeros((B, cout) + out, dtype=f64), torch.zeros((B, cout) + out, dtype=f64)
    for kx in range(k[0]):
        for ky in range(k[1]):
            for kz in range(k[2]):
                sl = xp[:, :, kx:kx + (out[0] - 1) * s[0] + 1:s[0], ky:ky + (out[1] - 1) * s[1] + 1:s[1],
                        kz:kz + (out[2] - 1) * s[2] + 1:s[2]]
                want += torch.einsum("bcxyz,nc->bnxyz", sl, w[:, :, kx, ky, kz])
                mag += torch.einsum("bcxyz,nc->bnxyz", sl.abs(), w[:, :, kx, ky, kz].abs())
    got, A = kb.ref_fwd(x, w, pad, stride=s)
    assert tuple(got.shape[2:]) == out
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(A, mag, rtol=1e-12, atol=1e-12)
    got_b, A_b = kb.ref_fwd(x, w, pad, stride=s, bias=bias, act=True)
    torch.testing.assert_close(got_b, F.leaky_relu(want + bias.view(1, -1, 1, 1, 1), 0.2), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(A_b, mag + bias.abs().view(1, -1, 1, 1, 1), rtol=1e-12, atol=1e-12)
    got_s, A_s = kb.ref_fwd(x, w, pad, stride=s, xs=(1, out[0]))
    torch.testing.assert_close(got_s, want[:, :, 1:], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(A_s, mag[:, :, 1:], rtol=1e-12, atol=1e-12)


# ---- CPU emulations of the kernels' arithmetic pass the bound ---------------------------------------------------------

def _fp32_tap_order(x, w, pad):
    """fp32 conv summed tap by tap in reverse order (a different fp32 summation order than the CPU conv's)"""
    k = w.shape[2:]
    xp = F.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    out = None
    X, Y, Z = (xp.shape[2 + i] - k[i] + 1 for i in range(3))
    for kx in reversed(range(k[0])):
        for ky in reversed(range(k[1])):
            for kz in reversed(range(k[2])):
                t = torch.einsum("bcxyz,nc->bnxyz", xp[:, :, kx:kx + X, ky:ky + Y, kz:kz + Z], w[:, :, kx, ky, kz])
                out = t if out is None else out + t
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("k,cin,cout", [((3, 3, 3), 32, 24), ((5, 5, 5), 16, 16), ((1, 1, 1), 64, 32)])
def test_bound_holds_for_emulated_kernel_arithmetic(dt, k, cin, cout):
    gen = torch.Generator().manual_seed(cin + cout + k[0])
    B, xyz = 2, (6, 7, 9)
    pad = tuple(kk // 2 for kk in k)
    taps = math.prod(k)
    x = _bf(torch.randn((B, cin) + xyz, generator=gen))
    w = _bf(torch.randn((cout, cin) + k, generator=gen) / math.sqrt(cin * taps))
    res = _bf(torch.randn((B, cout) + xyz, generator=gen))
    rho = kb.rho_for(dt)
    ratios = {}
    # forward + residual epilogue
    y = 0.2 * _fp32_tap_order(x, w, pad) + res
    y = y.to(dt).float()
    ref, A = kb.ref_fwd(x, w, pad, alpha=0.2, res=res, beta=1.0)
    ratios["fwd"] = kb.assert_within(y, ref, kb.bound(ref, A, taps * cin, rho), f"emul fwd {dt}")
    # input gradient
    gy = _bf(torch.randn((B, cout) + xyz, generator=gen))
    dx = _fp32_tap_order(gy, kb.dgrad_filter(w), tuple(kk - 1 - p for kk, p in zip(k, pad))).to(dt).float()
    ref, A = kb.ref_dgrad(gy, w, pad)
    ratios["dgrad"] = kb.assert_within(dx, ref, kb.bound(ref, A, taps * cout, rho), f"emul dgrad {dt}")
    # filter gradient: three fp32 split copies over the voxels, ordered fp32 sum
    n_parts = 3
    parts = []
    for s in range(n_parts):
        g = gy.clone()
        sel = torch.zeros(xyz[0], dtype=torch.bool)
        sel[s::n_parts] = True
        g[:, :, ~sel] = 0
        wv = torch.zeros((cout, cin) + k, requires_grad=True)
        (p,) = torch.autograd.grad(F.conv3d(x, wv, None, 1, pad), wv, g)
        parts.append(p)
    dw = parts[0]
    for p in parts[1:]:
        dw = dw + p
    ref, A = kb.ref_wgrad(x, gy, k, pad)
    ratios["wgrad"] = kb.assert_within(dw, ref, kb.bound(ref, A, B * math.prod(xyz) + n_parts, 0.0),
                                       f"emul wgrad {dt}", kind="filter")
    print("largest |err|/bound:", {n: f"{r:.3g}" for n, r in ratios.items()})
    assert max(ratios.values()) <= 1.0


# ---- small local errors pass the rel-L2 tolerances but fail the bound ---------------------------------------------------

def _fails(got, ref, bnd):
    bad, worst, _, _ = kb.check_within(got, ref, bnd)
    return bad > 0 and worst > 1.0


def test_one_dropped_tap_at_one_voxel_is_caught():
    """bf16 3x3x3 forward, 4 096 voxels: the output at one tile corner misses one tap.  The old check
    (rel-L2 < 4e-3 against the fp32 conv of the same bf16 operands) accepts it; the bound does not, and it names the
    voxel."""
    gen = torch.Generator().manual_seed(7)
    cin = cout = 16
    xyz, pad = (16, 16, 16), (1, 1, 1)
    x = _bf(torch.randn((1, cin) + xyz, generator=gen))
    w = _bf(torch.randn((cout, cin, 3, 3, 3), generator=gen) / math.sqrt(cin * 27))
    y32 = F.conv3d(x, w, None, 1, pad)
    v = (7, 7, 15)  # corner of an 8 x 8 x 16 tile
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))[0]
    contribs = [torch.einsum("c,nc->n", xp[:, v[0] + t // 9, v[1] + t // 3 % 3, v[2] + t % 3], w[:, :, t // 9, t // 3 % 3, t % 3])
                for t in range(27)]
    norms = torch.stack([c.norm() for c in contribs])
    contrib = contribs[int(norms.argsort()[13])]  # the tap of median weight at that voxel
    bad = y32.clone()
    bad[0, :, v[0], v[1], v[2]] -= contrib
    bad = _bf(bad)
    assert rel_l2(bad, y32) < 4e-3  # the blind spot of the old tolerance
    ref, A = kb.ref_fwd(x, w, pad)
    bnd = kb.bound(ref, A, 27 * cin, kb.RHO_BF16)
    kb.assert_within(_bf(y32), ref, bnd, "unmutated")
    assert _fails(bad, ref, bnd)
    with pytest.raises(AssertionError, match=r"x=7, y=7, z=15"):
        kb.assert_within(bad, ref, bnd, "dropped tap")


def test_one_filter_gradient_element_off_by_1e3_relative_is_caught():
    """one element of an fp32 filter gradient off by 1e-3 of its value passes rel-L2 < 2e-5 but not the bound"""
    gen = torch.Generator().manual_seed(3)
    cin = cout = 16
    B, xyz, k, pad = 2, (6, 6, 8), (3, 3, 3), (1, 1, 1)
    x = _bf(torch.randn((B, cin) + xyz, generator=gen))
    gy = _bf(torch.randn((B, cout) + xyz, generator=gen))
    ref, A = kb.ref_wgrad(x, gy, k, pad)
    dw = ref.float()
    flat = dw.view(-1)
    i = int((flat.abs() - flat.abs().square().mean().sqrt()).abs().argmin())  # an element of typical size
    flat[i] *= 1 + 1e-3
    assert rel_l2(dw, ref) < 2e-5
    bnd = kb.bound(ref, A, B * math.prod(xyz), 0.0)
    kb.assert_within(ref.float(), ref, bnd, "unmutated", kind="filter")
    assert _fails(dw, ref, bnd)
    n, c = i // (cin * 27), (i // 27) % cin
    with pytest.raises(AssertionError, match=rf"n={n}, tap={i % 27}, c={c}\)"):
        kb.assert_within(dw, ref, bnd, "off by 1e-3", kind="filter")


def test_one_voxel_missing_from_one_split_is_caught():
    """deterministic split form of a 64 -> 64 3x3x3 filter gradient (B = 2, ragged z extent 14: the last tile of 4
    z-levels holds 2): split 1's partial sum lacks the product of the last voxel of a ragged last tile for one
    (n, tap, c).  The ordered sum passes rel-L2 < 2e-5; the bound names the element."""
    gen = torch.Generator().manual_seed(5)
    cin = cout = 64
    B, xyz, k, pad = 2, (8, 16, 14), (3, 3, 3), (1, 1, 1)
    x = _bf(torch.randn((B, cin) + xyz, generator=gen))
    gy = _bf(torch.randn((B, cout) + xyz, generator=gen))
    n_parts = 3
    tiles_z = torch.arange(xyz[2]) // 4  # z tiles of 4 levels, dealt round-robin to the splits
    parts = []
    for s in range(n_parts):
        g = gy.clone()
        g[..., tiles_z % n_parts != s] = 0
        wv = torch.zeros((cout, cin) + k, requires_grad=True)
        (p,) = torch.autograd.grad(F.conv3d(x, wv, None, 1, pad), wv, g)
        parts.append(p)
    ref, A = kb.ref_wgrad(x, gy, k, pad)
    bnd = kb.bound(ref, A, B * math.prod(xyz) + n_parts, 0.0)
    # the last voxel of the ragged last z tile (z = 13, tile 3 -> split 0) of sample 1: the product it adds at
    # (n, tap, c) = gy[1, n, v] * x[1, c, v + tap - 1]; take the (n, c, tap) with the product nearest 0.3
    s_bad = int(tiles_z[-1]) % n_parts
    v = (3, 9, 13)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))[1]
    best = None
    for t in range(27):
        kx, ky, kz = t // 9, (t // 3) % 3, t % 3
        prod = torch.outer(gy[1, :, v[0], v[1], v[2]], xp[:, v[0] + kx, v[1] + ky, v[2] + kz])
        if prod.abs().max() == 0:
            continue
        j = int((prod.abs() - 0.3).abs().argmin())
        cand = (abs(float(prod.view(-1)[j]) - 0.3), t, j // cin, j % cin, float(prod.view(-1)[j]))
        best = cand if best is None or cand < best else best
    _, t, n, c, p = best
    parts[s_bad][n, c, t // 9, (t // 3) % 3, t % 3] -= p
    dw = parts[0]
    for q in parts[1:]:
        dw = dw + q
    assert rel_l2(dw, ref) < 2e-5
    assert _fails(dw, ref, bnd)
    with pytest.raises(AssertionError, match=rf"n={n}, tap={t}, c={c}\)"):
        kb.assert_within(dw, ref, bnd, "missing voxel", kind="filter")


# ---- guards --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_guards_report_a_single_stray_write(dt):
    shape, win = (2, 3, 4, 5, 24), (8, 12)
    g = kb.Guarded(shape, dt, "cpu", window=win, fill=1.0)
    assert bool((g.window_view() == 1.0).all())
    g.window_view().fill_(2.0)  # writes inside the window are the kernel's business
    kb.assert_guards_intact(g, label="clean")
    if dt == torch.float32:
        assert torch.isnan(g.t[..., :8]).all()
    else:
        assert torch.isfinite(g.t[..., :8].float()).all() and bool((g.t[..., :8] != 0).all())
    # one channel outside the window
    g.t[1, 2, 3, 4, 20] = 0.0
    with pytest.raises(AssertionError, match=r"index \(1, 2, 3, 4, 20\) outside the channel window"):
        kb.assert_guards_intact(g, label="window")
    # one element past the end / in front of the tensor
    for where, pos in (("past its end", g.guard + g.t.numel() + 17), ("before the tensor", g.guard - 3)):
        h = kb.Guarded(shape, dt, "cpu")
        kb.assert_guards_intact(h)
        h.base[pos] = 1.0
        with pytest.raises(AssertionError, match=where):
            kb.assert_guards_intact(h)
    # a sentinel NaN re-written as another NaN is a write too (bit-for-bit comparison)
    if dt == torch.float32:
        h = kb.Guarded(shape, dt, "cpu")
        h.base[5] = float("nan")
        with pytest.raises(AssertionError):
            kb.assert_guards_intact(h)


# ---- the streaming 1x1x1 kernel's epilogue: a subtly wrong kernel fails the bound of ref_pointwise ---------------------

def _bits(v):
    """bf16 scalar from its bit pattern"""
    return torch.tensor([v - 65536 if v >= 32768 else v], dtype=torch.int16).view(torch.bfloat16)[0]


NEG_ZERO, POS_SUB, NEG_SUB = 0x8000, 0x0001, 0x8001


class _Stream:
    """an accumulating masked 128 -> 256 input gradient on 665 voxels (42 strips of 16, the last holds 9), every
    epilogue term in use: dx = alpha * dy @ W + beta * acc[:, :128] + beta2 * res2[:, :128], columns [224, 256)
    masked by the sign of columns [8, 40) of a saved output.  ``emul`` is the kernel's arithmetic in fp32 (accumulator
    start bias + beta/alpha * res + beta2/alpha * res2, final * alpha, mask, one bf16 store) with switches for the
    mistakes a kernel could make."""
    nvox, red, n_out, c1, y_off, win = 665, 128, 256, 128, 8, (224, 256)
    alpha, beta, beta2, slope = 0.2 * 0.3, 0.3, 1.0, 0.2

    def __init__(self):
        gen = torch.Generator().manual_seed(41)
        self.dy = _bf(torch.randn(self.nvox, self.red, generator=gen))
        self.w = _bf(torch.randn(self.n_out, self.red, generator=gen) / math.sqrt(self.red))
        self.acc = _bf(torch.randn(self.nvox, self.n_out, generator=gen))    # dx's layout: the buffer's old contents
        self.res2 = _bf(torch.randn(self.nvox, self.n_out, generator=gen))
        self.y = torch.randn(self.nvox, 48, generator=gen).bfloat16()
        plain = self.dy @ self.w.T
        # (-0.0 and a positive subnormal where the unmasked value is large: a wrong classification must show)
        self.v0, self.v1 = 37, 650
        self.j0 = int(plain[self.v0, self.win[0]:].abs().argmax())
        self.j1 = int(plain[self.v1, self.win[0]:].abs().argmax())
        self.y[self.v0, self.y_off + self.j0] = _bits(NEG_ZERO)
        self.y[self.v1, self.y_off + self.j1] = _bits(POS_SUB)
        self.y[5, self.y_off + 3] = _bits(NEG_SUB)
        self.y[6, self.y_off + 4] = 0.0
        my = self.y[:, self.y_off:self.y_off + 32]
        assert bool(my[self.v1, self.j1].double() > 0) and not bool(my[self.v0, self.j0].double() > 0)
        self.ref, self.A = kb.ref_pointwise(self.dy, self.w, alpha=self.alpha, res=self.acc, beta=self.beta,
                                            res_c1=self.c1, res2=self.res2, beta2=self.beta2, mask_y=my,
                                            mask_win=self.win, mask_slope=self.slope)
        self.bnd = kb.bound(self.ref, self.A, self.red + 3, kb.RHO_BF16)

    def emul(self, *, res_c1=None, res2_c1=None, beta=None, beta2=None, win=None, y_off=None, flip=()):
        f = lambda v: torch.tensor(float(v), dtype=torch.float32)
        c1 = self.c1 if res_c1 is None else res_c1
        c2 = self.c1 if res2_c1 is None else res2_c1
        alpha = f(self.alpha)
        rs1 = f(self.beta if beta is None else beta) / alpha
        rs2 = f(self.beta2 if beta2 is None else beta2) / alpha
        start = torch.zeros(self.nvox, self.n_out)
        start[:, :c1] += rs1 * self.acc[:, :c1]
        start[:, :c2] += rs2 * self.res2[:, :c2]
        out = (start + self.dy @ self.w.T) * alpha
        m0, m1 = self.win if win is None else win
        yo = self.y_off if y_off is None else y_off
        pos = self.y[:, yo:yo + (m1 - m0)].float() > 0
        for v, j in flip:
            pos[v, j] = ~pos[v, j]
        out[:, m0:m1] *= torch.where(pos, torch.ones(()), f(self.slope))
        return _bf(out)

    def violations(self, got):
        _, _, _, ratio = kb.check_within(got, self.ref, self.bnd)
        return {(int(v), int(c)) for v, c in (ratio > 1.0).nonzero().tolist()}


@pytest.fixture(scope="module")
def stream():
    return _Stream()


def test_ref_pointwise_equals_the_1x1x1_conv_references():
    """on a 1x1x1 conv ``ref_pointwise`` is ``ref_fwd`` / ``ref_dgrad`` of the same operands (scalars exact in fp32:
    ``ref_pointwise`` takes them as the C side receives them)"""
    gen = torch.Generator().manual_seed(9)
    B, cin, cout, xyz = 2, 12, 7, (3, 4, 5)
    x = torch.randn((B, cin) + xyz, generator=gen, dtype=f64)
    w = torch.randn((cout, cin, 1, 1, 1), generator=gen, dtype=f64)
    bias = torch.randn(cout, generator=gen, dtype=f64)
    res = torch.randn((B, cout) + xyz, generator=gen, dtype=f64)
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
    want, wa = kb.ref_fwd(x, w, (0, 0, 0), bias=bias, act=True, slope=0.25, alpha=0.5, res=res, beta=0.25)
    got, ga = kb.ref_pointwise(rows(x), w.view(cout, cin), bias=bias, act=True, slope=0.25, alpha=0.5,
                               res=rows(res), beta=0.25)
    torch.testing.assert_close(got, rows(want), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ga, rows(wa), rtol=1e-12, atol=1e-12)
    gy = torch.randn((B, cout) + xyz, generator=gen, dtype=f64)
    h = torch.randn((B, cin) + xyz, generator=gen, dtype=f64)
    acc = torch.randn((B, cin) + xyz, generator=gen, dtype=f64)
    want, wa = kb.ref_dgrad(gy, w, (0, 0, 0), alpha=0.5, mask_y=h, slope=0.25, acc=acc)
    got, ga = kb.ref_pointwise(rows(gy), w.view(cout, cin).T, alpha=0.5, res=rows(acc), beta=1.0, mask_y=rows(h),
                               mask_win=(0, cin), mask_slope=0.25)
    torch.testing.assert_close(got, rows(want), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ga, rows(wa), rtol=1e-12, atol=1e-12)
    # partial residuals, a mask window, scalars as fp32
    r2 = torch.randn((B * math.prod(xyz), cin), generator=gen, dtype=f64)
    got, _ = kb.ref_pointwise(rows(gy), w.view(cout, cin).T, alpha=0.3, res=rows(acc), beta=0.7, res_c1=8, res2=r2,
                              beta2=0.1, mask_y=rows(h)[:, :4], mask_win=(8, 12), mask_slope=0.2)
    a32, b32, c32, s32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.3, 0.7, 0.1, 0.2))
    want = a32 * rows(gy) @ w.view(cout, cin)
    want[:, :8] += b32 * rows(acc)[:, :8] + c32 * r2[:, :8]
    want[:, 8:12] *= torch.where(rows(h)[:, :4] > 0, 1.0, s32)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_stream_emulation_is_within_the_bound(stream):
    worst = kb.assert_within(stream.emul(), stream.ref, stream.bnd, "emul stream 1x1x1")
    assert worst <= 1.0 and not stream.violations(stream.emul())


def _rejected(s, got, region, min_hits, label):
    """``got`` violates the bound inside ``region`` (a predicate on (voxel, column)) only, at >= ``min_hits`` elements,
    and the assertion's message names elements of it"""
    bad = s.violations(got)
    assert len(bad) >= min_hits, (label, len(bad))
    assert all(region(v, c) for v, c in bad), (label, sorted(bad)[:5])
    with pytest.raises(AssertionError) as e:
        kb.assert_within(got, s.ref, s.bnd, label)
    # (the message lists the five worst elements with their ratios: those above 1 are the violations it names)
    named = [(int(v), int(c)) for v, c, q in
             re.findall(r"^\s+\((\d+), (\d+)\):.* ratio (\S+)$", str(e.value), flags=re.M) if float(q) > 1.0]
    assert named and all(region(v, c) for v, c in named), (label, str(e.value))
    return named


STREAM_MUTATIONS = {  # name -> (emul switches, region of the wrong elements, least number of violations)
    "res_on_8_channels_too_many": (dict(res_c1=136), lambda v, c: 128 <= c < 136, 665 * 8 * 9 // 10),
    "res2_past_res_c1": (dict(res2_c1=256), lambda v, c: c >= 128, 665 * 128 * 9 // 10),
    "res2_dropped": (dict(beta2=0.0), lambda v, c: c < 128, 665 * 128 * 9 // 10),
    "mask_window_shifted_by_8": (dict(win=(216, 248)), lambda v, c: c >= 216, 665 * 8),
    "mask_read_at_y_off_plus_8": (dict(y_off=16), lambda v, c: c >= 224, 665 * 32 // 4),
    "acc_beta_ignored": (dict(beta=1.0), lambda v, c: c < 128, 665 * 128 * 9 // 10),
}


@pytest.mark.parametrize("name", list(STREAM_MUTATIONS))
def test_stream_epilogue_mutation_is_caught(stream, name):
    kw, region, min_hits = STREAM_MUTATIONS[name]
    _rejected(stream, stream.emul(**kw), region, min_hits, name)


@pytest.mark.parametrize("which", ["negative_zero_taken_as_positive", "positive_subnormal_taken_as_not_positive"])
def test_stream_mask_sign_of_special_values_is_caught(stream, which):
    s = stream
    v, j = (s.v0, s.j0) if which.startswith("negative") else (s.v1, s.j1)
    named = _rejected(s, s.emul(flip=[(v, j)]), lambda vv, c: (vv, c) == (v, s.win[0] + j), 1, which)
    assert named[0] == (v, s.win[0] + j)


def test_stream_exchanged_strips_are_caught(stream):
    s = stream
    got = s.emul()
    a, b = got[48:64].clone(), got[320:336].clone()  # strips 3 and 20
    got[48:64], got[320:336] = b, a
    _rejected(s, got, lambda v, c: 48 <= v < 64 or 320 <= v < 336, 32 * 256 * 9 // 10, "strips exchanged")


def test_stream_stale_tail_is_caught(stream):
    s = stream
    got = s.emul()
    tail = s.nvox - s.nvox % 16
    assert s.nvox % 16 == 9
    got[tail:] = s.acc[tail:]  # the last strip's voxels keep the buffer's old contents
    _rejected(s, got, lambda v, c: v >= tail, 9 * 256 * 9 // 10, "stale tail")


# ---- the stride-1 halo-tile kernel's further epilogue forms (ref_fwd / ref_dgrad keyword forms) ------------------------

def test_tile_reference_forms_equal_a_direct_composition():
    """each keyword form of ``ref_fwd`` / ``ref_dgrad`` against float64 autograd and plain torch ops written out here;
    the defaults still give the earlier result bit for bit"""
    gen = torch.Generator().manual_seed(23)
    B, cin, cout, xyz, k, pad = 2, 6, 12, (4, 5, 6), (3, 3, 3), (1, 1, 1)
    bc = lambda t: t.view(1, -1, 1, 1, 1)
    x = torch.randn((B, cin) + xyz, generator=gen, dtype=f64).requires_grad_(True)
    w = torch.randn((cout, cin) + k, generator=gen, dtype=f64)
    bias = torch.randn(cout, generator=gen, dtype=f64)
    y = F.conv3d(x, w, None, 1, pad)
    res = torch.randn(y.shape, generator=gen, dtype=f64)
    cs = torch.rand((B, cout), generator=gen, dtype=f64).view(B, cout, 1, 1, 1)
    yd = y.detach()
    # act_c1: bias + LeakyReLU below it, raw sums from it on; residual after
    want = torch.cat([F.leaky_relu(yd[:, :4] + bc(bias[:4]), 0.1), yd[:, 4:]], 1) * cs * 0.3 + 0.7 * res
    got, A = kb.ref_fwd(x, w, pad, bias=bias, act=True, slope=0.1, chan_scale=cs, alpha=0.3, res=res, beta=0.7, act_c1=4)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    # act2: the residual joins in front of the activation; with act_c1 < Cout the rest is conv + beta * res
    want = 0.3 * F.leaky_relu(yd + bc(bias) - 0.7 * res, 0.1)
    got, A = kb.ref_fwd(x, w, pad, bias=bias, slope=0.1, alpha=0.3, res=res, beta=-0.7, act2=True)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    want = torch.cat([F.leaky_relu(yd[:, :8] + bc(bias[:8]) + res[:, :8], 0.1), yd[:, 8:] + res[:, 8:]], 1)
    got, _ = kb.ref_fwd(x, w, pad, bias=bias, slope=0.1, res=res, beta=1.0, act2=True, act_c1=8)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # forward-form mask on a channel window, last
    h = torch.randn((B, 4) + xyz, generator=gen, dtype=f64)
    want = F.leaky_relu(yd + bc(bias), 0.1) + 0.5 * res
    want[:, 4:8] *= torch.where(h > 0, 1.0, 0.25)
    got, A = kb.ref_fwd(x, w, pad, bias=bias, act=True, slope=0.1, res=res, beta=0.5, mask_y=h, mask_win=(4, 8),
                        mask_slope=0.25)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    # input gradient: partial accumulate with its own weight, mask on a sub-window
    gy = torch.randn(y.shape, generator=gen, dtype=f64)
    (dx,) = torch.autograd.grad(y, x, gy)
    acc = torch.randn(dx.shape, generator=gen, dtype=f64)
    hm = torch.randn((B, 2) + xyz, generator=gen, dtype=f64)
    want = 0.5 * dx
    want[:, :4] += 0.3 * acc[:, :4]
    want[:, 2:4] *= torch.where(hm > 0, 1.0, 0.2)
    got, A = kb.ref_dgrad(gy, w, pad, alpha=0.5, acc=acc, acc_c1=4, acc_beta=0.3, mask_y=hm, mask_win=(2, 4))
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((A >= got.abs() - 1e-12).all())
    # keep together with a mask, in the kernel's order: equal to the earlier order (it commutes without acc)
    hf = torch.randn(dx.shape, generator=gen, dtype=f64)
    keep = torch.rand((B, cin), generator=gen, dtype=f64)
    keep[0, 1] = keep[1, 4] = 0.0
    got, A = kb.ref_dgrad(gy, w, pad, alpha=0.5, mask_y=hf, keep=keep, mask_win=(0, cin))
    old, A_old = kb.ref_dgrad(gy, w, pad, alpha=0.5, mask_y=hf, keep=keep)
    torch.testing.assert_close(got, 0.5 * dx * torch.where(hf > 0, 1.0, 0.2) * keep.view(B, cin, 1, 1, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got, old, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(A, A_old, rtol=1e-12, atol=1e-12)
    with pytest.raises(AssertionError, match="keep together with an accumulate"):
        kb.ref_dgrad(gy, w, pad, mask_y=hf, keep=keep, acc=acc, mask_win=(0, cin))
    # the mask's sign convention on the special values
    sp = torch.tensor([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -126, -3e38, 1e-45, -1e-45], dtype=torch.float32)
    assert kb._lrelu_mask(sp, 0.25).tolist() == [0.25, 0.25, 1.0, 0.25, 1.0, 0.25, 1.0, 0.25]


class _TileForms:
    """the halo-tile epilogue forms on a 3x3x3 conv over (5, 6, 9) voxels, B = 2, with fp32 emulations of the kernel's
    arithmetic (fp32 conv of the bf16-exact operands, the epilogue of conv_tile_impl.h :679-713 in fp32, one bf16 store)
    that carry a switch for each mistake a kernel could make.

    fwd1: 16 -> 32, bias + LeakyReLU below act_c1 = 16, channel scale, alpha, residual.   fwd2: the same conv, act = 2.
    dg1: produced 32 <- reduction 16, accumulate below acc_c1 = 16 with acc_beta = 0.5, mask on [8, 24).
    dg2: the same gradient with keep (zeros among it) and the mask on all 32 channels."""
    B, xyz, cin, cout, c1 = 2, (5, 6, 9), 16, 32, 16
    alpha, beta, slope, acc_beta, mslope = 0.7, 0.3, 0.2, 0.5, 0.2
    acc_c1, win = 16, (8, 24)

    def __init__(self):
        gen = torch.Generator().manual_seed(57)
        B, xyz, cin, cout = self.B, self.xyz, self.cin, self.cout
        r = lambda *s: _bf(torch.randn(*s, generator=gen))
        self.x, self.w = r((B, cin) + xyz), _bf(torch.randn((cout, cin, 3, 3, 3), generator=gen) / math.sqrt(27 * cin))
        self.bias, self.res = r(cout), r((B, cout) + xyz)
        self.cs = _bf(torch.rand((B, cout), generator=gen) + 0.5)
        f = kb._f32
        self.fwd1 = kb.ref_fwd(self.x, self.w, (1, 1, 1), bias=self.bias, act=True, slope=f(self.slope), chan_scale=self.cs,
                               alpha=f(self.alpha), res=self.res, beta=f(self.beta), act_c1=self.c1)
        self.fwd2 = kb.ref_fwd(self.x, self.w, (1, 1, 1), bias=self.bias, slope=f(self.slope), alpha=f(self.alpha),
                               res=self.res, beta=f(self.beta), act2=True, act_c1=self.c1)
        # input gradient of a conv 32 -> 16: produced channels 32, reduction 16
        self.gy, self.wd = r((B, cin) + xyz), _bf(torch.randn((cin, cout, 3, 3, 3), generator=gen) / math.sqrt(27 * cin))
        self.acc = r((B, cout) + xyz)
        self.y = torch.randn((B, cout) + xyz, generator=gen).bfloat16()
        self.keep = _bf(torch.rand((B, cout), generator=gen) + 0.5)
        self.keep[0, 5] = self.keep[1, 20] = self.keep[1, 31] = 0.0
        plain = F.conv3d(self.gy, kb.dgrad_filter(self.wd), None, 1, 1)
        # -0.0 and a positive subnormal inside the window [8, 24), where the unmasked value is large
        m0, m1 = self.win
        mag = (plain[:, m0:m1] + self.acc_beta * torch.cat([self.acc[:, m0:self.acc_c1],
                                                            torch.zeros_like(self.acc[:, self.acc_c1:m1])], 1)).abs()
        i0 = int(mag[0].argmax())
        i1 = int(mag[1].argmax())
        self.e0 = (0,) + tuple(int(v) for v in np_unravel(i0, mag[0].shape))
        self.e1 = (1,) + tuple(int(v) for v in np_unravel(i1, mag[1].shape))
        self.y[self.e0[0], m0 + self.e0[1], self.e0[2], self.e0[3], self.e0[4]] = _bits(NEG_ZERO)
        self.y[self.e1[0], m0 + self.e1[1], self.e1[2], self.e1[3], self.e1[4]] = _bits(POS_SUB)
        self.dg1 = kb.ref_dgrad(self.gy, self.wd, (1, 1, 1), alpha=f(self.alpha), acc=self.acc, acc_c1=self.acc_c1,
                                acc_beta=f(self.acc_beta), mask_y=self.y[:, m0:m1], slope=f(self.mslope), mask_win=self.win)
        self.dg2 = kb.ref_dgrad(self.gy, self.wd, (1, 1, 1), alpha=f(self.alpha), mask_y=self.y, slope=f(self.mslope),
                                keep=self.keep, mask_win=(0, cout))

    def bound(self, form, extra=0):
        ref, A = getattr(self, form)
        return kb.bound(ref, A, 27 * self.cin + extra, kb.RHO_BF16)

    def emul_fwd(self, *, act2=False, act_c1=None, bias_c1=None, res_after=False):
        t = lambda v: torch.tensor(float(v), dtype=torch.float32)
        bc = lambda v: v.view(1, -1, 1, 1, 1)
        ac1 = self.c1 if act_c1 is None else act_c1
        bias = self.bias.clone()
        bias[self.c1 if bias_c1 is None else bias_c1:] = 0.0
        v = F.conv3d(self.x, self.w, None, 1, 1) + bc(bias)
        if act2 and not res_after:
            v = v + t(self.beta) * self.res
        v = torch.cat([torch.where(v[:, :ac1] > 0, v[:, :ac1], v[:, :ac1] * t(self.slope)), v[:, ac1:]], 1)
        if act2:  # (res_after: the join moved behind the activation, everything else as the kernel has it)
            return _bf((v + t(self.beta) * self.res if res_after else v) * t(self.alpha))
        v = v * (self.cs.view(self.B, self.cout, 1, 1, 1) * t(self.alpha))
        return _bf(v + t(self.beta) * self.res)

    def emul_dgrad(self, *, keep=False, no_keep=False, acc_c1=None, win=None, znext=False, flip=()):
        t = lambda v: torch.tensor(float(v), dtype=torch.float32)
        v = F.conv3d(self.gy, kb.dgrad_filter(self.wd), None, 1, 1)
        if keep:
            scale = torch.ones_like(self.keep) if no_keep else self.keep
            v = v * (scale.view(self.B, self.cout, 1, 1, 1) * t(self.alpha))
            m0, m1 = 0, self.cout
        else:
            v = v * t(self.alpha)
            c1 = self.acc_c1 if acc_c1 is None else acc_c1
            v[:, :c1] += t(self.acc_beta) * self.acc[:, :c1]
            m0, m1 = self.win if win is None else win
        # the mask source stays where the caller put it: a kernel that moves its window reads the row at (c - its c0)
        y0 = 0 if keep else self.win[0]
        ys = self.y[:, y0:y0 + (m1 - m0)].float()
        if znext:
            ys = torch.roll(ys, -1, dims=4)
        pos = ys > 0
        for e in flip:
            pos[e] = ~pos[e]
        v[:, m0:m1] *= torch.where(pos, torch.ones(()), t(self.mslope))
        return _bf(v)

    def violations(self, got, form, extra=0):
        ref, _ = getattr(self, form)
        _, _, _, ratio = kb.check_within(got, ref, self.bound(form, extra))
        return {tuple(int(i) for i in e) for e in (ratio > 1.0).nonzero().tolist()}


def np_unravel(i, shape):
    out = []
    for s in reversed(shape):
        out.append(i % s)
        i //= s
    return tuple(reversed(out))


@pytest.fixture(scope="module")
def tile_forms():
    return _TileForms()


def test_tile_form_emulations_are_within_the_bound(tile_forms):
    s = tile_forms
    runs = {"fwd1": (s.emul_fwd(), 0), "fwd2": (s.emul_fwd(act2=True), 1), "dg1": (s.emul_dgrad(), 1),
            "dg2": (s.emul_dgrad(keep=True), 0)}
    for form, (got, extra) in runs.items():
        ref, _ = getattr(s, form)
        assert kb.assert_within(got, ref, s.bound(form, extra), f"emul tile {form}") <= 1.0
    # K-step shares (WK = 4): four partial fp32 sums over the taps meet in share order
    parts = [F.conv3d(s.gy, kb.dgrad_filter(s.wd) * sel.view(1, 1, 3, 3, 3), None, 1, 1)
             for sel in (torch.arange(27) % 4 == q for q in range(4))]
    v = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    ref, A = kb.ref_dgrad(s.gy, s.wd, (1, 1, 1))
    assert kb.assert_within(_bf(v), ref, kb.bound(ref, A, 27 * s.cin + 4, kb.RHO_BF16), "emul tile WK=4") <= 1.0


N_VOX = 2 * 5 * 6 * 9
TILE_MUTATIONS = {  # name -> (form, K extra, emulation switches, region of the wrong elements (b, c, x, y, z), least hits)
    "activation_past_act_c1": ("fwd1", 0, "fwd", dict(act_c1=32), lambda e: e[1] >= 16, N_VOX * 16 // 4),
    "bias_past_act_c1": ("fwd1", 0, "fwd", dict(bias_c1=32), lambda e: e[1] >= 16, N_VOX * 16 * 8 // 10),
    "act2_res_after_the_activation": ("fwd2", 1, "fwd", dict(act2=True, res_after=True), lambda e: e[1] < 16,
                                      N_VOX * 16 // 4),
    "accumulate_past_acc_c1": ("dg1", 1, "dgrad", dict(acc_c1=20), lambda e: 16 <= e[1] < 20, N_VOX * 4 * 8 // 10),
    "mask_window_shifted_by_4": ("dg1", 1, "dgrad", dict(win=(12, 28)), lambda e: 8 <= e[1] < 28, N_VOX * 8 // 4),
    "mask_from_the_next_voxel_along_z": ("dg1", 1, "dgrad", dict(znext=True), lambda e: 8 <= e[1] < 24, N_VOX * 16 // 4),
    "keep_dropped": ("dg2", 0, "dgrad", dict(keep=True, no_keep=True), lambda e: True, N_VOX * 3),
}


def _tile_rejected(s, got, form, extra, region, min_hits, label):
    bad = s.violations(got, form, extra)
    assert len(bad) >= min_hits, (label, len(bad))
    assert all(region(e) for e in bad), (label, sorted(bad)[:5])
    ref, _ = getattr(s, form)
    with pytest.raises(AssertionError) as ei:
        kb.assert_within(got, ref, s.bound(form, extra), label)
    named = [tuple(int(v) for v in m[:5]) for m in
             re.findall(r"^\s+\(b=(\d+), c=(\d+), x=(\d+), y=(\d+), z=(\d+)\):.* ratio (\S+)$", str(ei.value), flags=re.M)
             if float(m[5]) > 1.0]
    assert named and all(region(e) for e in named), (label, str(ei.value))
    return named


@pytest.mark.parametrize("name", list(TILE_MUTATIONS))
def test_tile_epilogue_mutation_is_caught(tile_forms, name):
    form, extra, which, kw, region, min_hits = TILE_MUTATIONS[name]
    s = tile_forms
    got = s.emul_fwd(**kw) if which == "fwd" else s.emul_dgrad(**kw)
    if name == "keep_dropped":  # every channel whose keep factor is not 1 is wrong; the dropped ones (keep = 0) certainly
        zero = {(0, 5), (1, 20), (1, 31)}
        bad = s.violations(got, form, extra)
        assert {(e[0], e[1]) for e in bad} >= zero
        region = lambda e: float(s.keep[e[0], e[1]]) != 1.0
    _tile_rejected(s, got, form, extra, region, min_hits, name)


@pytest.mark.parametrize("which", ["negative_zero_taken_as_positive", "positive_subnormal_taken_as_not_positive"])
def test_tile_mask_sign_of_special_values_is_caught(tile_forms, which):
    s = tile_forms
    e = s.e0 if which.startswith("negative") else s.e1
    at = (e[0], s.win[0] + e[1]) + e[2:]
    named = _tile_rejected(s, s.emul_dgrad(flip=[e]), "dg1", 1, lambda q: q == at, 1, which)
    assert named[0] == at


# ---- completeness of tests/test_conv_tile_matrix.py -------------------------------------------------------------------

STRIDE1_UNITS = ("narrow", "narrow_masked", "n128", "n144", "wide", "masked", "small", "tm3", "simple_narrow",
                 "simple_n128", "simple_small", "f32", "f32_wide", "f32_masked")


def _launch_ct_instantiations(src):
    """every ``launch_ct<...>`` of a translation unit as (WM, WN, TM, TN, TPK, MASK, F32, WK, SIMPLE), a ``TPK``
    argument expanded over the ``run<n>`` its dispatcher calls and narrowed by an enclosing ``if constexpr (TPK == 2)``"""
    src = re.sub(r"//[^\n]*", "", src)
    dispatched = sorted({int(n) for n in re.findall(r"\brun<(\d)>\(", src)})
    only2 = []  # character ranges of `if constexpr (TPK == 2) { ... }` blocks
    for m in re.finditer(r"if constexpr \(TPK == 2\) \{", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        only2.append((m.end(), i))
    out = set()
    for m in re.finditer(r"launch_ct<([^>]*)>\(", src):
        args = [a.strip() for a in m.group(1).split(",")]
        args += ["false", "BF16", "1", "0"][len(args) - 5:]
        assert len(args) == 9, m.group(0)
        tpks = [int(args[4])] if args[4].isdigit() else dispatched
        if args[4] == "TPK" and any(lo <= m.start() < hi for lo, hi in only2):
            tpks = [t for t in tpks if t == 2]
        assert tpks, m.group(0)
        word = {"true": 1, "false": 0, "BF16": 0, "F32": 1}
        for t in tpks:
            v = [int(a) if a.isdigit() else word[a] for a in args[:4] + [str(t)] + args[5:]]
            out.add(tuple(v))
    return out


def test_every_stride1_instantiation_has_a_matrix_row_or_a_reason():
    """the ``launch_ct<...>`` of the stride-1 translation units, read from the sources, are exactly the instantiations
    test_conv_tile_matrix.py names: a row that reaches it, or an entry of UNREACHABLE that says why none can"""
    import os

    import test_conv_tile_matrix as mx

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan_sr_wind_field_amd", "csrc")
    in_src = {}
    for unit in STRIDE1_UNITS:
        with open(os.path.join(csrc, f"conv_tile_{unit}.hip")) as f:
            for inst in _launch_ct_instantiations(f.read()):
                in_src.setdefault(inst, []).append(unit)
    units = {n[len("conv_tile_"):-len(".hip")] for n in os.listdir(csrc) if n.startswith("conv_tile_") and n.endswith(".hip")}
    assert units - {"strided"} == set(STRIDE1_UNITS), "a new conv_tile_*.hip: add it to STRIDE1_UNITS and to the matrix"
    assert in_src and all(len(u) == 1 for u in in_src.values()), "an instantiation in two translation units"
    rows = {r[8] for r in mx.INSTANTIATION_ROWS}
    named = rows | set(mx.UNREACHABLE)
    missing = {i: u for i, u in in_src.items() if i not in named}
    assert not missing, f"instantiations without a row in test_conv_tile_matrix.py: {missing}"
    assert not named - set(in_src), f"rows that name an instantiation the sources do not hold: {sorted(named - set(in_src))}"
    assert not rows & set(mx.UNREACHABLE)


# ---- BatchNorm: references, fp32 emulations of every kernel in its own order, and the mistakes they must not hide ----------

def test_bn_references_equal_float64_autograd():
    """the chain sums -> mean -> shifted sums -> finalize -> apply -> backward sums -> dx of the BatchNorm references is
    ``F.batch_norm`` (training) + ``F.leaky_relu`` under float64 autograd; two ordered running-statistics updates are
    ``nn.BatchNorm3d`` called twice.  (Scalars exact in fp32: the references take them as the C side receives them.)"""
    gen = torch.Generator().manual_seed(11)
    B, C, xyz = 2, 6, (4, 4, 8)
    eps, mom, slope = 2.0 ** -17, 0.125, 0.25
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
    gamma = (1 + 0.1 * torch.randn(C, generator=gen, dtype=f64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=gen, dtype=f64)).requires_grad_(True)
    bn = torch.nn.BatchNorm3d(C, eps=eps, momentum=mom).double()
    rm0, rv0 = torch.randn(C, generator=gen, dtype=f64), torch.rand(C, generator=gen, dtype=f64) + 0.5
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    groups = []
    for call in range(2):
        x = (0.3 + 1.5 * torch.randn((B, C) + xyz, generator=gen, dtype=f64)).requires_grad_(True)
        gy = torch.randn((B, C) + xyz, generator=gen, dtype=f64)
        n = x.numel() // C
        bn(x.detach())
        y = F.leaky_relu(F.batch_norm(x, None, None, gamma, beta, True, mom, eps), slope)
        gx, gg, gb = torch.autograd.grad((y * gy).sum(), (x, gamma, beta))
        xr, gr = rows(x.detach()), rows(gy)
        s, _ = kb.ref_bn_sums(xr)
        mean, _ = kb.ref_bn_mean(s[:C], n)
        s2, _ = kb.ref_bn_sums(xr, mean)
        fin, _ = kb.ref_bn_finalize(s2[:C], s2[C:], n, mean, eps, mom)
        groups.append((s2[:C], s2[C:], mean))
        close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)
        close(mean, x.detach().mean(dim=(0, 2, 3, 4)))
        close(fin["var"], x.detach().var(dim=(0, 2, 3, 4), unbiased=False))
        yr, _ = kb.ref_bn_apply(xr, mean, fin["invstd"], gamma.detach(), beta.detach(), True, slope)
        close(yr, rows(y.detach()))
        bs, _ = kb.ref_bn_bwd_sums(gr, yr, xr, mean, fin["invstd"], True, slope)
        close(bs[:C], gb)
        close(bs[C:], gg)
        gp, _ = kb.ref_bn_bwd_dy(gr, yr, True, slope)
        for g_in, act_y in ((gp, None), (gr, yr)):  # the training form (g' written back) and the folded mask
            dx, _ = kb.ref_bn_bwd_apply(g_in, xr, act_y, slope, mean, fin["invstd"], gamma.detach(), bs, 1.0 / n)
            close(dx, rows(gx))
        ev, _ = kb.ref_bn_bwd_apply(gr, xr, yr, slope, mean, fin["invstd"], gamma.detach(), None, 0.0)
        close(ev, gp * (gamma.detach() * fin["invstd"]).view(1, -1))
    run, _, _ = kb.ref_bn_running(groups, n, eps, mom, rm0, rv0)
    close(run["rm"], bn.running_mean)
    close(run["rv"], bn.running_var)


def _emul_rows_sum(part):
    """``chan_sum_final_kernel`` / ``bn_rows_sum``: the column sums of part (rows, C2) in fp32, thread = (row lane,
    column), four accumulators over rows r, r + lanes, r + 2 lanes, r + 3 lanes, then the row lanes in order"""
    rows, C2 = part.shape
    fl = 1024 // C2
    sh = []
    for rl in range(fl):
        a = [torch.zeros(C2) for _ in range(4)]
        r = rl
        while r + 3 * fl < rows:
            for u in range(4):
                a[u] = a[u] + part[r + u * fl]
            r += 4 * fl
        while r < rows:
            a[0] = a[0] + part[r]
            r += fl
        sh.append((a[0] + a[1]) + (a[2] + a[3]))
    out = sh[0]
    for s in sh[1:]:
        out = out + s
    return out


def _emul_v4_reduce(ta, tb, *, drop_lane_of=None, drop_trip=None):
    """``bn_reduce_v4_kernel`` + the final kernel on the per-element fp32 terms ta, tb (nvox, C): every thread adds its
    voxels trip by trip (step = rows * lanes), lane 0 adds the lanes in order, the final kernel adds the rows.
    ``drop_lane_of`` = workgroup whose last voxel lane is left out, ``drop_trip`` = trip every thread skips."""
    nvox, C = ta.shape
    lanes, rows = kb.bn_v4_geometry(C, nvox)
    step = rows * lanes
    trips = -(-nvox // step)
    parts = []
    for t in (ta, tb):
        pad = torch.zeros(trips * step, C)
        pad[:nvox] = t
        pad = pad.view(trips, rows, lanes, C)
        acc = torch.zeros(rows, lanes, C)
        for i in range(trips):
            if i != drop_trip:
                acc = acc + pad[i]
        if drop_lane_of is not None:
            acc[drop_lane_of, lanes - 1] = 0.0
        a = acc[:, 0]
        for l in range(1, lanes):
            a = a + acc[:, l]
        parts.append(a)
    return _emul_rows_sum(torch.cat(parts, dim=1)), trips, rows


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _bn_rows(C, nvox, dt, seed):
    """x (0.3 + 1.5 randn; in fp32 channel 1 at 1000 +- 1; channel 2 constant), dy, and a saved output with special
    values, as the kernels' element type holds them (fp32 tensors, bf16-exact for bf16)"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(nvox, C, generator=gen)
    if dt == torch.float32 and C > 1:
        x[:, 1] = 1000.0 + torch.randn(nvox, generator=gen)
    if C > 2:
        x[:, 2] = 0.75
    dy = torch.randn(nvox, C, generator=gen)
    y = torch.randn(nvox, C, generator=gen).to(dt)
    return (x.to(dt).float(), dy.to(dt).float(), y)


def _emul_stats(x, shift, **kw):
    d = x if shift is None else x - shift.view(1, -1)
    return _emul_v4_reduce(d, d * d, **kw)


def _emul_bwd_reduce(dy, y, x, mean, invstd, act, slope, flip=(), **kw):
    g = dy
    if act:
        pos = y.float() > 0
        for v, c in flip:
            pos[v, c] = ~pos[v, c]
        g = dy * torch.where(pos, torch.ones(()), _f(slope))
    return _emul_v4_reduce(g, g * (x - mean.view(1, -1)) * invstd.view(1, -1), **kw) + (g,)


BN_REDUCE_SHAPES = [(4, 1), (4, 257), (12, 1361), (48, 1000), (32, 630), (32, 512 * 50 + 3), (320, 333),
                    (256, 32768 + 5)]


def _bad(got, ref, bnd):
    return kb.check_within(got, ref, bnd)[0]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,nvox", BN_REDUCE_SHAPES)
def test_bn_reduce_emulation_is_within_the_bound(dt, C, nvox):
    """both BatchNorm reductions in fp32 in the v4 kernel's order (threads, trips, lanes, rows) against
    ``ref_bn_sums`` / ``ref_bn_bwd_sums`` with K = nvox + rows, and the written-back dy with K = 1"""
    x, dy, y = _bn_rows(C, nvox, dt, 3 * C + nvox)
    s0, _, rows = _emul_stats(x, None)
    ref, A = kb.ref_bn_sums(x)
    kb.assert_within(s0, ref, kb.bound(ref, A, nvox + rows, 0.0), f"emul bn_stats[{C}x{nvox}]")
    mean = s0[:C] / _f(nvox)
    s2, _, _ = _emul_stats(x, mean)
    ref, A = kb.ref_bn_sums(x, mean)
    kb.assert_within(s2, ref, kb.bound(ref, A, nvox + rows, 0.0), f"emul bn_stats shifted[{C}x{nvox}]")
    invstd = torch.rsqrt((s2[C:] / _f(nvox) - (s2[:C] / _f(nvox)) ** 2).clamp_min(0) + _f(1e-5))
    bs, _, _, g = _emul_bwd_reduce(dy, y, x, mean, invstd, True, 0.2)
    ref, A = kb.ref_bn_bwd_sums(dy, y, x, mean, invstd, True, 0.2)
    kb.assert_within(bs, ref, kb.bound(ref, A, nvox + rows, 0.0), f"emul bn_bwd_reduce[{C}x{nvox}]")
    gref, ga = kb.ref_bn_bwd_dy(dy, y, True, 0.2)
    kb.assert_within(g.to(dt), gref, kb.bound(gref, ga, 1, kb.rho_for(dt)), f"emul bn_bwd_reduce dy[{C}x{nvox}]")


BN_REDUCE_MUTATIONS = {  # name -> ((C, nvox), emulation switches, which tables take the wrong channel)
    "last_voxel_lane_of_a_workgroup_left_out": ((12, 1361), dict(drop_lane_of=1), False),
    "last_voxel_lane_of_the_only_workgroup_left_out": ((4, 257), dict(drop_lane_of=0), False),
    "second_trip_left_out": ((4, 257), dict(drop_trip=1), False),
    "second_trip_of_a_capped_grid_left_out": ((256, 32768 + 5), dict(drop_trip=1), False),
    "shift_or_mean_of_channel_c_plus_1": ((4, 1), dict(), True),
    "shift_or_mean_of_channel_c_plus_1_two_rows": ((12, 1361), dict(), True),
}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(BN_REDUCE_MUTATIONS))
def test_bn_reduce_mutation_is_caught(dt, name):
    (C, nvox), kw, roll = BN_REDUCE_MUTATIONS[name]
    x, dy, y = _bn_rows(C, nvox, dt, 3 * C + nvox)
    _, rows = kb.bn_v4_geometry(C, nvox)
    if "drop_trip" in kw:
        assert -(-nvox // (rows * kb.bn_v4_geometry(C, nvox)[0])) >= 2
    mean = (x.double().mean(0) + 0.01).float()  # (a shift near the mean, as pass 2 gets it)
    invstd = torch.rsqrt(x.double().var(0, unbiased=False).float() + _f(1e-5))
    wrong = mean.roll(-1) if roll else mean
    ref, A = kb.ref_bn_sums(x, mean)
    bnd = kb.bound(ref, A, nvox + rows, 0.0)
    assert not _bad(_emul_stats(x, mean)[0], ref, bnd)
    assert _bad(_emul_stats(x, wrong, **kw)[0], ref, bnd) >= 1, name
    ref, A = kb.ref_bn_bwd_sums(dy, y, x, mean, invstd, True, 0.2)
    bnd = kb.bound(ref, A, nvox + rows, 0.0)
    assert not _bad(_emul_bwd_reduce(dy, y, x, mean, invstd, True, 0.2)[0], ref, bnd)
    assert _bad(_emul_bwd_reduce(dy, y, x, wrong, invstd, True, 0.2, **kw)[0], ref, bnd) >= 1, name


def _emul_finalize(s1, s2, cnt, mean, eps, momentum, rm0=None, rv0=None, *, cnt_off=0.0, unbiased_invstd=False):
    """``bn_finalize_channel`` in fp32, every product and sum rounded on its own"""
    cnt, eps, m = _f(cnt) + _f(cnt_off), _f(eps), _f(momentum)
    dm = s1 / cnt
    var = (s2 / cnt - dm * dm).clamp_min(0.0)
    ub = cnt / torch.maximum(cnt - 1.0, _f(1.0))
    invstd = torch.rsqrt((var * ub if unbiased_invstd else var) + eps)
    if rm0 is None:
        return invstd, None, None
    keep = _f(1.0) - m
    return invstd, keep * rm0 + m * mean, keep * rv0 + m * (var * ub)


def _finalize_case(C, cnt, seed=5):
    gen = torch.Generator().manual_seed(seed)
    d = 1.5 * torch.randn(max(cnt, 1), C, generator=gen, dtype=f64)
    d[:, C // 2] = 0.0  # a constant channel: var = 0
    s1 = (1e-3 * torch.randn(C, generator=gen)).float() * cnt  # (the shifted sum is near 0, not 0)
    s2 = (d * d).sum(0).float()
    mean = (0.3 + torch.randn(C, generator=gen)).float()
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    return s1, s2, mean, rm0, rv0


@pytest.mark.parametrize("cnt", [1, 630])
@pytest.mark.parametrize("momentum", [0.1, 0.0])
def test_bn_finalize_emulation_is_within_the_bound(cnt, momentum):
    s1, s2, mean, rm0, rv0 = _finalize_case(300, cnt)
    ref, A = kb.ref_bn_finalize(s1, s2, cnt, mean, 1e-5, momentum, rm0, rv0)
    bnd = kb.bn_finalize_bounds(ref, A, 1e-5)
    invstd, rm, rv = _emul_finalize(s1, s2, cnt, mean, 1e-5, momentum, rm0, rv0)
    for k, got in (("invstd", invstd), ("rm", rm), ("rv", rv)):
        kb.assert_within(got, ref[k], bnd[k], f"emul bn_finalize {k}[cnt {cnt}, m {momentum}]")
    if momentum == 0.0:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    m, _ = kb.ref_bn_mean(s1, cnt)
    kb.assert_within(s1 / _f(cnt), m, kb.bound(m, m.abs(), 1, 0.0), "emul bn_mean")
    # G ordered updates of the same running statistics (bn_train_stats)
    groups, rmg, rvg = [], rm0, rv0
    for g in range(3):
        sg = _finalize_case(300, cnt, seed=6 + g)[:3]
        groups.append(sg)
        _, rmg, rvg = _emul_finalize(*sg[:2], cnt, sg[2], 1e-5, momentum, rmg, rvg)
    run, ra, _ = kb.ref_bn_running(groups, cnt, 1e-5, momentum, rm0, rv0)
    rb = kb.bn_finalize_bounds(run, ra, 1e-5, steps=3)
    kb.assert_within(rmg, run["rm"], rb["rm"], f"emul bn running mean x3[cnt {cnt}, m {momentum}]")
    kb.assert_within(rvg, run["rv"], rb["rv"], f"emul bn running var x3[cnt {cnt}, m {momentum}]")


@pytest.mark.parametrize("name", ["cnt_off_by_one", "unbiased_factor_on_invstd_variance"])
def test_bn_finalize_mutation_is_caught(name):
    cnt = 630
    s1, s2, mean, rm0, rv0 = _finalize_case(4, cnt)
    ref, A = kb.ref_bn_finalize(s1, s2, cnt, mean, 1e-5, 0.1, rm0, rv0)
    bnd = kb.bn_finalize_bounds(ref, A, 1e-5)
    kw = dict(cnt_off=-1.0) if name.startswith("cnt") else dict(unbiased_invstd=True)
    invstd, rm, rv = _emul_finalize(s1, s2, cnt, mean, 1e-5, 0.1, rm0, rv0, **kw)
    assert _bad(invstd, ref["invstd"], bnd["invstd"]) >= 1, name
    if name.startswith("cnt"):  # cnt / (cnt - 1) of 629 reaches the running variance too
        assert _bad(rv, ref["rv"], bnd["rv"]) >= 1, name
        assert _bad(_emul_finalize(s1, s2, cnt, mean, 1e-5, 0.1, rm0, rv0, cnt_off=1.0)[0], ref["invstd"],
                    bnd["invstd"]) >= 1


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,nvox", [(32, 630), (48, 1000), (32, 512 * 50 + 3)])
def test_bn_train_stats_emulation_is_within_the_finalize_bounds(dt, C, nvox):
    """the fused chain of ``bn_train_stats`` (v4 sums, mean, shifted v4 sums, finalize; two groups in order) in fp32
    against ``ref_bn_finalize`` / ``ref_bn_running`` of the FLOAT64 sums of x shifted by the fp32 mean: the fp32 sums in
    between need no allowance of their own, and ``cnt`` off by one in the fused finalize is caught at every size"""
    gen = torch.Generator().manual_seed(C + nvox)
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    for cnt_off in (0.0, -1.0):
        rm, rv, groups, bad = rm0, rv0, [], 0
        for g in range(2):
            x = _bn_rows(C, nvox, dt, 5 * C + nvox + g)[0]
            mean = _emul_stats(x, None)[0][:C] / _f(nvox)
            s2 = _emul_stats(x, mean)[0]
            invstd, rm, rv = _emul_finalize(s2[:C], s2[C:], nvox, mean, 1e-5, 0.1, rm, rv, cnt_off=cnt_off)
            ref, _ = kb.ref_bn_sums(x, mean)
            groups.append((ref[:C], ref[C:], mean))
            fin, fa = kb.ref_bn_finalize(ref[:C], ref[C:], nvox, mean, 1e-5, 0.1)
            bnd = kb.bn_finalize_bounds(fin, fa, 1e-5)["invstd"]
            if cnt_off:
                bad += _bad(invstd, fin["invstd"], bnd)
            else:
                kb.assert_within(invstd, fin["invstd"], bnd, f"emul bn_train_stats invstd[{C}x{nvox}]")
        run, ra, _ = kb.ref_bn_running(groups, nvox, 1e-5, 0.1, rm0, rv0)
        rb = kb.bn_finalize_bounds(run, ra, 1e-5, steps=2)
        if cnt_off:
            assert bad >= C // 2 and _bad(rv, run["rv"], rb["rv"]) >= 1
        else:
            kb.assert_within(rm, run["rm"], rb["rm"], f"emul bn_train_stats running mean[{C}x{nvox}]")
            kb.assert_within(rv, run["rv"], rb["rv"], f"emul bn_train_stats running var[{C}x{nvox}]")


def _bn_tables(x, C, seed):
    gen = torch.Generator().manual_seed(seed)
    mean = x.double().mean(0).float()
    invstd = torch.rsqrt(x.double().var(0, unbiased=False).float() + _f(1e-5))
    gamma = 1 + 0.1 * torch.randn(C, generator=gen)
    beta = 0.1 * torch.randn(C, generator=gen)
    sums = torch.cat([torch.randn(C, generator=gen), torch.randn(C, generator=gen)]) * 20.0
    return mean, invstd, gamma, beta, sums


def _emul_apply(x, mean, invstd, gamma, beta, act, slope, dt):
    r = lambda t: t.view(1, -1)
    v = (x - r(mean)) * r(invstd) * r(gamma) + r(beta)
    if act:
        v = torch.where(v > 0, v, v * _f(slope))
    return v.to(dt)


def _emul_bwd_apply(g, x, act_y, slope, mean, invstd, gamma, sums, inv_n, dt, *, v8=False, threads=None, flip=(),
                    no_inv_n_on_xhat=False, reuse_trip0=False):
    """``bn_bwd_apply_kernel`` (one element per thread: constants by i % C) or ``bn_bwd_apply_v8_kernel`` (``threads``
    threads of 8 elements, constants by the FIRST vector of the thread when ``reuse_trip0``, as the kernel keeps them)
    in fp32, each in its own order of products"""
    nvox, C = g.shape
    n = _f(inv_n)
    v = g
    if act_y is not None:
        pos = act_y.float() > 0
        for vv, c in flip:
            pos[vv, c] = ~pos[vv, c]
        v = g * torch.where(pos, torch.ones(()), _f(slope))
    if not v8:
        r = lambda t: t.view(1, -1)
        if sums is not None:
            xh = (x - r(mean)) * r(invstd)
            t2 = xh * r(sums[C:]) if no_inv_n_on_xhat else xh * r(sums[C:]) * n
            v = v - r(sums[:C]) * n - t2
        return (v * r(gamma) * r(invstd)).to(dt)
    i = torch.arange(nvox * C) // 8
    k = torch.arange(nvox * C) % 8
    true_c = (i * 8 + k) % C
    c = ((i % threads) * 8 + k) % C if reuse_trip0 else true_c
    sc = (gamma * invstd)[c]
    v = v.reshape(-1)
    if sums is not None:
        a0 = (sums[:C] * n)[c]
        a1 = (sums[C:] * invstd if no_inv_n_on_xhat else sums[C:] * n * invstd)[c]
        v = v - a0 - (x.reshape(-1) - mean[c]) * a1
    return (v * sc).view(nvox, C).to(dt)


BN_APPLY_SHAPES = [(1, 630), (4, 630), (12, 630), (256, 630)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,nvox", BN_APPLY_SHAPES)
def test_bn_apply_emulations_are_within_the_bound(dt, C, nvox):
    x, dy, y = _bn_rows(C, nvox, dt, 7 * C + nvox)
    mean, invstd, gamma, beta, sums = _bn_tables(x, C, C)
    for act in (True, False):
        ref, A = kb.ref_bn_apply(x, mean, invstd, gamma, beta, act, 0.2)
        kb.assert_within(_emul_apply(x, mean, invstd, gamma, beta, act, 0.2, dt), ref,
                         kb.bound(ref, A, 4, kb.rho_for(dt)), f"emul bn_apply[{C}x{nvox} act {act}]")
    for s in (sums, None):
        for ay in (y, None):
            ref, A = kb.ref_bn_bwd_apply(dy, x, ay, 0.2, mean, invstd, gamma, s, 1.0 / nvox)
            bnd = kb.bound(ref, A, 8, kb.rho_for(dt))
            tag = f"[{C}x{nvox} sums {s is not None} act_y {ay is not None}]"
            kb.assert_within(_emul_bwd_apply(dy, x, ay, 0.2, mean, invstd, gamma, s, 1.0 / nvox, dt), ref, bnd,
                             "emul bn_bwd_apply" + tag)
            if dt == torch.bfloat16 and C % 8 == 0:  # the 8-wide order: 128 threads x 8 = 4 x C elements per trip
                got = _emul_bwd_apply(dy, x, ay, 0.2, mean, invstd, gamma, s, 1.0 / nvox, dt, v8=True, threads=128,
                                      reuse_trip0=True)
                kb.assert_within(got, ref, bnd, "emul bn_bwd_apply v8" + tag)


class _Apply:
    """a bf16 C = 8 layer on 630 voxels with the special values of the saved output placed where g is largest"""
    C, nvox, dt = 8, 630, torch.bfloat16

    def __init__(self):
        self.x, self.dy, self.y = _bn_rows(self.C, self.nvox, self.dt, 77)
        self.mean, self.invstd, self.gamma, self.beta, self.sums = _bn_tables(self.x, self.C, 78)
        self.inv_n = 1.0 / self.nvox
        order = self.dy.abs().flatten().argsort(descending=True)
        self.at = [(int(i) // self.C, int(i) % self.C) for i in order[:4]]
        for (v, c), bits in zip(self.at, (NEG_ZERO, POS_SUB, NEG_SUB, 0x0000)):
            self.y[v, c] = _bits(bits)

    def ref(self, sums, act_y):
        ref, A = kb.ref_bn_bwd_apply(self.dy, self.x, act_y, 0.2, self.mean, self.invstd, self.gamma, sums, self.inv_n)
        return ref, kb.bound(ref, A, 8, kb.rho_for(self.dt))

    def emul(self, sums, act_y, **kw):
        return _emul_bwd_apply(self.dy, self.x, act_y, 0.2, self.mean, self.invstd, self.gamma, sums, self.inv_n,
                               self.dt, **kw)


@pytest.fixture(scope="module")
def bn_apply_case():
    return _Apply()


@pytest.mark.parametrize("v8", [False, True], ids=["scalar", "v8"])
def test_bn_bwd_apply_missing_inv_n_on_the_xhat_term_is_caught(bn_apply_case, v8):
    s = bn_apply_case
    ref, bnd = s.ref(s.sums, None)
    assert not _bad(s.emul(s.sums, None, v8=v8, threads=128), ref, bnd)
    assert _bad(s.emul(s.sums, None, v8=v8, threads=128, no_inv_n_on_xhat=True), ref, bnd) >= s.nvox


def test_bn_bwd_apply_v8_constants_of_trip_0_on_other_channels_are_caught(bn_apply_case):
    """the 8-wide kernel keeps the constants of its first vector: right while threads * 8 is a multiple of C (the host
    checks that C divides 256), wrong on every trip whose first channel differs"""
    s = bn_apply_case
    x, dy, y = _bn_rows(32, s.nvox, s.dt, 79)
    mean, invstd, gamma, beta, sums = _bn_tables(x, 32, 80)
    ref, A = kb.ref_bn_bwd_apply(dy, x, None, 0.2, mean, invstd, gamma, sums, s.inv_n)
    bnd = kb.bound(ref, A, 8, kb.RHO_BF16)
    emul = lambda threads: _emul_bwd_apply(dy, x, None, 0.2, mean, invstd, gamma, sums, s.inv_n, s.dt, v8=True,
                                           threads=threads, reuse_trip0=True)
    assert not _bad(emul(128), ref, bnd)  # 128 * 8 elements per trip: a multiple of C
    # 129 threads: trip t starts 8 t channels further on; only trips 0, 4, 8, .. keep their channels
    assert _bad(emul(129), ref, bnd) >= x.numel() // 2


@pytest.mark.parametrize("v8", [False, True], ids=["scalar", "v8"])
@pytest.mark.parametrize("which", ["negative_zero_taken_as_positive", "positive_subnormal_taken_as_not_positive"])
def test_bn_mask_sign_of_special_values_is_caught(bn_apply_case, which, v8):
    """the folded LeakyReLU derivative at -0.0 and at a positive subnormal, in the eval form of bn_bwd_apply (both
    kernels' orders) and in bn_bwd_reduce's written-back dy"""
    s = bn_apply_case
    v, c = s.at[0] if which.startswith("negative") else s.at[1]
    assert bool(s.y[v, c].double() > 0) == which.startswith("positive")
    ref, bnd = s.ref(None, s.y)
    assert not _bad(s.emul(None, s.y, v8=v8, threads=128), ref, bnd)
    got = s.emul(None, s.y, v8=v8, threads=128, flip=[(v, c)])
    _, _, _, ratio = kb.check_within(got, ref, bnd)
    assert [(int(a), int(b)) for a, b in (ratio > 1.0).nonzero().tolist()] == [(v, c)]
    gref, ga = kb.ref_bn_bwd_dy(s.dy, s.y, True, 0.2)
    gb = kb.bound(gref, ga, 1, kb.RHO_BF16)
    g = _emul_bwd_reduce(s.dy, s.y, s.x, s.mean, s.invstd, True, 0.2)[3].to(s.dt)
    assert not _bad(g, gref, gb)
    keep = kb._lrelu_mask(s.y, 0.2) == 1.0
    assert torch.equal(g[keep].view(torch.int16), s.dy.to(s.dt)[keep].view(torch.int16))
    g = _emul_bwd_reduce(s.dy, s.y, s.x, s.mean, s.invstd, True, 0.2, flip=[(v, c)])[3].to(s.dt)
    _, _, _, ratio = kb.check_within(g, gref, gb)
    assert [(int(a), int(b)) for a, b in (ratio > 1.0).nonzero().tolist()] == [(v, c)]


# ---- the network boundary: stencils, content loss, z-fold, plane sums - references, fp32 emulations, mutations ---------------

BOUNDARY_SMALL = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 2, 1, 1), (1, 1, 2, 1), (1, 2, 2, 2), (1, 3, 3, 3), (2, 1, 6, 5),
                  (2, 5, 1, 6), (2, 5, 6, 1), (2, 5, 7, 9)]
COEF = torch.tensor([0.31, -0.17, 0.23, 0.41, 0.136, 0.07])


def _close(a, b, tol=1e-11):
    torch.testing.assert_close(a, b, rtol=tol, atol=tol)


@pytest.mark.parametrize("shape", [(1, 2, 2, 2), (1, 3, 3, 3), (2, 5, 7, 9), (2, 2, 6, 3)])
@pytest.mark.parametrize("coords", ["random", "heights"])
def test_boundary_references_equal_float64_autograd_of_the_oracle(shape, coords):
    """``ref_wind_gradient``, its adjoint, the 14 statistics and d loss / d SR against ``oracle/physics.py`` and fp64
    autograd of it (extents >= 2: the oracle has no axis of length 1)"""
    from oracle import physics as ophys

    hr, sr, x, y, zc = (t.double() for t in kb.boundary_inputs(shape, coords, seed=41))
    srr = sr.clone().requires_grad_(True)
    jh, js = ophys.wind_gradient(hr, x, y, zc), ophys.wind_gradient(srr, x, y, zc)
    _close(kb.ref_wind_gradient(sr, x, y, zc)[0], js.detach())
    gy = torch.randn(js.shape, generator=torch.Generator().manual_seed(3), dtype=f64)
    (want,) = torch.autograd.grad((js * gy).sum(), srr, retain_graph=True)
    _close(kb.ref_wind_gradient_bwd(gy, x, y, zc)[0], want)
    d3 = lambda j: j[:, 0] + j[:, 4] + j[:, 8]  # noqa: E731
    d2 = lambda j: j[:, 0] + j[:, 4]  # noqa: E731
    sums = [((js[:, :6] - jh[:, :6]) ** 2).sum(), ((js[:, 6:] - jh[:, 6:]) ** 2).sum(), ((d3(jh) - d3(js)) ** 2).sum(),
            ((d2(jh) - d2(js)) ** 2).sum(), (hr - srr).abs().sum(), ((hr - srr) ** 2).sum()]
    mx = [f(j.detach()) for j in (jh, js) for f in (lambda j: j[:, :6].abs().max(), lambda j: j[:, 6:].max(),
                                                    lambda j: d3(j).abs().max(), lambda j: d2(j).abs().max())]
    ref, bnd = kb.ref_physics_stats(hr, sr, x, y, zc)
    _close(ref, torch.stack([s.detach() for s in sums] + mx), 1e-10)
    assert bool((bnd > 0).all())
    coef = COEF.double()
    (want,) = torch.autograd.grad(sum(c * s for c, s in zip(coef, sums)), srr)
    (res, _), (dsr, _) = kb.ref_physics_bwd(hr, sr, x, y, zc, coef)
    _close(dsr, want, 1e-10)
    # the residual IS d loss / d J_sr
    jl = js.detach().clone().requires_grad_(True)
    loss = (coef[0] * ((jl[:, :6] - jh[:, :6]) ** 2).sum() + coef[1] * ((jl[:, 6:] - jh[:, 6:]) ** 2).sum()
            + coef[2] * ((d3(jh) - d3(jl)) ** 2).sum() + coef[3] * ((d2(jh) - d2(jl)) ** 2).sum())
    _close(res, torch.autograd.grad(loss, jl)[0], 1e-10)


def test_boundary_reference_against_the_recorded_jacobians(golden):
    """``ref_wind_gradient`` of the recorded HR / SR against the Jacobian stacks the reference project produced in fp32
    (tests/golden/physics.npz), inside the stencil's own bound"""
    g = golden("physics.npz")
    T = lambda k: torch.from_numpy(g[k])  # noqa: E731
    for src, want in (("HR", "grad_hr"), ("SR", "grad_sr")):
        ref, M = kb.ref_wind_gradient(T(src), T("x"), T("y"), T("Z"))
        kb.assert_within(T(want), ref, kb.bound(ref, M, kb.K_STENCIL, 0.0), f"recorded jacobian {src}")


def test_boundary_references_on_an_axis_of_length_one():
    for shape, dead in (((2, 1, 6, 5), 0), ((2, 5, 1, 6), 1), ((2, 5, 6, 1), 2), ((1, 1, 1, 1), None)):
        hr, sr, x, y, zc = kb.boundary_inputs(shape, "random", seed=5)
        J, M = kb.ref_wind_gradient(sr, x, y, zc)
        for k in range(3):
            if dead is None or k == dead:
                assert not J[:, 3 * k:3 * k + 3].any() and not M[:, 3 * k:3 * k + 3].any()
            else:
                assert bool((M[:, 3 * k:3 * k + 3] > 0).all())
        g = torch.randn(J.shape, dtype=f64)
        if dead is not None:
            g2 = g.clone()
            g2[:, 3 * dead:3 * dead + 3] = 7.0  # the dead axis' gradient reaches nothing
            assert torch.equal(kb.ref_wind_gradient_bwd(g, x, y, zc)[0], kb.ref_wind_gradient_bwd(g2, x, y, zc)[0])


# -- the kernels' arithmetic in fp32, in their own order

def _emul_rows(co, end_row_interior=False, contract=False):
    """``deriv_row`` (stencil.h) along the last axis of fp32 coordinates, every operation rounded on its own;
    ``contract``: hr * hr - hl * hl as the compiler may fuse it, fma(hr, hr, -(hl * hl)) - one rounding fewer, and a
    centre weight that is the rounding error of hl * hl where hr == hl"""
    n = co.shape[-1]
    a, b, c = (torch.zeros_like(co) for _ in range(3))
    if n < 2:
        return a, b, c
    if n >= 3:
        hl, hr = co[..., 1:-1] - co[..., :-2], co[..., 2:] - co[..., 1:-1]
        den = hl * hr * (hl + hr)
        num = (hr.double() * hr.double() - (hl * hl).double()).float() if contract else hr * hr - hl * hl
        a[..., 1:-1], b[..., 1:-1], c[..., 1:-1] = -(hr * hr) / den, num / den, (hl * hl) / den
    h = co[..., 1] - co[..., 0]
    b[..., 0], c[..., 0] = -1.0 / h, 1.0 / h
    h = co[..., -1] - co[..., -2]
    if end_row_interior:  # the last row takes the weights of the interior row below it
        assert n >= 3
        a[..., -1], b[..., -1], c[..., -1] = a[..., -2], b[..., -2], c[..., -2]
    else:
        a[..., -1], b[..., -1] = -1.0 / h, 1.0 / h
    return a, b, c


def _co(co, dim):
    return co if co.dim() == 1 else co.movedim(dim, -1)


def _emul_jacobian(f, x, y, zc, drop=None, end_row_interior=None, contract=False):
    """``jacobian`` (physics_loss.hip :33) / ``wind_gradient_kernel``: (a f- + b f0) + c f+ per axis.  ``drop`` =
    (channel 0..8, b, comp, x, y, z): the forward face tap (c f+) of that element is left out; ``end_row_interior``:
    the axis (0..2) whose last row takes interior weights."""
    out = []
    for k, co in enumerate((x, y, zc)):
        ff = f.movedim(2 + k, -1)
        a, b, c = _emul_rows(_co(co, 2 + k), end_row_interior == k, contract)
        ta, tb, tc = a * kb._shift(ff, -1), b * ff, c * kb._shift(ff, 1)
        tc = tc.movedim(-1, 2 + k).clone()
        if drop is not None and drop[0] // 3 == k:
            assert drop[0] % 3 == drop[2]
            tc[drop[1], drop[2], drop[3], drop[4], drop[5]] = 0.0
        out.append((ta + tb).movedim(-1, 2 + k) + tc)
    return torch.cat(out, 1)


def _butterfly(v, op):
    """the xor shuffles 32, 16, .., 1 over the last axis (64 lanes); every lane ends with the same value"""
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., idx ^ off])
    return v[..., 0]


def _emul_stats_kernel(hr, sr, x, y, zc, zmax_start=-math.inf, jac=_emul_jacobian):
    """``physics_stats_kernel`` + ``physics_stats_final_kernel``: per-thread partials over its trips, the wave
    butterflies, the four waves in order, then per statistic one wave over the rows (sums in double) -> (14,) fp32"""
    jh, js = jac(hr, x, y, zc), jac(sr, x, y, zc)
    B = hr.shape[0]
    nvox = hr.numel() // 3
    grid = kb.physics_rows(nvox)
    nthr = grid * 256
    trips = -(-nvox // nthr)
    vox = lambda t: t.movedim(1, -1).reshape(nvox, t.shape[1])  # (voxel, channel)  # noqa: E731
    jh, js = vox(jh), vox(js)
    d = js - jh
    h2, s2 = jh[:, 0] + jh[:, 4], js[:, 0] + js[:, 4]
    h3, s3 = h2 + jh[:, 8], s2 + js[:, 8]
    dp = vox(hr) - vox(sr)
    sum_terms = [(d * d)[:, :6], (d * d)[:, 6:], ((h3 - s3) * (h3 - s3))[:, None], ((h2 - s2) * (h2 - s2))[:, None],
                 dp.abs(), dp * dp]
    max_terms = [jh[:, :6].abs(), jh[:, 6:], h3.abs()[:, None], h2.abs()[:, None],
                 js[:, :6].abs(), js[:, 6:], s3.abs()[:, None], s2.abs()[:, None]]
    starts = [0.0, zmax_start, 0.0, 0.0, 0.0, zmax_start, 0.0, 0.0]

    def per_thread(t, start, op):
        acc = torch.full((nthr,), start, dtype=torch.float32)
        valid = torch.zeros(trips * nthr, dtype=torch.bool)
        valid[:nvox] = True
        pad = torch.zeros(trips * nthr, t.shape[1])
        pad[:nvox] = t
        for i in range(trips):
            for c in range(t.shape[1]):
                nxt = op(acc, pad[i * nthr:(i + 1) * nthr, c])
                acc = torch.where(valid[i * nthr:(i + 1) * nthr], nxt, acc)
        return acc.view(grid, 4, 64)

    out = []
    for t in sum_terms:
        w = _butterfly(per_thread(t, 0.0, torch.add), torch.add)  # (grid, 4)
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        lanes = torch.zeros(64, dtype=f64)
        for r in range(grid):
            lanes[r % 64] = lanes[r % 64] + part[r].double()
        out.append(_butterfly(lanes, torch.add).float())
    for t, st in zip(max_terms, starts):
        w = _butterfly(per_thread(t, st, torch.maximum), torch.maximum)
        part = torch.maximum(torch.maximum(torch.maximum(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])
        lanes = part[0].repeat(64)
        for r in range(grid):
            lanes[r % 64] = torch.maximum(lanes[r % 64], part[r])
        out.append(_butterfly(lanes, torch.maximum))
    return torch.stack(out)


def _emul_residual(hr, sr, x, y, zc, coef, div2_on_8=False, jac=_emul_jacobian):
    """``physics_residual_kernel`` (:139)"""
    jh, js = jac(hr, x, y, zc), jac(sr, x, y, zc)
    g = [2.0 * c for c in coef[:4]]
    o = torch.zeros_like(js)
    for k in range(9):
        gg = g[0] if k < 6 else g[1]
        if gg != 0:
            o[:, k] = gg * (js[:, k] - jh[:, k])
    d2 = (js[:, 0] + js[:, 4]) - (jh[:, 0] + jh[:, 4])
    d3 = d2 + (js[:, 8] - jh[:, 8])
    t3 = g[2] * d3 if g[2] != 0 else torch.zeros_like(d3)
    t = t3 + (g[3] * d2 if g[3] != 0 else torch.zeros_like(d2))
    o[:, 0] += t
    o[:, 4] += t
    o[:, 8] += t if div2_on_8 else t3
    return o


def _emul_adjoint(g, x, y, zc, weight_of_row_x=False):
    """``wind_gradient_bwd_kernel`` (:1142): acc = 0, then per axis b_j g_j, c_{j-1} g_{j-1}, a_{j+1} g_{j+1} in that
    order.  ``weight_of_row_x``: along x the lower neighbour's weight is taken from row x, not x - 1."""
    acc = torch.zeros_like(g[:, :3])
    for k, co in enumerate((x, y, zc)):
        gg = g[:, 3 * k:3 * k + 3].movedim(2 + k, -1)
        a, b, c = _emul_rows(_co(co, 2 + k))
        lower = c * kb._shift(gg, -1) if (weight_of_row_x and k == 0) else kb._shift(c * gg, -1)
        lower[..., 0] = 0.0
        for term in (b * gg, lower, kb._shift(a * gg, 1)):
            acc = acc + term.movedim(-1, 2 + k)
    return acc


def _emul_dsr(res, hr, sr, x, y, zc, coef, sign0=0.0, **kw):
    """``physics_adjoint_kernel`` (:175)"""
    phys = any(float(c) != 0 for c in coef[:4])
    acc = _emul_adjoint(res, x, y, zc, **kw) if phys else torch.zeros_like(sr)
    d = sr - hr
    sgn = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, sign0)).float()
    c1, c2 = coef[4], 2.0 * coef[5]
    pix = (c1 * sgn if c1 != 0 else torch.zeros_like(d)) + (c2 * d if c2 != 0 else torch.zeros_like(d))
    return acc + pix


def _near_uniform_case():
    """the nearly uniform grid with one large centre value: b = (hr^2 - hl^2) / den cancels almost completely there"""
    hr, sr, x, y, zc = kb.boundary_inputs((1, 6, 7, 40), "near_odd", seed=9)
    sr[0, :, 3, 3, 20] = 1.0e6
    return hr, sr, x, y, zc


def _boundary_cases():
    for shape in BOUNDARY_SMALL:
        for coords in ("random", "uniform", "near", "heights"):
            yield f"{shape} {coords}", kb.boundary_inputs(shape, coords, seed=sum(shape))
    yield "near uniform", _near_uniform_case()


def test_stencil_emulations_are_within_the_bound():
    """wind gradient forward and adjoint, residual and d loss / d SR in fp32 in the kernels' order, on the matrix's
    small shapes and on the nearly uniform grid: K = 12, 19, 23, 24"""
    worst = {}
    for name, (hr, sr, x, y, zc) in _boundary_cases():
        J, M = kb.ref_wind_gradient(sr, x, y, zc)
        r = {"J": kb.assert_within(_emul_jacobian(sr, x, y, zc), J, kb.bound(J, M, kb.K_STENCIL, 0.0), f"emul wind_gradient[{name}]")}
        g = torch.randn(J.shape, generator=torch.Generator().manual_seed(1))
        ref, A = kb.ref_wind_gradient_bwd(g, x, y, zc)
        r["adj"] = kb.assert_within(_emul_adjoint(g, x, y, zc), ref, kb.bound(ref, A, kb.K_ADJOINT, 0.0), f"emul wind_gradient_bwd[{name}]")
        res = _emul_residual(hr, sr, x, y, zc, COEF)
        (rr, ra), (dr, da) = kb.ref_physics_bwd(hr, sr, x, y, zc, COEF, residual=res)
        r["res"] = kb.assert_within(res, rr, kb.bound(rr, ra, kb.K_RESIDUAL, 0.0), f"emul residual[{name}]")
        r["dsr"] = kb.assert_within(_emul_dsr(res, hr, sr, x, y, zc, COEF), dr, kb.bound(dr, da, kb.K_DSR, 0.0), f"emul dsr[{name}]")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[ratio] stencil emulations, worst |err|/bound:", {k: round(v, 4) for k, v in worst.items()})


def test_pre_cancellation_magnitude_is_what_keeps_the_near_uniform_grid_inside():
    """with |b| |f_i| in place of (hr^2 + hl^2) / |den| |f_i| the SAME correct emulation leaves the bound by orders of
    magnitude at the large centre value: a hole in the bound, not an error of the arithmetic"""
    hr, sr, x, y, zc = _near_uniform_case()
    J, M = kb.ref_wind_gradient(sr, x, y, zc)
    s = sr.double()
    weak = []
    for k, co in enumerate((x, y, zc)):
        ff = s.movedim(2 + k, -1)
        a, b, c, _ = kb._stencil_rows(_co(co.double(), 2 + k))
        weak.append((a.abs() * kb._shift(ff, -1).abs() + b.abs() * ff.abs() + c.abs() * kb._shift(ff, 1).abs()).movedim(-1, 2 + k))
    for contract in (False, True):
        got = _emul_jacobian(sr, x, y, zc, contract=contract)
        good = kb.assert_within(got, J, kb.bound(J, M, kb.K_STENCIL, 0.0), f"near-uniform grid, contract {contract}")
        bad, worst, top, _ = kb.check_within(got, J, kb.bound(J, torch.cat(weak, 1), kb.K_STENCIL, 0.0))
        print(f"[ratio] near-uniform grid, contract {contract}: {good:.3g} of the bound, {worst:.3g} of the one from |b|")
        assert bad and worst > 10.0 and all(kb._coords(i, tuple(J.shape), "act").endswith("x=3, y=3, z=20)") for i in top[:bad])


STATS_SHAPES = BOUNDARY_SMALL + [(1, 20, 41, 20)]


@pytest.mark.parametrize("shape", STATS_SHAPES, ids=str)
def test_stats_emulation_is_within_the_bound(shape):
    worst = 0.0
    for coords in (("random", "heights") if shape != (1, 20, 41, 20) else ("random",)):
        hr, sr, x, y, zc = kb.boundary_inputs(shape, coords, seed=7 + sum(shape))
        ref, bnd, tight = kb.ref_physics_stats(hr, sr, x, y, zc, tight_sums=True)
        got = _emul_stats_kernel(hr, sr, x, y, zc)
        kb.assert_within(got, ref, bnd, f"emul physics_stats[{shape} {coords}]")
        worst = max(worst, kb.assert_within(got[:6], ref[:6], tight, f"emul physics_stats sums, propagated[{shape} {coords}]"))
        assert bool((tight <= bnd[:6]).all())
    hr, sr, x, y, zc = _near_uniform_case()
    ref, bnd, tight = kb.ref_physics_stats(hr, sr, x, y, zc, tight_sums=True)
    got = _emul_stats_kernel(hr, sr, x, y, zc)
    kb.assert_within(got, ref, bnd, "emul physics_stats[near uniform]")
    kb.assert_within(got[:6], ref[:6], tight, "emul physics_stats sums, propagated[near uniform]")
    print(f"[ratio] physics_stats emulation {shape}: {worst:.3g} of the sums' narrower bound")


def _violations(got, ref, bnd):
    return [tuple(i) for i in (kb.check_within(got, ref, bnd)[3] > 1.0).nonzero().tolist()]


def test_one_dropped_face_tap_at_one_voxel_is_caught():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    J, M = kb.ref_wind_gradient(sr, x, y, zc)
    bnd = kb.bound(J, M, kb.K_STENCIL, 0.0)
    for ch, at in ((0, (1, 0, 3, 6, 8)), (4, (0, 1, 4, 5, 0)), (8, (1, 2, 0, 0, 7))):  # the last interior row of each axis
        assert _violations(_emul_jacobian(sr, x, y, zc, drop=(ch,) + at), J, bnd) == [(at[0], ch, at[2], at[3], at[4])]
    # the residual and the statistics see it too: channel 0 carries both divergence terms
    drop = (0, 1, 0, 3, 6, 8)
    jac = lambda f, *a: _emul_jacobian(f, *a, drop=drop if f is sr else None)  # noqa: E731
    (rr, ra), _ = kb.ref_physics_bwd(hr, sr, x, y, zc, COEF)
    rb = kb.bound(rr, ra, kb.K_RESIDUAL, 0.0)
    assert not _violations(_emul_residual(hr, sr, x, y, zc, COEF), rr, rb)
    assert _violations(_emul_residual(hr, sr, x, y, zc, COEF, jac=jac), rr, rb) == [(1, k, 3, 6, 8) for k in (0, 4, 8)]


def test_interior_row_used_at_an_end_is_caught():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    J, M = kb.ref_wind_gradient(sr, x, y, zc)
    bnd = kb.bound(J, M, kb.K_STENCIL, 0.0)
    for axis in range(3):
        bad = _violations(_emul_jacobian(sr, x, y, zc, end_row_interior=axis), J, bnd)
        last = sr.shape[2 + axis] - 1
        assert bad and all(i[1] // 3 == axis and i[2 + axis] == last for i in bad)
        assert len(bad) == sr.numel() // sr.shape[2 + axis], "every element of the end face"


def test_adjoint_neighbour_weight_of_the_wrong_row_is_caught():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    g = torch.randn((2, 9, 5, 7, 9), generator=torch.Generator().manual_seed(4))
    g[:, 3:] = 0.0  # the x axis alone: no other axis' magnitude covers the error
    ref, A = kb.ref_wind_gradient_bwd(g, x, y, zc)
    bnd = kb.bound(ref, A, kb.K_ADJOINT, 0.0)
    assert not _violations(_emul_adjoint(g, x, y, zc), ref, bnd)
    bad = _violations(_emul_adjoint(g, x, y, zc, weight_of_row_x=True), ref, bnd)
    assert bad and all(i[2] >= 1 for i in bad) and len(bad) == 2 * 3 * 4 * 7 * 9  # every element with a lower neighbour
    # through the content loss, all axes live: still every such x-row is reported
    res = _emul_residual(hr, sr, x, y, zc, COEF)
    dr, da = kb.ref_physics_adjoint(res, hr, sr, x, y, zc, COEF)
    db = kb.bound(dr, da, kb.K_DSR, 0.0)
    assert not _violations(_emul_dsr(res, hr, sr, x, y, zc, COEF), dr, db)
    bad = _violations(_emul_dsr(res, hr, sr, x, y, zc, COEF, weight_of_row_x=True), dr, db)
    assert len(bad) > 0.5 * 2 * 3 * 4 * 7 * 9 and all(i[2] >= 1 for i in bad)


def test_div2_term_on_channel_8_is_caught():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    (rr, ra), _ = kb.ref_physics_bwd(hr, sr, x, y, zc, COEF)
    bad = _violations(_emul_residual(hr, sr, x, y, zc, COEF, div2_on_8=True), rr, kb.bound(rr, ra, kb.K_RESIDUAL, 0.0))
    assert bad and all(i[1] == 8 for i in bad) and len(bad) > 0.95 * 630
    one_hot = torch.tensor([0.0, 0.0, 0.0, 0.41, 0.0, 0.0])  # the route on its own: channel 8 must stay +0.0
    (rr, ra), _ = kb.ref_physics_bwd(hr, sr, x, y, zc, one_hot)
    assert not rr[:, 8].any()
    bad = _violations(_emul_residual(hr, sr, x, y, zc, one_hot, div2_on_8=True), rr, kb.bound(rr, ra, kb.K_RESIDUAL, 0.0))
    assert bad and all(i[1] == 8 for i in bad)


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 1, 1, 2)], ids=str)
def test_signed_maximum_started_at_zero_is_caught(shape):
    """all z-derivatives negative: maxima 1 and 5 are negative, and a start value of 0 - which idle lanes and the first
    comparison would keep - is reported at exactly those two entries"""
    hr, sr, x, y, zc = kb.boundary_inputs(shape, "heights", seed=6, descending=True)
    ref, bnd = kb.ref_physics_stats(hr, sr, x, y, zc)
    assert float(ref[6 + 1]) < 0 and float(ref[6 + 5]) < 0
    assert not _violations(_emul_stats_kernel(hr, sr, x, y, zc), ref, bnd)
    assert _violations(_emul_stats_kernel(hr, sr, x, y, zc, zmax_start=0.0), ref, bnd) == [(7,), (11,)]


def test_sign_of_zero_returned_as_one_is_caught():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    at = [(0, 0, 0, 0, 0), (1, 2, 4, 6, 8), (0, 1, 2, 3, 4)]
    for i in at:
        sr[i] = hr[i]
    for coef in (COEF, torch.tensor([0.0, 0.0, 0.0, 0.0, 0.136, 0.0])):
        res = _emul_residual(hr, sr, x, y, zc, coef)
        dr, da = kb.ref_physics_adjoint(res, hr, sr, x, y, zc, coef)
        db = kb.bound(dr, da, kb.K_DSR, 0.0)
        assert not _violations(_emul_dsr(res, hr, sr, x, y, zc, coef), dr, db)
        assert sorted(_violations(_emul_dsr(res, hr, sr, x, y, zc, coef, sign0=1.0), dr, db)) == sorted(at)


def test_nan_in_sr_reaches_the_sr_maxima_and_the_sums_only():
    hr, sr, x, y, zc = kb.boundary_inputs((2, 5, 7, 9), "random", seed=2)
    sr[-1, 0, -1, -1, -1] = float("nan")  # component u of the last voxel: it enters every SR statistic
    ref, _ = kb.ref_physics_stats(hr, sr, x, y, zc)
    got = _emul_stats_kernel(hr, sr, x, y, zc)
    want = [True] * 6 + [False] * 4 + [True] * 4
    assert torch.isnan(ref).tolist() == want and torch.isnan(got).tolist() == want


# -- z-fold and plane sums

def _emul_zfold(t, bias, C, KZ, pz, drop=None):
    """``zfold_kernel`` (:1005): acc = bias, then the taps in order.  ``drop`` = (b, c, x, y, z): that output leaves out
    its tap at z + kz - pz = Z - 1."""
    B, Z = t.shape[0], t.shape[-1]
    tt = t.reshape((B, C, KZ) + tuple(t.shape[2:]))
    acc = torch.zeros((B, C) + tuple(t.shape[2:]))
    if bias is not None:
        acc = acc + bias.view(1, C, 1, 1, 1)
    for k in range(KZ):
        s = kb._shift(tt[:, :, k], k - pz)
        if drop is not None and drop[4] + k - pz == Z - 1:
            s[drop] = 0.0
        acc = acc + s
    return acc


ZFOLD_SHAPES = [(2, 3, 5, 2, 4, 3, 7), (1, 1, 1, 0, 1, 1, 1), (2, 3, 5, 0, 3, 2, 6), (2, 3, 5, 4, 3, 2, 6),
                (1, 2, 5, 2, 3, 3, 2), (1, 3, 3, 1, 2, 2, 1)]


def _zfold_case(B, C, KZ, pz, X, Y, Z, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return 10.0 + torch.randn((B, C * KZ, X, Y, Z), generator=gen), torch.randn(C, generator=gen)


@pytest.mark.parametrize("row", ZFOLD_SHAPES, ids=str)
def test_zfold_emulation_is_within_the_bound_and_equals_a_direct_sum(row):
    B, C, KZ, pz, X, Y, Z = row
    t, bias = _zfold_case(*row)
    for bb in (bias, None):
        ref, A = kb.ref_zfold(t, bb, C, KZ, pz)
        direct = torch.zeros_like(ref)
        for c in range(C):
            for z in range(Z):
                for k in range(KZ):
                    if 0 <= z + k - pz < Z:
                        direct[:, c, :, :, z] += t[:, c * KZ + k, :, :, z + k - pz].double()
        _close(ref, direct + (0 if bb is None else bb.double().view(1, C, 1, 1, 1)))
        kb.assert_within(_emul_zfold(t, bb, C, KZ, pz), ref, kb.bound(ref, A, KZ + 1, 0.0), f"emul zfold[{row}]")
    # the adjoint as a copy: <zfold(t), g> = <t, zunfold(g)> exactly in float64
    g = torch.randn((B, C, X, Y, Z), generator=torch.Generator().manual_seed(1))
    d = kb.ref_zunfold(g, KZ, pz, C * KZ + 2)
    assert not d[..., C * KZ:].any()
    lhs = (kb.ref_zfold(t, None, C, KZ, pz)[0] * g.double()).sum()
    rhs = (t.double().permute(0, 2, 3, 4, 1) * d[..., :C * KZ].double()).sum()
    _close(lhs, rhs, 1e-10)


def test_zfold_dropped_tap_at_the_last_level_is_caught():
    row = (2, 3, 5, 2, 4, 3, 7)
    B, C, KZ, pz, X, Y, Z = row
    t, bias = _zfold_case(*row)
    ref, A = kb.ref_zfold(t, bias, C, KZ, pz)
    bnd = kb.bound(ref, A, KZ + 1, 0.0)
    for at in ((1, 2, 3, 2, 6), (0, 0, 0, 0, 4)):  # z = Z - 1 (its centre tap) and z = 4 (its last tap)
        assert _violations(_emul_zfold(t, bias, C, KZ, pz, drop=at), ref, bnd) == [at]


def _emul_plane_sum(src, drop_last_of_group=None):
    """``plane_sum_kernel`` (:1091) + ``chan_sum_final_kernel``: 256 threads per (channel, row) walk the samples of the
    row's batch group and its voxel slice, butterfly, (sh0 + sh1) + (sh2 + sh3), then the rows.
    ``drop_last_of_group``: that batch group stops one sample early."""
    B, C = src.shape[:2]
    s = src.reshape(B, C, -1)
    V = s.shape[2]
    rv, bper, rows = kb.plane_sum_rows(B, V)
    per = -(-V // rv)
    part = torch.zeros(rows, C)
    for row in range(rows):
        sl, bg = row % rv, row // rv
        v0, v1 = sl * per, min(sl * per + per, V)
        b0, b1 = bg * bper, min(bg * bper + bper, B)
        if drop_last_of_group == bg:
            b1 -= 1
        n = max(v1 - v0, 0)
        trips = max(-(-n // 256), 1)
        pad = torch.zeros(max(b1 - b0, 0), C, trips * 256)
        pad[:, :, :n] = s[b0:b1, :, v0:v1]
        acc = torch.zeros(C, 256)
        for b in range(pad.shape[0]):
            for i in range(trips):
                acc = acc + pad[b, :, i * 256:(i + 1) * 256]
        w = _butterfly(acc.view(C, 4, 64), torch.add)
        part[row] = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    return _emul_rows_sum(part), rows, bper


def _plane_case(B, C, V, seed=0):
    x = torch.randn((B, C, V), generator=torch.Generator().manual_seed(seed))
    x[:, C // 2] += 1000.0  # one channel at 1000 +- 1
    return x


@pytest.mark.parametrize("B,C,V", [(1, 1, 1), (1, 3, 16385), (5, 3, 1000), (600, 3, 64), (601, 3, 64), (3, 1024, 300)])
def test_plane_sum_emulation_is_within_the_bound(B, C, V):
    x = _plane_case(B, C, V)
    got, rows, bper = _emul_plane_sum(x)
    ref, A = kb.ref_plane_sum(x)
    w = kb.assert_within(got, ref, kb.bound(ref, A, B * V + rows, 0.0), f"emul plane_sum[{B}x{C}x{V}]")
    print(f"[ratio] plane_sum emulation ({B}, {C}, {V}): rows {rows} bper {bper} ratio {w:.3g}")


def test_plane_sum_last_sample_of_a_ragged_group_left_out_is_caught():
    B, C, V = 601, 3, 64
    rv, bper, rows = kb.plane_sum_rows(B, V)
    assert (rv, bper, rows) == (1, 2, 301) and B % bper == 1, "the last group holds one sample of two"
    x = _plane_case(B, C, V)
    ref, A = kb.ref_plane_sum(x)
    bnd = kb.bound(ref, A, B * V + rows, 0.0)
    assert not _violations(_emul_plane_sum(x)[0], ref, bnd)
    # 64 ordinary values out of 38 464 are below what a sum's bound can see in the randn channels (their A is
    # 30 000, the loss about 8): the channel at 1000 shows it, as does a planted sample of magnitude 1000
    assert (1,) in _violations(_emul_plane_sum(x, drop_last_of_group=rows - 1)[0], ref, bnd)
    x[B - 1] += 1000.0
    ref, A = kb.ref_plane_sum(x)
    assert _violations(_emul_plane_sum(x, drop_last_of_group=rows - 1)[0], ref, kb.bound(ref, A, B * V + rows, 0.0)) == [(0,), (1,), (2,)]


# ---------------------------------------------------------------------------------------------------------------------
# the table Adam family: reference against torch.optim.Adam, fp32 emulations of the kernels' arithmetic, mutants
# ---------------------------------------------------------------------------------------------------------------------

ADAM_HYPER = [(8e-5, 0.5, 0.999, 1e-8, 0.0, 1), (8e-5, 0.9, 0.999, 1e-8, 0.01, 2), (1e-2, 0.5, 0.999, 1e-8, 0.01, 1000),
              (0.5, 0.9, 0.99, 1e-8, 0.0, 100000)]
ADAM_SIZES = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1027, 32767, 32768, 32769, 65541]


def _adam_k(lr, b1, b2, eps, wd, step, *, step_off=0, omb2_f32=False, f32_hyper=False):
    """the eight ``AdamK`` constants as fp32 tensors (``adam_k``, elementwise.hip :608): double arithmetic, rounded once"""
    h = list(kb.adam_hyper(lr, (b1, b2), eps, wd, step - step_off, f32_hyper))
    if step_off:  # (the decay factors are not the mutant's business)
        h[:4] = kb.adam_hyper(lr, (b1, b2), eps, wd, step)[:4]
    k = [_f(x) for x in h]
    if omb2_f32:
        k[3] = _f(1.0) - _f(b2)
    return k


def _fma(a, b, c):
    """fp32 a * b + c with one rounding (the product of two fp32 values is exact in float64)"""
    return (a.double() * b.double() + c.double()).float()


def _emul_adam(p, g, m, v, k, *, contract=False, eps_inside=False, no_wd=False, decoupled=False, lr=None, tail_of=None):
    """``adam_one`` (elementwise.hip :618) in fp32, operation for operation; ``contract``: with the fused
    multiply-adds a compiler may form.  The switches are the mutants of the tests below; ``tail_of`` = n leaves the
    elements from 4 (n >> 2) on as they were."""
    b1, omb1, b2, omb2, ss, bc2s, eps, wd = k
    p0, m0, v0 = p, m, v
    if decoupled:
        p = p * (_f(1.0) - _f(lr) * wd)
    elif not no_wd and float(wd) != 0.0:
        g = _fma(wd, p, g) if contract else g + wd * p
    if contract:
        m = _fma(b1, m, omb1 * g)
        v = _fma(b2, v, omb2 * g * g)
    else:
        m = b1 * m + omb1 * g
        v = b2 * v + omb2 * g * g
    den = torch.sqrt(v + eps) / bc2s if eps_inside else torch.sqrt(v) / bc2s + eps
    q = m / den
    p = _fma(-ss, q, p) if contract else p - ss * q
    if tail_of is not None:
        t = 4 * (tail_of >> 2)
        p, m, v = (torch.cat([a[:t], a0[t:]]) for a, a0 in ((p, p0), (m, m0), (v, v0)))
    return p, m, v


def _adam_ratios(got, ref):
    """per output: (elements outside the bound, worst |err| / bound)"""
    return [kb.check_within(a, r, b)[:2] for a, (r, b) in zip(got, ref)]


def test_ref_adam_equals_torch_adam_in_float64():
    """``kb.ref_adam`` iterated over four steps against ``torch.optim.Adam`` on float64 CPU tensors (single-tensor
    form), parameters and both moments, for every hyper-parameter set's lr, betas and weight decay"""
    for lr, b1, b2, eps, wd, _ in ADAM_HYPER:
        gen = torch.Generator().manual_seed(3)
        p0 = torch.randn(257, generator=gen)
        w = p0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False, fused=False)
        p, m, v = p0.double(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
        for step in range(1, 5):
            g = torch.randn(257, generator=gen)
            w.grad = g.double()
            opt.step()
            (p, _), (m, _), (v, _) = kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step)
            st = opt.state[w]
            for a, b in ((p, w.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert float((a - b).abs().max()) <= 1e-13 * (1.0 + float(b.abs().max())), (lr, step)
    # the clip coefficient is a plain factor on the gradient
    g = torch.randn(9, generator=gen)
    z = torch.zeros(9)
    a = kb.ref_adam(z, g, z, z, 1e-2, (0.5, 0.999), 1e-8, 0.0, 1, coef=0.25)
    b = kb.ref_adam(z, (0.25 * g.double()), z, z, 1e-2, (0.5, 0.999), 1e-8, 0.0, 1)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))
    assert all(bool((x[1] >= y[1]).all()) for x, y in zip(a, b))  # (its three roundings widen the bound)


@pytest.mark.parametrize("contract", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("hyper", ADAM_HYPER, ids=lambda h: f"lr{h[0]}-b{h[1]}-wd{h[4]}-t{h[5]}")
def test_adam_emulation_is_within_the_bound(hyper, contract):
    """fp32 ``adam_one`` over every size of the matrix with its planted elements; the worst ratios are the CPU column of
    the calibration in kernel_bounds.py"""
    lr, b1, b2, eps, wd, step = hyper
    worst = [0.0, 0.0, 0.0]
    for n in ADAM_SIZES:
        p, g, m, v = kb.adam_case(n, step, n)
        got = _emul_adam(p, g, m, v, _adam_k(*hyper), contract=contract)
        res = _adam_ratios(got, kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step))
        assert all(bad == 0 for bad, _ in res), (n, res)
        worst = [max(w, r) for w, (_, r) in zip(worst, res)]
        # the planted elements: |g| = 1e-25 squares to zero in fp32 and the 2^-100 floor covers the reference's 1e-53
        tiny = g.abs() == 1e-25
        if bool(tiny.any()) and step == 1 and wd == 0.0:
            assert bool((got[2][tiny] == 0).all())
            rv, bv = kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step)[2]
            assert bool((rv[tiny] > 0).all()) and bool((rv[tiny] < kb.TINY).all()) and bool((bv[tiny] >= kb.TINY).all())
        still = (g == 0) & (m == 0) & (v == 0)
        if wd == 0.0 and bool(still.any()):
            assert torch.equal(got[0][still], p[still]) and not bool(got[1][still].any() or got[2][still].any())
    print(f"[emul] adam p / m / v worst ratios {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f}")
    assert max(worst) < 0.5


def test_adam_clip_emulation_is_within_the_bound():
    """the clip launch's arithmetic: c = max_norm / (total + 1e-6f) in fp32, g' = fl(c g) written back (K = 3), then
    ``adam_one`` on g' against ``ref_adam(coef=...)``"""
    hyper = ADAM_HYPER[2]
    lr, b1, b2, eps, wd, step = hyper
    p, g, m, v = kb.adam_case(1027, step, 5, plant=False)
    total = g.double().pow(2).sum().sqrt().float()
    for factor in (1 - 2.0 ** -10, 0.25):
        mx = _f(float(total) * factor)
        c32 = mx / (total + _f(1e-6))
        c64 = kb.clip_coef(total, float(mx))
        assert c64 < 1.0
        g1 = g * c32
        ref = c64 * g.double()
        assert kb.check_within(g1, ref, kb.bound(ref, ref.abs(), kb.K_CLIP_G, 0.0))[0] == 0
        res = _adam_ratios(_emul_adam(p, g1, m, v, _adam_k(*hyper)),
                           kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step, coef=c64))
        print(f"[emul] adam behind a clip of {factor:.4f}: p / m / v ratios " + " / ".join(f"{r:.3f}" for _, r in res))
        assert all(bad == 0 and r < 0.5 for bad, r in res), res


ADAM_MUTANTS = {  # name -> (emulation switches, constant switches, hyper rows it can show in, outputs it must leave)
    "bias_corrections_at_step_minus_1": (dict(), dict(step_off=1), (1, 2), "p"),
    "eps_inside_the_square_root": (dict(eps_inside=True), dict(), (0, 1, 2, 3), "p"),
    "weight_decay_dropped": (dict(no_wd=True), dict(), (1, 2), "pmv"),
    "decoupled_weight_decay": (dict(decoupled=True), dict(), (1, 2), "pmv"),
    "one_minus_beta2_in_fp32": (dict(), dict(omb2_f32=True), (0, 1, 2), "v"),
    "tail_left_as_it_was": (dict(tail=True), dict(), (0, 1, 2, 3), "pmv"),
}


@pytest.mark.parametrize("name", list(ADAM_MUTANTS))
def test_adam_mutant_is_rejected(name):
    """each mutant of ``adam_one`` leaves the bound of the outputs named for it, in every hyper-parameter row where it
    differs from the kernel at all.  Measured at n = 1027 without planted elements (elements outside the bound, worst
    |err| / bound):

    * bias corrections at step - 1 (rows with 1 < step <= 1000; at step 100 000 both corrections are 1 either way): p',
      821 of 1027 by up to 9000 at step 2, 717 by up to 38 at step 1000;
    * eps inside the root: p', every element with v' = 0 - a fifth of the tensor, set up here with g = 0, m = 0.25 - by
      1e5 (sqrt(eps) = 1e-4 in place of eps = 1e-8), and a few more where sqrt(v') is near sqrt(eps);
    * weight decay dropped: m' on 1026-1027 elements by 4e4-2e5, v' on 940-950 by 2e4-1e5, p' on 14 (lr = 8e-5, ratio
      20) to 1025 (lr = 1e-2, ratio 3e4); decoupled (AdamW) weight decay: the same m' and v', p' on 12 and 1004;
    * 1 - beta2 in fp32: v' on all 1027 elements at step 1 and on the 80-90 where the new term dominates later, by 5.5
      (the constant is out by 1.3e-5 relative) - THE FORM OF ``adam_kernel`` (elementwise.hip :597), the single-tensor
      entry ``wsr_adam_step``: rejected against torch's double hyper-parameters, accepted against the fp32 ones that
      entry receives, which is how test_optimizer_matrix.py references it.  The table kernels (``adam_k`` :608) take the
      constant in double and round once;
    * the n & 3 tail elements left as they were: m' and v' on all 3 by 3e3-5e5, p' on 1 to 3 of them by 9 (lr = 8e-5,
      |p| large beside the update) to 5e4."""
    emu, con, rows, outs = ADAM_MUTANTS[name]
    n = 1027
    for hi in rows:
        hyper = ADAM_HYPER[hi]
        lr, b1, b2, eps, wd, step = hyper
        p, g, m, v = kb.adam_case(n, step, 17 + hi, plant=False)
        if name == "eps_inside_the_square_root":
            v[::5] = 0.0  # (with g = 0 the denominator is eps alone: sqrt(eps) instead is out by 1e4)
            g[::5] = 0.0
            m[::5] = 0.25
        ref = kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step)
        good = _adam_ratios(_emul_adam(p, g, m, v, _adam_k(*hyper)), ref)
        assert all(bad == 0 for bad, _ in good), (name, hi, good)
        kw = dict(emu)
        if kw.pop("tail", False):
            kw["tail_of"] = n
        res = _adam_ratios(_emul_adam(p, g, m, v, _adam_k(*hyper, **con), lr=lr, **kw), ref)
        print(f"[mutant] {name} hyper {hi}: p {res[0]}, m {res[1]}, v {res[2]}")
        for o in outs:
            bad, worst = res["pmv".index(o)]
            assert bad >= 1 and worst > 2.0, (name, hi, o, res)
        if name == "tail_left_as_it_was":
            assert res[1][0] >= (n & 3) - (1 if step == 1 else 0)
        if name == "one_minus_beta2_in_fp32":  # accepted where the entry point is referenced from what it receives
            ref32 = kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step, f32_hyper=True)
            k32 = _adam_k(*hyper, f32_hyper=True)
            assert float(k32[3]) == float(_f(1.0) - _f(b2))  # 1 - float(beta2) is exact
            assert all(bad == 0 for bad, _ in _adam_ratios(_emul_adam(p, g, m, v, k32), ref32))


def _butterfly64(s):
    """``wg256_sum`` (elementwise.hip :659): xor butterfly over each wave of 64, then (sh0 + sh1) + (sh2 + sh3)"""
    s = s.view(4, 64)
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return (s[0, 0] + s[1, 0]) + (s[2, 0] + s[3, 0])


def _emul_grad_sqnorm(g, vec=True, skip_tail=False):
    """``grad_sqnorm_multi_kernel`` (:668) in fp32: four accumulators per thread over its float4s (stride 256), the tail
    into a0, (a0 + a1) + (a2 + a3), the butterfly and the four wave sums"""
    n = g.numel()
    acc = torch.zeros(256, 4)
    done = 0
    if vec:
        n4 = n >> 2
        trips = -(-n4 // 256)
        pad = torch.zeros(trips * 256 * 4)
        pad[:4 * n4] = g[:4 * n4]
        for t in pad.view(trips, 256, 4):
            acc = acc + t * t
        done = 4 * n4
    if not skip_tail:
        rest = g[done:]
        trips = -(-rest.numel() // 256)
        pad = torch.zeros(trips * 256)
        pad[:rest.numel()] = rest
        for t in pad.view(trips, 256):
            acc[:, 0] = acc[:, 0] + t * t
    return _butterfly64((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3]))


@pytest.mark.parametrize("vec", [True, False], ids=["float4", "scalar"])
def test_grad_sqnorm_emulation_is_within_the_bound_and_the_spike_shows_a_dropped_element(vec):
    """K = n + 10 holds for the kernel's order at every size; one ordinary element of 32 768 is below it (3e-5 of the
    sum against a bound of 1.7e-4), so a spike of 1024 stands at each designed index: left out of the tail it moves the
    partial by 6e3 (n = 32 767) to 3e5 (n = 5) bounds"""
    for n in ADAM_SIZES:
        if n > kb.ADAM_CHUNK:
            continue
        g = kb.adam_case(n, 2, n, plant=False)[1]
        ref, bnd = kb.ref_grad_sqnorm(g)
        assert kb.check_within(_emul_grad_sqnorm(g, vec), ref, bnd)[0] == 0, n
        if n >= 32767:
            assert float((g[5] ** 2).double() / bnd) < 1.0  # an ordinary element cannot be seen
        for i in sorted({0, 4 * (n >> 2), n - 1, min(n - 1, 4 * 256 + 2)} & set(range(n))):
            s = g.clone()
            s[i] = 1024.0
            ref, bnd = kb.ref_grad_sqnorm(s)
            assert kb.check_within(_emul_grad_sqnorm(s, vec), ref, bnd)[0] == 0, (n, i)
            if vec and n & 3 and i >= 4 * (n >> 2):
                bad, worst, _, _ = kb.check_within(_emul_grad_sqnorm(s, vec, skip_tail=True), ref, bnd)
                assert bad == 1 and worst > 1e3, (n, i, worst)


def _emul_clip_total(partials, drop=None):
    """the head of ``adam_multi_clip_kernel`` (:699-701): thread t adds partials[t], [t + 256], ... in double, the
    butterfly in double, one square root, one rounding to fp32"""
    n = partials.numel()
    trips = -(-n // 256)
    pad = torch.zeros(trips * 256, dtype=torch.float64)
    pad[:n] = partials.double()
    if drop is not None:
        pad[drop] = 0.0
    s = torch.zeros(256, dtype=torch.float64)
    for t in pad.view(trips, 256):
        s = s + t
    return _butterfly64(s).sqrt().float()


@pytest.mark.parametrize("n_jobs", [1, 2, 255, 256, 257, 512, 513, 600])
def test_clip_total_emulation_is_within_the_bound_and_a_dropped_partial_is_rejected(n_jobs):
    """K = n_jobs + 2.  With one partial dominating, dropping it (index 256: the second trip of thread 0) leaves the
    bound by 4e4 (600 jobs) to 6e5 (one job); an ordinary partial at index 256 is rejected too, by 84 among 257 and 40
    among 600 (the double sum is exact to 1e-16, the bound a few 1e-5 of the total)."""
    gen = torch.Generator().manual_seed(n_jobs)
    for big in sorted({0, 255, 256, 511, 512, n_jobs - 1} & set(range(n_jobs))):
        part = torch.rand(n_jobs, generator=gen) + 0.5
        part[big] = 1024.0 ** 2
        ref, bnd = kb.ref_clip_total(part)
        assert kb.check_within(_emul_clip_total(part), ref, bnd)[0] == 0
        bad, worst, _, _ = kb.check_within(_emul_clip_total(part, drop=big), ref, bnd)
        assert bad == 1 and worst > 1e4, (n_jobs, big, worst)
    if n_jobs > 256:
        part = torch.rand(n_jobs, generator=gen) + 0.5
        ref, bnd = kb.ref_clip_total(part)
        bad, worst, _, _ = kb.check_within(_emul_clip_total(part, drop=256), ref, bnd)
        print(f"[mutant] partial 256 of {n_jobs} dropped: ratio {worst:.3g}")
        assert bad == 1 and worst > 10.0


def test_clip_coefficient_mutants_are_rejected():
    """the coefficient left unclamped above 1 (max_norm = total (1 + 2^-10): every one of the 1027 g' out by
    2^-10 / 1.65e-6 = 590 bounds instead of bit-identical) and ``total + 1e-6`` omitted at a norm of 1e-7 (coef 0.5 instead of 0.045: every g' out
    by 6e6 bounds)"""
    g = kb.adam_case(1027, 2, 9, plant=False)[1]
    total = g.double().pow(2).sum().sqrt().float()
    mx = _f(float(total) * (1 + 2.0 ** -10))
    c64 = kb.clip_coef(total, float(mx))
    assert c64 == 1.0
    ref = c64 * g.double()
    bnd = kb.bound(ref, ref.abs(), kb.K_CLIP_G, 0.0)
    unclamped = g * (mx / (total + _f(1e-6)))
    bad, worst, _, _ = kb.check_within(unclamped, ref, bnd)
    assert bad >= 1000 and worst > 100, (bad, worst)
    tiny = g * _f(1e-7 / float(total))
    t = tiny.double().pow(2).sum().sqrt().float()
    mx = _f(0.5e-7)
    c64 = kb.clip_coef(t, float(mx))
    assert 0.04 < c64 < 0.05
    ref = c64 * tiny.double()
    bnd = kb.bound(ref, ref.abs(), kb.K_CLIP_G, 0.0)
    assert kb.check_within(tiny * (mx / (t + _f(1e-6))), ref, bnd)[0] == 0
    bad, worst, _, _ = kb.check_within(tiny * (mx / t), ref, bnd)
    assert bad >= 1000 and worst > 1e5, (bad, worst)
    # non-finite totals: inf gives a zero coefficient, NaN stays NaN
    assert kb.clip_coef(float("inf"), 1.0) == 0.0 and math.isnan(kb.clip_coef(float("nan"), 1.0))
    assert kb.clip_coef(3.0, float("inf")) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the glue kernels: lrelu_bwd, chan_axpby, upsample2_bwd, chan_sum
# ---------------------------------------------------------------------------------------------------------------------

GLUE_SPECIALS = {torch.bfloat16: (0x0000, -0x8000, 0x0001, -0x7FFF), torch.float32: (0, -0x80000000, 1, -0x7FFFFFFF)}
GLUE_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _glue_case(nvox, C, B, dt, seed):
    """(g, y, chan_scale): g bf16-exact, y with +0.0, -0.0 and both subnormals planted, keep factors {0, 1, 1.25}"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(nvox, C, generator=gen).to(dt)
    y = torch.randn(nvox, C, generator=gen).to(dt)
    vv = torch.arange(nvox)
    yb = y.view(GLUE_INT[dt])
    yb[vv, (vv * 5) % C] = torch.tensor(GLUE_SPECIALS[dt], dtype=GLUE_INT[dt])[vv % 4]
    cs = torch.tensor([1.25, 1.0, 0.0, 1.25])[torch.randint(0, 4, (B, C), generator=gen)]
    return g, y, cs


def _emul_lrelu_bwd(g, y, slope, cs, vpb, dt, *, sample0=False, flip=None):
    """``lrelu_bwd_kernel`` (:191) in fp32: m = (y > 0 ? 1 : slope) [* scale], g * m, one store"""
    pos = y.float() > 0
    if flip is not None:
        pos = pos ^ flip
    mm = torch.where(pos, torch.ones(()), _f(slope))
    if cs is not None:
        b = torch.arange(g.shape[0]) // vpb
        mm = mm * cs[torch.zeros_like(b) if sample0 else b]
    return (g.float() * mm).to(dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_lrelu_bwd_emulation_and_mutants(dt):
    """inside K = 2 (worst ratio 0.97 bf16, 0.044 fp32).  ``chan_scale`` of sample 0 used for every sample: rejected on
    6615 of the second sample's 10 080 elements - wherever the two samples' keep factors differ - by 50 and more, and by
    1e30 where the right factor is 0 and the bound is the 2^-100 floor; no element of sample 0 moves.  -0.0 taken as
    positive: all 118 planted elements on kept channels, by 1e3 (bf16) / 3e6 (fp32); a positive subnormal taken as not
    positive: all 98, by 200 / 6e5 (0.8 |g| against rho |ref| or 23 u |ref|)."""
    nvox, C, B = 630, 32, 2
    g, y, cs = _glue_case(nvox, C, B, dt, 4)
    ref, a, f = kb.ref_lrelu_bwd(g, y, 0.2, cs, nvox // B)
    bnd = kb.bound(ref, a, 2, kb.rho_for(dt))
    got = _emul_lrelu_bwd(g, y, 0.2, cs, nvox // B, dt)
    assert kb.check_within(got, ref, bnd)[0] == 0
    same = f == 1.0
    assert bool(same.any()) and torch.equal(got.view(GLUE_INT[dt])[same], g.view(GLUE_INT[dt])[same])
    bad, worst, _, ratio = kb.check_within(_emul_lrelu_bwd(g, y, 0.2, cs, nvox // B, dt, sample0=True), ref, bnd)
    assert bad >= 100 and worst > 50 and not bool((ratio[:nvox // B] > 1).any()), (bad, worst)
    bits = y.view(GLUE_INT[dt])
    sp = GLUE_SPECIALS[dt]
    kept = cs[torch.arange(nvox) // (nvox // B)] != 0
    for pat in (sp[1], sp[2]):
        flip = (bits == pat)
        assert int(flip.sum()) >= nvox // 4 - 1
        bad, worst, _, ratio = kb.check_within(_emul_lrelu_bwd(g, y, 0.2, cs, nvox // B, dt, flip=flip), ref, bnd)
        hit = flip & kept & (g.float() != 0)
        assert bool((ratio[hit] > 1).all()) and bad == int(hit.sum()) and worst > 50, (pat, bad, worst)


def test_chan_axpby_reading_dst_at_beta_zero_is_rejected():
    """beta * dst taken at beta == 0: 0 * NaN poisons every element (a non-finite result is an infinite ratio)"""
    gen = torch.Generator().manual_seed(1)
    s = torch.randn(77, 16, generator=gen).bfloat16()
    d = torch.full((77, 16), float("nan"))
    for al, be in ((1.0, 0.0), (0.2, 0.0), (1.0, 1.0), (1.0, 0.2), (-0.5, 2.0)):
        d0 = d if be == 0.0 else torch.randn(77, 16, generator=gen).bfloat16().float()
        ref, a = kb.ref_chan_axpby(s, d0, al, be)
        for dt in (torch.bfloat16, torch.float32):
            bnd = kb.bound(ref, a, 3, kb.rho_for(dt))
            o = _f(al) * s.float()
            got = o if be == 0.0 else o + _f(be) * d0
            assert kb.check_within(got.to(dt), ref, bnd)[0] == 0, (al, be)
            if be == 0.0:
                assert kb.check_within((o + _f(be) * d0).to(dt), ref, bnd)[0] == ref.numel()


def test_upsample2_bwd_reference_and_a_missing_fine_voxel():
    """the reference is the adjoint of nearest up-sampling (float64 autograd); the kernel's order of the three additions
    is inside K = 3; one of the four fine voxels left out is rejected on 477-480 of 480 elements, by 5e4 and more in
    bf16 and 5e5 in fp32"""
    gen = torch.Generator().manual_seed(2)
    dy = torch.randn(2, 6, 4, 5, 8, generator=gen).bfloat16()
    ref, a = kb.ref_upsample2_bwd(dy)
    x = torch.zeros(2, 3, 2, 5, 8, dtype=torch.float64, requires_grad=True)
    up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    (gx,) = torch.autograd.grad(up, x, dy.double())
    assert torch.equal(gx, ref)
    f = dy.float()
    parts = [f[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    for dt in (torch.bfloat16, torch.float32):
        bnd = kb.bound(ref, a, 3, kb.rho_for(dt))
        assert kb.check_within((((parts[0] + parts[1]) + parts[2]) + parts[3]).to(dt), ref, bnd)[0] == 0
        for k in range(4):
            got = sum(q for i, q in enumerate(parts) if i != k)
            bad, worst, _, _ = kb.check_within(got.to(dt), ref, bnd)
            assert bad >= int((parts[k] != 0).sum()) * 0.9 and worst > 30, (k, bad, worst)


def _emul_chan_sum(x, scale=1.0, *, drop_last_lane_of=None, twice_in_tail=False, group_shift=False):
    """``chan_sum_kernel`` (:875) + ``chan_sum_final_kernel`` (:909) in fp32 on window rows (nvox, C): thread =
    (voxel lane, 4-channel group) walks v = row lanes + lane + k step, eight voxels per trip of the unrolled loop -
    added in index order, so the order is the plain one - then the tail loop; lane 0 adds the lanes in order; the final
    kernel adds the rows.  Returns (out, partial table)."""
    nvox, C = x.shape
    _, lanes, rows = kb.chan_sum_geometry(C, nvox)
    step = rows * lanes
    if group_shift:
        x = x.roll(-4, dims=1)
    trips = -(-nvox // step)
    pad = torch.zeros(trips * step, C)
    pad[:nvox] = x
    pad = pad.view(trips, rows, lanes, C)
    acc = torch.zeros(rows, lanes, C)
    for k in range(trips):
        acc = acc + pad[k]
    if twice_in_tail:  # thread (row 0, lane 0): its first voxel after the unrolled trips, once more
        n0 = -(-nvox // step)  # voxels of that thread
        k = 8 * (n0 // 8) if n0 % 8 else n0 - 1
        acc[0, 0] = acc[0, 0] + pad[k, 0, 0]
    if drop_last_lane_of is not None:
        acc[drop_last_lane_of, lanes - 1] = 0.0
    part = acc[:, 0]
    for l in range(1, lanes):
        part = part + acc[:, l]
    return _f(scale) * _emul_rows_sum(part), part


CHAN_SUM_ROWS = [(4, 1), (4, 4097), (12, 1361), (48, 1000), (128, 8 * 16 + 1), (144, 3000), (1020, 300), (1024, 8197),
                 (128, 65541)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,nvox", CHAN_SUM_ROWS)
def test_chan_sum_emulation_is_within_the_bound(dt, C, nvox):
    gen = torch.Generator().manual_seed(C + nvox)
    x = (0.2 + torch.randn(nvox, C, generator=gen)).to(dt).float()
    _, lanes, rows = kb.chan_sum_geometry(C, nvox)
    for scale in (1.0, 0.2):
        out, part = _emul_chan_sum(x, scale)
        ref, a = kb.ref_chan_sum(x, scale)
        r = kb.check_within(out, ref, kb.bound(ref, a, nvox + rows, 0.0))
        print(f"[emul] chan_sum ({C}, {nvox}) scale {scale}: ratio {r[1]:.4f}")
        assert r[0] == 0 and r[1] < 0.5, r[:2]
    pref, pa = kb.ref_chan_sum_partials(x, C, nvox)
    assert kb.check_within(part, pref, kb.bound(pref, pa, -(-nvox // rows) + lanes, 0.0))[0] == 0
    assert torch.equal(pref.sum(0), kb.ref_chan_sum(x)[0]) or float((pref.sum(0) - x.double().sum(0)).abs().max()) < 1e-9


CHAN_SUM_MUTANTS = {  # name -> ((C, nvox), emulation switch, spike voxel or None)
    "last_lane_of_a_workgroup_dropped": ((12, 1361), dict(drop_last_lane_of=1), None),
    "last_lane_of_a_capped_grid_dropped": ((128, 65541), dict(drop_last_lane_of=511), "last_lane"),
    "tail_voxel_taken_twice": ((128, 65541), dict(twice_in_tail=True), "tail"),
    "tail_voxel_taken_twice_one_lane": ((1024, 8197), dict(twice_in_tail=True), "tail"),
    "channel_group_g_read_at_g_plus_1": ((48, 1000), dict(group_shift=True), None),
}


@pytest.mark.parametrize("name", list(CHAN_SUM_MUTANTS))
def test_chan_sum_mutant_is_rejected(name):
    """measured (channels outside the bound, worst |err| / bound): the last lane's voxels of workgroup 1 dropped at
    (12, 1361): 12 of 12, 190; on the capped rows one voxel in 65 541 is below the bound, which is why those rows carry
    a spike of 1024: the last lane of workgroup 511 dropped at (128, 65 541): 128 of 128, 79; the tail voxel of thread 0
    taken twice: 128 of 128, 79, and at (1024, 8197) 1024 of 1024, 1600; the channel group of thread g read at
    4 (g + 1) at (48, 1000): 48 of 48, 8e4 (the channels' means differ by 0.5)"""
    (C, nvox), kw, spike = CHAN_SUM_MUTANTS[name]
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(nvox, C, generator=gen) + torch.arange(C) % 7 * 0.5).bfloat16().float()
    _, lanes, rows = kb.chan_sum_geometry(C, nvox)
    step = rows * lanes
    if spike == "tail":
        n0 = -(-nvox // step)
        assert n0 % 8 == 1 and n0 > 8  # unrolled trips, then one tail voxel
        x[8 * (n0 // 8) * step] = 1024.0
    elif spike == "last_lane":
        x[511 * lanes + lanes - 1] = 1024.0
    ref, a = kb.ref_chan_sum(x)
    bnd = kb.bound(ref, a, nvox + rows, 0.0)
    assert kb.check_within(_emul_chan_sum(x)[0], ref, bnd)[0] == 0
    bad, worst, _, _ = kb.check_within(_emul_chan_sum(x, **kw)[0], ref, bnd)
    print(f"[mutant] chan_sum {name}: {bad} of {C} channels outside, worst ratio {worst:.3g}")
    assert bad >= C // 2 and worst > 10.0, (name, bad, worst)
