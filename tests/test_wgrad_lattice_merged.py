"""The four xy-parity classes of a lattice-form filter gradient in one launch (``conv_wgrad_parts_lat4``).

A lattice-form filter gradient is a set of stride-1 2x2xKZ' gradients, one per parity class (a, b):

* up-conv form (``wsr_conv_t.lat = 2``, the sub-pixel form of nearest x(2,2,1) + 3x3x3): class (a, b) contracts the
  un-sampled input, low pads (1 - a, 1 - b, 1), with the lattice (2x + a, 2y + b, z) of the output gradient;
* strided form (``lat = 3``, the discriminator's (4,4,3) stride (2,2,sz) convs): class (a, b) of z-class zc contracts
  the input lattice (2x + 1 - a, 2y + 1 - b, mz*z + oz), low pads (1 - a, 1 - b, pz), with the whole output gradient.

The merged launch runs the four classes of one tap shape side by side with S splits PER CLASS, each split walking the
tile list a single-class launch with the same S walks - so at a forced ``WSR_WGRAD_S`` the split copies and the reduced
class gradients must be the per-class launches' bit for bit.  Every gradient is also held to tests/kernel_bounds.py's
bound against float64 of the bf16 operands (K = voxels of the class + S), every output buffer is guarded.

Extents: the up-conv cases take the un-sampled input 8x8x16; the strided cases take descriptor input extents 8x8x8
(``wsr_conv_t`` with lat = 3: Xi, Yi, Zi are the LATTICE's extents - the stored tensor is 16x16x(8*sz)), which gives a
class 8 tiles so that S = 3 can be forced, plus the stored-8x8x8 volume (two tiles per class: S = 1 and 2).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import reload_wsr_env
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = torch.bfloat16


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def _ndhwc(t, ctot):
    """logical (B, C, X, Y, Z) -> NDHWC buffer of ``ctot`` channels holding it at [0, C); channels past C are NaN
    (never read: C is a multiple of 8 here)"""
    B, C, X, Y, Z = t.shape
    buf = torch.full((B, X, Y, Z, ctot), float("nan"), dtype=DT, device=DEV)
    buf[..., :C] = t.permute(0, 2, 3, 4, 1).to(DEV).to(DT)
    return buf


def _ref_class(xc, gc, k, lo):
    """float64 filter gradient (and its magnitude sum) of a stride-1 same-size conv with LOW pads ``lo`` (high pads
    k - 1 - lo): (Cout, Cin) + k"""
    pad = []
    for kk, p in reversed(list(zip(k, lo))):
        pad += [p, kk - 1 - p]
    out = []
    for xx, gg in ((xc.double(), gc.double()), (xc.double().abs(), gc.double().abs())):
        w = torch.zeros((gg.shape[1], xx.shape[1]) + tuple(k), dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv3d(F.pad(xx, pad), w), w, gg)
        out.append(g)
    return out


class Lattice:
    """operands, descriptors (four per-class ones and the merged one) and float64 class references of one launch"""

    def __init__(self, form, cin, cout, lat_xyz, B=2, sz=1, zc=0, seed=0):
        o = ops()
        X, Y, Z = lat_xyz
        gen = torch.Generator().manual_seed(seed + 7 * cin + cout + 3 * sz + zc + Z)
        self.form, self.cin, self.cout, self.B = form, cin, cout, B
        if form == "up":
            self.k, pz, tail = (2, 2, 3), 1, ()
            x = torch.randn((B, cin, X, Y, Z), generator=gen).bfloat16().float()
            gy = torch.randn((B, cout, 2 * X, 2 * Y, Z), generator=gen).bfloat16().float()
            gctot = cout + 16  # (the last up-conv's output gradient is a window of the concat buffer)
        else:
            kzp = 3 if sz == 1 else (1 if zc == 0 else 2)
            pz, mz, oz = (1, 1, 0) if sz == 1 else ((0, 2, 0) if zc == 0 else (1, 2, 1))
            self.k, tail = (2, 2, kzp), (mz, oz, True)
            x = torch.randn((B, cin, 2 * X, 2 * Y, mz * Z), generator=gen).bfloat16().float()
            gy = torch.randn((B, cout, X, Y, Z), generator=gen).bfloat16().float()
            gctot = cout
        self.taps = math.prod(self.k)
        self.vox = B * X * Y * Z
        self.xb, self.gb = _ndhwc(x, cin), _ndhwc(gy, gctot)
        self.d, self.ref = [], []
        for ph in range(4):
            a, b = ph >> 1, ph & 1
            lo = (1 - a, 1 - b, pz)
            off = (a, b) if form == "up" else (1 - a, 1 - b)
            self.d.append(o.make_desc(o.ConvGeom(cin, cout, self.k, (1, 1, 1), lo), DT, B, lat_xyz, cin, 0, gctot, 0,
                                      lat=off + (0,) + tail))
            if form == "up":
                xc, gc = x, gy[:, :, a::2, b::2, :]
            else:
                xc, gc = x[:, :, 1 - a::2, 1 - b::2, oz::mz], gy
            self.ref.append(_ref_class(xc, gc, self.k, lo))
        self.d4 = o.make_desc(o.ConvGeom(cin, cout, self.k, (1, 1, 1), (1, 1, pz)), DT, B, lat_xyz, cin, 0, gctot, 0,
                              lat=(0, 0, 4) + tail)

    def _reduce(self, parts4, n):
        """ordered reduce of the four classes' split copies -> ([4 master-layout gradients], guards)"""
        o = ops()
        dsts = [kb.Guarded((self.cout, self.cin) + self.k, torch.float32, DEV) for _ in range(4)]
        o.unpack_wgrad_reduce_multi(o.unpack_job_table(
            [(parts4[ph][0], dsts[ph].t, 1.0, n[ph], parts4[ph][0].numel()) for ph in range(4)]))
        torch.cuda.synchronize()
        return [d.t.cpu() for d in dsts], dsts

    def per_class(self):
        """-> (class gradients, split copies per class, splits per class)"""
        o = ops()
        guards, parts, n = [], [], []
        for ph in range(4):
            n.append(o.conv_wgrad_nparts(self.d[ph]))
            g = kb.Guarded((n[ph], self.cout, self.taps, self.cin), torch.float32, DEV)
            o.conv_wgrad_parts(self.d[ph], self.xb, self.gb, g.t, n[ph])
            guards.append(g)
            parts.append(g.t)
        out, dsts = self._reduce(parts, n)
        kb.assert_guards_intact(*guards, *dsts, label="per-class parts / reduced dw")
        return out, [p.cpu() for p in parts], n

    def merged(self):
        """-> (class gradients, split copies (4, n, Cout, taps, Cin), splits per class)"""
        o = ops()
        n = o.conv_wgrad_nparts_lat4(self.d4)
        assert n > 0, "the merged form declined this shape"
        g = kb.Guarded((4, n, self.cout, self.taps, self.cin), torch.float32, DEV)
        o.conv_wgrad_parts_lat4(self.d4, self.xb, self.gb, g.t, n)
        out, dsts = self._reduce([g.t[ph] for ph in range(4)], [n] * 4)
        kb.assert_guards_intact(g, *dsts, label="merged parts / reduced dw")
        return out, g.t.cpu(), n

    def check(self, got, S, label):
        for ph in range(4):
            ref, A = self.ref[ph]
            kb.assert_within(got[ph], ref, kb.bound(ref, A, self.vox + S, 0.0), f"{label}[class {ph}]", kind="filter")


def _forced_split_checks(c, monkeypatch, splits, name):
    got = {}
    for S in splits:
        monkeypatch.setenv("WSR_WGRAD_S", str(S))
        reload_wsr_env()
        assert ops().conv_wgrad_nparts_lat4(c.d4) == S, (name, S)
        per, per_parts, n = c.per_class()
        assert n == [S] * 4, (name, S, n)
        mer, mer_parts, n4 = c.merged()
        assert n4 == S
        for ph in range(4):
            assert torch.equal(mer_parts[ph], per_parts[ph]), (name, S, ph)
            assert torch.equal(mer[ph], per[ph]), (name, S, ph)
        assert all(torch.isfinite(m).all() for m in mer)
        c.check(per, S, f"lat4 per-class {name} S={S}")
        c.check(mer, S, f"lat4 merged {name} S={S}")
        got[S] = mer
    lo, hi = splits
    for ph in range(4):
        ref, A = c.ref[ph]
        kb.assert_within(got[hi][ph], got[lo][ph].double(), kb.bound(ref, A, c.vox + hi, 0.0),
                         f"lat4 merged {name} S={lo} vs S={hi}[class {ph}]", kind="filter")


UP_CASES = [(128, 128), (32, 32), (32, 64)]


@pytest.mark.parametrize("cin,cout", UP_CASES, ids=[f"{a}to{b}" for a, b in UP_CASES])
def test_upconv_merged_equals_per_class_at_forced_split(hip, monkeypatch, cin, cout):
    """up-conv form, un-sampled input 8x8x16, B = 2; S forced to 1 and 3 (several tiles per workgroup, the LDS ring
    wraps, a split crosses the batch boundary): merged == per-class bit for bit, both within the bound, S = 1 and
    S = 3 agree within the bound, the plan query reports the forced S"""
    c = Lattice("up", cin, cout, (8, 8, 16))
    _forced_split_checks(c, monkeypatch, (1, 3), f"up {cin}->{cout}")


STRIDED_CASES = [  # id, sz, zc, cin, cout, lattice extents, forced splits
    ("s221", 1, 0, 32, 64, (8, 8, 8), (1, 3)),
    ("s222_z0", 2, 0, 64, 128, (8, 8, 8), (1, 3)),
    ("s222_z1", 2, 1, 64, 128, (8, 8, 8), (1, 3)),
    ("s221_first", 1, 0, 32, 32, (8, 8, 8), (1, 3)),
    # the stored tensor itself 8x8x8: two tiles per class, so the splits that can be forced are 1 and 2
    ("s221_stored8", 1, 0, 32, 64, (4, 4, 8), (1, 2)),
    ("s222_z1_stored8", 2, 1, 64, 128, (4, 4, 4), (1, 2)),
]


@pytest.mark.parametrize("name,sz,zc,cin,cout,lat_xyz,splits", STRIDED_CASES, ids=[c[0] for c in STRIDED_CASES])
def test_strided_merged_equals_per_class_at_forced_split(hip, monkeypatch, name, sz, zc, cin, cout, lat_xyz, splits):
    """strided form, strides (2,2,1) and (2,2,2) (z-classes of 1 and 2 taps; 3 taps without a z stride), B = 2: the
    same assertions as the up-conv form"""
    c = Lattice("strided", cin, cout, lat_xyz, sz=sz, zc=zc)
    _forced_split_checks(c, monkeypatch, splits, name)


def test_declined_shape_keeps_per_class_result(hip):
    """65 chunk pairs x 4 classes leave no split per class within one round of 256 workgroups: the merged plan reports
    0, the launch is refused (WSR_EUNSUPPORTED, nothing written) and the per-class launches still give the result"""
    o = ops()
    c = Lattice("strided", 2080, 32, (4, 4, 8))
    assert o.conv_wgrad_nparts_lat4(c.d4) == 0
    g = kb.Guarded((4, 1, c.cout, c.taps, c.cin), torch.float32, DEV)
    before = g.t.view(torch.int32).clone()
    with pytest.raises(RuntimeError):
        o.conv_wgrad_parts_lat4(c.d4, c.xb, c.gb, g.t, 1)
    torch.cuda.synchronize()
    assert torch.equal(g.t.view(torch.int32), before), "a refused launch wrote to its output"
    kb.assert_guards_intact(g, label="refused merged launch")
    per, _, n = c.per_class()
    c.check(per, max(n), "lat4 declined: per-class")


@pytest.mark.parametrize("form,cin,cout,lat_xyz,sz,zc", [("up", 128, 128, (8, 8, 16), 1, 0), ("up", 32, 64, (8, 8, 16), 1, 0),
                                                         ("strided", 32, 64, (8, 8, 8), 1, 0),
                                                         ("strided", 64, 128, (8, 8, 8), 2, 1)],
                         ids=["up128", "up32to64", "s221", "s222_z1"])
def test_unforced_split(hip, form, cin, cout, lat_xyz, sz, zc):
    """the planner's own S (256 / (4 x chunk pairs) per class against 256 / chunk pairs): merged and per-class differ in
    the summation order only - both within the bound of the reference, and of each other; two merged launches are
    bit-identical"""
    c = Lattice(form, cin, cout, lat_xyz, sz=sz, zc=zc, seed=5)
    per, _, n = c.per_class()
    mer, parts_a, n4 = c.merged()
    mer2, parts_b, _ = c.merged()
    for ph in range(4):
        assert torch.equal(mer[ph], mer2[ph]), ph
    assert torch.equal(parts_a, parts_b)
    c.check(per, max(n), f"lat4 unforced per-class {form}")
    c.check(mer, n4, f"lat4 unforced merged {form}")
    for ph in range(4):
        ref, A = c.ref[ph]
        kb.assert_within(mer[ph], per[ph].double(), kb.bound(ref, A, c.vox + max(max(n), n4), 0.0),
                         f"lat4 unforced merged vs per-class {form}[class {ph}]", kind="filter")


# ---------------------------------------------------------------------------------------------------------------------
# LFF bias gradient inside the 1x1x1 filter-gradient launch (``conv_wgrad_parts_bias``)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("xyz", [(4, 4, 16), (6, 10, 12)], ids=["4x4x16", "6x10x12"])
def test_lff_bias_sums_in_the_filter_gradient_launch(hip, xyz, B):
    """256 -> 128, 1x1x1: split s of the launch also stores the channel sums of its share of dy.  The filter gradient's
    split copies are ``conv_wgrad_parts``' bit for bit (what WSR_LFF_BIAS_FUSED=0 launches); the ordered sum of the
    bias rows is within ``kb.bound(ref, A, vox, 0)`` of the float64 column sums and agrees with the two-pass
    ``chan_sum`` path within the same bound.  4x4x16: whole 16-level tiles; 6x10x12: a partial last tile (12-level
    tiles, the plain z form)."""
    o = ops()
    cin, cout = 256, 128
    gen = torch.Generator().manual_seed(11 + B + xyz[2])
    x = torch.randn((B, cin) + xyz, generator=gen).bfloat16().float()
    gy = torch.randn((B, cout) + xyz, generator=gen).bfloat16().float()
    xb, gb = _ndhwc(x, cin), _ndhwc(gy, cout)
    vox = B * math.prod(xyz)
    d = o.make_desc(o.ConvGeom(cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0)), DT, B, xyz, cin, 0, cout, 0)
    n = o.conv_wgrad_nparts(d)
    assert o.conv_wgrad_nparts_bias(d) == n > 0
    plain = kb.Guarded((n, cout, 1, cin), torch.float32, DEV)
    o.conv_wgrad_parts(d, xb, gb, plain.t, n)
    fused = kb.Guarded((n, cout, 1, cin), torch.float32, DEV)
    bp = kb.Guarded((n, cout), torch.float32, DEV)
    o.conv_wgrad_parts_bias(d, xb, gb, fused.t, n, bp.t)
    dw = kb.Guarded((cout, cin, 1, 1, 1), torch.float32, DEV)
    db = kb.Guarded((cout,), torch.float32, DEV)
    o.unpack_wgrad_reduce_multi(o.unpack_job_table([(fused.t[0], dw.t, 1.0, n, fused.t[0].numel()),
                                                    (bp.t[0].view(1, 1, cout), db.t.view(1, cout, 1), 1.0, n, cout)]))
    torch.cuda.synchronize()
    kb.assert_guards_intact(plain, fused, bp, dw, db, label="lff bias")
    assert torch.equal(fused.t.cpu(), plain.t.cpu())
    ref, A = kb.ref_wgrad(x, gy, (1, 1, 1), (0, 0, 0))
    kb.assert_within(dw.t.cpu(), ref, kb.bound(ref, A, vox + n, 0.0), f"lff dW fused[{xyz} B={B}]", kind="filter")
    bref = gy.double().sum(dim=(0, 2, 3, 4))
    bA = gy.double().abs().sum(dim=(0, 2, 3, 4))
    bnd = kb.bound(bref, bA, vox, 0.0)
    assert torch.isfinite(db.t).all()
    kb.assert_within(db.t.cpu(), bref, bnd, f"lff db fused[{xyz} B={B}]", kind="filter")
    # the two-pass channel sum the fused form replaces
    two = kb.Guarded((cout,), torch.float32, DEV)
    rows = o.chan_sum_rows(cout, vox)
    if rows:
        pr = kb.Guarded((rows, cout), torch.float32, DEV)
        o.chan_sum_partials(gb, 0, cout, pr.t)
        o.unpack_wgrad_reduce_multi(o.unpack_job_table([(pr.t[0].view(1, 1, cout), two.t.view(1, cout, 1), 1.0, rows, cout)]))
    else:
        assert o.chan_sum(gb, 0, cout, two.t)
    torch.cuda.synchronize()
    kb.assert_guards_intact(two, label="two-pass db")
    kb.assert_within(db.t.cpu(), two.t.cpu().double(), bnd, f"lff db fused vs two-pass[{xyz} B={B}]", kind="filter")
    kb.assert_within(two.t.cpu(), bref, bnd, f"lff db two-pass[{xyz} B={B}]", kind="filter")


def test_bias_form_declines_other_shapes(hip):
    """the bias sums live in the 1x1x1 tile instantiation alone: a 3x3x3 conv and a thin 1x1x1 conv report 0"""
    o = ops()
    assert o.conv_wgrad_nparts_bias(o.make_desc(o.ConvGeom(64, 64, (3, 3, 3)), DT, 1, (4, 4, 16), 64, 0, 64, 0)) == 0
    assert o.conv_wgrad_nparts_bias(o.make_desc(o.ConvGeom(32, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0)), DT, 1, (4, 4, 16), 32, 0, 32, 0)) == 0
