"""Every instantiation of the two LDS-tile filter-gradient planners, checked element-wise against float64.

``wsr_wgrad_tile_bf16`` (conv_wgrad_tile.hip ``run_tile``) and ``wsr_wgrad_tile_f32`` (conv_wgrad_tile_f32.hip) pick a
template instantiation <TN, SPW, CT> from the taps and channel counts.  One case per instantiation (and per z-tile
form for bf16: Z16 = 16-level tiles, taken when Zo == 16, Zo % 16 == 0 or Zo > 64; otherwise Zo itself or 8 levels).
Every case runs a ragged volume (Zo not a multiple of 4 or 16 where the form allows, partial x / y tiles), Cout not a
multiple of 16, channel windows with in_off / out_off != 0 and ctot > C, and B = 2, through the atomic path
(``conv_wgrad``) and the split-copy path (``conv_wgrad_parts`` + ``unpack_wgrad_reduce_multi``), each against
tests/kernel_bounds.py's bound with every output buffer guarded; two split-copy launches are bit-identical.

Ring steady state: ``WSR_WGRAD_S`` forces the spatial split S (both planners).  With S = 1 and S = 3 on volumes of
>= 6 of the planner's largest tiles per sample (B = 2), every workgroup walks several tiles, its two-buffer LDS ring
wraps, and a split crosses the batch boundary.  ``conv_wgrad_nparts`` must report the forced S (which also shows
that the tile planner, not the per-tap fallback, took the shape); S = 1 and S = 3 agree within the bound.

bf16 planner (conv_wgrad_tile.hip ``run_tile``):

====================  ===============  ==========================================================================
instantiation         case id          branch (conv_wgrad_tile.hip)
====================  ===============  ==========================================================================
<8,1,8> Z16 / plain   b_881_z16/_nz    taps == 1, Cout >= 64, Cin >= 64 (:741-743)
<1,16,1> Z16 / plain  b_1161_*         taps > 28, Cout <= 16 (:745-746)
<3,16,1> Z16 / plain  b_3161_*         taps > 28, Cout % 48 == 0 (:747)
<2,16,1> Z16 / plain  b_2161_*         taps > 28, otherwise (:748)
<4,6,4> Z16 / plain   b_464_*          taps <= 12, Cout >= 64, Cin >= 64 (:751-753)
<2,3,2> Z16 / plain   b_232_*          taps <= 12, 16 < Cout <= 32 (:758-760)
<1,4,1> Z16 / plain   b_141_*          Cin <= 16, Cout <= 16 (:764-765)
<2,4,1> Z16 / plain   b_241_*          Cin <= 16, 16 < Cout <= 32 (:764-765)
<3,4,1> Z16 / plain   b_341_*          Cin <= 16, Cout % 48 == 0 (:771-772)
<1,7,2> Z16 / plain   b_172_*          <= 28 taps, Cout <= 16 (:776)
<2,7,2> Z16 / plain   b_272_*          <= 28 taps, Cout <= 32 (:777)
<4,7,2> Z16 / plain   b_472_*          <= 28 taps, otherwise (:778)
====================  ===============  ==========================================================================

fp32 planner (conv_wgrad_tile_f32.hip ``wsr_wgrad_tile_f32``; tiles of up to 16 z-levels, no Z16 form):

====================  ===============  ==========================================================================
<4,1,8>               f_418            taps == 1, Cout >= 64, Cin >= 64 (:302-304)
<1,16,1>              f_1161           taps > 28, Cout <= 16 (:307)
<3,16,1>              f_3161           taps > 28, Cout % 48 == 0 (:308)
<2,16,1>              f_2161           taps > 28, otherwise (:309)
<1,4,1>               f_141            Cin <= 16, Cout <= 16 (:311-312)
<4,4,1>               f_441            Cin <= 16, otherwise (:313)
<1,7,2>               f_172            Cout <= 16 (:315)
<2,7,2>               f_272            Cout <= 32 (:316)
<4,7,2>               f_472            otherwise (:317)
====================  ===============  ==========================================================================

(The 1x1x1 bf16 cases keep sum(voxels) % 128 != 0 or Zi % 16 == 0, so the planner does not re-shape the volume.
The 9-tap cases use a (1, 3, 3) kernel: a (3, 3, 1) one would take the flat 4-level tiles and never the Z16 form.)
"""
import math

import pytest
import torch

from conftest import reload_wsr_env, rel_l2
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NZ, Z16 = (10, 13, 19), (9, 10, 32)  # ragged volumes: z tiles of 8 (+3) / 16 levels, partial x / y tiles

BF16_CASES = [  # id, cin, cout, kernel, xyz
    ("b_881_nz", 136, 72, (1, 1, 1), NZ), ("b_881_z16", 136, 72, (1, 1, 1), Z16),
    ("b_1161_nz", 24, 12, (5, 5, 5), NZ), ("b_1161_z16", 24, 12, (5, 5, 5), Z16),
    ("b_3161_nz", 40, 48, (5, 5, 5), NZ), ("b_3161_z16", 40, 48, (5, 5, 5), Z16),
    ("b_2161_nz", 16, 24, (5, 5, 5), NZ), ("b_2161_z16", 16, 24, (5, 5, 5), Z16),
    ("b_464_nz", 64, 72, (1, 3, 3), NZ), ("b_464_z16", 64, 72, (1, 3, 3), Z16),
    ("b_232_nz", 40, 24, (1, 3, 3), NZ), ("b_232_z16", 40, 24, (1, 3, 3), Z16),
    ("b_141_nz", 16, 12, (3, 3, 3), NZ), ("b_141_z16", 16, 12, (3, 3, 3), Z16),
    ("b_241_nz", 8, 24, (3, 3, 3), NZ), ("b_241_z16", 8, 24, (3, 3, 3), Z16),
    ("b_341_nz", 16, 48, (3, 3, 3), NZ), ("b_341_z16", 16, 48, (3, 3, 3), Z16),
    ("b_172_nz", 40, 12, (3, 3, 3), NZ), ("b_172_z16", 40, 12, (3, 3, 3), Z16),
    ("b_272_nz", 40, 24, (3, 3, 3), NZ), ("b_272_z16", 40, 24, (3, 3, 3), Z16),
    ("b_472_nz", 40, 72, (3, 3, 3), NZ), ("b_472_z16", 40, 72, (3, 3, 3), Z16),
]
F32_CASES = [
    ("f_418", 68, 68, (1, 1, 1), NZ), ("f_1161", 20, 12, (5, 5, 5), NZ), ("f_3161", 20, 48, (5, 5, 5), NZ),
    ("f_2161", 12, 20, (5, 5, 5), NZ), ("f_141", 12, 12, (3, 3, 3), NZ), ("f_441", 12, 36, (3, 3, 3), NZ),
    ("f_172", 36, 12, (3, 3, 3), NZ), ("f_272", 36, 20, (3, 3, 3), NZ), ("f_472", 36, 68, (3, 3, 3), NZ),
]
CASES = [(torch.bfloat16,) + c for c in BF16_CASES] + [(torch.float32,) + c for c in F32_CASES]
IDS = [c[1] for c in CASES]


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def _rup(v, m):
    return (v + m - 1) // m * m


def _input(t, ctot, off, dt):
    """logical (B, C, X, Y, Z) -> NDHWC buffer of ``ctot`` channels holding it at [off, off + C); the rest of the
    16-byte piece holding the window's last channel is zero, every other channel NaN (never read)"""
    B, C, X, Y, Z = t.shape
    e = ops().piece_elems(dt)
    buf = torch.full((B, X, Y, Z, ctot), float("nan"), dtype=dt, device=DEV)
    buf[..., off:off + _rup(C, e)] = 0
    buf[..., off:off + C] = t.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    return buf


class Case:
    def __init__(self, dt, cin, cout, k, xyz, B=2, seed=0):
        o = ops()
        self.dt, self.cin, self.cout, self.k, self.xyz, self.B = dt, cin, cout, k, xyz, B
        e = o.piece_elems(dt)
        self.pad = tuple(kk // 2 for kk in k)
        self.taps = math.prod(k)
        gen = torch.Generator().manual_seed(seed + cin * 131 + cout + sum(k) + xyz[2])
        self.x = torch.randn((B, cin) + xyz, generator=gen).bfloat16().float()
        self.gy = torch.randn((B, cout) + xyz, generator=gen).bfloat16().float()
        in_off, out_off = e, e
        self.xb = _input(self.x, in_off + cin + 8, in_off, dt)
        self.gb = _input(self.gy, out_off + _rup(cout, 8) + 8, out_off, dt)
        self.d = o.make_desc(o.ConvGeom(cin, cout, k, (1, 1, 1), self.pad), dt, B, xyz, in_off + cin + 8, in_off,
                             out_off + _rup(cout, 8) + 8, out_off)
        self.vox = B * math.prod(xyz)
        self.ref, self.A = kb.ref_wgrad(self.x, self.gy, k, self.pad)

    def master(self, packed):
        """packed [Cout][taps][Cin] -> (Cout, Cin, KX, KY, KZ)"""
        return packed.permute(0, 2, 1).reshape((self.cout, self.cin) + self.k)

    def atomic(self):
        o = ops()
        n = o.conv_wgrad_nparts(self.d)
        g = kb.Guarded((self.cout, self.taps, self.cin), torch.float32, DEV, fill=0.0)
        o.conv_wgrad(self.d, self.xb, self.gb, g.t)
        torch.cuda.synchronize()
        kb.assert_guards_intact(g, label="dw (atomic)")
        return self.master(g.t.cpu()), n

    def parts(self, x2=None, x2_c0=0, d=None, xb=None):
        """split copies + ordered reduce -> (master-layout gradient, n_parts); the split count is the plan of the
        one-tensor descriptor (the two-tensor one holds more channels than its first tensor)"""
        o = ops()
        d = self.d if d is None else d
        n = o.conv_wgrad_nparts(self.d)
        p = kb.Guarded((n, self.cout, self.taps, self.cin), torch.float32, DEV)
        o.conv_wgrad_parts(d, self.xb if xb is None else xb, self.gb, p.t, n, x2=x2, x2_c0=x2_c0)
        dst = kb.Guarded((self.cout, self.cin) + self.k, torch.float32, DEV)
        table = o.unpack_job_table([(p.t[0], dst.t, 1.0, n, p.t[0].numel())])
        o.unpack_wgrad_reduce_multi(table)
        torch.cuda.synchronize()
        kb.assert_guards_intact(p, dst, label="parts / reduced dw")
        return dst.t.cpu(), n

    def check(self, got, K, label):
        return kb.assert_within(got, self.ref, kb.bound(self.ref, self.A, K, 0.0), label, kind="filter")


@pytest.fixture(scope="module")
def cases():
    """one Case (operands, device buffers, float64 reference) per geometry, built on first use and shared by the two
    parametrized tests below (pytest runs all of the first before any of the second); dropped with the module"""
    made = {}

    def get(*args):
        if args not in made:
            made[args] = Case(*args)
        return made[args]

    yield get
    made.clear()


@pytest.mark.parametrize("dt,name,cin,cout,k,xyz", CASES, ids=IDS)
def test_wgrad_tile_instantiation(hip, cases, dt, name, cin, cout, k, xyz):
    c = cases(dt, cin, cout, k, xyz)
    dw, n = c.atomic()
    assert rel_l2(dw, c.ref) < 2e-5, name
    c.check(dw, c.vox + n, f"wgrad {'bf16' if dt == torch.bfloat16 else 'fp32'} atomic[{name}]")
    dw1, n = c.parts()
    dw2, _ = c.parts()
    assert torch.equal(dw1, dw2), name  # deterministic split form: bit-identical launches
    c.check(dw1, c.vox + n, f"wgrad {'bf16' if dt == torch.bfloat16 else 'fp32'} parts[{name}]")


@pytest.mark.parametrize("dt,name,cin,cout,k,xyz", CASES, ids=IDS)
def test_wgrad_tile_ring_steady_state(hip, cases, monkeypatch, dt, name, cin, cout, k, xyz):
    c = cases(dt, cin, cout, k, xyz)
    got = {}
    for S in (1, 3):
        monkeypatch.setenv("WSR_WGRAD_S", str(S))
        reload_wsr_env()
        assert ops().conv_wgrad_nparts(c.d) == S, (name, S)
        got[S], n = c.parts()
        assert n == S
        c.check(got[S], c.vox + S, f"forced-S[{name} S={S}]")
    assert torch.isfinite(got[1]).all()
    kb.assert_within(got[3], got[1].double(), kb.bound(c.ref, c.A, c.vox + 3, 0.0), f"forced-S S1 vs S3[{name}]",
                     kind="filter")


def test_wgrad_tri_ring_steady_state(hip, monkeypatch):
    """stacked dense-block filter gradient (``conv_wgrad_tri``, four growth convs, conv i reads [0, nf + i*gc)) with
    forced S = 1 and 3: atomic and split-copy forms against the bound, per growth conv"""
    o = ops()
    dt, nf, gc, nconv, B, xyz = torch.bfloat16, 16, 8, 4, 2, NZ
    dense = nf + nconv * gc
    cin_w = nf + (nconv - 1) * gc
    gen = torch.Generator().manual_seed(78)
    x = torch.randn((B, dense) + xyz, generator=gen).bfloat16().float()
    g = torch.randn((B, dense) + xyz, generator=gen).bfloat16().float()
    xb, gb = _input(x, dense, 0, dt), _input(g, dense, 0, dt)
    d = o.make_desc(o.ConvGeom(cin_w, nconv * gc, (3, 3, 3)), dt, B, xyz, dense, 0, dense, nf)
    vox = B * math.prod(xyz)
    # float64 over all cin_w stacked input channels: conv i's gradient is its first nf + i*gc columns
    full = [kb.ref_wgrad(x[:, :cin_w], g[:, nf + i * gc:nf + (i + 1) * gc], (3, 3, 3), (1, 1, 1))
            for i in range(nconv)]
    refs = [(r[:, :nf + i * gc], a[:, :nf + i * gc]) for i, (r, a) in enumerate(full)]
    got = {}
    for S in (1, 3):
        monkeypatch.setenv("WSR_WGRAD_S", str(S))
        reload_wsr_env()
        n = o.conv_wgrad_nparts(d, nf, gc)
        assert n == S
        dwp = kb.Guarded((nconv * gc, 27, cin_w), torch.float32, DEV, fill=0.0)
        o.conv_wgrad_tri(d, xb, gb, dwp.t, nf, gc)
        parts = kb.Guarded((n, nconv * gc, 27, cin_w), torch.float32, DEV)
        o.conv_wgrad_parts(d, xb, gb, parts.t, n, nf, gc)
        dsts = [kb.Guarded((gc, nf + i * gc, 3, 3, 3), torch.float32, DEV) for i in range(nconv)]
        o.unpack_wgrad_reduce_multi(o.unpack_job_table(
            [(parts.t[0][i * gc:(i + 1) * gc], dsts[i].t, 1.0, n, parts.t[0].numel()) for i in range(nconv)]))
        torch.cuda.synchronize()
        kb.assert_guards_intact(dwp, parts, *dsts, label=f"tri S={S}")
        got[S] = []
        for i, (ref, A) in enumerate(refs):
            ci = nf + i * gc
            bnd = kb.bound(ref, A, vox + S, 0.0)
            atomic = dwp.t[i * gc:(i + 1) * gc, :, :ci].cpu().permute(0, 2, 1).reshape(gc, ci, 3, 3, 3)
            kb.assert_within(atomic, ref, bnd, f"tri atomic[S={S} conv {i}]", kind="filter")
            # columns [ci, cin_w) of conv i's rows are unspecified (windsr_hip.h wsr_conv3d_wgrad_tri): the kernel
            # either leaves them (still 0) or stores the products of the c-chunk it contracts anyway - anything
            # else there is a stray write
            rest = dwp.t[i * gc:(i + 1) * gc, :, ci:].cpu().permute(0, 2, 1).reshape(gc, cin_w - ci, 3, 3, 3)
            r_rest, a_rest = full[i][0][:, ci:], full[i][1][:, ci:]
            untouched = rest == 0
            kb.assert_within(rest, torch.where(untouched, 0.0, r_rest),
                             torch.where(untouched, kb.TINY, kb.bound(r_rest, a_rest, vox + S, 0.0)),
                             f"tri atomic unspecified columns[S={S} conv {i}]", kind="filter")
            kb.assert_within(dsts[i].t.cpu(), ref, bnd, f"tri parts[S={S} conv {i}]", kind="filter")
            got[S].append(dsts[i].t.cpu())
    for i, (ref, A) in enumerate(refs):
        kb.assert_within(got[3][i], got[1][i].double(), kb.bound(ref, A, vox + 3, 0.0), f"tri S1 vs S3[conv {i}]",
                         kind="filter")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_wgrad_concat_as_two_tensors_ring_steady_state(hip, monkeypatch, dt):
    """``conv_wgrad_parts(x2=...)`` (the generator's concat as two tensors: channels >= 128 from a second tensor) with
    forced S = 1 and 3 against the bound, and bit-identical to the same launch on the concatenated buffer"""
    o = ops()
    nf, tf, cout, B, xyz, k = 128, 16, 72, 2, NZ, (3, 3, 3)
    cin = nf + tf
    c = Case(dt, cin, cout, k, xyz, seed=2)
    xa = _input(c.x[:, :nf], nf, 0, dt)
    xt = _input(c.x[:, nf:], tf, 0, dt)
    d_two = o.make_desc(o.ConvGeom(cin, cout, k, (1, 1, 1), c.pad), dt, B, xyz, nf, 0, c.d.out_ctot, c.d.out_off,
                        cin=cin)
    for S in (1, 3):
        monkeypatch.setenv("WSR_WGRAD_S", str(S))
        reload_wsr_env()
        assert o.conv_wgrad_nparts(c.d) == S
        two, n = c.parts(x2=xt, x2_c0=nf, d=d_two, xb=xa)
        cat, _ = c.parts()
        assert torch.equal(two, cat), S
        c.check(two, c.vox + n, f"x2[{'bf16' if dt == torch.bfloat16 else 'fp32'} S={S}]")
