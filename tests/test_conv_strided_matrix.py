"""Every launch of the strided forward halo-tile conv, checked element-wise against float64.

``wsr_ct_run_strided`` (conv_tile_strided.hip) carries the discriminator's bf16 down-sampling convs - kernels (4, 4, k),
stride (2, 2, 1|2) - and the (3, 3, 3) stride (1, 1, 2) conv of the slicing tail.  It walks four spatial tile shapes
(:20, each with TZ = min(TZ, Zo)) until ``launch_ct`` (conv_tile_impl.h) accepts one, and picks the channel-group
width of ``launch_ct<8, 1, 2, TN, 2>`` - NTW = TN n-tiles of 16 channels - from Cout and the tile count (:26-29).
``launch_ct`` may then split the reduction (conv_tile_impl.h :924-940).  One case per row below.

Every case
* has bf16-exact operands, the weights scaled by 1 / sqrt(taps * Cin);
* reads its input from the channel window [8, 8 + Cin) of a wider NDHWC buffer whose other channels hold NaN (residuals
  likewise), and writes a ``kb.Guarded`` buffer with a channel window; the guards are compared after every launch;
* is held to ``kb.ref_fwd(..., stride=...)`` - float64 ``F.conv3d`` of the operands and of their magnitudes - with
  ``kb.bound(ref, A, K = taps * Cin + ksplit, rho)``, rho = 2^-8 for bf16 stores and 0 for the planar fp32 output;
* asserts its tile shape, NTW, group count and split count through ``hip_ops.last_tile_plan()``, the record
  ``launch_ct`` leaves of its most recent launch (the expected values below were derived from the host arithmetic by
  hand; the witness is what holds them).

Tile-shape rungs (Cin 32 -> Cout 24, output window [4, 28) of 32 channels, bias + LeakyReLU, TN 2, one ragged group).
L = ((TX-1)sx+KX)((TY-1)sy+KY)((TZ-1)sz+KZ) halo voxels = ceil(L / 32) DMA units of the 13 * 8 = 104 a workgroup has
(conv_tile_impl.h :854):

===========  ======================  ================  =========  =====================================================
case id      kernel / stride / pad   input (X,Y,Z), B  tile       what it reaches
===========  ======================  ================  =========  =====================================================
s221_z10     (4,4,3) (2,2,1) (1,1,1)  (13,10,10), 2    4x4x10     production z; odd X; partial x and y tiles
s222_edge    (4,4,3) (2,2,2) (1,1,1)  (10,12,34), 1    4x4x16     L = 3300 = exactly 104 units; Zo = 17: the second z
                                                                  tile has one level
k5_edge      (4,4,5) (2,2,2) (1,1,2)  (10,12,29), 1    4x4x15     L = 3300 again, through TZ = Zo = 15
k5_z16       (4,4,5) (2,2,2) (1,1,2)  (10,12,31), 1    4x4x8      {4,4,16} (L = 3500) and {4,8,8} (3420) refused
k4_z16       (4,4,4) (2,2,2) (1,1,1)  (10,18,33), 1    4x8x8      {4,4,16} refused (3400); {4,8,8} fits (3240)
k188         (1,8,8) (2,2,2) (0,3,3)  (7,12,32), 1     4x4x8      KY = KZ = 8 in the magic divisions; 3724 and 3388
                                                                  refused
off32        (1,8,8) (2,2,2) (0,3,3)  (3,171,171), 1   2x4x8      Cin 16 in a 16 384-channel buffer: the 9 + 1 x-planes
                                                                  a TX = 4 halo may span hold 4.31e9 >= 2^32 elements
                                                                  (conv_tile_impl.h :855-858), the 5 + 1 of TX = 2 do
                                                                  not.  The same operands in a 32-channel buffer:
                                                                  4x4x8
tail_s112    (3,3,3) (1,1,2) (1,1,1)  (9,11,21), 2     4x4x11     the slicing tail's conv
asym         (3,4,3) (1,2,1) (1,1,1)  (7,11,9), 2      4x4x9      strides that differ in x and y; ragged everywhere
pad0         (4,4,3) (2,2,1) (0,0,0)  (11,12,9), 1     4x4x7      ``gx_lo`` (:308) without padding; the last input
                                                                  x-plane is never read
===========  ======================  ================  =========  =====================================================

The fourth shape, {2,4,8}, is out of reach of the halo size: with <= 8 taps per axis, <= 125 in all (conv_geom_ok) and
strides <= 2 the third shape's halo has at most 14 x 14 x 15 = 2940 voxels = 92 units.  Only the 32-bit offset test
turns {4,4,8} away, which is what ``off32`` does (an input of 2.9 GB; the float64 reference sees its 16 window
channels).  A fifth shape, {2,2,8}, could never be taken and was removed from the list.

Widths and channel groups (conv_tile_strided.hip :26-29), on s221_z10 and k5_z16:

================  ====================================================================================================
c256              default switches, Cout 256: 8 tiles -> "few" -> TN 2 in 8 groups (Cout 24 above: one ragged group)
natural           Cout 256 on 32 tiles (nat_s221: output 13x13x2, B 2; nat_k5: output 5x13x16, B 2; Cin 16): 32 * 2 <
                  128 <= 32 * 4 -> TN 4 in 4 groups with nothing forced
wide64/72/144     WSR_CT_STRIDED_WIDE=1: Cout 64 -> TN 4; Cout 72 -> TN 8, a group of 4.5 n-tiles; Cout 144 -> TN 8 in
                  two groups of 128 + 16
================  ====================================================================================================

Split reduction (conv_tile_impl.h :924-940: workspace passed, <= 128 workgroups, >= 4 chunks of 16 channels): s221_z10,
s222_edge and tail_s112 with Cin 64 (ksplit 2) and Cin 256 (ksplit 8), each with ``use_ws=True`` and - the single-pass
epilogue of the same launch - ``use_ws=False`` (ksplit 1); two split launches are bit-identical.

Epilogue forms on s221_z10, at TN 2 (Cout 24) and TN 8 (Cout 72 under WSR_CT_STRIDED_WIDE=1), and at TN 2 with Cin 64
and a workspace, where the forms the split reduction excludes must show ksplit 1:

==========  ===========================================================================================================
bias        bias only, as in front of a BatchNorm                                               (Cin 64: ksplit 2)
bias_act    bias + LeakyReLU                                                                     (Cin 64: ksplit 2)
res         alpha = 0.7, bias, a residual from another tensor at res_off = 8, beta = 0.3        (Cin 64: ksplit 1)
scale_act   bias + LeakyReLU + ``chan_scale`` (B, Cout)                                          (Cin 64: ksplit 1)
planar      bias, planar fp32 output (rho 0; the scalar epilogue, :742)                          (Cin 64: ksplit 1)
scalar      bias + LeakyReLU into the window [2, 2 + Cout) of Cout + 6 channels: ``vec_ok`` = 0  (Cin 64: ksplit 1)
==========  ===========================================================================================================

Declined launches return False and leave a guarded output bit-for-bit untouched: an fp32 descriptor, WSR_CT_NOSTRIDE=1,
Cin = 20 and in_off = 4 (no whole 16-byte pieces), Cin = 24 (no tap-pair K-step: conv_tile_strided.hip :10 has no
instantiation for it), ``upsample`` together with a stride.

The generic route: every rung row (bias + LeakyReLU) also runs through ``conv_fwd`` (conv_igemm.hip), the kernel of
every strided conv in fp32 mode and of whatever the tile kernel declines, in bf16 and fp32 against the same reference,
K = taps * Cin + 1.
"""
import functools
import math

import pytest
import torch

from conftest import reload_wsr_env
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = torch.bfloat16
NAN = float("nan")
IN_OFF = 8
ALPHA, BETA, SLOPE = 0.7, 0.3, 0.2

# case id -> kernel, stride, pad, input (X, Y, Z), B
CASES = {
    "s221_z10": ((4, 4, 3), (2, 2, 1), (1, 1, 1), (13, 10, 10), 2),
    "s222_edge": ((4, 4, 3), (2, 2, 2), (1, 1, 1), (10, 12, 34), 1),
    "k5_edge": ((4, 4, 5), (2, 2, 2), (1, 1, 2), (10, 12, 29), 1),
    "k5_z16": ((4, 4, 5), (2, 2, 2), (1, 1, 2), (10, 12, 31), 1),
    "k4_z16": ((4, 4, 4), (2, 2, 2), (1, 1, 1), (10, 18, 33), 1),
    "k188": ((1, 8, 8), (2, 2, 2), (0, 3, 3), (7, 12, 32), 1),
    "off32": ((1, 8, 8), (2, 2, 2), (0, 3, 3), (3, 171, 171), 1),
    "tail_s112": ((3, 3, 3), (1, 1, 2), (1, 1, 1), (9, 11, 21), 2),
    "asym": ((3, 4, 3), (1, 2, 1), (1, 1, 1), (7, 11, 9), 2),
    "pad0": ((4, 4, 3), (2, 2, 1), (0, 0, 0), (11, 12, 9), 1),
    "nat_s221": ((4, 4, 3), (2, 2, 1), (1, 1, 1), (26, 26, 2), 2),
    "nat_k5": ((4, 4, 5), (2, 2, 2), (1, 1, 2), (10, 26, 31), 2),
}
OFF32_CTOT = 16384

# expected launch plans: (TX, TY, TZ, NTW, ngroups, ksplit)
RUNGS = {  # case -> (Cin, in_ctot or None = Cin + 16, plan)
    "s221_z10": (32, None, (4, 4, 10, 2, 1, 1)),
    "s222_edge": (32, None, (4, 4, 16, 2, 1, 1)),
    "k5_edge": (32, None, (4, 4, 15, 2, 1, 1)),
    "k5_z16": (32, None, (4, 4, 8, 2, 1, 1)),
    "k4_z16": (32, None, (4, 8, 8, 2, 1, 1)),
    "k188": (32, None, (4, 4, 8, 2, 1, 1)),
    "off32": (16, OFF32_CTOT, (2, 4, 8, 2, 1, 1)),
    "tail_s112": (32, None, (4, 4, 11, 2, 1, 1)),
    "asym": (32, None, (4, 4, 9, 2, 1, 1)),
    "pad0": (32, None, (4, 4, 7, 2, 1, 1)),
}
OFF32_SMALL_PLAN = (4, 4, 8, 2, 1, 1)  # the same conv in a 32-channel buffer
TILE = {"s221_z10": (4, 4, 10), "k5_z16": (4, 4, 8), "s222_edge": (4, 4, 16), "tail_s112": (4, 4, 11)}
WIDTHS = [  # id, case, Cin, Cout, WSR_CT_STRIDED_WIDE, plan
    ("s221_z10-c256", "s221_z10", 32, 256, False, TILE["s221_z10"] + (2, 8, 1)),
    ("k5_z16-c256", "k5_z16", 32, 256, False, TILE["k5_z16"] + (2, 8, 1)),
    ("s221-natural", "nat_s221", 16, 256, False, (4, 4, 2, 4, 4, 1)),
    ("k5-natural", "nat_k5", 16, 256, False, (4, 4, 8, 4, 4, 1)),
    ("s221_z10-wide64", "s221_z10", 32, 64, True, TILE["s221_z10"] + (4, 1, 1)),
    ("s221_z10-wide72", "s221_z10", 32, 72, True, TILE["s221_z10"] + (8, 1, 1)),
    ("s221_z10-wide144", "s221_z10", 32, 144, True, TILE["s221_z10"] + (8, 2, 1)),
    ("k5_z16-wide64", "k5_z16", 32, 64, True, TILE["k5_z16"] + (4, 1, 1)),
    ("k5_z16-wide72", "k5_z16", 32, 72, True, TILE["k5_z16"] + (8, 1, 1)),
    ("k5_z16-wide144", "k5_z16", 32, 144, True, TILE["k5_z16"] + (8, 2, 1)),
]
SPLITS = [(c, cin, ks) for c in ("s221_z10", "s222_edge", "tail_s112") for cin, ks in ((64, 2), (256, 8))]
FORMS = ["bias", "bias_act", "res", "scale_act", "planar", "scalar"]
SPLIT_FORMS = {"bias", "bias_act"}  # the forms the split reduction takes
EPILOGUES = ([(f, "tn2", 32, 24, TILE["s221_z10"] + (2, 1, 1)) for f in FORMS] +
             [(f, "tn8", 32, 72, TILE["s221_z10"] + (8, 1, 1)) for f in FORMS] +
             [(f, "tn2", 64, 24, TILE["s221_z10"] + (2, 1, 2 if f in SPLIT_FORMS else 1)) for f in FORMS])


def _all_plans():
    yield from (p for _, _, p in RUNGS.values())
    yield OFF32_SMALL_PLAN
    yield from (w[-1] for w in WIDTHS)
    for c, _, ks in SPLITS:
        yield TILE[c] + (2, 1, ks)
        yield TILE[c] + (2, 1, 1)
    yield from (e[-1] for e in EPILOGUES)


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def out_extent(case):
    k, s, p, xyz, _ = CASES[case]
    return tuple((xyz[i] + 2 * p[i] - k[i]) // s[i] + 1 for i in range(3))


def _bf(t):
    return t.bfloat16().float()


@functools.lru_cache(maxsize=None)
def operands(case, cin, cout):
    """bf16-exact logical operands of a case on the host (shared by every launch of it, never written to)"""
    k, s, p, xyz, B = CASES[case]
    gen = torch.Generator().manual_seed(1000 * list(CASES).index(case) + 7 * cin + cout)
    taps = k[0] * k[1] * k[2]
    oxyz = out_extent(case)
    return dict(x=_bf(torch.randn((B, cin) + xyz, generator=gen)),
                w=_bf(torch.randn((cout, cin) + k, generator=gen) / math.sqrt(taps * cin)),
                bias=_bf(torch.randn(cout, generator=gen)),
                res=_bf(torch.randn((B, cout) + oxyz, generator=gen)),
                cs=_bf(torch.rand((B, cout), generator=gen) + 0.5))


def _ref_kw(form, op):
    f32 = kb._f32  # scalars as the C side receives them
    kw = dict(bias=op["bias"])
    if form in ("bias_act", "scale_act", "scalar"):
        kw.update(act=True, slope=f32(SLOPE))
    if form == "scale_act":
        kw.update(chan_scale=op["cs"])
    if form == "res":
        kw.update(alpha=f32(ALPHA), res=op["res"], beta=f32(BETA))
    return kw


@functools.lru_cache(maxsize=None)
def _reference(case, cin, cout, form):
    k, s, p, _, _ = CASES[case]
    op = operands(case, cin, cout)
    return kb.ref_fwd(op["x"], op["w"], p, stride=s, **_ref_kw(form, op))


def reference(case, cin, cout, form):
    """(ref, A) in float64, computed once per (case, widths, form) and shared by the tile and the generic route
    (``scalar`` is bias + LeakyReLU into another window: the same values)"""
    return _reference(case, cin, cout, "bias_act" if form == "scalar" else form)


def ndhwc(t, ctot, off, dt=DT):
    """logical (B, C, X, Y, Z) host tensor -> the window [off, off + C) of an NDHWC device buffer, NaN elsewhere"""
    B, C_, X, Y, Z = t.shape
    buf = torch.full((B, X, Y, Z, ctot), NAN, dtype=dt, device=DEV)
    buf[..., off:off + C_] = t.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    return buf


def _launch_kw(form, op, dt=DT):
    kw = dict(bias=op["bias"].to(DEV))
    if form in ("bias_act", "scale_act", "scalar"):
        kw.update(act=True, slope=SLOPE)
    if form == "scale_act":
        kw.update(chan_scale=op["cs"].to(DEV).contiguous())
    if form == "res":
        kw.update(alpha=ALPHA, beta=BETA, res=ndhwc(op["res"], op["res"].shape[1] + 16, 8, dt), res_off=8)
    if form == "planar":
        kw.update(out_planar=True)
    return kw


def _output(case, cout, form, dt=DT):
    """guarded output of a form and the view of it that holds the logical (B, Cout, Xo, Yo, Zo) result"""
    B, oxyz = CASES[case][4], out_extent(case)
    if form == "planar":
        g = kb.Guarded((B, cout) + oxyz, torch.float32, DEV)
        return g, g.t, 0, cout
    out_off, out_ctot = (2, cout + 6) if form == "scalar" else (4, cout + 8)
    g = kb.Guarded((B,) + oxyz + (out_ctot,), dt, DEV, window=(out_off, cout))
    return g, g.window_view().permute(0, 4, 1, 2, 3), out_off, out_ctot


def assert_plan(want, label):
    p = ops().last_tile_plan()
    print(f"[plan] {label}: {p}")
    got = tuple(p[f] for f in ("TX", "TY", "TZ", "NTW", "ngroups", "ksplit"))
    assert got == tuple(want), f"{label}: launch plan {p}, expected (TX, TY, TZ, NTW, ngroups, ksplit) = {want}"


def run_tile(case, cin, cout, form, plan, *, use_ws=True, in_ctot=None, tag=""):
    """one launch of ``conv_fwd_tile``: True, the expected plan, intact guards, every element within the bound.
    Returns (worst |err| / bound, the window's bits)"""
    o = ops()
    k, s, p, xyz, B = CASES[case]
    op = operands(case, cin, cout)
    in_ctot = cin + 16 if in_ctot is None else in_ctot
    xb = ndhwc(op["x"], in_ctot, IN_OFF)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV))
    g, view, out_off, out_ctot = _output(case, cout, form)
    d = o.make_desc(o.ConvGeom(cin, cout, k, s, p), DT, B, xyz, in_ctot, IN_OFF, out_ctot, out_off)
    assert (d.Xo, d.Yo, d.Zo) == out_extent(case)
    label = f"strided tile {case}{tag}[{cin}->{cout} {form}{'' if use_ws else ' no-ws'}]"
    assert o.conv_fwd_tile(d, xb, wf, g.t, use_ws=use_ws, **_launch_kw(form, op)) is True, label
    assert_plan(plan, label)
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    ref, A = reference(case, cin, cout, form)
    taps = k[0] * k[1] * k[2]
    rho = 0.0 if form == "planar" else kb.RHO_BF16
    worst = kb.assert_within(view, ref, kb.bound(ref, A, taps * cin + plan[5], rho), label)
    bits = view.contiguous().view(torch.int32 if form == "planar" else torch.int16).cpu()
    return worst, bits


class wsr_env:
    """WSR_* switches for the launches inside, read again by the C side on entry and on exit"""

    def __init__(self, monkeypatch, **switches):
        self.mp, self.switches = monkeypatch, switches

    def __enter__(self):
        for name, v in self.switches.items():
            self.mp.setenv(name, str(v))
        reload_wsr_env()

    def __exit__(self, *exc):
        for name in self.switches:
            self.mp.delenv(name)
        reload_wsr_env()


# ---------------------------------------------------------------------------------------------------------------------
# the tables themselves
# ---------------------------------------------------------------------------------------------------------------------

def test_expected_plans_cover_every_rung_width_and_both_reductions():
    """what the cases below assert through the witness, taken together: four tile-shape rungs, the three widths, the
    single pass and the split reduction"""
    plans = set(_all_plans())
    assert {(4, 4, 16), (4, 8, 8), (4, 4, 8), (2, 4, 8)} <= {p[:3] for p in plans}
    for case in ("k5_z16", "k188"):  # 4x4x8 as the third shape, not the first one on a volume of 8 levels
        assert RUNGS[case][2][:3] == (4, 4, 8) and out_extent(case)[2] > 8
    assert {p[3] for p in plans} == {2, 4, 8}
    assert {1, 2, 8} <= {p[5] for p in plans}
    assert any(p[4] > 1 for p in plans)
    # the DMA-unit edge of the docstring: both edge cases have exactly 104 * 32 - 28 halo voxels
    for case in ("s222_edge", "k5_edge"):
        k, s, _, _, _ = CASES[case]
        t = RUNGS[case][2]
        L = math.prod((t[i] - 1) * s[i] + k[i] for i in range(3))
        assert L == 3300 and (L + 31) // 32 == 13 * 8


# ---------------------------------------------------------------------------------------------------------------------
# tile-shape rungs
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(RUNGS))
def test_tile_shape_rung(hip, case):
    cin, in_ctot, plan = RUNGS[case]
    assert run_tile(case, cin, 24, "bias_act", plan, in_ctot=in_ctot)[0] <= 1.0
    if case == "off32":  # the same operands where the halo's planes stay below 2^32 elements: the third shape
        small = run_tile(case, cin, 24, "bias_act", OFF32_SMALL_PLAN, in_ctot=32, tag=" small buffer")
        assert small[0] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# widths and channel groups
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wid,case,cin,cout,wide,plan", WIDTHS, ids=[w[0] for w in WIDTHS])
def test_channel_group_width(hip, monkeypatch, wid, case, cin, cout, wide, plan):
    if wide:
        with wsr_env(monkeypatch, WSR_CT_STRIDED_WIDE=1):
            worst, _ = run_tile(case, cin, cout, "bias_act", plan, tag=" wide")
    else:
        worst, _ = run_tile(case, cin, cout, "bias_act", plan)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# split reduction
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,cin,ks", SPLITS, ids=[f"{c}-cin{n}" for c, n, _ in SPLITS])
def test_split_reduction_and_single_pass(hip, case, cin, ks):
    split = [run_tile(case, cin, 24, "bias_act", TILE[case] + (2, 1, ks), tag=f" split {i}") for i in range(2)]
    single = run_tile(case, cin, 24, "bias_act", TILE[case] + (2, 1, 1), use_ws=False)
    assert max(split[0][0], split[1][0], single[0]) <= 1.0
    assert torch.equal(split[0][1], split[1][1]), f"{case} Cin {cin}: two split launches differ"


# ---------------------------------------------------------------------------------------------------------------------
# epilogue forms
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,width,cin,cout,plan", EPILOGUES, ids=[f"{e[0]}-{e[1]}-cin{e[2]}" for e in EPILOGUES])
def test_epilogue_form(hip, monkeypatch, form, width, cin, cout, plan):
    if width == "tn8":
        with wsr_env(monkeypatch, WSR_CT_STRIDED_WIDE=1):
            worst, _ = run_tile("s221_z10", cin, cout, form, plan, tag=" wide")
    else:
        worst, _ = run_tile("s221_z10", cin, cout, form, plan)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# declined launches
# ---------------------------------------------------------------------------------------------------------------------

def _declined(geom, dt, cin, in_ctot, in_off, label, xyz=(13, 10, 10), B=2, cout=24):
    o = ops()
    gen = torch.Generator().manual_seed(cin + in_off)
    taps = math.prod(geom.kernel)
    xb = ndhwc(_bf(torch.randn((B, cin) + xyz, generator=gen)), in_ctot, in_off, dt)
    w = _bf(torch.randn((cout, cin) + tuple(geom.kernel), generator=gen) / math.sqrt(taps * cin))
    wf = o.pack_filter_frag(w.to(DEV), dtype=dt)
    d = o.make_desc(geom, dt, B, xyz, in_ctot, in_off, cout + 8, 4)
    g = kb.Guarded((B, d.Xo, d.Yo, d.Zo, cout + 8), dt, DEV, window=(4, cout))
    snap = g.base.view(kb._INT_VIEW[dt]).clone()
    before = o.last_tile_plan()
    assert o.conv_fwd_tile(d, xb, wf, g.t, bias=torch.zeros(cout, device=DEV), act=True) is False, label
    torch.cuda.synchronize()
    assert torch.equal(g.base.view(kb._INT_VIEW[dt]), snap), label
    assert o.last_tile_plan() == before, label  # (no halo-tile launch was made)


@pytest.mark.parametrize("what", ["fp32", "nostride", "cin20", "in_off4", "cin24", "upsample"])
def test_declined_launch_writes_nothing(hip, monkeypatch, what):
    o = ops()
    k, s, p = CASES["s221_z10"][:3]

    def geom(cin, **kw):
        return o.ConvGeom(cin, 24, k, s, p, **kw)

    if what == "fp32":
        _declined(geom(32), torch.float32, 32, 48, 8, what)
    elif what == "nostride":
        with wsr_env(monkeypatch, WSR_CT_NOSTRIDE=1):
            _declined(geom(32), DT, 32, 48, 8, what)
    elif what == "cin20":
        _declined(geom(20), DT, 20, 40, 8, what)
    elif what == "in_off4":
        _declined(geom(32), DT, 32, 48, 4, what)
    elif what == "cin24":
        _declined(geom(24), DT, 24, 40, 8, what)
    else:
        _declined(geom(32, upsample=True), DT, 32, 48, 8, what, xyz=(6, 5, 10))


# ---------------------------------------------------------------------------------------------------------------------
# the generic route
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", list(RUNGS))
def test_generic_kernel_on_the_same_cases(hip, case, dt):
    o = ops()
    k, s, p, xyz, B = CASES[case]
    cin, in_ctot, _ = RUNGS[case]
    cout, form = 24, "bias_act"
    in_ctot = cin + 16 if in_ctot is None else in_ctot
    op = operands(case, cin, cout)
    xb = ndhwc(op["x"], in_ctot, IN_OFF, dt)
    wp = o.pack_filter(op["w"].contiguous().to(DEV), dt)
    g, view, out_off, out_ctot = _output(case, cout, form, dt)
    d = o.make_desc(o.ConvGeom(cin, cout, k, s, p), dt, B, xyz, in_ctot, IN_OFF, out_ctot, out_off)
    label = f"strided generic {case}[{'bf16' if dt == DT else 'fp32'}]"
    before = o.last_tile_plan()
    o.conv_fwd(d, xb, wp, g.t, **_launch_kw(form, op, dt))
    torch.cuda.synchronize()
    assert o.last_tile_plan() == before, label  # (the generic kernel, not a halo-tile launch)
    kb.assert_guards_intact(g, label=label)
    ref, A = reference(case, cin, cout, form)
    assert kb.assert_within(view, ref, kb.bound(ref, A, math.prod(k) * cin + 1, kb.rho_for(dt)), label) <= 1.0
