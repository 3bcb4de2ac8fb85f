"""The kernels at the network boundary - content loss, wind gradient, planar layout - element-wise against float64.

Every launch goes through the C entry points (``_lib.lib()``, as hip_ops.py calls them) so that every output lives in a
``kb.Guarded`` buffer: the Jacobians, the gradient, the 14 statistics, the ``1024 x 14`` partial table (pre-filled with
the sentinel: the rows past the launched workgroups must still hold it), the residual and ``dsr``.  Guards are compared
after every launch.  References and bounds: ``kernel_bounds.ref_wind_gradient`` .. ``ref_plane_sum`` (K in its
docstring), from the fp32 operands the kernel receives; the adjoint launch of the content loss is referenced from the
residual the first launch wrote.  One call per op goes through the ``hip_ops`` wrapper with backward.

Content loss and wind gradient (physics_loss.hip, elementwise.hip :1112 / :1142, stencil.h), shapes (B, X, Y, Z):

===================  ================================================================================================
shape                branch
===================  ================================================================================================
(1,1,1,1)            ``deriv_row`` n < 2 (stencil.h :15) on every axis: all derivatives 0; one thread, 255 idle lanes
                     keep the start values of the maxima (physics_loss.hip :54)
(1,1,1,2) (1,2,1,1)  one axis of two: the two one-sided rows (:16, :17), no interior row, the others n < 2
(1,1,2,1)
(1,2,2,2)            end rows only on every axis
(1,3,3,3)            one interior row (:18-20) per axis between the two ends
(2,1,6,5) (2,5,1,6)  a degenerate axis with the others live
(2,5,6,1)
(2,5,7,9)            630 voxels: three workgroups of the statistics pass, the last with 118 live lanes and two idle
                     waves; the batch boundary (voxel 315) inside workgroup 1: ``b * vol`` offsets of zc, hr, sr
(1,20,41,20)         16 400 voxels = 65 partial rows: lane 0 of ``physics_stats_final_kernel`` (:120) takes two rows
(1,37,71,100)        262 700 voxels: ``pl_grid`` (:223) capped at 1024 workgroups, 556 voxels on a second trip (:55)
(2,64,64,33)         270 336 voxels, 811 008 elements: ``ew_grid`` (elementwise.hip :18) capped at 2048 x 256, a
                     partial second trip of both wind-gradient kernels; the statistics pass capped as well
===================  ================================================================================================

Coordinates (``kb.boundary_inputs``): random non-uniform, exactly uniform, the nearly uniform ``100 i + 1e-5 i^1.5``
and data-like heights (about 1000 m, spacings of 5-50 m that vary per column); the heights differ between the samples.
Fields 10 + randn (the stencil cancels the mean), SR = HR + 0.1 randn, three planted elements with SR == HR.

The statistics' sums are held to two bounds.  The first, A = sum (M_sr + M_hr)^2, is several times the sum itself on
these fields (SR close to HR, a mean of 10 that the stencil cancels: at 630 voxels eight times, at 262 700 voxels two
hundred times): alone it would pass a sum of 0.  The second follows each entry's element bound through the square
(``kb.ref_physics_stats(tight_sums=True)``) and is a few thousandths of the sum.

Designed cases: a spike of 1024 on SR at flat voxel 0, 262 143, 262 144 and the last of (1,37,71,100) - over 262 700
terms neither bound of a sum can see one missing ordinary voxel (a term is 4e-6 of the sum, the narrower bound 3e-3 of
it), so the spike, which dominates every squared sum, moves sum |d| by sixty of its bounds and moves the SR maxima, and
the per-element gradient of the main rows are what cover the second trip.  A +1024 at voxel 0 (z = 0, the one-sided
row) only lowers the z-derivatives, so the signed
maximum is moved by a run with -1024 there.  Every z-derivative negative (maxima 1 and 5 below zero: a start value of
0 fails).  One NaN in component u of SR's last voxel (it enters J0, so every SR statistic; component w would miss
div2).  ``coef`` one-hot, each route on its own, the pixel routes bit for bit and +0.0 where SR == HR.  coef[0..3] == 0
with two equal levels in a column: residual +0.0 everywhere, dsr finite and the pixel term.  Determinism of the
statistics.

Layout kernels (elementwise.hip): ``planar_to_ndhwc_kernel`` :342 and ``ndhwc_to_planar_kernel`` :357 over the rows
(B, C, vpb, ctot, d_off, c_fill) of ``P2N_ROWS`` - a window inside the row, a single element, a window that ends at
ctot, no fill, and 655 360 elements for a second trip -, ``zfold_kernel`` :1005 / ``zunfold_kernel`` :1026 over
``ZFOLD_ROWS`` (pz = 0, pz = KZ - 1, KZ > Z with taps wholly outside, Z = 1, 589 824 outputs) and
``plane_sum_kernel`` :1091 with ``chan_sum_final_kernel`` :909 over ``PLANE_ROWS`` (one element; a second slice of one
voxel; bper = 1; ragged batch groups - 601 samples in groups of two; C = 1024, one final lane; 32 x 40960).  Copies are
compared as bit patterns (fp32: -0.0, infinities, subnormals and NaN payloads included; bf16: ``src.to(bfloat16)``, with
planted ties above an even and an odd code; fp32 subnormals are left out of the bf16 rows - how the conversion
instruction treats them is not established in the code).

What no test here can tell apart: whether a voxel of the statistics pass was visited on the first or the second trip
(only that it was visited once: the spike), and which of the two ``DISPATCH_T`` instantiations ran beyond the element
type of the buffer it was given.
"""
import ctypes
import functools

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
I32, I16 = torch.int32, torch.int16
COEF = torch.tensor([0.31, -0.17, 0.23, 0.41, 0.136, 0.07])
SENT32 = kb._SENTINEL_BITS[torch.float32]


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def call(name, *args):
    """the C entry point ``name`` on the current stream, raw pointers for tensors, as hip_ops.py calls it"""
    from gan_sr_wind_field_amd import _lib

    o = ops()
    conv = [ctypes.c_void_p(0) if a is None else (o._p(a) if isinstance(a, torch.Tensor) else a) for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, o._stream()), name)


def nan_out(shape, dt=torch.float32, window=None):
    return kb.Guarded(shape, dt, DEV, fill=NAN, window=window)


def done(*bufs, label):
    torch.cuda.synchronize()
    kb.assert_guards_intact(*bufs, label=label)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(I32 if t.dtype == torch.float32 else I16)


# ---------------------------------------------------------------------------------------------------------------------
# content loss and wind gradient
# ---------------------------------------------------------------------------------------------------------------------

class Case:
    """operands of one (shape, coords) row on the host and the device, the float64 Jacobians computed once"""

    def __init__(self, shape, coords, descending=False, seed=None):
        self.shape, self.coords = tuple(shape), coords
        self.tag = f"[{shape} {coords}]"
        seed = sum(shape) + 13 * len(coords) if seed is None else seed
        self.hr, self.sr, self.x, self.y, self.zc = kb.boundary_inputs(shape, coords, seed=seed, descending=descending)
        n = self.sr.numel()
        self.equal = sorted({0, n // 2, n - 1})  # planted SR == HR (flat element indices)
        for i in self.equal:
            self.sr.view(-1)[i] = self.hr.view(-1)[i]
        self.nvox = n // 3

    def host(self, sr=None, zc=None):
        return self.hr, self.sr if sr is None else sr, self.x, self.y, self.zc if zc is None else zc

    @functools.cached_property
    def jac(self):
        return (kb.ref_wind_gradient(self.hr, self.x, self.y, self.zc),
                kb.ref_wind_gradient(self.sr, self.x, self.y, self.zc))


@functools.lru_cache(maxsize=8)
def case(shape, coords):
    return Case(shape, coords)


def launch_stats(ops_host, label):
    """``wsr_physics_loss_stats`` into guarded buffers -> the 14 statistics on the host"""
    hr, sr, x, y, zc = (t.to(DEV) for t in ops_host)
    B, _, X, Y, Z = hr.shape
    stats = nan_out((14,))
    ws = kb.Guarded((kb.PL_ROWS, 14), torch.float32, DEV)  # (sentinel everywhere)
    call("wsr_physics_loss_stats", hr, sr, x, y, zc, stats.t, ws.t, B, X, Y, Z)
    done(stats, ws, label="physics_loss_stats" + label)
    rows = kb.physics_rows(B * X * Y * Z)
    wb = bits(ws.t)
    assert bool((wb[rows:] == SENT32).all()), f"partial rows past row {rows} written{label}"
    assert not bool((wb[:rows] == SENT32).any()), f"a partial of rows 0..{rows} not written{label}"
    return stats.t.cpu()


def ref_stats(c, sr=None):
    """(ref, bnd, narrower bound of the six sums) of a case, SR optionally replaced"""
    jac = c.jac if sr is None else (c.jac[0], kb.ref_wind_gradient(sr, c.x, c.y, c.zc))
    return kb.ref_physics_stats(*c.host(sr=sr), jac=jac, tight_sums=True)


def assert_stats(got, refs, label):
    """NaN exactly where the reference has NaN, every other entry within its bound, and the sums within the narrower
    bound that follows the element bounds through the squares (``kb.ref_physics_stats``)"""
    ref, bnd, tight = refs
    nan = torch.isnan(ref)
    assert torch.isnan(got).tolist() == nan.tolist(), f"{label}: NaN at {torch.isnan(got).tolist()}, want {nan.tolist()}"
    keep = ~nan
    print(f"[stats] {label}: got {got.tolist()}")
    kb.assert_within(got[keep], ref[keep], bnd[keep], label)
    if bool(keep[:4].all()):
        kb.assert_within(got[:4], ref[:4], tight[:4], label.replace("physics_stats", "physics_stats sums, propagated", 1))


def launch_bwd(ops_host, coef, label):
    """``wsr_physics_loss_bwd`` into guarded buffers -> (residual, dsr) on the host"""
    hr, sr, x, y, zc = (t.to(DEV) for t in ops_host)
    B, _, X, Y, Z = hr.shape
    res, dsr = nan_out((B, 9, X, Y, Z)), nan_out((B, 3, X, Y, Z))
    call("wsr_physics_loss_bwd", hr, sr, x, y, zc, coef.to(DEV), res.t, dsr.t, B, X, Y, Z)
    done(res, dsr, label="physics_loss_bwd" + label)
    return res.t.cpu(), dsr.t.cpu()


SMALL = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 2, 1, 1), (1, 1, 2, 1), (1, 2, 2, 2), (1, 3, 3, 3), (2, 1, 6, 5), (2, 5, 1, 6),
         (2, 5, 6, 1), (2, 5, 7, 9)]
ROWS = ([(s, c) for s in SMALL for c in ("random", "uniform", "near", "heights")]
        + [((1, 20, 41, 20), "random"), ((1, 20, 41, 20), "heights"), ((1, 37, 71, 100), "heights"),
           ((1, 37, 71, 100), "near"), ((2, 64, 64, 33), "random"), ((2, 64, 64, 33), "uniform")])


@pytest.mark.parametrize("shape,coords", ROWS, ids=lambda v: str(v).replace(" ", ""))
def test_content_loss_and_wind_gradient(hip, shape, coords):
    """both wind-gradient kernels, the statistics (twice: bit-identical), the residual and dsr of one row"""
    c = case(shape, coords)
    B, X, Y, Z = shape
    tag = c.tag
    hr, sr, x, y, zc = (t.to(DEV) for t in c.host())
    print(f"[row] {tag}: voxels {c.nvox} stats rows {kb.physics_rows(c.nvox)} trips {-(-c.nvox // (kb.physics_rows(c.nvox) * 256))} "
          f"element-wise trips {-(-3 * c.nvox // (2048 * 256))}")
    (jh, mh), (js, ms) = c.jac
    # forward of both fields
    for f, (J, M), name in ((hr, (jh, mh), "hr"), (sr, (js, ms), "sr")):
        out = nan_out((B, 9, X, Y, Z))
        call("wsr_wind_gradient", f, x, y, zc, out.t, B, X, Y, Z)
        done(out, label="wind_gradient" + tag)
        kb.assert_within(out.t, J, kb.bound(J, M, kb.K_STENCIL, 0.0), "wind_gradient" + tag)
    # adjoint of a random upstream gradient
    g = torch.randn((B, 9, X, Y, Z), generator=torch.Generator().manual_seed(3))
    df = nan_out((B, 3, X, Y, Z))
    call("wsr_wind_gradient_bwd", g.to(DEV), x, y, zc, df.t, B, X, Y, Z)
    done(df, label="wind_gradient_bwd" + tag)
    ref, A = kb.ref_wind_gradient_bwd(g, c.x, c.y, c.zc)
    kb.assert_within(df.t, ref, kb.bound(ref, A, kb.K_ADJOINT, 0.0), "wind_gradient_bwd" + tag)
    # statistics, twice
    got = launch_stats(c.host(), tag)
    assert_stats(got, ref_stats(c), "physics_stats" + tag)
    assert torch.equal(bits(launch_stats(c.host(), tag)), bits(got)), "statistics differ between two calls" + tag
    # residual, then dsr from the residual the kernel wrote
    res, dsr = launch_bwd(c.host(), COEF, tag)
    (rr, ra), (dr, da) = kb.ref_physics_bwd(*c.host(), COEF, residual=res, jac=c.jac)
    kb.assert_within(res, rr, kb.bound(rr, ra, kb.K_RESIDUAL, 0.0), "physics_residual" + tag)
    kb.assert_within(dsr, dr, kb.bound(dr, da, kb.K_DSR, 0.0), "physics_adjoint" + tag)


def test_hip_ops_wrappers_with_backward(hip):
    """``hip_ops.wind_gradient`` and ``hip_ops.physics_loss_stats`` through autograd at (2,5,7,9)"""
    o = ops()
    c = case((2, 5, 7, 9), "random")
    hr, sr, x, y, zc = (t.to(DEV) for t in c.host())
    (jh, mh), (js, ms) = c.jac
    f = sr.clone().requires_grad_(True)
    J = o.wind_gradient(f, x, y, zc)
    kb.assert_within(J.detach(), js, kb.bound(js, ms, kb.K_STENCIL, 0.0), "hip_ops.wind_gradient")
    g = torch.randn(J.shape, generator=torch.Generator().manual_seed(3))
    (J * g.to(DEV)).sum().backward()
    ref, A = kb.ref_wind_gradient_bwd(g, c.x, c.y, c.zc)
    kb.assert_within(f.grad, ref, kb.bound(ref, A, kb.K_ADJOINT, 0.0), "hip_ops.wind_gradient backward")
    f = sr.clone().requires_grad_(True)
    sums, mx = o.physics_loss_stats(hr, f, x, y, zc)
    assert_stats(torch.cat([sums.detach(), mx]).cpu(), ref_stats(c), "hip_ops.physics_stats")
    assert not mx.requires_grad
    (sums * COEF.to(DEV)).sum().backward()
    (rr, ra), (dr, da) = kb.ref_physics_bwd(*c.host(), COEF, jac=c.jac)
    # the residual stays inside the wrapper: its own error reaches dsr through the stencil weights' magnitudes
    through = kb.ref_wind_gradient_bwd(kb.bound(rr, ra, kb.K_RESIDUAL, 0.0), c.x, c.y, c.zc)[1]
    kb.assert_within(f.grad, dr, kb.bound(dr, da, kb.K_DSR, 0.0) + through, "hip_ops.physics_loss_stats backward")


BIG = (1, 37, 71, 100)
SPIKES = [(0, 1024.0), (0, -1024.0), (262143, 1024.0), (262144, 1024.0), (262699, 1024.0)]


@pytest.mark.parametrize("index,spike", SPIKES)
def test_spike_at_one_voxel_moves_the_statistics(hip, index, spike):
    """1024 on the three components of SR at one voxel of (1,37,71,100): first voxel, the last of the first trip, the
    first of the second trip, the last voxel.  The reference with the spike differs from the one without by more than
    four bounds (of the sums: the narrower ones) in every sum and every SR maximum it can reach, and the kernel matches
    the one with."""
    c = case(BIG, "heights")
    _, X, Y, Z = BIG
    sr = c.sr.clone()
    xi, yi, zi = index // (Y * Z), (index // Z) % Y, index % Z
    sr[0, :, xi, yi, zi] += spike
    base = ref_stats(c)[0]
    ref, bnd, tight = refs = ref_stats(c, sr)
    moved = ((ref - base).abs() > 4 * torch.cat([tight, bnd[6:]])).tolist()
    print(f"[spike] voxel {index} = ({xi}, {yi}, {zi}) {spike:+}: moved {moved}")
    lowers_only = zi == 0 and spike > 0  # the one-sided row at z = 0 sees -spike / h, the row above a negative weight
    want = [True] * 6 + [False] * 4 + [True, not lowers_only, True, True]
    assert moved == want
    assert bool((ref[[0, 1, 2, 3, 5]] > 2 * base[[0, 1, 2, 3, 5]]).all()), "the spike dominates the squared sums"
    assert_stats(launch_stats(c.host(sr=sr), f"[spike {index} {spike:+}]"), refs, f"physics_stats spike[{index} {spike:+}]")


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 1, 1, 2)], ids=str)
def test_every_z_derivative_negative(hip, shape):
    c = Case(shape, "heights", descending=True)
    ref = ref_stats(c)[0]
    assert bool((c.jac[0][0][:, 6:] < 0).all()) and bool((c.jac[1][0][:, 6:] < 0).all())
    got = launch_stats(c.host(), c.tag)
    assert_stats(got, ref_stats(c), "physics_stats negative z" + c.tag)
    assert float(got[6 + 1]) < 0 and float(got[6 + 5]) < 0 and float(ref[6 + 1]) < 0 and float(ref[6 + 5]) < 0


DESIGN_SHAPES = [((2, 5, 7, 9), "random"), ((1, 37, 71, 100), "heights"), ((2, 64, 64, 33), "random")]
DESIGN_IDS = ["630", "262700", "270336"]


@pytest.mark.parametrize("shape,coords", DESIGN_SHAPES, ids=DESIGN_IDS)
def test_one_nan_in_sr(hip, shape, coords):
    """NaN in component u of SR's last voxel: through ``nanmax`` in a lane, its wave, its row and the final wave into
    the four SR maxima, and into the six sums; the HR maxima stay finite and inside their bounds"""
    c = case(shape, coords)
    sr = c.sr.clone()
    sr[-1, 0, -1, -1, -1] = NAN
    refs = ref_stats(c, sr)
    assert torch.isnan(refs[0]).tolist() == [True] * 6 + [False] * 4 + [True] * 4
    assert_stats(launch_stats(c.host(sr=sr), c.tag + " NaN"), refs, "physics_stats NaN" + c.tag)


def pixel_term_bits(c, coef, sr=None):
    """coef[4] sign(d) or 2 coef[5] d in fp32 on the host: one rounding, so the kernel must give these bits"""
    d = (c.sr if sr is None else sr) - c.hr
    if float(coef[4]) != 0:
        return bits(coef[4] * torch.sign(d))
    return bits((2.0 * coef[5]) * d)


@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("shape,coords", DESIGN_SHAPES, ids=DESIGN_IDS)
def test_coef_one_hot(hip, shape, coords, k):
    """each of the six routes alone: the residual and dsr within their bounds; with only a pixel coefficient the
    residual is +0.0 everywhere and dsr the pixel term bit for bit, +0.0 at the planted SR == HR"""
    c = case(shape, coords)
    coef = torch.zeros(6)
    coef[k] = COEF[k]
    tag = f"{c.tag} coef[{k}]"
    res, dsr = launch_bwd(c.host(), coef, tag)
    (rr, ra), (dr, da) = kb.ref_physics_bwd(*c.host(), coef, residual=res, jac=c.jac)
    kb.assert_within(res, rr, kb.bound(rr, ra, kb.K_RESIDUAL, 0.0), "physics_residual one-hot" + tag)
    kb.assert_within(dsr, dr, kb.bound(dr, da, kb.K_DSR, 0.0), "physics_adjoint one-hot" + tag)
    live = {0: range(0, 6), 1: range(6, 9), 2: (0, 4, 8), 3: (0, 4)}.get(k, ())
    for ch in range(9):
        if ch not in live:
            assert not bool(bits(res[:, ch]).any()), f"residual channel {ch} not +0.0{tag}"
    if k >= 4:
        db = bits(dsr)
        assert torch.equal(db, pixel_term_bits(c, coef)), "pixel term not bit-identical" + tag
        assert not bool(db.view(-1)[c.equal].any()), "not +0.0 where SR == HR" + tag


@pytest.mark.parametrize("pix", [(4,), (5,), (4, 5)], ids=["l1", "l2", "both"])
@pytest.mark.parametrize("shape,coords", DESIGN_SHAPES, ids=DESIGN_IDS)
def test_no_physics_term_with_two_equal_levels(hip, shape, coords, pix):
    """coef[0..3] == 0 and a column with two equal heights (1 / dz = inf in the stencil rows): the residual is +0.0, dsr
    finite everywhere and the pixel term"""
    c = case(shape, coords)
    B, X, Y, Z = shape
    zc = c.zc.clone()
    zc[B - 1, 0, X // 2, Y // 2, Z - 1] = zc[B - 1, 0, X // 2, Y // 2, Z - 2]
    zc[0, 0, 0, 0, 1] = zc[0, 0, 0, 0, 0]
    coef = torch.zeros(6)
    for k in pix:
        coef[k] = COEF[k]
    tag = f"{c.tag} equal levels {pix}"
    res, dsr = launch_bwd(c.host(zc=zc), coef, tag)
    assert not bool(bits(res).any()), "residual not +0.0" + tag
    assert bool(torch.isfinite(dsr).all()), "non-finite dsr" + tag
    dr, da = kb.ref_physics_adjoint(res, c.hr, c.sr, c.x, c.y, zc, coef)
    kb.assert_within(dsr, dr, kb.bound(dr, da, kb.K_DSR, 0.0), "physics_adjoint equal levels" + tag)
    if len(pix) == 1:
        assert torch.equal(bits(dsr), pixel_term_bits(c, coef)), "pixel term not bit-identical" + tag


# ---------------------------------------------------------------------------------------------------------------------
# planar <-> NDHWC
# ---------------------------------------------------------------------------------------------------------------------

P2N_ROWS = [(2, 3, 120, 16, 4, 8), (1, 1, 1, 8, 0, 8), (2, 3, 120, 16, 8, 8), (1, 6, 77, 6, 0, 6), (2, 3, 40960, 8, 0, 8)]
F32_SPECIALS = [-0x80000000, 0x7F800000, -0x00800000, 0x00000001, -0x7FFFFFFF, 0x007FFFFF, 0x7FC12345, -0x003FFFFF]
#                -0.0        +inf        -inf         +-subnormals (three)                  NaN payloads (+, -)
BF16_SPECIALS = [-0x80000000, 0x7F800000, -0x00800000, 0x00000000]
TIES = [(0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (-0x407F8000, -0x4080), (-0x407E8000, -0x407E),
        (0x3F808001, 0x3F81), (0x3F817FFF, 0x3F81)]  # halfway above an even code, above an odd code, both signs; off ties


def planar_source(shape, dt, seed):
    """fp32 source with the special bit patterns of its destination type planted (see the module docstring)"""
    src = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    flat = src.view(-1).view(I32)
    planted = (F32_SPECIALS if dt == torch.float32 else BF16_SPECIALS + [t[0] for t in TIES])
    if flat.numel() >= 4 * len(planted):
        step = flat.numel() // len(planted)
        flat[torch.arange(len(planted)) * step + step // 2] = torch.tensor(planted, dtype=I32)
    if dt == torch.bfloat16 and flat.numel() >= 64:
        flat[1] = 0x7FC12345  # NaN stays NaN (its payload is not compared)
    return src


def test_the_bf16_reference_rounds_ties_to_even():
    """the host conversion the bf16 rows are compared with is round-to-nearest-even at the planted ties"""
    for f32, want in TIES:
        got = torch.tensor([f32], dtype=I32).view(torch.float32).to(torch.bfloat16).view(I16)
        assert int(got) == want, (hex(f32), hex(int(got)))


def expect_window(src_bcv, C, c_fill, dt):
    """(B, vpb, c_fill): the first C channels from the planar source, the rest +0.0, as the element type stores them"""
    B, _, vpb = src_bcv.shape
    out = torch.zeros((B, vpb, c_fill), dtype=torch.float32)
    out.view(I32)[..., :C] = src_bcv.view(I32).permute(0, 2, 1)
    return out if dt == torch.float32 else out.to(torch.bfloat16)


def assert_same_bits(got, want, label):
    """bit patterns equal; where ``want`` is a bf16 NaN, ``got`` is any NaN"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, label
    same = bits(got) == bits(want)
    if got.dtype == torch.bfloat16:
        same |= torch.isnan(got) & torch.isnan(want)
    if not bool(same.all()):
        bad = (~same).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{label}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: got "
                             f"{int(bits(got)[i]):#x} want {int(bits(want)[i]):#x}")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("row", P2N_ROWS, ids=str)
def test_planar_to_ndhwc_and_back(hip, row, dt):
    B, C, vpb, ctot, d_off, c_fill = row
    tag = f"[{row} {'bf16' if dt == torch.bfloat16 else 'fp32'}]"
    print(f"[row] planar_to_ndhwc{tag}: elements {B * vpb * c_fill} trips {-(-B * vpb * c_fill // (2048 * 256))}")
    src = planar_source((B, C, vpb), dt, seed=vpb + C)
    dst = kb.Guarded((B, vpb, ctot), dt, DEV, window=(d_off, c_fill))
    call("wsr_planar_to_ndhwc", src.to(DEV), dst.t, B, C, vpb, ctot, d_off, c_fill, ops().dtype_id(dt))
    done(dst, label="planar_to_ndhwc" + tag)
    want = expect_window(src, C, c_fill, dt)
    assert_same_bits(dst.window_view(), want, "planar_to_ndhwc" + tag)
    # back: the C source channels of the window the kernel wrote (sentinels around it), exact in both types
    back = nan_out((B, C, vpb))
    call("wsr_ndhwc_to_planar", dst.t, back.t, B, C, vpb, ctot, d_off, ops().dtype_id(dt))
    done(back, dst, label="ndhwc_to_planar" + tag)
    wrote = dst.window_view()[..., :C].cpu().float()  # (bf16 -> fp32 on the host is the same 16-bit shift)
    assert_same_bits(back.t, wrote.permute(0, 2, 1).contiguous(), "ndhwc_to_planar" + tag)
    if c_fill > C:  # the fill channels read back as +0.0 through their own offset
        fill = nan_out((B, c_fill - C, vpb))
        call("wsr_ndhwc_to_planar", dst.t, fill.t, B, c_fill - C, vpb, ctot, d_off + C, ops().dtype_id(dt))
        done(fill, label="ndhwc_to_planar fill" + tag)
        assert not bool(bits(fill.t).any()), "fill channels not +0.0" + tag


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_layout_wrappers(hip, dt):
    """``hip_ops.planar_to_ndhwc`` / ``ndhwc_to_planar`` on 5-D tensors, and the refusal of what is not planar fp32"""
    o = ops()
    B, C, X, Y, Z, ctot, off, fill = 2, 3, 4, 5, 6, 16, 8, 8
    src = planar_source((B, C, X * Y * Z), dt, seed=5)
    dst = kb.Guarded((B, X, Y, Z, ctot), dt, DEV, window=(off, fill))
    o.planar_to_ndhwc(src.view(B, C, X, Y, Z).to(DEV), dst.t, off, fill)
    done(dst, label="hip_ops.planar_to_ndhwc")
    want = expect_window(src, C, fill, dt)
    assert_same_bits(dst.window_view().reshape(B, -1, fill), want, "hip_ops.planar_to_ndhwc")
    back = o.ndhwc_to_planar(dst.t, C, off)
    wrote = dst.window_view()[..., :C].cpu().float().reshape(B, -1, C)
    assert_same_bits(back.reshape(B, C, -1), wrote.permute(0, 2, 1).contiguous(), "hip_ops.ndhwc_to_planar")
    with pytest.raises(ValueError):
        o.planar_to_ndhwc(src.view(B, C, X, Y, Z).to(DEV).to(torch.bfloat16), dst.t, off, fill)
    with pytest.raises(ValueError):
        o.planar_to_ndhwc(src.view(B, C, X, Y, Z).to(DEV).transpose(2, 3), dst.t, off, fill)


# ---------------------------------------------------------------------------------------------------------------------
# z-fold / z-unfold
# ---------------------------------------------------------------------------------------------------------------------

ZFOLD_ROWS = [(2, 3, 5, 2, 4, 3, 7), (1, 1, 1, 0, 1, 1, 1), (2, 3, 5, 0, 3, 2, 6), (2, 3, 5, 4, 3, 2, 6), (1, 2, 5, 2, 3, 3, 2),
              (1, 3, 3, 1, 2, 2, 1), (2, 3, 5, 2, 64, 64, 24)]
WINDOWS = [(16, 0, 16), (32, 8, 16), (15, 0, 15), (32, 16, 16)]  # (d_ctot, d_off, c_fill); the last ends at ctot


@pytest.mark.parametrize("row", ZFOLD_ROWS, ids=str)
def test_zfold(hip, row):
    B, C, KZ, pz, X, Y, Z = row
    gen = torch.Generator().manual_seed(KZ + Z)
    t = 10.0 + torch.randn((B, C * KZ, X, Y, Z), generator=gen)
    bias = torch.randn(C, generator=gen)
    print(f"[row] zfold[{row}]: outputs {B * C * X * Y * Z} trips {-(-B * C * X * Y * Z // (2048 * 256))}")
    td = t.to(DEV)
    for bb, name in ((bias, "bias"), (None, "no bias")):
        y = nan_out((B, C, X, Y, Z))
        call("wsr_zfold", td, y.t, None if bb is None else bb.to(DEV), B, C, KZ, pz, X * Y, Z)
        done(y, label=f"zfold[{row} {name}]")
        ref, A = kb.ref_zfold(t, bb, C, KZ, pz)
        kb.assert_within(y.t, ref, kb.bound(ref, A, KZ + 1, 0.0), f"zfold[{row} {name}]")
    if row == ZFOLD_ROWS[0]:  # the wrapper
        y = nan_out((B, C, X, Y, Z))
        ops().zfold(td, y.t, bias.to(DEV), KZ, pz)
        done(y, label="hip_ops.zfold")
        kb.assert_within(y.t, ref + bias.double().view(1, C, 1, 1, 1), kb.bound(ref, A + bias.abs().double().view(1, C, 1, 1, 1), KZ + 1, 0.0),
                         "hip_ops.zfold")
        with pytest.raises(ValueError):
            ops().zfold(td.transpose(2, 3), y.t, None, KZ, pz)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("row", ZFOLD_ROWS, ids=str)
def test_zunfold(hip, row, dt):
    """every element of the window is the bit pattern of its source voxel (bf16: its RNE) or +0.0"""
    B, C, KZ, pz, X, Y, Z = row
    g = planar_source((B, C, X, Y, Z), dt, seed=KZ + Z + 1)
    gd = g.to(DEV)
    windows = WINDOWS[:2] if X == 64 else WINDOWS
    for ctot, off, fill in windows:
        tag = f"[{row} window {(ctot, off, fill)} {'bf16' if dt == torch.bfloat16 else 'fp32'}]"
        d = kb.Guarded((B, X, Y, Z, ctot), dt, DEV, window=(off, fill))
        call("wsr_zunfold", gd, d.t, B, C, KZ, pz, X * Y, Z, ctot, off, fill, ops().dtype_id(dt))
        done(d, label="zunfold" + tag)
        want = kb.ref_zunfold(g, KZ, pz, fill)
        assert_same_bits(d.window_view(), want if dt == torch.float32 else want.to(torch.bfloat16), "zunfold" + tag)
    if row == ZFOLD_ROWS[0]:  # the wrapper, the last window
        d = kb.Guarded((B, X, Y, Z, ctot), dt, DEV, window=(off, fill))
        ops().zunfold(gd, d.t, KZ, pz, off, fill)
        done(d, label="hip_ops.zunfold")
        assert_same_bits(d.window_view(), want if dt == torch.float32 else want.to(torch.bfloat16), "hip_ops.zunfold")
        with pytest.raises(ValueError):
            ops().zunfold(gd.double(), d.t, KZ, pz, off, fill)


# ---------------------------------------------------------------------------------------------------------------------
# plane sums
# ---------------------------------------------------------------------------------------------------------------------

PLANE_ROWS = [(1, 1, 1), (1, 3, 16385), (5, 3, 1000), (600, 3, 64), (601, 3, 64), (3, 1024, 300), (32, 3, 40960)]


@pytest.mark.parametrize("B,C,V", PLANE_ROWS)
def test_plane_sum(hip, B, C, V):
    rv, bper, rows = kb.plane_sum_rows(B, V)
    print(f"[row] plane_sum[({B}, {C}, {V})]: voxel slices {rv} samples per group {bper} rows {rows} "
          f"last group {B - (rows // rv - 1) * bper} final lanes {1024 // C}")
    x = torch.randn((B, C, V), generator=torch.Generator().manual_seed(B + V))
    x[:, C // 2] += 1000.0  # one channel at 1000 +- 1
    out = nan_out((C,))
    part = kb.Guarded((512, C), torch.float32, DEV)
    call("wsr_plane_sum", x.to(DEV), B, C, V, out.t, part.t)
    done(out, part, label=f"plane_sum[({B}, {C}, {V})]")
    pb = bits(part.t)
    assert bool((pb[rows:] == SENT32).all()) and not bool((pb[:rows] == SENT32).any()), "partial rows"
    ref, A = kb.ref_plane_sum(x)
    kb.assert_within(out.t, ref, kb.bound(ref, A, B * V + rows, 0.0), f"plane_sum[({B}, {C}, {V})]")


def test_plane_sum_wrapper_and_refusals(hip):
    o = ops()
    x = torch.randn((5, 3, 10, 10, 10), generator=torch.Generator().manual_seed(2))
    out = nan_out((3,))
    o.plane_sum(x.to(DEV), out.t)
    done(out, label="hip_ops.plane_sum")
    ref, A = kb.ref_plane_sum(x)
    kb.assert_within(out.t, ref, kb.bound(ref, A, 5 * 1000 + 5, 0.0), "hip_ops.plane_sum")
    wide = torch.zeros((1, 1025, 4), device=DEV)
    with pytest.raises(RuntimeError, match="plane_sum"):
        o.plane_sum(wide, torch.zeros(1025, device=DEV))
    with pytest.raises(ValueError):
        o.plane_sum(x.to(DEV).to(torch.bfloat16), out.t)
    with pytest.raises(ValueError):
        o.plane_sum(x.to(DEV).transpose(2, 3), out.t)
    done(out, label="hip_ops.plane_sum refusals")
