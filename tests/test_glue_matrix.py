"""The activation-gradient and bias-gradient glue of the backward pass, element-wise against float64 at edge shapes.

``lrelu_bwd_kernel`` :191, ``chan_axpby_kernel`` :214, ``upsample2_bwd_kernel`` :236, ``chan_sum_kernel`` :875 and
``chan_sum_final_kernel`` :909 (elementwise.hip), both element types in every row, operands exact in bf16, through the
C entry points as ``hip_ops`` calls them.  Every written buffer is a ``kb.Guarded``; the guards - the bands around the
tensor AND the channels outside the window - are compared after every launch.

Window rows ``WIN_ROWS`` = (nvox, g_ctot, g_off, y_ctot, y_off, C, B) of ``lrelu_bwd_inplace`` (K = 2) and, with
dst = g's and src = y's geometry, of ``chan_axpby`` (K = 3):

==========================================  =========================================================================
row                                         branch
==========================================  =========================================================================
(1, 4, 0, 4, 0, 4, 1)                       one thread of one workgroup (``i < total`` :196, :218)
(630, 256, 96, 128, 32, 32, 2), scale       windows inside both rows; the batch boundary at voxel 315 inside a
                                            workgroup's range (``v / vox_per_b`` :205)
(1000, 144, 0, 144, 0, 144, 1)              c4 = 36: ``i / c4``, ``i % c4`` with a width that is no power of two
(16389, 128, 0, 128, 0, 128, 3), scale      524 448 threads' worth: the second trip behind the ``ew_grid`` cap :20;
                                            16 389 = 3 * 5463
(77, 64, 48, 32, 16, 16, 1)                 both windows end at ctot
==========================================  =========================================================================

The saved output y holds +0.0, -0.0, the smallest positive subnormal of the type and its negative (bit patterns; one per
voxel, in turn); ``kb._lrelu_mask`` decides their sign, and test_kernel_bounds.py shows that taking either the wrong way
leaves the bound.  The keep factors are {0, 1, 1.25}: where the whole factor is 1 the element comes back bit for bit,
a factor of 0 gives a zero of g's sign.  y = NaN is not asserted.  ``chan_axpby`` runs (alpha, beta) in {(1, 0),
(0.2, 0), (1, 1), (1, 0.2), (-0.5, 2)}; with beta = 0 the destination window holds NaN before the launch and must come
out finite (:224: not read).

``upsample2_bwd`` rows (B, Xi, Yi, Zi, C), K = 3: (1,1,1,1,4) one thread; (2,3,2,5,8) and (2,4,4,10,128) two samples
(``b = v / Xi`` :248); (1,1,7,1,32) and (1,5,1,3,144) axes of length one and c4 = 36; (1,16,16,33,256): 540 672 threads,
the second trip, dy of 8.65 M elements.  dx is NaN-filled.  Then dy one-hot in turn at each of the four fine positions
(:250 ``p``, ``p + rowY``, ``p + rowX``, ``p + rowX + rowY``) of the first and the last coarse voxel of each sample: dx is
that voxel's values at that coarse voxel and +0.0 elsewhere, exactly.

``chan_sum`` rows (C, ctot, off, nvox), K = nvox + rows, scale in {1, 0.2}:

=========================  ==========================================================================================
row                        branch
=========================  ==========================================================================================
(4, 4, 0, 1)               one group, 256 lanes of which one has a voxel; one row
(4, 8, 4, 4097)            256 lanes, grid 2 (:1728); a window
(12, 16, 4, 1361)          85 lanes, thread 255 idle (``vl < lanes`` :882), grid 2
(48, 256, 96, 1000)        21 lanes, four idle threads
(128, 128, 0, 129)         8 lanes, 2 rows; threads with one and with two voxels
(144, 144, 0, 3000)        7 lanes; the final kernel :909 with 7 row lanes
(1020, 1024, 4, 300)       255 groups, one lane, thread 255 idle; final kernel: 4 idle threads
(1024, 1024, 0, 8197)      one lane, grid capped at 512 (``WSR_CHAN_SUM_ROWS`` :1729); final kernel with one row lane
(128, 128, 0, 65541)       grid capped; 16 or 17 voxels per thread: the unrolled loop :885 twice, then the tail :892
=========================  ==========================================================================================

``chan_sum_rows`` must equal the workgroups launched: the partial table is a 512-row guarded buffer of sentinels, the
rows written are held to their own float64 sums (row r: the voxels with (v / lanes) % rows == r), the rows past them must
still hold the sentinel.  On the two capped rows one ordinary voxel is below the bound of the sum (see
test_kernel_bounds.py), so a spike of 1024 stands in turn at voxel 0, at 7 step (the last voxel of thread 0's first
unrolled batch), at 16 step (the voxel its tail loop takes: with 17 voxels per thread the unrolled loop ends at
16 step, not at 7 step) and at the last voxel.  One row runs the engine's own form (engine.py :1384-1386):
``chan_sum_partials``, then a ``wsr_unpack_wgrad_reduce_multi`` job over the partial rows, accumulate off and on.

What no test here can tell apart: which trip of a grid-stride loop took an element (only that it was taken once), and
whether a thread's voxels went through the unrolled loop or the tail loop of ``chan_sum_kernel`` - both add in index
order - beyond each being summed exactly once (the spikes).
"""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SLOPE = 0.2
DTS = [torch.bfloat16, torch.float32]
DT_IDS = ["bf16", "fp32"]
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SPECIALS = {torch.bfloat16: (0x0000, -0x8000, 0x0001, -0x7FFF),  # +0.0, -0.0, +subnormal, -subnormal
            torch.float32: (0x00000000, -0x80000000, 0x00000001, -0x7FFFFFFF)}
SENTINEL = kb._SENTINEL_BITS[torch.float32]

# (nvox, g_ctot, g_off, y_ctot, y_off, C, B, scale?)
WIN_ROWS = [(1, 4, 0, 4, 0, 4, 1, False), (630, 256, 96, 128, 32, 32, 2, True), (1000, 144, 0, 144, 0, 144, 1, False),
            (16389, 128, 0, 128, 0, 128, 3, True), (77, 64, 48, 32, 16, 16, 1, False)]
WIN_IDS = ["one", "windows-batch2", "c144", "second-trip-batch3", "window-ends-at-ctot"]


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def name_of(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


def done(*bufs, label):
    torch.cuda.synchronize()
    kb.assert_guards_intact(*bufs, label=label)


def window_case(row, dt, seed):
    """(g, y, chan_scale) on the CPU: window rows (nvox, C) of ``dt`` and fp32 keep factors (B, C)"""
    nvox, _, _, _, _, C, B, _ = row
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(nvox, C, generator=gen).to(dt)
    y = torch.randn(nvox, C, generator=gen).to(dt)
    v = torch.arange(nvox)
    y.view(INT[dt])[v, (v * 5) % C] = torch.tensor(SPECIALS[dt], dtype=INT[dt])[v % 4]
    cs = torch.tensor([1.25, 1.0, 0.0, 1.25])[torch.randint(0, 4, (B, C), generator=gen)]
    return g, y, cs


def in_row(t, ctot, off, dt, gen):
    """the window rows ``t`` (nvox, C) inside full rows (nvox, ctot) of random values, on the device"""
    full = torch.randn(t.shape[0], ctot, generator=gen).to(dt)
    full[:, off:off + t.shape[1]] = t
    return full.to(DEV)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("row", WIN_ROWS, ids=WIN_IDS)
def test_lrelu_bwd_inplace(hip, row, dt):
    o = ops()
    nvox, g_ctot, g_off, y_ctot, y_off, C, B, scaled = row
    tag = f"[{name_of(dt)} {row}]"
    print(f"[row] lrelu_bwd{tag}: {nvox * (C >> 2)} threads' worth, {-(-nvox * (C >> 2) // (2048 * 256))} trip(s)")
    g, y, cs = window_case(row, dt, 100 + nvox)
    gen = torch.Generator().manual_seed(1)
    if nvox >= 4:
        assert all(bool((y.view(INT[dt]) == s).any()) for s in SPECIALS[dt])
    gd = kb.Guarded((B, nvox // B, g_ctot), dt, DEV, window=(g_off, C), fill=g.to(DEV).view(B, nvox // B, C))
    yd = in_row(y, y_ctot, y_off, dt, gen).view(B, nvox // B, y_ctot)
    csd = cs.to(DEV) if scaled else None
    o.lrelu_bwd_(gd.t, g_off, yd, y_off, C, SLOPE, csd)
    done(gd, label="lrelu_bwd" + tag)
    ref, a, f = kb.ref_lrelu_bwd(g, y, SLOPE, cs if scaled else None, nvox // B)
    got = gd.window_view().reshape(nvox, C).cpu()
    kb.assert_within(got, ref, kb.bound(ref, a, 2, kb.rho_for(dt)), "lrelu_bwd" + tag)
    same = f == 1.0
    assert nvox < 4 or bool(same.any())
    assert torch.equal(got.view(INT[dt])[same], g.view(INT[dt])[same]), "changed where the factor is 1" + tag
    zero = f == 0.0
    assert not scaled or bool(zero.any())
    assert bool((got[zero] == 0).all()) and torch.equal(torch.signbit(got[zero].float()), torch.signbit(g[zero].float())), \
        "a keep factor of 0 must give a zero of g's sign" + tag


AXPBY = [(1.0, 0.0), (0.2, 0.0), (1.0, 1.0), (1.0, 0.2), (-0.5, 2.0)]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("row", WIN_ROWS, ids=WIN_IDS)
def test_chan_axpby(hip, row, dt):
    o = ops()
    nvox, d_ctot, d_off, s_ctot, s_off, C, _, _ = row
    gen = torch.Generator().manual_seed(200 + nvox)
    src = torch.randn(nvox, C, generator=gen).to(dt)
    dst0 = torch.randn(nvox, C, generator=gen).to(dt)
    sd = in_row(src, s_ctot, s_off, dt, gen)
    for alpha, beta in AXPBY:
        tag = f"[{name_of(dt)} {row[:6]} alpha {alpha} beta {beta}]"
        dd = kb.Guarded((nvox, d_ctot), dt, DEV, window=(d_off, C), fill=NAN if beta == 0.0 else dst0.to(DEV))
        o.chan_axpby(dd.t, d_off, sd, s_off, C, alpha, beta)
        done(dd, label="chan_axpby" + tag)
        ref, a = kb.ref_chan_axpby(src, dst0, alpha, beta)
        got = dd.window_view().cpu()
        assert bool(torch.isfinite(got.float()).all()), "beta = 0 read the destination" + tag
        kb.assert_within(got, ref, kb.bound(ref, a, 3, kb.rho_for(dt)), f"chan_axpby beta {'0' if beta == 0 else 'on'}" + tag)
        if alpha == 1.0 and beta == 0.0:
            assert torch.equal(got.view(INT[dt]), src.view(INT[dt])), "a copy must be exact" + tag


UP_ROWS = [(1, 1, 1, 1, 4), (2, 3, 2, 5, 8), (1, 1, 7, 1, 32), (1, 5, 1, 3, 144), (2, 4, 4, 10, 128),
           (1, 16, 16, 33, 256)]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("row", UP_ROWS, ids=str)
def test_upsample2_bwd(hip, row, dt):
    o = ops()
    B, Xi, Yi, Zi, C = row
    tag = f"[{name_of(dt)} {row}]"
    total = B * Xi * Yi * Zi * (C >> 2)
    print(f"[row] upsample2_bwd{tag}: {total} threads' worth, {-(-total // (2048 * 256))} trip(s)")
    gen = torch.Generator().manual_seed(300 + Xi * Yi * Zi)
    dy = torch.randn(B, 2 * Xi, 2 * Yi, Zi, C, generator=gen).to(dt)
    dyd = dy.to(DEV)
    dx = kb.Guarded((B, Xi, Yi, Zi, C), dt, DEV, fill=NAN)
    o.upsample2_bwd(dyd, dx.t)
    done(dx, label="upsample2_bwd" + tag)
    ref, a = kb.ref_upsample2_bwd(dy)
    kb.assert_within(dx.t, ref, kb.bound(ref, a, 3, kb.rho_for(dt)), "upsample2_bwd" + tag)
    # one-hot: each fine position of the first and the last coarse voxel of each sample
    vals = (1.0 + torch.arange(C) % 5).to(dt).to(DEV)
    for b in range(B):
        for cx, cy, cz in ((0, 0, 0), (Xi - 1, Yi - 1, Zi - 1)):
            for i in (0, 1):
                for j in (0, 1):
                    dyd.zero_()
                    dyd[b, 2 * cx + i, 2 * cy + j, cz] = vals
                    dx = kb.Guarded((B, Xi, Yi, Zi, C), dt, DEV, fill=NAN)
                    o.upsample2_bwd(dyd, dx.t)
                    done(dx, label="upsample2_bwd one-hot" + tag)
                    want = torch.zeros((B, Xi, Yi, Zi, C), dtype=dt, device=DEV)
                    want[b, cx, cy, cz] = vals
                    assert torch.equal(dx.t.view(INT[dt]), want.view(INT[dt])), \
                        f"one-hot at sample {b} coarse {(cx, cy, cz)} fine ({i}, {j})" + tag


CS_ROWS = [(4, 4, 0, 1), (4, 8, 4, 4097), (12, 16, 4, 1361), (48, 256, 96, 1000), (128, 128, 0, 8 * 16 + 1),
           (144, 144, 0, 3000), (1020, 1024, 4, 300), (1024, 1024, 0, 8197), (128, 128, 0, 65541)]


def launch_chan_sum(x, ctot, off, C, nvox, scale, tag):
    """``wsr_chan_sum`` as ``hip_ops.chan_sum`` calls it, with a guarded 512-row partial table of the test's own.
    Returns (out, partial table) as ``Guarded``"""
    from gan_sr_wind_field_amd import _lib
    o = ops()
    out = kb.Guarded((C,), torch.float32, DEV, fill=NAN)
    part = kb.Guarded((o.CHAN_SUM_ROWS, C), torch.float32, DEV)
    o.check(_lib.lib().wsr_chan_sum(o._p(x), ctot, off, C, nvox, scale, o._p(out.t), o._p(part.t), o.dtype_id(x.dtype),
                                    o._stream()), "chan_sum")
    done(out, part, label="chan_sum" + tag)
    return out, part


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("row", CS_ROWS, ids=str)
def test_chan_sum(hip, row, dt):
    o = ops()
    C, ctot, off, nvox = row
    groups, lanes, rows = kb.chan_sum_geometry(C, nvox)
    step = rows * lanes
    tag = f"[{name_of(dt)} {row}]"
    print(f"[row] chan_sum{tag}: groups {groups} lanes {lanes} rows {rows} voxels per thread <= {-(-nvox // step)} "
          f"final lanes {1024 // C}")
    assert o.chan_sum_rows(C, nvox) == rows, "chan_sum_rows disagrees with the launch geometry"
    gen = torch.Generator().manual_seed(400 + C + nvox)
    x = (0.2 + torch.randn(nvox, C, generator=gen)).to(dt)
    full = torch.randn(nvox, ctot, generator=gen).to(dt)
    full[:, off:off + C] = x
    xd = full.to(DEV)
    sentinel = torch.full((1,), SENTINEL, dtype=torch.int32)
    for scale in (1.0, 0.2):
        out, part = launch_chan_sum(xd, ctot, off, C, nvox, scale, tag)
        ref, a = kb.ref_chan_sum(x, scale)
        kb.assert_within(out.t, ref, kb.bound(ref, a, nvox + rows, 0.0), f"chan_sum scale {scale}" + tag)
        pt = part.t.cpu()
        assert bool((pt[rows:].view(torch.int32) == sentinel).all()), "a partial row past the launched workgroups" + tag
        pref, pa = kb.ref_chan_sum_partials(x, C, nvox)
        kb.assert_within(pt[:rows], pref, kb.bound(pref, pa, -(-nvox // rows) + lanes, 0.0), "chan_sum partial rows" + tag)
    # the partial pass on its own
    pr = kb.Guarded((rows, C), torch.float32, DEV)
    o.chan_sum_partials(xd, off, C, pr.t)
    done(pr, label="chan_sum_partials" + tag)
    assert torch.equal(pr.t.cpu().view(torch.int32), pt[:rows].view(torch.int32)), "the two entry points differ" + tag
    # capped rows: a spike at the voxels where the loops of thread 0 part
    if rows == o.CHAN_SUM_ROWS:
        assert -(-nvox // step) == 17  # two unrolled batches and one tail voxel for the first threads
        for v in (0, 7 * step, 16 * step, nvox - 1):
            xs = x.clone()
            xs[v] = 1024.0
            xd[v, off:off + C] = 1024.0
            out, _ = launch_chan_sum(xd, ctot, off, C, nvox, 1.0, tag)
            xd[v, off:off + C] = x[v].to(DEV)
            ref, a = kb.ref_chan_sum(xs, 1.0)
            bnd = kb.bound(ref, a, nvox + rows, 0.0)
            assert float((1024.0 / bnd).min()) > 20  # (left out or doubled, the spike is far outside)
            kb.assert_within(out.t, ref, bnd, "chan_sum spike" + tag)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_chan_sum_engine_form(hip, dt, accumulate):
    """the LFF bias gradient as the engine takes it: ``chan_sum_partials`` into (rows, nf), then the ordered reduce of
    the rows as split copies of a (1, 1, nf) packed filter into the (1, nf, 1) master gradient, scaled"""
    o = ops()
    nf, nvox, scale = 128, 16 * 6 * 6 * 10, 0.2
    _, lanes, rows = kb.chan_sum_geometry(nf, nvox)
    tag = f"[{name_of(dt)} nf {nf} nvox {nvox} rows {rows} accumulate {int(accumulate)}]"
    gen = torch.Generator().manual_seed(5)
    x = (0.2 + torch.randn(nvox, nf, generator=gen)).to(dt)
    d0 = torch.randn(nf, generator=gen)
    pr = kb.Guarded((rows, nf), torch.float32, DEV)
    o.chan_sum_partials(x.to(DEV), 0, nf, pr.t)
    dst = kb.Guarded((nf,), torch.float32, DEV, fill=d0.to(DEV) if accumulate else NAN)
    table = o.unpack_job_table([(pr.t[0].view(1, 1, nf), dst.t.view(1, nf, 1), scale, rows, nf)])
    if accumulate:  # (wsr_unpack_job_t.accumulate: the int32 behind ``scale``)
        table[0, 4] += 1 << 32
    o.unpack_wgrad_reduce_multi(table)
    done(pr, dst, label="chan_sum engine form" + tag)
    ref, a = kb.ref_chan_sum(x, scale)
    if accumulate:
        ref, a = ref + d0.double(), a + d0.double().abs()
    kb.assert_within(dst.t, ref, kb.bound(ref, a, nvox + rows, 0.0), "chan_sum engine form" + tag)
