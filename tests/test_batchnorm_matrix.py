"""Every BatchNorm kernel of the discriminator, checked element-wise against float64 at the shapes where its branches part.

Each stage is held to its ``kernel_bounds.ref_bn_*`` reference computed FROM THE fp32 INPUTS THE KERNEL ITSELF RECEIVED
(the shift / mean / invstd / sums tables an earlier launch produced are read back and fed to the reference as they are),
so the stages are isolated and no error compounds.  Activations are bf16-exact in the bf16 rows.  Every output is a
``kb.Guarded`` buffer, ``sums``, ``mean``, ``invstd``, ``work`` and ``dx`` pre-filled with NaN, the in-place ``dy``
guarded too, and the guards are compared after every launch.

Reductions ``bn_stats`` (no shift; the fp32 mean of the first pass as shift) and ``bn_bwd_reduce`` (act on / off),
K = nvox + rows.  ``lanes = 256 / (C / 4)`` and ``rows = min(512, ceil(nvox / (16 lanes)))`` are computed here from the
formulas of ``bn_v4_grid`` (elementwise.hip :997) and printed with the row; the library offers no witness for them.
A thread walks voxels ``row * lanes + lane + trip * rows * lanes``: up to 16 trips below the cap, more above it.

=================  ==================  ==============================================================================
C                  nvox                branch (elementwise.hip)
=================  ==================  ==============================================================================
4                  1, 257              bn_reduce_v4_kernel :939, one group of 256 lanes; 257: lane 0 alone takes a
                                       second voxel (:961); final kernel :909 with one row
12                 1361                groups = 3, lanes = 85: thread 255 idle (``vl < lanes`` :956), 2 rows
48                 1000                groups = 12, lanes = 21: threads 252-255 idle
32, 64, 128, 256   630 = (2, 5, 7, 9)  the discriminator's widths (Discriminator_3D.py: bf, 2 bf, 4 bf, 8 bf with
                                       bf = 32); the batch boundary falls inside a row
32                 512 * 50 + 3        51 rows, 16 final lanes: rows 0-2 take the unrolled-by-four loop (:917) and a
                                       remainder (:923), the others the remainder loop alone
4                  4096 * 389 + 17     390 rows with 128 final lanes: lanes 0-5 unroll, the others do not
320                333                 lanes = 3, 240 active threads; C2 = 640: the final kernel has one row lane
256                32768 + 5           grid capped at 512 rows (:1000): a partial seventeenth trip
512                16384 + 37          lanes = 2, C2 = 1024, grid capped
1, 2               1, 300, 70001       the scalar atomic kernels bn_stats_kernel :374 / bn_bwd_reduce_kernel :489 (the
                                       wrappers reach them for no other width here), one and several workgroups
                                       (``bn_grid`` :1506); sums zeroed by the wrapper, K = nvox + workgroups
=================  ==================  ==============================================================================

x is ``0.3 + 1.5 randn``; in the fp32 rows channel 1 sits at 1000 +- 1; one channel is constant (variance 0): channel 2,
at C = 2 channel 1 (bf16) or 0 (fp32); the C = 1 rows hold the ordinary channel alone.  The
saved output ``y`` holds +0.0, -0.0, a positive and a negative subnormal (set as bit patterns, two of them per voxel)
among ordinary values; ``kb._lrelu_mask`` decides their sign.  The written-back dy is held to g' with K = 1 and must
equal its input bit for bit wherever the mask is 1 (everywhere with act off).

Per-channel tails: ``bn_mean_kernel`` :402 and ``bn_finalize_kernel`` :464 at C in {4, 256, 300} (300: the second
workgroup partial), the count on the host and through ``count_dev`` (the host value then deliberately wrong),
cnt in {1, 630} (``cnt - 1`` clamp :456), running statistics present and absent, momentum in {0.1, 0.0} - with 0.0
they come back bit-identical.  ``bn_train_stats`` (:1316: bn_reduce_v4_kernel with gridDim.y = G :948,
bn_final_mean_kernel :1287, bn_final_finalize_kernel :1296, bn_rows_sum :1261) at (G, C, nvox_g) in {(1, 32, 630),
(2, 48, 1000), (3, 32, 512 * 50 + 3), (2, 512, 16384 + 37)}: its sums never leave the device, so ``work[g]`` is held
to the references of x itself - the mean to ``ref_bn_sums / cnt`` with K = nvox + rows + 1, invstd to
``ref_bn_finalize`` of the float64 sums shifted by the mean the kernel wrote, with ``bn_finalize``'s own bound and
nothing added for the fp32 sums in between - and the running statistics after G ordered updates to
``kb.ref_bn_running``, K = 3G and 5G.

Apply: ``bn_apply_kernel`` :476 (act on / off, K = 4) and the one-element ``bn_bwd_apply_kernel`` :523 (K = 8) over
sums in {given, None} x act_y in {given, None}, at C in {1, 4, 12, 256} with 630 voxels and C = 12 with 50000 voxels =
600 000 elements: more than one trip of 2048 * 256 threads with a stride that is no multiple of C.

``bn_bwd_apply_v8_kernel`` :543, bf16 only, the forms (sums, no act_y) of training, (no sums, act_y) of a generator
iteration and (sums, act_y), at (C, nvox) = (256, 32768) - exactly 8 << 20 elements -, (256, 32768 + 3) - total / 8
no multiple of 256, the last trip partial -, (64, 131072 + 5) and (8, 2^20 + 3), K = 8: the same bound as the
one-element kernel.  The same data meets the same bound on the one-element route: at 8 << 20 minus C elements, and
with all four tensors one bf16 element into a larger allocation (not 16-byte aligned: the fall-back of :1638, not a
misaligned ``uint4`` access).  NO WITNESS tells the two kernels apart: which one ran rests on the condition at
:1637 (bf16, total >= 8 << 20, C % 8 == 0, 256 % C == 0, 16-byte aligned pointers) alone.
"""
import functools
import math

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
EPS, SLOPE = 1e-5, 0.2
DTS = [torch.bfloat16, torch.float32]
DT_IDS = ["bf16", "fp32"]
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SPECIALS = {torch.bfloat16: (0x0000, -0x8000, 0x0001, -0x7FFF),  # +0.0, -0.0, +subnormal, -subnormal
            torch.float32: (0x00000000, -0x80000000, 0x00000001, -0x7FFFFFFF)}


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def make_rows(C, nvox, dt, seed):
    """(x, dy, y) as CPU tensors of ``dt``: the operands of one layer (see the module docstring)"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(nvox, C, generator=gen)
    big = 1 if dt == torch.float32 and C >= 2 else None
    const = 2 if C >= 3 else ((0 if big == 1 else 1) if C == 2 else None)
    if big is not None:
        x[:, big] = 1000.0 + torch.randn(nvox, generator=gen)
    if const is not None:
        x[:, const] = 0.75
    dy = torch.randn(nvox, C, generator=gen).to(dt)
    y = torch.randn(nvox, C, generator=gen).to(dt)
    v = torch.arange(nvox)
    pat = torch.tensor(SPECIALS[dt], dtype=INT[dt])
    yb = y.view(INT[dt])
    yb[v, (v * 5) % C] = pat[v % 4]
    yb[v, (v * 5 + 11) % C] = pat[(v + 2) % 4]
    return x.to(dt), dy, y


def assert_specials(y, dt):
    bits = y.view(INT[dt])
    s = SPECIALS[dt]
    assert all(bool((bits == p).any()) for p in s)
    assert bool((y.double()[bits == s[2]] > 0).all()) and bool((y.double()[bits == s[3]] < 0).all())
    assert not bool((y.double()[bits == s[1]] > 0).any())


def nan_out(shape, dt=torch.float32):
    return kb.Guarded(shape, dt, DEV, fill=NAN)


def done(*bufs, label):
    torch.cuda.synchronize()
    kb.assert_guards_intact(*bufs, label=label)


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------

REDUCE_ROWS = ([(4, 1), (4, 257), (12, 1361), (48, 1000)] + [(c, 630) for c in (32, 64, 128, 256)]
               + [(32, 512 * 50 + 3), (4, 4096 * 389 + 17), (320, 333), (256, 32768 + 5), (512, 16384 + 37)]
               + [(c, n) for c in (1, 2) for n in (1, 300, 70001)])


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("C,nvox", REDUCE_ROWS)
def test_reductions(hip, dt, C, nvox):
    """bn_stats (unshifted, shifted), bn_mean, bn_finalize and bn_bwd_reduce (act on, off) of one layer, each stage
    against its reference from the fp32 tables the stage was given"""
    o = ops()
    lanes, rows = kb.bn_v4_geometry(C, nvox)
    tag = f"[{'bf16' if dt == torch.bfloat16 else 'fp32'} C {C} nvox {nvox}]"
    print(f"[row] reductions{tag}: lanes {lanes} rows {rows} trips "
          f"{-(-nvox // (rows * lanes)) if lanes else '-'} final lanes {1024 // (2 * C) if lanes else '-'}")
    x, dy, y = make_rows(C, nvox, dt, 1000 + 7 * C + nvox % 1009)
    if nvox >= 4:
        assert_specials(y, dt)
    shape5 = (2, 5, 7, 9, C) if nvox == 630 else (nvox, C)
    xd, yd = x.to(DEV).view(shape5), y.to(DEV).view(shape5)
    K = nvox + rows
    # pass 1: plain sums, the mean
    s0 = nan_out((2 * C,))
    o.bn_stats(xd, s0.t)
    done(s0, label="bn_stats" + tag)
    ref, A = kb.ref_bn_sums(x)
    kb.assert_within(s0.t, ref, kb.bound(ref, A, K, 0.0), "bn_stats" + tag)
    mean = nan_out((C,))
    o.bn_mean(s0.t, mean.t, float(nvox))
    done(mean, s0, label="bn_mean" + tag)
    ref, A = kb.ref_bn_mean(s0.t[:C].cpu(), nvox)
    kb.assert_within(mean.t, ref, kb.bound(ref, A, 1, 0.0), "bn_mean" + tag)
    # pass 2: sums shifted by that fp32 mean, invstd
    s2 = nan_out((2 * C,))
    o.bn_stats(xd, s2.t, shift=mean.t)
    done(s2, mean, label="bn_stats shifted" + tag)
    ref, A = kb.ref_bn_sums(x, mean.t.cpu())
    kb.assert_within(s2.t, ref, kb.bound(ref, A, K, 0.0), "bn_stats shifted" + tag)
    invstd = nan_out((C,))
    o.bn_finalize(s2.t, mean.t, invstd.t, float(nvox), EPS, 0.1, None, None)
    done(invstd, s2, mean, label="bn_finalize" + tag)
    s2c = s2.t.cpu()
    ref, A = kb.ref_bn_finalize(s2c[:C], s2c[C:], nvox, mean.t.cpu(), EPS, 0.1)
    kb.assert_within(invstd.t, ref["invstd"], kb.bn_finalize_bounds(ref, A, EPS)["invstd"], "bn_finalize invstd" + tag)
    # backward sums, dy written back under the mask
    mc, ic = mean.t.cpu(), invstd.t.cpu()
    for act in (True, False):
        g = kb.Guarded(shape5, dt, DEV, fill=dy.to(DEV).view(shape5))
        bs = nan_out((2 * C,))
        o.bn_bwd_reduce(g.t, yd, xd, mean.t, invstd.t, act, SLOPE, bs.t)
        done(bs, g, label=f"bn_bwd_reduce act {act}" + tag)
        ref, A = kb.ref_bn_bwd_sums(dy, y, x, mc, ic, act, SLOPE)
        kb.assert_within(bs.t, ref, kb.bound(ref, A, K, 0.0), f"bn_bwd_reduce act {int(act)}" + tag)
        got = g.t.view(nvox, C).cpu()
        gref, ga = kb.ref_bn_bwd_dy(dy, y, act, SLOPE)
        kb.assert_within(got, gref, kb.bound(gref, ga, 1, kb.rho_for(dt)), f"bn_bwd_reduce dy act {int(act)}" + tag)
        same = kb._lrelu_mask(y, SLOPE) == 1.0 if act else torch.ones_like(got, dtype=torch.bool)
        assert torch.equal(got.view(INT[dt])[same], dy.view(INT[dt])[same]), "dy changed where the mask is 1" + tag


# ---------------------------------------------------------------------------------------------------------------------
# per-channel tails
# ---------------------------------------------------------------------------------------------------------------------

def tail_case(C, cnt, seed):
    gen = torch.Generator().manual_seed(seed)
    d = 1.5 * torch.randn(cnt, C, generator=gen, dtype=torch.float64)
    d[:, C // 2] = 0.0  # a constant channel: var = 0
    s1 = (1e-3 * torch.randn(C, generator=gen)).float() * cnt  # (the shifted sum is near 0, not 0)
    s2 = (d * d).sum(0).float()
    mean = (0.3 + torch.randn(C, generator=gen)).float()
    return s1, s2, mean, torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5


@pytest.mark.parametrize("cnt", [1, 630])
@pytest.mark.parametrize("C", [4, 256, 300])
def test_mean_and_finalize(hip, C, cnt):
    o = ops()
    s1, s2, mean, rm0, rv0 = tail_case(C, cnt, 31 * C + cnt)
    sums = torch.cat([s1, s2]).to(DEV)
    cnt_dev = torch.tensor([float(cnt)], device=DEV)
    for on_dev in (False, True):
        host = 7.0 if on_dev else float(cnt)  # (count_dev wins over the host value)
        tag = f"[C {C} cnt {cnt} {'count_dev' if on_dev else 'host count'}]"
        m = nan_out((C,))
        o.bn_mean(sums, m.t, host, cnt_dev if on_dev else None)
        done(m, label="bn_mean" + tag)
        ref, A = kb.ref_bn_mean(s1, cnt)
        kb.assert_within(m.t, ref, kb.bound(ref, A, 1, 0.0), "bn_mean" + tag)
        for running in (True, False):
            for momentum in (0.1, 0.0):
                lab = tag[:-1] + f" running {int(running)} m {momentum}]"
                invstd = nan_out((C,))
                rm = kb.Guarded((C,), torch.float32, DEV, fill=rm0.to(DEV))
                rv = kb.Guarded((C,), torch.float32, DEV, fill=rv0.to(DEV))
                o.bn_finalize(sums, mean.to(DEV), invstd.t, host, EPS, momentum, rm.t if running else None,
                              rv.t if running else None, cnt_dev if on_dev else None)
                done(invstd, rm, rv, label="bn_finalize" + lab)
                ref, A = kb.ref_bn_finalize(s1, s2, cnt, mean, EPS, momentum, rm0, rv0)
                bnd = kb.bn_finalize_bounds(ref, A, EPS)
                kb.assert_within(invstd.t, ref["invstd"], bnd["invstd"], "bn_finalize invstd" + lab)
                if running and momentum != 0.0:
                    kb.assert_within(rm.t, ref["rm"], bnd["rm"], "bn_finalize running mean" + lab)
                    kb.assert_within(rv.t, ref["rv"], bnd["rv"], "bn_finalize running var" + lab)
                else:  # absent, or momentum 0: bit-identical
                    assert torch.equal(rm.t.cpu().view(torch.int32), rm0.view(torch.int32)), lab
                    assert torch.equal(rv.t.cpu().view(torch.int32), rv0.view(torch.int32)), lab


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("G,C,nvox", [(1, 32, 630), (2, 48, 1000), (3, 32, 512 * 50 + 3), (2, 512, 16384 + 37)])
def test_train_stats(hip, dt, G, C, nvox):
    o = ops()
    lanes, rows = kb.bn_v4_geometry(C, nvox)
    tag = f"[{'bf16' if dt == torch.bfloat16 else 'fp32'} G {G} C {C} nvox_g {nvox}]"
    print(f"[row] bn_train_stats{tag}: lanes {lanes} rows {rows} per group, final lanes {1024 // (2 * C)}")
    momentum = 0.1
    xs = [make_rows(C, nvox, dt, 2000 + 13 * C + g)[0] * (1.0 + 0.5 * g) for g in range(G)]  # (groups differ in spread)
    xs = [t.to(dt) for t in xs]
    gen = torch.Generator().manual_seed(5 * C + G)
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    work = nan_out((G, 2 * C))
    rm = kb.Guarded((C,), torch.float32, DEV, fill=rm0.to(DEV))
    rv = kb.Guarded((C,), torch.float32, DEV, fill=rv0.to(DEV))
    assert o.bn_train_stats(torch.stack(xs).to(DEV), G, work.t, EPS, momentum, rm.t, rv.t)
    done(work, rm, rv, label="bn_train_stats" + tag)
    w = work.t.cpu()
    groups = []
    for g in range(G):
        ref, A = kb.ref_bn_sums(xs[g])
        mref = ref[:C] / nvox
        kb.assert_within(w[g, :C], mref, kb.bound(ref[:C], A[:C], nvox + rows + 1, 0.0) / nvox,
                         "bn_train_stats mean" + tag)
        ref, A = kb.ref_bn_sums(xs[g], w[g, :C])
        groups.append((ref[:C], ref[C:], w[g, :C]))
        fin, fa = kb.ref_bn_finalize(ref[:C], ref[C:], nvox, w[g, :C], EPS, momentum)
        kb.assert_within(w[g, C:], fin["invstd"], kb.bn_finalize_bounds(fin, fa, EPS)["invstd"],
                         "bn_train_stats invstd" + tag)
    run, ra, _ = kb.ref_bn_running(groups, nvox, EPS, momentum, rm0, rv0)
    bnd = kb.bn_finalize_bounds(run, ra, EPS, steps=G)
    kb.assert_within(rm.t, run["rm"], bnd["rm"], "bn_train_stats running mean" + tag)
    kb.assert_within(rv.t, run["rv"], bnd["rv"], "bn_train_stats running var" + tag)


# ---------------------------------------------------------------------------------------------------------------------
# apply, forward and backward
# ---------------------------------------------------------------------------------------------------------------------

def make_tables(x, C, seed):
    """fp32 (mean, invstd, gamma, beta, sums) of a layer, CPU"""
    gen = torch.Generator().manual_seed(seed)
    xd = x[:4096].double()
    mean = xd.mean(0).float()
    invstd = torch.rsqrt(xd.var(0, unbiased=False).float() + EPS)
    gamma = 1 + 0.1 * torch.randn(C, generator=gen)
    beta = 0.1 * torch.randn(C, generator=gen)
    sums = 20.0 * torch.randn(2 * C, generator=gen)
    return mean, invstd, gamma, beta, sums


FORMS = {"sums": (True, False), "act_y": (False, True), "sums_act_y": (True, True), "neither": (False, False)}


def run_bwd_apply(o, dt, C, nvox, ops_cpu, tables, form, label, *, offset=0):
    """one ``bn_bwd_apply`` launch of ``form`` on (x, dy, y) and its check with K = 8; ``offset``: every tensor starts
    that many elements into its allocation"""
    x, dy, y = ops_cpu
    mean, invstd, gamma, _, sums = tables
    with_sums, with_act = FORMS[form]
    inv_n = 1.0 / nvox

    def dev(t):
        if not offset:
            return t.to(DEV)
        base = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
        v = base[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    dx = kb.Guarded((nvox, C), dt, DEV, fill=NAN, guard=kb.GUARD_ELEMS + offset)
    xd, gd, yd = dev(x), dev(dy), dev(y)
    if offset:
        assert all(t.data_ptr() % 16 == 2 * offset for t in (xd, gd, yd, dx.t))
    md, isd, gmd, sd = (t.to(DEV) for t in (mean, invstd, gamma, sums))
    assert o.bn_bwd_apply(gd, xd, dx.t, md, isd, gmd, sd if with_sums else None, inv_n if with_sums else 0.0,
                          act_y=yd if with_act else None, slope=SLOPE)
    done(dx, label=label)
    assert torch.equal(gd.cpu().view(INT[dt]), dy.view(INT[dt])), "the gradient is an input: " + label
    ref, A = kb.ref_bn_bwd_apply(dy, x, y if with_act else None, SLOPE, mean, invstd, gamma,
                                 sums if with_sums else None, inv_n)
    return kb.assert_within(dx.t, ref, kb.bound(ref, A, 8, kb.rho_for(dt)), label)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("C,nvox", [(1, 630), (4, 630), (12, 630), (256, 630), (12, 50000)])
def test_apply(hip, dt, C, nvox):
    o = ops()
    tag = f"[{'bf16' if dt == torch.bfloat16 else 'fp32'} C {C} nvox {nvox}]"
    print(f"[row] apply{tag}: {nvox * C} elements, {-(-nvox * C // (2048 * 256))} trip(s)")
    rows = make_rows(C, nvox, dt, 3000 + 11 * C + nvox % 997)
    x, dy, y = rows
    assert_specials(y, dt)
    tables = make_tables(x.float(), C, C + nvox)
    mean, invstd, gamma, beta, _ = tables
    for act in (True, False):
        out = nan_out((nvox, C), dt)
        o.bn_apply_lrelu(x.to(DEV), out.t, mean.to(DEV), invstd.to(DEV), gamma.to(DEV), beta.to(DEV), act, SLOPE)
        done(out, label=f"bn_apply act {act}" + tag)
        ref, A = kb.ref_bn_apply(x, mean, invstd, gamma, beta, act, SLOPE)
        kb.assert_within(out.t, ref, kb.bound(ref, A, 4, kb.rho_for(dt)), f"bn_apply act {int(act)}" + tag)
    for form in FORMS:
        run_bwd_apply(o, dt, C, nvox, rows, tables, form, f"bn_bwd_apply {form}" + tag)


# ---------------------------------------------------------------------------------------------------------------------
# the 8-wide backward apply (bf16, >= 8 << 20 elements) and the same data on the one-element route
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def big_case(C, nvox):
    rows = make_rows(C, nvox, torch.bfloat16, 4000 + C)
    assert_specials(rows[2], torch.bfloat16)
    return rows, make_tables(rows[0].float(), C, 4001 + C)


V8_SHAPES = [(256, 32768), (256, 32768 + 3), (64, 131072 + 5), (8, 2 ** 20 + 3)]


@pytest.mark.parametrize("form", ["sums", "act_y", "sums_act_y"])
@pytest.mark.parametrize("C,nvox", V8_SHAPES)
def test_bwd_apply_v8(hip, C, nvox, form):
    assert nvox * C >= 8 << 20 and C % 8 == 0 and 256 % C == 0  # the condition at :1637 (the pointers: torch's allocator)
    threads = min(2048, -(-nvox * C // 8 // 256)) * 256
    print(f"[row] bn_bwd_apply v8[C {C} nvox {nvox} {form}]: {nvox * C // 8} vectors, {threads} threads, "
          f"{-(-nvox * C // 8 // threads)} trips, last trip {nvox * C // 8 % threads or threads} vectors")
    rows, tables = big_case(C, nvox)
    run_bwd_apply(ops(), torch.bfloat16, C, nvox, rows, tables, form, f"bn_bwd_apply v8 {form}[C {C} nvox {nvox}]")


def test_bwd_apply_just_below_the_v8_threshold(hip):
    """8 << 20 minus C elements of the (256, 32768) data: the one-element kernel, the same bound"""
    C, nvox = 256, 32768
    rows, tables = big_case(C, nvox)
    rows = tuple(t[:nvox - 1] for t in rows)
    assert (nvox - 1) * C == (8 << 20) - C
    run_bwd_apply(ops(), torch.bfloat16, C, nvox - 1, rows, tables, "sums_act_y", "bn_bwd_apply scalar route[below 8 << 20]")


def test_bwd_apply_misaligned_views_take_the_scalar_route(hip):
    """the (256, 32768) data with every tensor one bf16 element into its allocation: :1638 sends it to the one-element
    kernel"""
    C, nvox = 256, 32768
    rows, tables = big_case(C, nvox)
    run_bwd_apply(ops(), torch.bfloat16, C, nvox, rows, tables, "sums_act_y", "bn_bwd_apply scalar route[misaligned]",
                  offset=1)
