"""The table Adam family, checked element-wise against float64 at the sizes and alignments where its branches part.

``adam_multi_kernel`` :626, ``grad_sqnorm_multi_kernel`` :668, ``adam_multi_clip_kernel`` :694, ``adam_multi_ema_kernel``
:774, ``adam_multi_clip_ema_kernel`` :813 and the single-tensor ``adam_kernel`` :590 (all elementwise.hip), through
``hip_ops`` as the optimizer calls them.  The reference is ``kb.ref_adam``: ``torch.optim.Adam``'s definition in float64
from the fp32 tensors the kernel receives and the hyper-parameters as Python doubles, with the propagated bounds of
kernel_bounds.py.  p, g, m, v, the shadow, the partials and the total are ``kb.Guarded`` buffers; the guards are compared
after every launch.

One launch per row over ONE job table that holds a tensor of every size (``ROW_SIZES``, 23 jobs):

=========================  ==========================================================================================
n                          branch (elementwise.hip)
=========================  ==========================================================================================
1, 2, 3                    n4 = 0: the float4 loop :637 does not run, the scalar loop :648 takes everything
4, 8                       one and two float4s, no tail
5, 7                       tails of 1 and 3 (``done = n4 << 2`` :646)
255, 256, 257              63 / 64 float4s: a quarter of the threads busy; tails 3, 0, 1
1023, 1024, 1025, 1027     255 and 256 float4s - the last thread idle, every thread once - tails 3, 0, 1, 3
32 767, 32 768             8191 / 8192 float4s: 32 trips of ``i += 256``; the scalar path: 128 trips
32 769                     a full chunk plus a job of ONE element (``adam_job_table``, hip_ops.py :994)
65 541                     two chunks and a job of 5
=========================  ==========================================================================================

Alignment rows (``ALIGN``): all of p, g, m, v 16-byte aligned (``vec`` :629, :711, :780, :832); each of the four alone
4, 8 and 12 bytes off (guard bands of 1025..1027 elements) - any one sends ALL four down the scalar path, and for
``grad_sqnorm_multi_kernel`` g alone decides (:675).  The shadow is 4 bytes off where the quad is aligned (``evec``
:781, ``ema_load4`` / ``ema_store4`` element by element) and aligned where the quad is not; one row has everything
aligned.  A job's chunk offset is a multiple of 128 KiB, so every chunk of a tensor shares its alignment.

Hyper-parameter rows ``HYPER`` = (lr, beta1, beta2, eps, wd, step): the training values at step 1 (state zero:
bc1 = 1 - beta1, step_size = lr / 0.5) and step 2 with weight decay, then lr = 1e-2 at step 1000 and lr = 0.5 at step
100 000 (bias corrections 1 to the last bit), where the update and not |p| is the dominant term of p's bound.

Planted elements (``kb.adam_case``) at 0, 4 (n >> 2) - the first tail element -, n - 1 and, past a chunk, 32 768 and
65 535 (the first and the last element of the second job): in turn g = m = v = 0 (with wd = 0: p back bit for bit,
m' = v' = +0.0); g = 0, v = 0, m = 0.25 (the denominator is eps alone); g = +-1e-25 with v = 0 (g^2 underflows in fp32,
the reference's 1e-53 lies under the 2^-100 floor: shown in test_kernel_bounds.py); g = 1e15.

Forms over every (alignment, hyper) row, each from the same initial bits: ``adam_multi``; ``grad_sqnorm_multi``, whose
partials are held to the float64 sum with K = n + 10; ``adam_multi_clip`` with max_norm = total (1 + 2^-10) - coef
clamped to 1 (:705), g and the update bit-identical to ``adam_multi`` -, with ``inf`` (measure only, :1689: g untouched)
and with total (1 - 2^-10), which clips: the written-back g' against coef * g with K = 3, coef in float64 from the fp32
total the kernel wrote, p', m', v' against ``ref_adam(coef=...)``; ``total_out`` against the float64 root of the fp32
partials, K = n_jobs + 2; ``adam_multi_ema`` and ``adam_multi_clip_ema``: p, g, m, v bit-identical to the form without
the shadow, the shadow inside test_ema.py's ``step_bound`` of the p' the launch wrote.

``test_partials_spike``: over 32 768 terms the bound of a partial cannot see one ordinary element (3e-5 of the sum, the
bound 1.7e-4), so a spike of 1024 stands in turn at 0, 4 (n >> 2), n - 1 and at lanes x, y, z, w of the float4 thread 1
takes on its second trip (element 4 (256 + 1) + lane), aligned and with g 4 bytes off.

``test_total_over_job_counts``: n_jobs in {1, 2, 255, 256, 257, 512, 513, 600} from tensors of 1 to 7 elements - one to
three trips of ``for (i = threadIdx.x; i < n_jobs; i += 256)`` :700 - with one job's partial dominating at 0, 255, 256,
511, 512 and the last.

``test_non_finite_total``: one ``inf`` in one job's gradient under a finite bound gives total = inf, coef = 0 in EVERY
workgroup: every other g' is 0 with g's sign, m' = beta1 m within the bound, the planted element NaN; one NaN gives every
g' NaN.  Plain arithmetic on non-finite values.

``test_legacy_adam_step``: ``wsr_adam_step`` (:1656) at n in {1, 257, 2048 * 256 + 5} - the last a second grid-stride
trip behind the ``ew_grid`` cap :20 - referenced from the fp32 hyper-parameters it receives (``f32_hyper``), where
``1.f - beta`` :596-597 is exact.

``test_table_adam_step``: ``TableAdam.step()`` with two parameter groups, clipping and the moving average on, three steps;
every step referenced from the device state read back before it.

What no test here can tell apart: whether the float4 or the scalar loop updated an element (both are ``adam_one``; only
that every element was updated exactly once), which workgroup's copy of the coefficient an element was scaled with
beyond its value, and whether the compiler contracted ``adam_one``'s products into fused multiply-adds (the bound holds
either way, test_kernel_bounds.py).
"""
import math

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
ROW_SIZES = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 1027, 32767, 32768, 32769, 65541]
HYPER = [(8e-5, 0.5, 0.999, 1e-8, 0.0, 1), (8e-5, 0.9, 0.999, 1e-8, 0.01, 2), (1e-2, 0.5, 0.999, 1e-8, 0.01, 1000),
         (0.5, 0.9, 0.99, 1e-8, 0.0, 100000)]
HYPER_IDS = ["lr8e-5-step1", "lr8e-5-wd-step2", "lr1e-2-wd-step1000", "lr0.5-step100000"]
# (elements off the 16-byte alignment of p, g, m, v, shadow)
ALIGN = [(0, 0, 0, 0, 0), (0, 0, 0, 0, 1)] + [tuple(k if j == i else 0 for j in range(4)) + (0,)
                                              for i in range(4) for k in (1, 2, 3)]
ALIGN_IDS = ["aligned", "shadow+4"] + [f"{'pgmv'[i]}+{4 * k}" for i in range(4) for k in (1, 2, 3)]
EMA_D = 0.999


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Quads:
    """the tensors of one row on the device: per tensor five ``Guarded`` (p, g, m, v, shadow) at the row's alignment,
    their job table and shadow pointer table; ``load`` puts the initial bits back (the pointers, so the tables, stay)"""

    def __init__(self, cpu, align, shadows=None):
        self.cpu = cpu  # [(p, g, m, v)] fp32 CPU
        self.sizes = [q[0].numel() for q in cpu]
        self.align = align
        self.buf = [[kb.Guarded((n,), torch.float32, DEV, guard=kb.GUARD_ELEMS + a) for a in align] for n in self.sizes]
        for row in self.buf:
            for b, a in zip(row, align):
                assert b.t.data_ptr() % 16 == 4 * a
        gen = torch.Generator().manual_seed(99)
        self.shadow0 = shadows or [torch.randn(n, generator=gen) for n in self.sizes]
        quads = [tuple(b.t for b in row[:4]) for row in self.buf]
        self.table = ops().adam_job_table(quads)
        self.ema_table = ops().ema_ptr_table(quads, [row[4].t for row in self.buf])
        self.n_jobs = self.table.shape[0]
        assert self.n_jobs == len(kb.adam_jobs(self.sizes))
        self.load()

    def load(self, g=None):
        for i, (row, q) in enumerate(zip(self.buf, self.cpu)):
            for b, t in zip(row[:4], q):
                b.t.copy_(t)
            if g is not None:
                row[1].t.copy_(g[i])
            row[4].t.copy_(self.shadow0[i])

    def read(self, k):
        """tensor k of every quad (0 p, 1 g, 2 m, 3 v, 4 shadow) as one flat CPU vector"""
        return torch.cat([row[k].t.cpu() for row in self.buf])

    def flat(self, k):
        return torch.cat([q[k] for q in self.cpu]) if k < 4 else torch.cat(self.shadow0)

    def done(self, *extra, label):
        torch.cuda.synchronize()
        kb.assert_guards_intact(*[b for row in self.buf for b in row], *extra, label=label)


def check_adam(q, ref, kernel, tag):
    """p', m', v' of the row against ``ref`` = ``kb.ref_adam`` of the flat vectors; returns the bits read"""
    got = [q.read(k) for k in (0, 2, 3)]
    for name, gt, (r, b) in zip(("p", "exp_avg", "exp_avg_sq"), got, ref):
        kb.assert_within(gt, r, b, f"{kernel} {name}{tag}")
    return [bits(t) for t in got]


@pytest.mark.parametrize("hyper", HYPER, ids=HYPER_IDS)
@pytest.mark.parametrize("align", ALIGN, ids=ALIGN_IDS)
def test_adam_forms(hip, align, hyper):
    o = ops()
    lr, b1, b2, eps, wd, step = hyper
    hp = (lr, b1, b2, eps, wd, step)
    tag = f"[{ALIGN_IDS[ALIGN.index(align)]} {HYPER_IDS[HYPER.index(hyper)]}]"
    cpu = [kb.adam_case(n, step, 31 * HYPER.index(hyper) + i) for i, n in enumerate(ROW_SIZES)]
    q = Quads(cpu, align)
    jobs = kb.adam_jobs(q.sizes)
    offs = [0]
    for n in q.sizes:
        offs.append(offs[-1] + n)
    print(f"[row] adam{tag}: {q.n_jobs} jobs, tensors start at flat {offs[:-1]}")
    P, G, M, V, E0 = (q.flat(k) for k in range(5))
    g_bits = bits(G)
    ref = kb.ref_adam(P, G, M, V, lr, (b1, b2), eps, wd, step)

    # adam_multi
    o.adam_multi(q.table, *hp)
    q.done(label="adam_multi" + tag)
    plain = check_adam(q, ref, "adam_multi", tag)
    assert torch.equal(bits(q.read(1)), g_bits), "adam_multi wrote the gradient" + tag
    if wd == 0.0:
        still = (G == 0) & (M == 0) & (V == 0)
        assert int(still.sum()) >= 4
        assert torch.equal(plain[0][still], bits(P)[still]), "p moved where g = m = v = 0" + tag
        assert not bool(plain[1][still].any() or plain[2][still].any()), "m', v' not +0.0 where g = m = v = 0" + tag

    # adam_multi_ema: the same bits, the shadow within its bound of the p' written
    q.load()
    o.adam_multi_ema(q.table, q.ema_table, *hp, EMA_D)
    q.done(label="adam_multi_ema" + tag)
    got = [bits(q.read(k)) for k in (0, 2, 3)]
    assert all(torch.equal(a, b) for a, b in zip(got, plain)), "adam_multi_ema: p, m, v differ from adam_multi" + tag
    assert torch.equal(bits(q.read(1)), g_bits)
    p_new = q.read(0)
    kb.assert_within(q.read(4), EMA_D * E0.double() + (1.0 - EMA_D) * p_new.double(),
                     kb.ema_step_bound(EMA_D, E0, p_new), "adam_multi_ema shadow" + tag)

    # the partials
    q.load()
    part = kb.Guarded((q.n_jobs,), torch.float32, DEV, fill=NAN)
    o.grad_sqnorm_multi(q.table, part.t)
    q.done(part, label="grad_sqnorm_multi" + tag)
    assert torch.equal(bits(q.read(1)), g_bits)
    pr = [kb.ref_grad_sqnorm(cpu[i][1][off:off + n]) for i, off, n in jobs]
    kb.assert_within(part.t, torch.stack([r for r, _ in pr]), torch.stack([b for _, b in pr]),
                     "grad_sqnorm_multi partials" + tag)
    pc = part.t.cpu()
    tref, tbnd = kb.ref_clip_total(pc)
    t32 = kb._f32(tref)

    def clip_launch(max_norm, ema, label):
        q.load()
        total = kb.Guarded((1,), torch.float32, DEV, fill=NAN)
        if ema:
            o.adam_multi_clip_ema(q.table, q.ema_table, part.t, max_norm, *hp, EMA_D, total_norm=total.t[0])
        else:
            o.adam_multi_clip(q.table, part.t, max_norm, *hp, total_norm=total.t[0])
        q.done(part, total, label=label)
        assert torch.equal(bits(part.t), bits(pc)), "the clip launch wrote the partials: " + label
        kb.assert_within(total.t, tref.view(1), tbnd.view(1), "adam_multi_clip total" + tag)
        return float(total.t.cpu()[0])

    # a bound just above the norm: coef clamped to 1; inf: measure only - both bit-identical to adam_multi
    for max_norm in (t32 * (1 + 2.0 ** -10), math.inf):
        lab = f"adam_multi_clip max_norm {'inf' if math.isinf(max_norm) else 'above'}" + tag
        total = clip_launch(max_norm, False, lab)
        c = kb.clip_coef(total, max_norm)
        assert c == 1.0 and (math.isinf(max_norm) or kb._f32(max_norm) / (total + 1e-6) > 1 + 2.0 ** -12), (lab, c)
        assert torch.equal(bits(q.read(1)), g_bits), "g changed under a bound that does not clip: " + lab
        got = [bits(q.read(k)) for k in (0, 2, 3)]
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), "p, m, v differ from adam_multi: " + lab

    # a bound just below the norm: clips
    max_norm = t32 * (1 - 2.0 ** -10)
    clipped = None
    for ema in (False, True):
        lab = f"adam_multi_clip{'_ema' if ema else ''} clipping" + tag
        total = clip_launch(max_norm, ema, lab)
        c = kb.clip_coef(total, max_norm)
        assert c < 1 - 2.0 ** -12, (lab, c)
        got = [bits(q.read(k)) for k in range(4)]
        if not ema:
            gref = c * G.double()
            kb.assert_within(q.read(1), gref, kb.bound(gref, gref.abs(), kb.K_CLIP_G, 0.0),
                             "adam_multi_clip g" + tag)
            check_adam(q, kb.ref_adam(P, G, M, V, lr, (b1, b2), eps, wd, step, coef=c), "adam_multi_clip", tag)
            clipped = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, clipped)), "clip_ema: p, g, m, v differ from clip" + tag
            p_new = q.read(0)
            kb.assert_within(q.read(4), EMA_D * E0.double() + (1.0 - EMA_D) * p_new.double(),
                             kb.ema_step_bound(EMA_D, E0, p_new), "adam_multi_clip_ema shadow" + tag)


@pytest.mark.parametrize("goff", [0, 1], ids=["aligned", "g+4"])
def test_partials_spike(hip, goff):
    """a spike of 1024 at each designed index of each size moves the job's partial by what the float64 sum says"""
    o = ops()
    sizes = [s for s in ROW_SIZES if s <= kb.ADAM_CHUNK]
    gen = torch.Generator().manual_seed(8)
    cpu = [tuple(torch.randn(n, generator=gen) for _ in range(4)) for n in sizes]
    q = Quads(cpu, (0, goff, 0, 0, 0))
    places = [("first", lambda n: 0), ("tail", lambda n: 4 * (n >> 2)), ("last", lambda n: n - 1)] + \
             [(f"trip2 lane {'xyzw'[l]}", lambda n, l=l: 4 * 257 + l) for l in range(4)]
    for name, at in places:
        gs = []
        for n, quad in zip(sizes, cpu):
            g = quad[1].clone()
            if 0 <= at(n) < n:
                g[at(n)] = 1024.0
            gs.append(g)
        q.load(g=gs)
        part = kb.Guarded((q.n_jobs,), torch.float32, DEV, fill=NAN)
        o.grad_sqnorm_multi(q.table, part.t)
        q.done(part, label="grad_sqnorm_multi spike " + name)
        pr = [kb.ref_grad_sqnorm(g) for g in gs]
        kb.assert_within(part.t, torch.stack([r for r, _ in pr]), torch.stack([b for _, b in pr]),
                         f"grad_sqnorm_multi spike[{name} {'g+4' if goff else 'aligned'}]")
        if name == "first":  # the spike is far above every bound: without it the sum would be out
            r32768, b32768 = pr[sizes.index(32768)]
            assert 1024.0 ** 2 > 1e3 * float(b32768)


@pytest.mark.parametrize("n_jobs", [1, 2, 255, 256, 257, 512, 513, 600])
def test_total_over_job_counts(hip, n_jobs):
    o = ops()
    sizes = [1 + i % 7 for i in range(n_jobs)]
    gen = torch.Generator().manual_seed(n_jobs)
    n = sum(sizes)
    flat = [kb.Guarded((n,), torch.float32, DEV, fill=0.0) for _ in range(4)]
    views, off = [], 0
    for s in sizes:
        views.append(tuple(b.t[off:off + s] for b in flat))
        off += s
    table = o.adam_job_table(views)
    assert table.shape[0] == n_jobs
    g0 = 0.1 * torch.randn(n, generator=gen)
    for big in sorted({0, 255, 256, 511, 512, n_jobs - 1} & set(range(n_jobs))):
        tag = f"[n_jobs {n_jobs} dominant {big}]"
        g = g0.clone()
        start = sum(sizes[:big])
        g[start:start + sizes[big]] = 1024.0
        flat[1].t.copy_(g)
        part = kb.Guarded((n_jobs,), torch.float32, DEV, fill=NAN)
        total = kb.Guarded((1,), torch.float32, DEV, fill=NAN)
        o.grad_sqnorm_multi(table, part.t)
        o.adam_multi_clip(table, part.t, math.inf, *HYPER[0], total_norm=total.t[0])
        torch.cuda.synchronize()
        kb.assert_guards_intact(*flat, part, total, label="total" + tag)
        assert torch.equal(bits(flat[1].t), bits(g)), "measure only: g untouched" + tag
        pc = part.t.cpu()
        pr = []
        off = 0
        for s in sizes:
            pr.append(kb.ref_grad_sqnorm(g[off:off + s]))
            off += s
        kb.assert_within(pc, torch.stack([r for r, _ in pr]), torch.stack([b for _, b in pr]),
                         "grad_sqnorm_multi small jobs" + tag)
        tref, tbnd = kb.ref_clip_total(pc)
        assert float(pc[big]) > 0.9 * float(tref) ** 2  # (that job's partial is nearly all of the sum)
        kb.assert_within(total.t, tref.view(1), tbnd.view(1), "adam_multi_clip total over n_jobs" + tag)


@pytest.mark.parametrize("what", ["inf", "nan"])
def test_non_finite_total(hip, what):
    o = ops()
    lr, b1, b2, eps, wd, step = hp = HYPER[0][:5] + (3,)
    sizes = [1, 7, 257, 32769]
    gen = torch.Generator().manual_seed(21)
    cpu = []
    for n in sizes:
        p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        cpu.append((p, g, 0.3 * torch.randn(n, generator=gen), (0.5 * torch.randn(n, generator=gen)) ** 2))
    cpu[2][1][100] = float(what)
    cpu[1][1][3] = -0.0
    q = Quads(cpu, (0, 0, 0, 0, 0))
    P, G, M, V = (q.flat(k) for k in range(4))
    at = 1 + 7 + 100
    part = kb.Guarded((q.n_jobs,), torch.float32, DEV, fill=NAN)
    total = kb.Guarded((1,), torch.float32, DEV, fill=NAN)
    o.grad_sqnorm_multi(q.table, part.t)
    o.adam_multi_clip(q.table, part.t, 1.0, *hp, total_norm=total.t[0])
    q.done(part, total, label="non-finite " + what)
    t = float(total.t.cpu()[0])
    g1 = q.read(1)
    if what == "nan":
        assert math.isnan(t) and bool(torch.isnan(g1).all())
        return
    assert t == math.inf and kb.clip_coef(t, 1.0) == 0.0
    others = torch.ones(G.numel(), dtype=torch.bool)
    others[at] = False
    assert math.isnan(float(g1[at]))
    want = torch.where(torch.signbit(G), -0.0, 0.0).float()
    assert torch.equal(bits(g1)[others], bits(want)[others]), "g' is not a zero of g's sign in every workgroup"
    (_, _), (mr, mb), (vr, vb) = kb.ref_adam(P, torch.zeros_like(G), M, V, lr, (b1, b2), eps, wd, step)
    assert torch.equal(mr, b1 * M.double())
    kb.assert_within(q.read(2)[others], mr[others], mb[others], "adam_multi_clip exp_avg[inf total]")
    kb.assert_within(q.read(3)[others], vr[others], vb[others], "adam_multi_clip exp_avg_sq[inf total]")


@pytest.mark.parametrize("hyper", HYPER, ids=HYPER_IDS)
@pytest.mark.parametrize("n", [1, 257, 2048 * 256 + 5])
def test_legacy_adam_step(hip, n, hyper):
    """``wsr_adam_step`` against the fp32 hyper-parameters it receives; 2048 * 256 + 5: five elements on the second trip"""
    o = ops()
    lr, b1, b2, eps, wd, step = hyper
    p, g, m, v = kb.adam_case(n, step, 77 + HYPER.index(hyper))
    bufs = [kb.Guarded((n,), torch.float32, DEV, fill=t.to(DEV)) for t in (p, g, m, v)]
    o.adam_step(*[b.t for b in bufs], lr, b1, b2, eps, wd, step)
    torch.cuda.synchronize()
    tag = f"[n {n} {HYPER_IDS[HYPER.index(hyper)]}]"
    kb.assert_guards_intact(*bufs, label="adam_step" + tag)
    assert torch.equal(bits(bufs[1].t), bits(g))
    ref = kb.ref_adam(p, g, m, v, lr, (b1, b2), eps, wd, step, f32_hyper=True)
    for name, k, (r, b) in zip(("p", "exp_avg", "exp_avg_sq"), (0, 2, 3), ref):
        kb.assert_within(bufs[k].t, r, b, f"adam_step {name}" + tag)


def test_table_adam_step(hip):
    """``TableAdam.step()``: two parameter groups, clipping and the moving average on, three steps - each step's p', g',
    m', v', shadow and norm against float64 from the device state read back before it"""
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(13)
    shapes = [[(70001,), (5,)], [(33, 7, 3, 3, 3), (1,)]]
    params = [[torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in grp] for grp in shapes]
    groups = [dict(params=params[0], lr=1e-2, weight_decay=0.01), dict(params=params[1], lr=8e-5, betas=(0.9, 0.99))]
    max_norm, d = 20.0, 0.99
    opt = TableAdam(groups, lr=1e-3, betas=(0.5, 0.999), eps=1e-8, max_grad_norm=max_norm, ema_decay=d)
    flat_params = [p for grp in params for p in grp]
    for step in (1, 2, 3):
        before = []
        for p in flat_params:
            p.grad = (0.5 * torch.randn(p.shape, generator=gen)).to(DEV)
            st = opt.state.get(p, {})
            zero = torch.zeros(p.shape)
            before.append((p.detach().cpu(), p.grad.cpu(), st["exp_avg"].cpu() if st else zero,
                           st["exp_avg_sq"].cpu() if st else zero))
        e_before = [e.cpu() for e in opt.ema_shadows]
        opt.step()
        torch.cuda.synchronize()
        norms = opt.last_grad_norm.cpu()
        k = 0
        for gi, (grp, pg) in enumerate(zip(params, opt.param_groups)):
            quads = before[k:k + len(grp)]
            sq = sum(float(q[1].double().pow(2).sum()) for q in quads)
            n_max = max(q[0].numel() for q in quads)
            tref = torch.tensor(math.sqrt(sq), dtype=torch.float64)
            # the partials' bound through the root (relative: half), then the root's own
            n_jobs = len(kb.adam_jobs([q[0].numel() for q in quads]))
            tb = 0.5 * kb.bound(tref, tref, min(n_max, kb.ADAM_CHUNK) + 10, 0.0) + kb.bound(tref, tref, n_jobs + 2, 0.0)
            kb.assert_within(norms[gi].view(1), tref.view(1), tb.view(1), f"TableAdam norm[step {step} group {gi}]")
            c = kb.clip_coef(float(norms[gi]), max_norm)
            assert c < 1.0
            for j, p in enumerate(grp):
                p0, g0, m0, v0 = (t.flatten() for t in quads[j])
                tag = f"[step {step} group {gi} tensor {j}]"
                gref = c * g0.double()
                kb.assert_within(p.grad.flatten(), gref, kb.bound(gref, gref.abs(), kb.K_CLIP_G, 0.0),
                                 "TableAdam g" + tag)
                ref = kb.ref_adam(p0, g0, m0, v0, pg["lr"], pg["betas"], pg["eps"], pg["weight_decay"], step, coef=c)
                st = opt.state[p]
                for name, got, (r, b) in zip(("p", "exp_avg", "exp_avg_sq"),
                                             (p.detach(), st["exp_avg"], st["exp_avg_sq"]), ref):
                    kb.assert_within(got.flatten(), r, b, f"TableAdam {name}" + tag)
                e0, pn = e_before[k + j].flatten(), p.detach().cpu().flatten()
                kb.assert_within(opt.ema_shadows[k + j].flatten(), d * e0.double() + (1.0 - d) * pn.double(),
                                 kb.ema_step_bound(d, e0, pn), "TableAdam shadow" + tag)
            k += len(grp)
