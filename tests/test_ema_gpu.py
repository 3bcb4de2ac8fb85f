"""[EMA] on the MI355X: the two kernels (``wsr_adam_multi_ema``, ``wsr_adam_multi_clip_ema``) against float64 and
against the kernels they extend, the GAN's training with and without the section, the swap scope through the
generator program's packed-filter caches, checkpoint resume, and ``run.py --train --test``.

The per-element bound of one shadow update and the K-step bound are derived in tests/test_ema.py (three roundings per
term: the constant's, the product's, the sum's)."""
import csv
import math
import os

import pytest
import torch

from conftest import REPO
from test_ema import replay, step_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(70001,), (33, 7, 3, 3, 3), (128,), (5,), (1,), (32768,), (32769,)]
HYPER = dict(lr=8e-5, beta1=0.5, beta2=0.999, eps=1e-8, weight_decay=0.01)


def _make(seed=11):
    """[(p, g, m, v)] and the shadows, the same bits and the same alignments for the same seed.  Beside the aligned
    tensors: a quad whose four tensors and shadow sit 4 bytes off the 16-byte alignment (the scalar path), and two
    aligned quads whose SHADOW alone is misaligned (the float4 path, the shadow moved element by element)."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(shape, off=0, pos=False):
        n = math.prod(shape)
        t = torch.randn(n + off, generator=gen)
        if pos:
            t = t * t
        return t.to(DEV)[off:].view(shape)

    quads, shadows = [], []
    for shape, off_q, off_e in [(s, 0, 0) for s in SHAPES] + [((40001,), 1, 1), ((4099,), 0, 1), ((36000,), 0, 3)]:
        quads.append((rnd(shape, off_q), rnd(shape, off_q), rnd(shape, off_q) * 0.1, rnd(shape, off_q, pos=True) * 0.01))
        shadows.append(rnd(shape, off_e))
    assert any(q[0].data_ptr() % 16 for q in quads) and any(e.data_ptr() % 16 and q[0].data_ptr() % 16 == 0
                                                            for q, e in zip(quads, shadows))
    return quads, shadows


def _bits(t):
    """fp32 tensors as their bit patterns (NaN equals NaN, -0 differs from 0); others (BatchNorm's counter) as they are"""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run_ema(d, seed=11, plant=False, clip=None):
    from gan_sr_wind_field_amd import hip_ops

    quads, shadows = _make(seed)
    if plant:
        for i, e in enumerate(shadows):
            e.view(-1)[::3] = float("inf") if i % 2 else float("nan")
    old = [e.clone() for e in shadows]
    table = hip_ops.adam_job_table(quads)
    ptrs = hip_ops.ema_ptr_table(quads, shadows)
    assert ptrs.shape[0] == table.shape[0] > len(quads)  # (tensors above 32 768 elements are cut into chunks)
    norm = None
    if clip is None:
        hip_ops.adam_multi_ema(table, ptrs, *HYPER.values(), 3, d)
    else:
        partials = torch.empty(table.shape[0], dtype=torch.float32, device=DEV)
        norm = torch.empty((), dtype=torch.float32, device=DEV)
        hip_ops.grad_sqnorm_multi(table, partials)
        hip_ops.adam_multi_clip_ema(table, ptrs, partials, clip, *HYPER.values(), 3, d, total_norm=norm)
    return quads, shadows, old, norm


def _run_plain(seed=11, clip=None):
    from gan_sr_wind_field_amd import hip_ops

    quads, _ = _make(seed)
    table = hip_ops.adam_job_table(quads)
    norm = None
    if clip is None:
        hip_ops.adam_multi(table, *HYPER.values(), 3)
    else:
        partials = torch.empty(table.shape[0], dtype=torch.float32, device=DEV)
        norm = torch.empty((), dtype=torch.float32, device=DEV)
        hip_ops.grad_sqnorm_multi(table, partials)
        hip_ops.adam_multi_clip(table, partials, clip, *HYPER.values(), 3, total_norm=norm)
    return quads, norm


# ---------------------------------------------------------------------------------------------------- 5, 6, 7: kernels
@pytest.mark.parametrize("d", [0.999, 0.5])
def test_ema_kernel_equals_float64_leaves_adam_alone_and_is_reproducible(hip, d):
    quads, shadows, old, _ = _run_ema(d)
    ref, _ = _run_plain()
    for i, (q, r) in enumerate(zip(quads, ref)):
        for name, a, b in zip("pgmv", q, r):
            assert _same_bits(a, b), (i, name)
    worst = 0.0
    for i, (q, e, e0) in enumerate(zip(quads, shadows, old)):
        p_new = q[0].cpu()
        want = d * e0.cpu().double() + (1.0 - d) * p_new.double()
        err = (e.cpu().double() - want).abs()
        bound = step_bound(d, e0.cpu(), p_new)
        print(f"tensor {i} n={p_new.numel()}: max err / bound = {float((err / bound).max()):.3f}")
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (i, float((err / bound).max()))
    assert 0 < worst <= 1
    again = _run_ema(d)[1]
    for i, (a, b) in enumerate(zip(shadows, again)):
        assert _same_bits(a, b), i


def test_ema_kernel_decay_zero_copies_whatever_the_shadow_held(hip):
    for plant in (False, True):
        quads, shadows, old, _ = _run_ema(0.0, plant=plant)
        assert not plant or not all(bool(torch.isfinite(o).all()) for o in old)
        ref, _ = _run_plain()
        for i, (q, r, e) in enumerate(zip(quads, ref, shadows)):
            assert _same_bits(q[0], r[0]) and _same_bits(e, q[0]), (i, plant)


@pytest.mark.parametrize("bound", [0.5, math.inf], ids=["clips", "measures_only"])
def test_clip_ema_kernel_leaves_the_clipped_step_alone(hip, bound):
    d = 0.999
    quads, shadows, old, norm = _run_ema(d, clip=bound)
    ref, norm_ref = _run_plain(clip=bound)
    assert _same_bits(norm, norm_ref) and (float(norm) > 100 * 0.5)
    for i, (q, r) in enumerate(zip(quads, ref)):
        for name, a, b in zip("pgmv", q, r):
            assert _same_bits(a, b), (i, name)
    g0 = _make()[0]
    assert any(not _same_bits(q[1], o[1]) for q, o in zip(quads, g0)) == math.isfinite(bound)  # g written back iff it clips
    for i, (q, e, e0) in enumerate(zip(quads, shadows, old)):
        p_new = q[0].cpu()
        want = d * e0.cpu().double() + (1.0 - d) * p_new.double()
        assert bool(((e.cpu().double() - want).abs() <= step_bound(d, e0.cpu(), p_new)).all()), i
    for a, b in zip(shadows, _run_ema(d, clip=bound)[1]):
        assert _same_bits(a, b)


def test_ema_wrappers_refuse_bad_arguments(hip):
    from gan_sr_wind_field_amd import hip_ops

    quads, shadows = _make()
    table = hip_ops.adam_job_table(quads)
    ptrs = hip_ops.ema_ptr_table(quads, shadows)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            hip_ops.adam_multi_ema(table, ptrs, *HYPER.values(), 1, bad)
    with pytest.raises(ValueError, match="one row per job"):
        hip_ops.adam_multi_ema(table, ptrs[:-1], *HYPER.values(), 1, 0.5)
    with pytest.raises(ValueError, match="one shadow per parameter"):
        hip_ops.ema_ptr_table(quads, shadows[:-1])
    with pytest.raises(ValueError, match="shares"):
        hip_ops.ema_ptr_table(quads[:1], [quads[0][0]])
    # the C entry point itself: 0 <= decay < 1
    assert hip.wsr_adam_multi_ema(table.data_ptr(), ptrs.data_ptr(), table.shape[0], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1,
                                  1.0, None) != 0


# ---------------------------------------------------------------------------------------------------- model level
LOCAL_INI = os.path.join(REPO, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini")


def _build_gan(ema, decay=0.9, start_iter=0, dtype="fp32", clip=False, folder=None):
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from oracle import nets as onets

    cfg = Config(LOCAL_INI)
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = 0, DEV
    cfg.compute_dtype = dtype
    cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 16, 1, 8
    cfg.generator.terrain_number_of_features = 8
    cfg.generator.dropout_probability = cfg.discriminator.dropout_probability = 0.0
    cfg.discriminator.num_features = 8
    cfg.gan_config.number_of_z_layers = 4
    cfg.training.use_instance_noise = False
    cfg.training.use_noisy_labels = False
    cfg.training.niter = 150000
    cfg.grad_clip.clip_generator = clip
    cfg.generator.max_norm = 1e-2
    cfg.ema.present, cfg.ema.decay, cfg.ema.start_iter = ema, decay, start_iter
    if folder is not None:
        cfg.env.this_runs_folder = str(folder)
    torch.manual_seed(2001)
    gan = wind_field_GAN_3D(cfg)
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=8, hr_kern=5, upscale=4)
    ds = onets.DSpec(bf=8, nz=4, enable_slicing=True)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
    if ema:
        gan.reset_ema()
    return gan, cfg


def _batch():
    from oracle.gan import synthetic_batch

    return tuple(t.to(DEV) for t in synthetic_batch(2, 16, 4, 4, seed=2001))


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipped"])
def test_training_is_not_perturbed_and_shadows_follow_the_replay(hip, clip):
    """iterations 0..7 with ``d_g_train_ratio`` 2: generator steps at 0, 3 and 6; ``start_iter`` 3: the first copies,
    the other two average"""
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    LR, HR, Z, x, y = _batch()
    d = 0.9
    runs = {}
    for ema in (False, True):
        gan, cfg = _build_gan(ema, decay=d, start_iter=3, clip=clip)
        assert isinstance(gan.optimizer_G, TableAdam) and (gan.optimizer_G.ema_decay is not None) == ema
        assert gan.optimizer_D.ema_decay is None
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 2, 1)
        g_steps, losses, shadows = [], [], []
        gan.optimizer_G.register_step_post_hook(
            lambda *_, g=gan, s=g_steps: s.append([p.detach().cpu().clone() for p in g.G.parameters()]))
        for it in range(8):
            gan.optimize_parameters(LR, HR, Z, it)
            losses.append([float(v.detach()) for v in gan.get_G_train_loss_dict_ref().values()]
                          + [float(gan.get_D_loss_dict_ref()["train_loss"].detach())])
            if ema:
                shadows.append([e.cpu().clone() for e in gan.ema_shadows])
        runs[ema] = (gan, losses, g_steps, shadows)
    (plain, l0, s0, _), (gan, l1, g_steps, shadows) = runs[False], runs[True]
    assert len(g_steps) == len(s0) == 3
    assert l0 == l1
    for net in ("G", "D"):
        for (k, u), (_, v) in zip(getattr(plain, net).state_dict().items(), getattr(gan, net).state_dict().items()):
            assert _same_bits(u, v), (net, k)
    assert set(gan.optimizer_G.state_dict()) == {"state", "param_groups"}
    for e, w in zip(shadows[0], g_steps[0]):
        assert _same_bits(e, w)  # before start_iter the shadow is the weights
    for it in (1, 2, 4, 5, 7):  # discriminator iterations leave the shadows alone
        assert all(_same_bits(a, b) for a, b in zip(shadows[it], shadows[it - 1])), it
    names = [k for k, _ in gan.G.named_parameters()]
    worst = 0.0
    for i, e in enumerate(shadows[-1]):
        ws = [s[i] for s in g_steps]
        want, bound = replay(lambda k: 0.0 if k == 0 else d, torch.zeros_like(ws[0]), ws)
        err = (e.double() - want).abs()
        ok = err <= bound
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool(ok.all()), (names[i], float((err / bound).max()))
        assert not _same_bits(e, ws[-1]), names[i]
    print(f"largest shadow error / K-step bound over {len(names)} tensors: {worst:.3f}")
    sd = gan.G_ema_state_dict()
    assert list(sd) == list(gan.G.state_dict()) and all(_same_bits(sd[k].cpu(), e) for k, e in zip(sd, shadows[-1]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scope_runs_the_shadow_weights_and_leaves_no_stale_pack(hip, dtype):
    LR, HR, Z, x, y = _batch()
    gan, cfg = _build_gan(True, decay=0.5, dtype=dtype)
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 1)
    for it in range(4):
        gan.optimize_parameters(LR, HR, Z, it)
    gan.G.eval()
    with torch.no_grad():
        before = gan.G(LR, Z).clone()
        with gan.ema_scope():
            inside = gan.G(LR, Z).clone()
            inside_again = gan.G(LR, Z).clone()
        after = gan.G(LR, Z).clone()
        other, _ = _build_gan(False, dtype=dtype)
        other.G.load_state_dict(gan.G_ema_state_dict())
        other.G.eval()
        want = other.G(LR, Z)
        assert _same_bits(inside, want) and _same_bits(inside_again, want)
        assert _same_bits(after, before) and not _same_bits(inside, before)
        # a body that raises: the live weights are back, and so are their packed copies
        with pytest.raises(KeyError):
            with gan.ema_scope():
                gan.G(LR, Z)
                raise KeyError("body")
        assert _same_bits(gan.G(LR, Z), before)
    # training goes on with the live weights: the same step as a model that never entered the scope
    twin, cfg2 = _build_gan(True, decay=0.5, dtype=dtype)
    twin.feed_xy_niter(x, y, torch.tensor(cfg2.training.niter, device=DEV), 1, 1)
    for it in range(4):
        twin.optimize_parameters(LR, HR, Z, it)
    for g in (gan, twin):
        for it in (4, 5):
            g.optimize_parameters(LR, HR, Z, it)
    for (k, u), (_, v) in zip(gan.G.state_dict().items(), twin.G.state_dict().items()):
        assert _same_bits(u, v), k
    for i, (a, b) in enumerate(zip(gan.ema_shadows, twin.ema_shadows)):
        assert _same_bits(a, b), i


def test_checkpoint_resume_with_shadows_equals_uninterrupted_run(hip, tmp_path):
    LR, HR, Z, x, y = _batch()

    def fresh():
        gan, cfg = _build_gan(True, decay=0.9, start_iter=2, folder=tmp_path)
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 1)
        return gan

    a = fresh()
    for it in (1, 2, 3, 4):
        a.optimize_parameters(LR, HR, Z, it)
    a.save_model(str(tmp_path), 0, 4)
    saved = torch.load(str(tmp_path / "G_ema_4.pth"), map_location="cpu")
    weights = torch.load(str(tmp_path / "G_4.pth"), map_location="cpu")
    assert list(saved) == list(weights) and all(saved[k].shape == weights[k].shape for k in saved)
    assert any(not torch.equal(saved[k], weights[k]) for k in saved)
    assert set(torch.load(str(tmp_path / "state_4.pth"), map_location="cpu")["optimizers"][0]) == {"state", "param_groups"}
    for it in (5, 6, 7, 8):
        a.optimize_parameters(LR, HR, Z, it)

    b = fresh()
    assert b.load_model(str(tmp_path / "G_4.pth"), str(tmp_path / "D_4.pth"), str(tmp_path / "state_4.pth")) == (0, 4)
    for k, e in zip(saved, b.ema_shadows):
        assert _same_bits(e.cpu(), saved[k]), k
    b.G.train()
    for it in (5, 6, 7, 8):
        b.optimize_parameters(LR, HR, Z, it)
    for net in ("G", "D"):
        sa, sb = getattr(a, net).state_dict(), getattr(b, net).state_dict()
        for k in sa:
            assert _same_bits(sa[k], sb[k]), (net, k)
    for i, (ea, eb) in enumerate(zip(a.ema_shadows, b.ema_shadows)):
        assert _same_bits(ea, eb), i


# ---------------------------------------------------------------------------------------------------- run.py
def test_run_train_and_test_with_ema(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))

    def rows(name):
        with open(os.path.join("test_output", f"{name}____metrics.csv")) as f:
            return list(csv.reader(f))

    def run(name, flags, section, **env):
        ini = str(tmp_path / f"{name}.ini")
        cfg = _write_ini(ini)
        cfg.name = name
        for k, v in env.items():
            setattr(cfg.env, k, v)
        with open(ini, "w") as f:
            f.write(cfg.asINI() + section)
        runmod.main(flags + ["--cfg", ini])
        return os.path.join(str(tmp_path), "runs", name)

    section = "\n[EMA]\ndecay = 0.5\nstart_iter = 3\n"
    dir_a = run("ema_on", ["--train", "--test"], section)
    for f in ("G_6.pth", "G_ema_6.pth", "D_6.pth", "state_6.pth"):
        assert os.path.isfile(os.path.join(dir_a, f)), f
    with open(os.path.join(dir_a, "config.ini")) as f:
        assert "[EMA]\ndecay = 0.5\nstart_iter = 3\nvalidate_with_ema = True\ntest_with_ema = True\n" in f.read()
    g, e = (torch.load(os.path.join(dir_a, f), map_location="cpu") for f in ("G_6.pth", "G_ema_6.pth"))
    assert list(g) == list(e) and any(not torch.equal(g[k], e[k]) for k in g)
    dir_b = run("ema_live", ["--train", "--test"], section + "test_with_ema = False\n")
    assert os.path.isfile(os.path.join(dir_b, "G_ema_6.pth"))
    # a configuration without the section pointed at the averaged weights
    dir_c = run("ema_file", ["--test"], "", generator_load_path=os.path.join(dir_a, "G_ema_6.pth"),
                discriminator_load_path=os.path.join(dir_a, "D_6.pth"),
                state_load_path=os.path.join(dir_a, "state_6.pth"))
    assert not os.path.exists(os.path.join(dir_c, "G_ema_6.pth"))
    a, b, c = rows("ema_on"), rows("ema_live"), rows("ema_file")
    assert len(a) == len(b) == len(c) > 1
    assert a == c
    assert a[0] == b[0] and a[1:] != b[1:]
    # the section without the file: --test names what is missing
    os.remove(os.path.join(dir_a, "G_ema_6.pth"))
    with pytest.raises(FileNotFoundError, match="G_ema_6.pth"):
        run("ema_on", ["--test"], section)
