"""[GRAD_CLIP] on the CPU: the config section, TableAdam's clipping on its torch fallback, and clipping under data
parallelism (world 2 over gloo, the product wind_field_GAN_3D with the CPU oracle's networks, as test_dist_gloo.py).

The norm must come from the AVERAGED gradients - clipping in front of the step pre-hook that waits for the gradient
collectives would clip each rank's own gradients and the replicas would drift apart."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO

LOCAL_INI = os.path.join(REPO, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini")
SECTION = ("[GRAD_CLIP]\nclip_generator = True\nclip_discriminator = True\nmax_norm_discriminator = 0.25\n"
           "log_grad_norms = True\n")


def _ini_with(tmp_path, extra: str, name="c.ini") -> str:
    with open(LOCAL_INI) as f:
        text = f.read()
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text + "\n" + extra)
    return path


# ---------------------------------------------------------------------------------------------------- config
def test_section_absent_gives_defaults_and_unchanged_text(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    cfg = Config(LOCAL_INI)
    gc = cfg.grad_clip
    assert (gc.clip_generator, gc.clip_discriminator, gc.max_norm_discriminator, gc.log_grad_norms) == \
        (False, False, 1.0, False)
    text = cfg.asINI()
    assert "GRAD_CLIP" not in text and "clip_generator" not in text
    # the text of a config without the extension: loading it again gives the same text
    path = str(tmp_path / "round.ini")
    with open(path, "w") as f:
        f.write(text)
    assert Config(path).asINI() == text
    # a file with the section prints the same text plus the section
    with_sec = Config(_ini_with(tmp_path, SECTION)).asINI()
    assert Config(LOCAL_INI).asINI() == text  # (the singleton section reset by the next load)
    assert with_sec == text + "\n" + SECTION


def test_section_present_parsed_printed_and_reparsed(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    cfg = Config(_ini_with(tmp_path, "[GRAD_CLIP]\nclip_discriminator = True\nmax_norm_discriminator = 0.5\n"))
    gc = cfg.grad_clip
    assert (gc.clip_generator, gc.clip_discriminator, gc.max_norm_discriminator, gc.log_grad_norms) == \
        (False, True, 0.5, False)
    text = cfg.asINI()
    assert "[GRAD_CLIP]\nclip_generator = False\nclip_discriminator = True\nmax_norm_discriminator = 0.5\n" \
           "log_grad_norms = False\n" in text
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.grad_clip) == vars(gc) and again.asINI() == text


@pytest.mark.parametrize("bad", ["0", "-1.0", "nan", "inf"])
def test_bad_bounds_raise(tmp_path, bad):
    from gan_sr_wind_field_amd.config.config import Config

    with pytest.raises(ValueError, match="max_norm_discriminator"):
        Config(_ini_with(tmp_path, f"[GRAD_CLIP]\nclip_discriminator = True\nmax_norm_discriminator = {bad}\n"))
    with open(LOCAL_INI) as f:
        text = f.read().replace("max_norm = 1.0", f"max_norm = {bad}")
    path = str(tmp_path / "g.ini")
    with open(path, "w") as f:
        f.write(text + "\n[GRAD_CLIP]\nclip_generator = True\n")
    with pytest.raises(ValueError, match=r"\[GENERATOR\] max_norm"):
        Config(path)
    with open(path, "w") as f:  # a bound that does not clip is not checked
        f.write(text + "\n[GRAD_CLIP]\nclip_generator = False\nmax_norm_discriminator = -3\n")
    Config(path)


# ---------------------------------------------------------------------------------------------------- TableAdam
@pytest.mark.parametrize("bound", [0.5, 1e4], ids=["clips", "does_not_clip"])
def test_table_adam_clip_on_cpu_equals_torch(bound):
    """CPU tensors take torch's path: clip_grad_norm_ over the group, then torch's (fused) Adam - the same bits"""
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(3)
    shapes = [(700,), (3, 7, 3), (5,)]
    ref_p = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    my_p = [p.detach().clone().requires_grad_(True) for p in ref_p]
    kw = dict(lr=1e-3, betas=(0.5, 0.999), weight_decay=0.01, fused=True)
    ref = torch.optim.Adam(ref_p, **kw)
    opt = TableAdam(my_p, max_grad_norm=bound, **kw)
    coefs = []
    for _ in range(4):
        for rp, mp_ in zip(ref_p, my_p):
            g = torch.randn(rp.shape, generator=gen)
            rp.grad, mp_.grad = g.clone(), g.clone()
        n_ref = torch.nn.utils.clip_grad_norm_(ref_p, bound)
        ref.step()
        opt.step()
        coefs.append(bound / (float(n_ref) + 1e-6))
        assert torch.equal(opt.last_grad_norm, n_ref)
        for rp, mp_ in zip(ref_p, my_p):
            assert torch.equal(mp_.grad, rp.grad) and torch.equal(mp_.detach(), rp.detach())
    assert (min(coefs) < 1) == (bound < 1)


def test_table_adam_bound_checks():
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    p = [torch.zeros(3, requires_grad=True)]
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_grad_norm"):
            TableAdam(p, max_grad_norm=bad)
    opt = TableAdam(p)
    assert opt.max_grad_norm is None and opt.last_grad_norm is None
    opt.max_grad_norm = 2
    assert opt.max_grad_norm == 2.0


def test_table_adam_track_only_leaves_the_step_alone():
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(4)
    ref_p = [torch.randn(40, generator=gen).requires_grad_(True)]
    my_p = [ref_p[0].detach().clone().requires_grad_(True)]
    ref, opt = torch.optim.Adam(ref_p, lr=1e-2, fused=True), TableAdam(my_p, lr=1e-2, track_grad_norm=True)
    g = torch.randn(40, generator=gen) * 100
    ref_p[0].grad, my_p[0].grad = g.clone(), g.clone()
    ref.step()
    opt.step()
    assert torch.equal(my_p[0].detach(), ref_p[0].detach()) and torch.equal(my_p[0].grad, g)
    assert torch.equal(opt.last_grad_norm, torch.linalg.vector_norm(g))


# ---------------------------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


G_KEYS = ("model.0.0.weight", "hr_convs.2.weight", "model.1.module.0.RDBs.1.LFF.bias")


def _build_gan(clip: bool):
    import oracle_nets
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as mod
    from oracle import nets as onets

    mod.Generator_3D = oracle_nets.OracleGenerator
    mod.Discriminator_3D = oracle_nets.OracleDiscriminator
    cfg = Config(LOCAL_INI)
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = None, torch.device("cpu")
    cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 16, 1, 8
    cfg.generator.terrain_number_of_features = 4
    cfg.generator.dropout_probability = cfg.discriminator.dropout_probability = 0.0
    cfg.discriminator.num_features = 4
    cfg.gan_config.number_of_z_layers = 4
    cfg.training.use_instance_noise = False
    cfg.training.use_noisy_labels = False
    cfg.training.niter = 150000
    if clip:  # bounds far below these networks' gradient norms: both clips engage
        cfg.generator.max_norm = 1e-3
        gc = cfg.grad_clip
        gc.clip_generator = gc.clip_discriminator = gc.log_grad_norms = True
        gc.max_norm_discriminator = 1e-3
    torch.manual_seed(2001)
    gan = mod.wind_field_GAN_3D(cfg)
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=4, hr_kern=5, upscale=4)
    ds = onets.DSpec(bf=4, nz=4, enable_slicing=True)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
    return gan, cfg


def _g_and_d_iteration(gan, cfg, LR, HR, Z, x, y):
    """it 0: a generator iteration, it 1: a discriminator iteration (period 1, ratio 1)"""
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter), 1, 1)
    out = {}
    gan.optimize_parameters(LR, HR, Z, 0)
    sd = gan.G.state_dict()
    out.update({"G." + k: sd[k].clone() for k in G_KEYS})
    out.update({"gradG." + k: dict(gan.G.named_parameters())[k].grad.clone() for k in G_KEYS})
    gan.optimize_parameters(LR, HR, Z, 1)
    out.update({"D." + k: v.clone() for k, v in gan.D.state_dict().items() if v.is_floating_point()})
    out.update({"gradD.cls." + k: v.grad.clone() for k, v in gan.D.classifier.named_parameters()})
    out["clippedD"] = torch.stack([p.grad.double().pow(2).sum() for p in gan.D.parameters() if p.grad is not None]).sum().sqrt()
    out.update({"norm." + k: v.clone() for k, v in gan.get_grad_norms().items()})
    return out


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from gan_sr_wind_field_amd import dist as wdist
    from oracle.gan import synthetic_batch

    assert wdist.init_from_env("gloo")
    gan, cfg = _build_gan(clip=True)
    wdist.attach(gan, bucket_mb=0.05, sync_bn=True)
    LR, HR, Z, x, y = synthetic_batch(world, 16, 4, 4, seed=2001)
    sl = slice(rank, rank + 1)
    torch.save(_g_and_d_iteration(gan, cfg, LR[sl], HR[sl], Z[sl], x, y), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_clipped_steps_equal_full_batch(tmp_path, monkeypatch):
    """G (per-parameter hooks on the CPU stand-ins): the clipped two-rank step equals the clipped full-batch step.  D,
    classifier head included (``_avg_param``, averaged inside ``wait()``): the replicas stay bit-identical and the
    clipped gradients have the bound's norm.  (The CPU stand-in discriminator keeps per-rank BatchNorm statistics, so
    its two-rank step is not the full-batch one; the HIP discriminator's is, see test_grad_clip_gpu.py.)"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle.gan import synthetic_batch

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as mod
    for name in ("Generator_3D", "Discriminator_3D"):  # (_build_gan swaps in the stand-ins: put the product's back after)
        monkeypatch.setattr(mod, name, getattr(mod, name))
    gan, cfg = _build_gan(clip=True)
    LR, HR, Z, x, y = synthetic_batch(world, 16, 4, 4, seed=2001)
    ref = _g_and_d_iteration(gan, cfg, LR, HR, Z, x, y)
    assert float(ref["norm.G"]) > 1e-2 and float(ref["norm.D"]) > 1e-2  # the bounds (1e-3) clip
    for k, v in ref.items():
        if "running_" not in k:  # (per-rank BatchNorm running statistics: see above)
            assert torch.equal(r0[k], r1[k]), k
        if k in ("norm.D", "clippedD") or k.startswith(("D.", "gradD.")):
            continue
        if k.startswith("norm."):
            np.testing.assert_allclose(float(r0[k]), float(v), rtol=1e-4, err_msg=k)
        elif k.startswith("grad"):  # the clipped gradients: norm 1e-3 over the whole network
            np.testing.assert_allclose(r0[k].numpy(), v.numpy(), rtol=1e-3, atol=1e-9, err_msg=k)
        else:
            np.testing.assert_allclose(r0[k].numpy(), v.numpy(), rtol=2e-5, atol=1e-7, err_msg=k)
    # the clipped generator gradients have norm max_norm (to torch's 1e-6 in the denominator)
    sq = sum(float(p.grad.double().pow(2).sum()) for p in gan.G.parameters() if p.grad is not None)
    assert abs(math.sqrt(sq) - 1e-3) < 1e-6
    for r in (r0, r1, ref):
        assert float(r["norm.D"]) > 1e-2 and abs(float(r["clippedD"]) - 1e-3) < 1e-6
