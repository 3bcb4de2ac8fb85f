"""[GRAD_CLIP] on the MI355X: the two kernels (``wsr_grad_sqnorm_multi``, ``wsr_adam_multi_clip``), TableAdam's
clipped fast path against ``clip_grad_norm_`` + ``torch.optim.Adam`` on the CPU, the GAN's clipped G and D steps,
``run.py --train`` with the section, and a two-rank clipped step through the HIP programs."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(70001,), (33, 7, 3, 3, 3), (128,), (5,), (32768,), (32769,)]


def _table(grads):
    from gan_sr_wind_field_amd import hip_ops

    quads = [(torch.zeros_like(g), g, torch.zeros_like(g), torch.zeros_like(g)) for g in grads]
    return hip_ops.adam_job_table(quads), quads


def test_grad_sqnorm_kernel_equals_float64_and_is_reproducible(hip):
    from gan_sr_wind_field_amd import hip_ops

    gen = torch.Generator().manual_seed(7)
    cpu = [torch.randn(s, generator=gen) * (1 + i) for i, s in enumerate(SHAPES)]
    grads = [g.to(DEV) for g in cpu]
    base = torch.randn(40001, generator=gen)
    grads.append(base.to(DEV)[1:])  # a view 4 bytes off the 16-byte alignment: the scalar path
    cpu.append(base[1:])
    table, _ = _table(grads)
    assert any(g.data_ptr() % 16 for g in grads)
    partials = torch.empty(table.shape[0], dtype=torch.float32, device=DEV)
    hip_ops.grad_sqnorm_multi(table, partials)
    first = partials.clone()
    hip_ops.grad_sqnorm_multi(table, partials)
    assert torch.equal(first.view(torch.int32), partials.view(torch.int32))
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in cpu))
    got = math.sqrt(float(partials.double().sum()))
    assert abs(got - want) / want <= 1e-6, (got, want)
    # the clip launch's own reduction of the partials (measure-only: nothing is written but the norm and the update)
    norm = torch.empty((), dtype=torch.float32, device=DEV)
    hip_ops.adam_multi_clip(table, partials, math.inf, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, total_norm=norm)
    assert abs(float(norm) - want) / want <= 1e-6
    for g, c in zip(grads, cpu):
        assert torch.equal(g.cpu(), c)  # measure-only leaves the gradients alone


@pytest.mark.parametrize("bound,scales,clipped", [
    (0.5, [1.0] * 6, [True] * 6),
    (20.0, [1.0, 1e-3, 1.0, 1e-3, 1e-3, 1.0], [True, False, True, False, False, True]),
    (1e6, [1.0] * 6, [False] * 6)], ids=["every_step", "some_steps", "never"])
def test_table_adam_clip_equals_torch(hip, bound, scales, clipped):
    """TableAdam(max_grad_norm) on the device == clip_grad_norm_ + torch.optim.Adam on the CPU: six steps with weight
    decay, a learning-rate change and a state_dict round trip; the clipped .grad and the returned norm too"""
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(5)
    ref_p = [torch.randn(s, generator=gen).requires_grad_(True) for s in SHAPES]
    dev_p = [p.detach().clone().to(DEV).requires_grad_(True) for p in ref_p]
    kw = dict(lr=8e-5, betas=(0.5, 0.999), weight_decay=0.01)
    ref = torch.optim.Adam(ref_p, **kw)
    opt = TableAdam(dev_p, max_grad_norm=bound, **kw)
    for it in range(6):
        if it == 3:
            sd = opt.state_dict()
            opt = TableAdam(dev_p, max_grad_norm=bound, **kw)
            opt.load_state_dict(sd)
            for o_ in (ref, opt):
                o_.param_groups[0]["lr"] = 4e-5
        for rp, dp in zip(ref_p, dev_p):
            g = torch.randn(rp.shape, generator=gen) * scales[it]
            rp.grad, dp.grad = g.clone(), g.to(DEV)
        n_ref = torch.nn.utils.clip_grad_norm_(ref_p, bound)
        ref.step()
        opt.step()
        assert (bound / (float(n_ref) + 1e-6) < 1) == clipped[it], it
        assert opt.last_grad_norm.device == DEV and opt.last_grad_norm.dim() == 0
        assert abs(float(opt.last_grad_norm) - float(n_ref)) <= 2e-6 * float(n_ref), it
        for rp, dp in zip(ref_p, dev_p):
            assert rel_l2(dp.grad, rp.grad) < 1e-6, it
    for rp, dp in zip(ref_p, dev_p):
        assert rel_l2(dp.detach(), rp.detach()) < 1e-6
    sd, sd_ref = opt.state_dict(), ref.state_dict()
    for i in range(len(SHAPES)):
        assert float(sd["state"][i]["step"]) == 6.0
        assert rel_l2(sd["state"][i]["exp_avg_sq"], sd_ref["state"][i]["exp_avg_sq"]) < 1e-6
        assert rel_l2(sd["state"][i]["exp_avg"], sd_ref["state"][i]["exp_avg"]) < 1e-6


def test_table_adam_track_only_is_the_plain_step_bitwise(hip):
    from gan_sr_wind_field_amd.tools.table_adam import TableAdam

    gen = torch.Generator().manual_seed(6)
    a = [torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in SHAPES]
    b = [p.detach().clone().requires_grad_(True) for p in a]
    oa, ob = TableAdam(a, lr=1e-3, weight_decay=0.01), TableAdam(b, lr=1e-3, weight_decay=0.01, track_grad_norm=True)
    for _ in range(3):
        for pa, pb in zip(a, b):
            g = torch.randn(pa.shape, generator=gen).to(DEV)
            pa.grad, pb.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    assert oa.last_grad_norm is None and float(ob.last_grad_norm) > 0
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb) and torch.equal(pa.grad, pb.grad)


# ---------------------------------------------------------------------------------------------------- model level
LOCAL_INI = os.path.join(REPO, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini")


def _build_gan(clip, track=False, device_index=0, bound=1e-2):
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from oracle import nets as onets

    dev = torch.device(f"cuda:{device_index}")
    cfg = Config(LOCAL_INI)
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = device_index, dev
    cfg.compute_dtype = "fp32"
    cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 16, 1, 8
    cfg.generator.terrain_number_of_features = 8
    cfg.generator.dropout_probability = cfg.discriminator.dropout_probability = 0.0
    cfg.discriminator.num_features = 8
    cfg.gan_config.number_of_z_layers = 4
    cfg.training.use_instance_noise = False
    cfg.training.use_noisy_labels = False
    cfg.training.niter = 150000
    gc = cfg.grad_clip
    gc.clip_generator = gc.clip_discriminator = clip
    gc.log_grad_norms = clip or track
    cfg.generator.max_norm = gc.max_norm_discriminator = bound
    torch.manual_seed(2001)
    gan = wind_field_GAN_3D(cfg)
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=8, hr_kern=5, upscale=4)
    ds = onets.DSpec(bf=8, nz=4, enable_slicing=True)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
    return gan, cfg


def _capture(opt, log):
    """step pre-hook: the step's inputs (parameters, gradients, optimizer state) as CPU copies"""
    def hook(o, *_):
        params = [p for g in o.param_groups for p in g["params"]]
        sd = copy.deepcopy(o.state_dict())
        sd["state"] = {k: {n: t.detach().cpu() for n, t in v.items()} for k, v in sd["state"].items()}
        log.append(dict(p=[p.detach().cpu().clone() for p in params],
                        g=[None if p.grad is None else p.grad.detach().cpu().clone() for p in params], sd=sd,
                        group={k: v for k, v in o.param_groups[0].items() if k != "params"}))
    opt.register_step_pre_hook(hook)


def _torch_step(rec, bound):
    """clip_grad_norm_ + torch.optim.Adam on CPU copies of a captured step's inputs"""
    p = [t.clone().requires_grad_(True) for t in rec["p"]]
    for t, g in zip(p, rec["g"]):
        t.grad = None if g is None else g.clone()
    grp = rec["group"]
    ref = torch.optim.Adam(p, lr=grp["lr"], betas=grp["betas"], eps=grp["eps"], weight_decay=grp["weight_decay"])
    if rec["sd"]["state"]:
        ref.load_state_dict(rec["sd"])
    norm = torch.nn.utils.clip_grad_norm_([t for t in p if t.grad is not None], bound)
    ref.step()
    return p, norm


def _iterations(gan, cfg, n=3):
    from oracle.gan import synthetic_batch

    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    dev = cfg.device
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    norms = []
    for it in range(n):  # it 0: G, 1: D, 2: G (period 1, ratio 1)
        gan.optimize_parameters(LR.to(dev), HR.to(dev), Z.to(dev), it)
        norms.append({k: None if v is None else float(v) for k, v in gan.get_grad_norms().items()})
    return norms


def test_gan_clipped_steps_equal_torch_clip_and_adam(hip):
    bound = 1e-2
    gan, cfg = _build_gan(clip=True, bound=bound)
    logs = {"G": [], "D": []}
    _capture(gan.optimizer_G, logs["G"])
    _capture(gan.optimizer_D, logs["D"])
    norms = _iterations(gan, cfg)
    assert len(logs["G"]) == 2 and len(logs["D"]) == 1
    for w, net, opt in (("G", gan.G, gan.optimizer_G), ("D", gan.D, gan.optimizer_D)):
        rec = logs[w][-1]
        p_ref, n_ref = _torch_step(rec, bound)
        assert bound / (float(n_ref) + 1e-6) < 1e-1, (w, float(n_ref))  # the clip engages
        got_n = float(opt.last_grad_norm)
        assert abs(got_n - float(n_ref)) <= 1e-5 * float(n_ref), (w, got_n, float(n_ref))
        params = [p for g in opt.param_groups for p in g["params"]]
        for i, (p, r) in enumerate(zip(params, p_ref)):
            assert rel_l2(p.detach(), r.detach()) < 1e-6, (w, i)
            if r.grad is not None:
                # (the two norms - fp32 sums over table chunks here, per-tensor norms in torch - differ in the last
                # bits, and so do the coefficients: the clipped gradients carry that difference)
                assert rel_l2(p.grad, r.grad) < 3e-6, (w, i)
    assert norms[0]["G"] is not None and norms[0]["D"] is None and norms[1]["D"] is not None
    assert norms[2]["D"] == norms[1]["D"]  # a G iteration leaves D's norm alone


def test_gan_without_section_is_the_plain_step(hip):
    """no section: no clipping, no norms; the same model measuring its norms only (coefficient pinned to 1) takes the
    same steps bit for bit"""
    plain, cfg = _build_gan(clip=False)
    assert plain.optimizer_G.max_grad_norm is None and not plain.optimizer_G.track_grad_norm
    n_plain = _iterations(plain, cfg)
    assert all(v is None for n in n_plain for v in n.values())
    track, cfg2 = _build_gan(clip=False, track=True)
    n_track = _iterations(track, cfg2)
    assert n_track[-1]["G"] > 0 and n_track[-1]["D"] > 0
    for a, b in ((plain.G, track.G), (plain.D, track.D)):
        for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(u, v), k


# ---------------------------------------------------------------------------------------------------- run.py --train
def test_run_train_with_grad_clip(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    cls = gmod.wind_field_GAN_3D
    orig_opt = cls.optimize_parameters
    runs = {}
    section = ("\n[GRAD_CLIP]\nclip_generator = True\nclip_discriminator = True\nmax_norm_discriminator = 0.01\n"
               "log_grad_norms = True\n")
    for tag, extra in (("plain", ""), ("clip", section)):
        ini = str(tmp_path / f"{tag}.ini")
        cfg = _write_ini(ini)
        cfg.name = f"e2e_{tag}"
        cfg.generator.max_norm = 0.01
        with open(ini, "w") as f:
            f.write(cfg.asINI() + extra)
        norms = []

        def rec_opt(self, LR, HR, Z, it, norms=norms):
            orig_opt(self, LR, HR, Z, it)
            norms.append({k: None if v is None else float(v) for k, v in self.get_grad_norms().items()})

        monkeypatch.setattr(cls, "optimize_parameters", rec_opt)
        runmod.main(["--train", "--cfg", ini])
        G = torch.load(os.path.join(str(tmp_path), "runs", cfg.name, "G_6.pth"), map_location="cpu")
        with open(os.path.join(str(tmp_path), "runs", cfg.name, "config.ini")) as f:
            snapshot = f.read()
        runs[tag] = (norms, G, snapshot)
    (n_plain, G_plain, s_plain), (n_clip, G_clip, s_clip) = runs["plain"], runs["clip"]
    assert all(v is None for n in n_plain for v in n.values()) and "GRAD_CLIP" not in s_plain
    assert "[GRAD_CLIP]\nclip_generator = True\n" in s_clip
    last = n_clip[-1]
    for k in ("G", "D"):
        assert last[k] is not None and math.isfinite(last[k]) and last[k] > 0, (k, last)
    assert any(not torch.equal(G_plain[k], G_clip[k]) for k in G_plain)


# ---------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from gan_sr_wind_field_amd import dist as wdist

    torch.cuda.set_device(0)
    assert wdist.init_from_env("gloo")
    gan, cfg = _build_gan(clip=True)
    wdist.attach(gan, bucket_mb=0.02, sync_bn=True)
    torch.save(_dp_iterations(gan, cfg, slice(2 * rank, 2 * rank + 2)), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _dp_iterations(gan, cfg, sl):
    from oracle.gan import synthetic_batch

    LR, HR, Z, x, y = synthetic_batch(4, 16, 4, 4, seed=2001)
    dev = cfg.device
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    out = {}
    gan.optimize_parameters(LR[sl].to(dev), HR[sl].to(dev), Z[sl].to(dev), 0)  # G-iteration
    out["normG"] = gan.get_grad_norms()["G"].cpu()
    out.update({"gradG." + k: p.grad.detach().cpu().clone() for k, p in gan.G.named_parameters() if p.grad is not None})
    gan.optimize_parameters(LR[sl].to(dev), HR[sl].to(dev), Z[sl].to(dev), 1)  # D-iteration, classifier head included
    out["normD"] = gan.get_grad_norms()["D"].cpu()
    out.update({"gradD." + k: p.grad.detach().cpu().clone() for k, p in gan.D.named_parameters() if p.grad is not None})
    out.update({"G." + k: v.detach().cpu().clone() for k, v in gan.G.state_dict().items()})
    out.update({"D." + k: v.detach().cpu().clone() for k, v in gan.D.state_dict().items()})
    return out


def test_two_rank_clipped_step_equals_full_batch_hip(hip, tmp_path):
    """two ranks on cuda:0 over gloo, clipping on for G and D: the replicas stay bit-identical (the norm is taken from
    the averaged gradients, bucketed and per-parameter) and equal the clipped full-batch step"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    world, port = 2, _free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    gan, cfg = _build_gan(clip=True)
    ref = _dp_iterations(gan, cfg, slice(0, 4))
    assert float(ref["normG"]) > 0.1 and float(ref["normD"]) > 0.1  # bound 1e-2: both clip
    for k, v in ref.items():
        assert torch.equal(r0[k], r1[k]), k
    np.testing.assert_allclose(float(r0["normG"]), float(ref["normG"]), rtol=1e-4)
    np.testing.assert_allclose(float(r0["normD"]), float(ref["normD"]), rtol=2.5e-2)
    gG = torch.cat([r0[k].reshape(-1) for k in ref if k.startswith("gradG.")])
    gG_ref = torch.cat([ref[k].reshape(-1) for k in ref if k.startswith("gradG.")])
    assert rel_l2(gG, gG_ref) < 1e-4 and abs(float(gG.double().norm()) - 1e-2) < 1e-7
    gD = torch.cat([r0[k].reshape(-1) for k in ref if k.startswith("gradD.")])
    gD_ref = torch.cat([ref[k].reshape(-1) for k in ref if k.startswith("gradD.")])
    # (the discriminator iteration's input comes from weights that already took one sign(g) step: the bound of the
    # other two-rank D tests)
    assert rel_l2(gD, gD_ref) < 2.5e-2 and abs(float(gD.double().norm()) - 1e-2) < 1e-7
    for k in ref:
        if k.startswith("G."):
            a, b = r0[k].numpy(), ref[k].numpy()
            bad = np.abs(a - b) > 2e-6 + 5e-4 * np.abs(b)
            assert bad.mean() <= 0.02, (k, float(bad.mean()))
