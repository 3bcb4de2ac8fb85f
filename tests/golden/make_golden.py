"""Generate the golden fixtures by running the REAL reference on the CPU.

Runs only in the build container (``/root/reference`` is not shipped to the GPU
box):  ``python tests/golden/make_golden.py``  ->  ``tests/golden/*.npz``.

Only data (inputs, expected outputs, seeds) is written; no reference source is
copied.  Weights come from ``oracle.nets.deterministic_state`` and are loaded
into the reference modules with ``load_state_dict`` so fixtures stay small.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(1, REF)
sys.path.insert(2, HERE)

# netCDF4 is only used by the reference's download code (download_data.py:14-15)
_nc = types.ModuleType("netCDF4")
_nc.Dataset = object
_nc.MFDataset = object
sys.modules.setdefault("netCDF4", _nc)

from oracle import nets as onets  # noqa: E402
from oracle.gan import synthetic_batch  # noqa: E402

from CNN_models import torch_blocks as ref_blocks  # noqa: E402
from CNN_models.Discriminator_3D import Discriminator_3D as RefD  # noqa: E402
from CNN_models.Generator_3D_Resnet_ESRGAN import Generator_3D as RefG  # noqa: E402
from GAN_models import wind_field_GAN_3D as ref_gan  # noqa: E402
from config.config import Config as RefConfig  # noqa: E402
import process_data as ref_pd  # noqa: E402
import tools.trainingtricks as ref_tricks  # noqa: E402

torch.set_num_threads(8)


def np_(t):
    return t.detach().cpu().numpy()


#: largest committed file: a fixture above it is written as byte pieces NAME.000, NAME.001, ... (conftest's
#: ``golden`` joins them again)
PIECE_BYTES = 1_000_000


def save(name, **arrays):
    import glob
    import io

    path = os.path.join(HERE, name)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    data = buf.getvalue()
    for old in glob.glob(glob.escape(path)) + glob.glob(glob.escape(path) + ".[0-9][0-9][0-9]"):
        os.remove(old)
    if len(data) <= PIECE_BYTES:
        with open(path, "wb") as f:
            f.write(data)
    else:
        for i in range(0, len(data), PIECE_BYTES):
            with open(f"{path}.{i // PIECE_BYTES:03d}", "wb") as f:
                f.write(data[i:i + PIECE_BYTES])
    print(f"wrote {name}: {len(data) / 1024:.1f} KiB")


# --------------------------------------------------------------------------- #
# 1. per-op conv cases (every (k, stride, pad, bias, act) combination on the path)
# --------------------------------------------------------------------------- #
from cases import CONV_CASES  # noqa: E402


def gen_conv_cases():
    out = {}
    for idx, (name, cin, cout, k, s, p, bias, act, xyz, B) in enumerate(CONV_CASES):
        g = torch.Generator().manual_seed(1000 + idx)
        if bias:
            m = torch.nn.Conv3d(cin, cout, k, s, p)
            layers = [m] + ([torch.nn.LeakyReLU(0.2)] if act else [])
            mod = torch.nn.Sequential(*layers)
        else:
            mod = ref_blocks.create_conv_lrelu_layer(cin, cout, k, stride=s, padding=p, lrelu=act)
            m = mod[0]
        with torch.no_grad():
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5)
            if bias:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        x = torch.randn((B, cin) + xyz, generator=g, requires_grad=True)
        y = mod(x)
        gy = torch.randn(y.shape, generator=g)
        (y * gy).sum().backward()
        out[f"{name}.x"] = np_(x)
        out[f"{name}.w"] = np_(m.weight)
        if bias:
            out[f"{name}.b"] = np_(m.bias)
            out[f"{name}.db"] = np_(m.bias.grad)
        out[f"{name}.y"] = np_(y)
        out[f"{name}.gy"] = np_(gy)
        out[f"{name}.dx"] = np_(x.grad)
        out[f"{name}.dw"] = np_(m.weight.grad)
    save("conv_cases.npz", **out)


# --------------------------------------------------------------------------- #
# 2. blocks: RDB, RRDB, UpConv, discriminator block (reference helpers)
# --------------------------------------------------------------------------- #
def gen_blocks():
    out = {}
    g = torch.Generator().manual_seed(77)
    rrdb = ref_blocks.RRDB(16, 8, 5, lff_kern_size=1, mode="3D")
    with torch.no_grad():
        for p in rrdb.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.05))
    x = torch.randn((2, 16, 5, 4, 6), generator=g, requires_grad=True)
    y = rrdb(x)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    out["rrdb.x"], out["rrdb.y"], out["rrdb.gy"], out["rrdb.dx"] = np_(x), np_(y), np_(gy), np_(x.grad)
    for k, v in rrdb.state_dict().items():
        out[f"rrdb.sd.{k}"] = np_(v)
    for k, v in rrdb.named_parameters():
        out[f"rrdb.grad.{k}"] = np_(v.grad)

    up = ref_blocks.create_UpConv_block(8, 8, scale=2, mode="3D")
    with torch.no_grad():
        up[1][0].weight.copy_(torch.randn(up[1][0].weight.shape, generator=g) * 0.1)
    x = torch.randn((2, 8, 3, 4, 5), generator=g, requires_grad=True)
    y = up(x)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    out["up.x"], out["up.w"], out["up.y"], out["up.gy"] = np_(x), np_(up[1][0].weight), np_(y), np_(gy)
    out["up.dx"], out["up.dw"] = np_(x.grad), np_(up[1][0].weight.grad)
    save("blocks.npz", **out)


# --------------------------------------------------------------------------- #
# 3. reduced-size Generator / Discriminator (outputs + all parameter grads)
# --------------------------------------------------------------------------- #
G_SMALL = dict(in_channels=4, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8)


def build_ref_G(spec: onets.GSpec):
    G = RefG(spec.in_channels, spec.out_channels, spec.nf, spec.n_rrdb, upscale=spec.upscale,
             hr_kern_size=spec.hr_kern, number_of_RDB_convs=spec.n_rdb_convs, RDB_gc=spec.gc,
             lff_kern_size=spec.lff_kern, RDB_residual_scaling=spec.rdb_scale,
             RRDB_residual_scaling=spec.rrdb_scale, terrain_number_of_features=spec.tf,
             dropout_probability=spec.dropout_p)
    return G


def build_ref_D(spec: onets.DSpec):
    return RefD(spec.in_channels, spec.bf, feat_kern_size=spec.feat_kern, number_of_z_layers=spec.nz,
                enable_slicing=spec.enable_slicing, dropout_probability=spec.dropout_p, normalization_type=spec.norm)


def gen_generators(cases=((4, 6, 5), (8, 4, 4)), in_ch=4):
    """``in_ch``: 3 + include_pressure + include_z_channel + include_above_ground_channel (wind_field_GAN_3D.py:93-96)"""
    for scale, n, nz in cases:
        spec = onets.GSpec(upscale=scale, **dict(G_SMALL, in_channels=in_ch))
        G = build_ref_G(spec)
        shapes = onets.g_param_shapes(spec)
        ref_shapes = {k: tuple(v.shape) for k, v in G.state_dict().items()}
        assert list(ref_shapes.items()) == list(shapes.items()), "G key/shape manifest mismatch"
        sd = onets.deterministic_state(shapes, seed=11 + scale, scale=0.7)
        G.load_state_dict(sd)
        G.eval()
        LR, HR, Z, x, y = synthetic_batch(2, n, nz, scale, seed=5 + scale, in_ch=in_ch)
        assert LR.shape[1] == in_ch
        out = G(LR, Z)
        g = torch.Generator().manual_seed(99)
        gy = torch.randn(out.shape, generator=g)
        (out * gy).sum().backward()
        arrays = {"out": np_(out), "gy": np_(gy)}
        for k, p in G.named_parameters():
            arrays[f"grad.{k}"] = np_(p.grad)
        save(f"g_small_s{scale}.npz" if in_ch == 4 else f"g_small_s{scale}_c{in_ch}.npz", **arrays)


def gen_discriminators(cases=((True, 64, 4, "batch"), (False, 128, 3, "batch"), (False, 128, 21, "batch"))):
    for slicing, xy, nz, norm in cases:
        spec = onets.DSpec(bf=4, nz=nz, enable_slicing=slicing, norm=norm)
        D = build_ref_D(spec)
        shapes = onets.d_param_shapes(spec)
        ref_shapes = {k: tuple(v.shape) for k, v in D.state_dict().items()}
        assert list(ref_shapes.items()) == list(shapes.items()), "D key/shape manifest mismatch"
        sd = onets.deterministic_state(shapes, seed=31 + nz, scale=1.0)
        D.load_state_dict(sd)
        g = torch.Generator().manual_seed(7)
        x = torch.rand((2, 3, xy, xy, nz), generator=g) * 2 - 1
        x.requires_grad_(True)
        arrays = {"x_seed": np.array(7)}  # x = rand(generator seed 7) * 2 - 1, regenerated by the tests
        D.eval()
        arrays["out_eval"] = np_(D(x))
        D.train()
        out = D(x)
        gy = torch.tensor([[1.0], [-0.5]])
        (out * gy).sum().backward()
        arrays["out_train"] = np_(out)
        arrays["dx_sub"] = np_(x.grad[:, :, ::4, ::4, :])
        arrays["dx_abs_sum"] = np.array(float(x.grad.double().abs().sum()))
        for k, p in D.named_parameters():
            arrays[f"grad.{k}"] = np_(p.grad)
        for k, v in D.state_dict().items():
            if "running_" in k or "num_batches" in k:
                arrays[f"after.{k}"] = np_(v)
        tag = ("slice" if slicing else "full") + f"_z{nz}" + ("" if norm == "batch" else f"_{norm}")
        save(f"d_small_{tag}.npz", **arrays)


# --------------------------------------------------------------------------- #
# 4. physics operators / metrics / tricks
# --------------------------------------------------------------------------- #
def gen_physics():
    LR, HR, Z, x, y = synthetic_batch(2, 5, 6, 4, seed=3)
    g = torch.Generator().manual_seed(17)
    SR = HR + 0.1 * torch.randn(HR.shape, generator=g)
    x = x + torch.rand(x.shape, generator=g) * 30.0  # exercise the non-uniform branch too
    grad_hr = ref_pd.calculate_gradient_of_wind_field(HR[:, :3], x, y, Z)
    grad_sr = ref_pd.calculate_gradient_of_wind_field(SR[:, :3], x, y, Z)
    norms = ref_gan.get_norm_factors_of_gradients(grad_hr, grad_sr)
    psnr = ref_gan.calculate_PSNR(HR, SR)
    psnr_sr, psnr_tri = ref_gan.compute_PSNR_for_SR_and_trilinear(
        LR, HR, SR, torch.tensor(4.0), torch.tensor(1e-8), interpolate=True, scale=4)
    torch.manual_seed(123)
    noise = ref_tricks.instance_noise(torch.tensor(2.0), HR.shape, torch.tensor(7), torch.tensor(100))
    torch.manual_seed(124)
    labels = ref_tricks.noisy_labels(True, 6, true_label_val=torch.tensor(0.93), false_label_val=torch.tensor(0.0))
    save("physics.npz", HR=np_(HR), SR=np_(SR), LR=np_(LR), Z=np_(Z), x=np_(x), y=np_(y),
         grad_hr=np_(grad_hr), grad_sr=np_(grad_sr), norms=np.array([float(v) for v in norms]),
         psnr=np.array(float(psnr)), psnr_sr=np.array(float(psnr_sr)), psnr_tri=np.array(float(psnr_tri)),
         noise=np_(noise), labels=np_(labels))


# --------------------------------------------------------------------------- #
# 5. train-step traces from the real wind_field_GAN_3D
# --------------------------------------------------------------------------- #
def reduced_cfg(use_noise: bool, dropout: float, period: int = 2, tf: int = 4, bf: int = 4):
    cfg = RefConfig(os.path.join(REF, "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id = None
    cfg.device = torch.device("cpu")
    cfg.generator.num_features = 16
    cfg.generator.num_RRDB = 1
    cfg.generator.RDB_growth_chan = 8
    cfg.generator.terrain_number_of_features = tf
    cfg.generator.dropout_probability = dropout
    cfg.discriminator.num_features = bf
    cfg.discriminator.dropout_probability = dropout
    cfg.gan_config.number_of_z_layers = 4
    cfg.training.use_instance_noise = use_noise
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = period
    return cfg


def specs_from_cfg(cfg):
    gs = onets.GSpec(in_channels=4, nf=cfg.generator.num_features, n_rrdb=cfg.generator.num_RRDB,
                     gc=cfg.generator.RDB_growth_chan, tf=cfg.generator.terrain_number_of_features,
                     hr_kern=cfg.generator.hr_kern_size, upscale=cfg.scale,
                     dropout_p=cfg.generator.dropout_probability)
    ds = onets.DSpec(bf=cfg.discriminator.num_features, nz=cfg.gan_config.number_of_z_layers,
                     enable_slicing=cfg.gan_config.enable_slicing,
                     dropout_p=cfg.discriminator.dropout_probability)
    return gs, ds


def gen_trace(tag: str, use_noise: bool, dropout: float, its, tf: int = 4, bf: int = 4):
    cfg = reduced_cfg(use_noise, dropout, tf=tf, bf=bf)
    torch.manual_seed(2001)
    gan = ref_gan.wind_field_GAN_3D(cfg)
    gs, ds = specs_from_cfg(cfg)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter), cfg.training.d_g_train_ratio,
                      cfg.training.d_g_train_period)
    torch.manual_seed(4242)  # RNG state at the first optimize_parameters call
    keys = ["total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"]
    rows, kinds, dloss, wsum_g, wsum_d, lrs = [], [], [], [], [], []
    for it in its:
        gan.optimize_parameters(LR, HR, Z, it)
        if it > 2 * cfg.training.d_g_train_period:
            gan.update_learning_rate()
        is_g = (it // cfg.training.d_g_train_period) % (cfg.training.d_g_train_ratio + 1) == 0
        kinds.append(1 if is_g else 0)
        rows.append([float(gan.get_G_train_loss_dict_ref()[k]) for k in keys])
        dloss.append(float(gan.get_D_loss_dict_ref()["train_loss"]))
        wsum_g.append([float(gan.G.state_dict()[k].double().abs().sum())
                       for k in ("model.0.0.weight", "hr_convs.2.weight", "model.1.module.0.RDBs.1.LFF.bias")])
        wsum_d.append([float(gan.D.state_dict()[k].double().abs().sum())
                       for k in ("features.0.0.0.weight", "classifier.2.weight", "features.1.1.1.running_var")])
        lrs.append(gan.optimizer_G.param_groups[0]["lr"])
    final_G = {f"final_G.{k}": np_(v) for k, v in gan.G.state_dict().items()
               if k in ("model.0.0.weight", "hr_convs.2.weight", "hr_convs.2.bias")}
    final_D = {f"final_D.{k}": np_(v) for k, v in gan.D.state_dict().items()
               if k in ("features.0.0.0.weight", "classifier.2.weight", "features.4.1.running_mean")}
    save(f"gan_trace_{tag}.npz", its=np.array(list(its)), kinds=np.array(kinds), G_losses=np.array(rows),
         D_loss=np.array(dloss), wsum_g=np.array(wsum_g), wsum_d=np.array(wsum_d), lr=np.array(lrs),
         use_noise=np.array(use_noise), dropout=np.array(dropout), **final_G, **final_D)


def gen_c1_full():
    """The SHIPPED local configuration at full width (34.77 M-parameter G, bf 32 D with slicing, LR 16x16x10 ->
    HR 64x64x10, batch 1 - BASELINE.json configs[0]): one G-iteration and one D-iteration of the reference's
    ``wind_field_GAN_3D`` with dropout and instance noise off.  Recorded: the eval-mode SR field (sub-sampled),
    D's eval logit on HR, the 8 generator loss entries, the discriminator loss, L2 norms and abs-sums of EVERY
    parameter gradient of both iterations and a few whole gradient tensors."""
    cfg = RefConfig(os.path.join(REF, "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id = None
    cfg.device = torch.device("cpu")
    cfg.generator.dropout_probability = 0.0
    cfg.discriminator.dropout_probability = 0.0
    cfg.training.use_instance_noise = False
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = 1
    torch.manual_seed(2001)
    gan = ref_gan.wind_field_GAN_3D(cfg)
    gs, ds = specs_from_cfg(cfg)
    assert (gs.nf, gs.n_rrdb, gs.gc, gs.tf, ds.bf, ds.enable_slicing) == (128, 16, 32, 16, 32, True)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=101, scale=0.3))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=103, scale=1.0))
    LR, HR, Z, x, y = synthetic_batch(1, 16, 10, 4, seed=2001)
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter), 1, 1)
    gan.G.eval()
    gan.D.eval()
    with torch.no_grad():
        sr = gan.G(LR, Z)
        d_hr = gan.D(HR)
    keys = ["total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"]
    out = {"sr_sub": np_(sr[:, :, ::2, ::2, :]), "sr_abs_sum": np.array(float(sr.double().abs().sum())),
           "d_hr_eval": np_(d_hr)}
    gan.optimize_parameters(LR, HR, Z, 0)  # G-iteration
    out["G_losses"] = np.array([float(gan.get_G_train_loss_dict_ref()[k]) for k in keys])
    gG = {k: p.grad for k, p in gan.G.named_parameters()}
    out["gG_keys"] = np.array(list(gG))
    out["gG_l2"] = np.array([float(v.double().norm()) for v in gG.values()])
    out["gG_abs"] = np.array([float(v.double().abs().sum()) for v in gG.values()])
    for k in ("model.0.0.weight", "model.1.module.0.RDBs.0.LFF.bias", "model.1.module.15.RDBs.2.LFF.bias",
              "terrain_convs.0.0.weight", "hr_convs.2.bias"):
        out["gG." + k] = np_(gG[k])
    out["gG8.model.1.module.7.RDBs.1.conv3.conv.0.weight"] = np_(gG["model.1.module.7.RDBs.1.conv3.conv.0.weight"][:8])
    gan.optimize_parameters(LR, HR, Z, 1)  # D-iteration
    out["D_loss"] = np.array(float(gan.get_D_loss_dict_ref()["train_loss"]))
    gD = {k: p.grad for k, p in gan.D.named_parameters()}
    out["gD_keys"] = np.array(list(gD))
    out["gD_l2"] = np.array([float(v.double().norm()) for v in gD.values()])
    out["gD_abs"] = np.array([float(v.double().abs().sum()) for v in gD.values()])
    for k in ("features.0.0.0.weight", "features.4.1.weight", "classifier.2.weight", "features.2.0.1.bias"):
        out["gD." + k] = np_(gD[k])
    # conditioning yard-stick for the fp32 tolerances: distance of the reference's fp32 generator gradients from
    # an fp64 evaluation of the same G-iteration (the oracle in double; 48 dense blocks deep, so the first layers
    # accumulate a few 1e-4 of rounding)
    from c1_case import c1_oracle_step
    r64 = c1_oracle_step(torch.float64)
    out["gG_floor"] = np.array([float((gG[k].double() - r64["gG"][k]).norm() / r64["gG"][k].norm()) for k in gG])
    out["G_losses_fp64"] = np.array(r64["G_losses"])
    save("c1_full_step.npz", **out)


def gen_data():
    """Dataset contract: the REFERENCE's process_data / download_data functions run on a small
    synthetic HARMONIE-SIMRA-format dataset (written by the product's deterministic writer, seed 2001) in a
    scratch directory: normalisation factors and the chronological split of ``preprosess``, ``reformat_to_torch``
    for the channel-flag combinations, z-interpolation and its inverse, beta-distributed slice sampling and the
    rot90 / flip augmentation with the u, v sign rules (``CustomizedDataset.__getitem__`` under seeded numpy RNG)."""
    import tempfile
    from datetime import date

    import download_data as ref_dl
    from gan_sr_wind_field_amd import process_data as pd_

    XD, ZD = {"start": 0, "max": 32, "step": 1}, {"start": 0, "max": 6, "step": 1}
    d0, d1 = date(2018, 3, 1), date(2018, 3, 2)
    out = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("./data/downloaded_raw_bessaker_data", exist_ok=True)
            pd_.write_synthetic_dataset(d0, d1, XD, XD, ZD, seed=2001)
            for tag, kw in (("slice_aug", dict(include_pressure=False, include_z_channel=True, interpolate_z=False,
                                                enable_slicing=True, slice_size=16, train_aug_rot=True,
                                                train_aug_flip=True)),
                            ("interp", dict(include_pressure=True, include_z_channel=True, interpolate_z=True,
                                            include_above_ground_channel=True, enable_slicing=False))):
                tr, te, va, x, y = ref_pd.preprosess(X_DICT=XD, Y_DICT=XD, Z_DICT=ZD, start_date=d0, end_date=d1,
                                                     COARSENESS_FACTOR=4, **kw)
                out[f"{tag}.n"] = np.array([len(tr), len(te), len(va)])
                out[f"{tag}.first_names"] = np.array([tr.filenames[0], te.filenames[0], va.filenames[0]])
                out[f"{tag}.norms"] = np.array([tr.Z_MIN, tr.Z_MAX, tr.Z_ABOVE_GROUND_MAX, tr.UVW_MAX, tr.P_MIN, tr.P_MAX])
                out[f"{tag}.x"], out[f"{tag}.y"] = np_(x), np_(y)
                np.random.seed(77)
                for i in range(6 if tag == "slice_aug" else 2):  # 6 draws: every rotation count and flip state occurs
                    LR, HR, Z = tr[i]
                    out[f"{tag}.train{i}.LR"], out[f"{tag}.train{i}.HR"], out[f"{tag}.train{i}.Z"] = np_(LR), np_(HR), np_(Z)
                item = te[0]
                out[f"{tag}.test0.LR"], out[f"{tag}.test0.HR"], out[f"{tag}.test0.Z"] = (np_(t) for t in item[:3])
                out[f"{tag}.test0.name"] = np.array(item[3])
                if tag == "interp":
                    out["interp.test0.HR_raw"], out["interp.test0.Z_raw"] = np_(item[4]), np_(item[5])
                    # inverse of the z-interpolation applied to the interpolated HR field
                    out["interp.test0.HR_back"] = np_(ref_dl.reverse_interpolate_z_axis(
                        item[1].numpy()[None], item[5].numpy()[None], item[2].numpy()[None]))
                LR, HR, Z = va[1]
                out[f"{tag}.val1.LR"] = np_(LR)
        finally:
            os.chdir(cwd)
    save("dataset_contract.npz", **out)


def gen_init_manifest():
    """Seeded-init checksums of the full-size nets (RNG-order parity of init_weights)."""
    cfg = RefConfig(os.path.join(REF, "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id = None
    cfg.device = torch.device("cpu")
    torch.manual_seed(2001)
    gan = ref_gan.wind_field_GAN_3D(cfg)
    arrays = {}
    for net, tag in ((gan.G, "G"), (gan.D, "D")):
        sd = net.state_dict()
        arrays[f"{tag}.keys"] = np.array(list(sd.keys()))
        arrays[f"{tag}.shapes"] = np.array([str(tuple(v.shape)) for v in sd.values()])
        arrays[f"{tag}.abs_sum"] = np.array([float(v.double().abs().sum()) for v in sd.values()])
        arrays[f"{tag}.first"] = np.array([float(v.reshape(-1)[0]) if v.numel() else 0.0 for v in sd.values()])
    arrays["G.n_params"] = np.array(sum(p.numel() for p in gan.G.parameters()))
    arrays["D.n_params"] = np.array(sum(p.numel() for p in gan.D.parameters()))
    arrays["str_cfg_head"] = np.array(str(cfg)[:4000])
    save("init_manifest.npz", **arrays)


def gen_config_golden():
    """Parsed values + INI round trip of the reference Config on its shipped local ini."""
    import json
    cfg = RefConfig(os.path.join(REF, "config", "wind_field_GAN_3D_config_local.ini"))
    sections = {"DEFAULT": {k: v for k, v in vars(cfg).items()}}
    for name in ("env", "gan_config", "generator", "discriminator", "training", "dataset_train", "dataset_val",
                 "dataset_test"):
        sections[name] = dict(vars(getattr(cfg, name)))
    with open(os.path.join(HERE, "config_golden.json"), "w") as f:
        json.dump({"sections": sections, "asINI": cfg.asINI()}, f, indent=1, default=str)
    print("wrote config_golden.json")


if __name__ == "__main__":
    which = sys.argv[1:] or ["conv", "blocks", "G", "D", "physics", "trace", "init", "config", "c1", "data", "Dinst", "G16", "Gch"]
    if "config" in which:
        gen_config_golden()
    if "conv" in which:
        gen_conv_cases()
    if "blocks" in which:
        gen_blocks()
    if "G" in which:
        gen_generators()
    if "G16" in which:  # scale = 16 (pretrained_models/upscale16_pix4_no_adv_no_slicing/config.ini:5): four UpConv stages
        # (LR 3 x 3 x 5; NOT 3 x 3 x 4: at that size and these seeds one LeakyReLU input of the trunk sits within fp32
        # rounding of zero - the reference's fp32 gradients, an fp64 evaluation and the HIP path then differ pairwise by
        # 2e-3 on everything below it, a property of the input, found in round 5)
        gen_generators(((16, 3, 5),))
    if "Gch" in which:  # generator input widths 3 / 5 / 6: every other combination of the three channel switches
        for c in (3, 5, 6):
            gen_generators(((4, 6, 5),), in_ch=c)
    if "D" in which:
        gen_discriminators()
    if "Dinst" in which:  # normalization_type = "instance" (torch_blocks.py:26-30), both slicing modes (the tail stays "batch")
        gen_discriminators(((False, 128, 3, "instance"), (True, 64, 4, "instance")))
    if "physics" in which:
        gen_physics()
    if "trace" in which:
        gen_trace("plain", use_noise=False, dropout=0.0, its=[1, 2, 3, 4, 5, 6])
        gen_trace("noise", use_noise=True, dropout=0.1, its=[1, 2, 3, 4, 5])
        # channel widths the bf16 kernels accept (terrain features / D base width multiples of 8)
        gen_trace("plain_w8", use_noise=False, dropout=0.0, its=[1, 2, 3, 4, 5, 6], tf=8, bf=8)
    if "c1" in which:
        gen_c1_full()
    if "data" in which:
        gen_data()
    if "init" in which:
        gen_init_manifest()
