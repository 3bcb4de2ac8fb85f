"""GPU parity of the fused HIP programs (Generator_3D, Discriminator_3D, the GAN
train step) against fixtures recorded from the reference and against the oracle.

Tolerances (rel-L2): fp32 outputs 2e-5, fp32 gradients 2e-4 (reference noise floor
fp32-vs-fp64 is 1.2e-6); bf16 outputs 2e-2; bf16 gradients per tensor
2e-2 + twice the distance of the oracle's bf16-storage emulation from fp32 on that
tensor (``_emulated_bf16_bounds``; full-size cases: test_hip_fullsize_parity.py).
"""
import numpy as np
import pytest
import torch

from conftest import reload_wsr_env, rel_l2
from oracle import gan as ogan
from oracle import nets as onets

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"


def build_G(spec, dtype, seed, scale=0.7):
    from gan_sr_wind_field_amd.CNN_models.Generator_3D_Resnet_ESRGAN import Generator_3D

    G = Generator_3D(spec.in_channels, spec.out_channels, spec.nf, spec.n_rrdb, upscale=spec.upscale,
                     hr_kern_size=spec.hr_kern, RDB_gc=spec.gc, terrain_number_of_features=spec.tf,
                     dropout_probability=spec.dropout_p, use_mixed_precision=dtype == torch.bfloat16)
    sd = onets.deterministic_state(onets.g_param_shapes(spec), seed=seed, scale=scale)
    G.load_state_dict(sd)
    return G.to(DEV), sd


def build_D(spec, dtype, seed):
    from gan_sr_wind_field_amd.CNN_models.Discriminator_3D import Discriminator_3D

    D = Discriminator_3D(spec.in_channels, spec.bf, feat_kern_size=spec.feat_kern, number_of_z_layers=spec.nz,
                         enable_slicing=spec.enable_slicing, dropout_probability=spec.dropout_p,
                         use_mixed_precision=dtype == torch.bfloat16, normalization_type=spec.norm)
    sd = onets.deterministic_state(onets.d_param_shapes(spec), seed=seed, scale=1.0)
    D.load_state_dict(sd)
    return D.to(DEV), sd


@pytest.mark.parametrize("scale,n,nz", [(4, 6, 5), (8, 4, 4), (16, 3, 5)])  # x16: reference pretrained_models/upscale16_*/config.ini:5
def test_generator_fp32_vs_reference(golden, hip, scale, n, nz):
    g = golden(f"g_small_s{scale}.npz")
    spec = onets.GSpec(upscale=scale, in_channels=4, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8)
    G, _ = build_G(spec, torch.float32, 11 + scale)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, n, nz, scale, seed=5 + scale)
    out = G(LR.to(DEV), Z.to(DEV))
    assert out.shape == (2, 3, scale * n, scale * n, nz) and out.dtype == torch.float32
    assert rel_l2(out, T(g["out"])) < 2e-5
    (out * T(g["gy"]).to(DEV)).sum().backward()
    worst = max(rel_l2(p.grad, T(g[f"grad.{k}"])) for k, p in G.named_parameters())
    for k, p in G.named_parameters():
        assert rel_l2(p.grad, T(g[f"grad.{k}"])) < 2e-4, (k, worst)
    # no-grad forward saves nothing and gives the same numbers
    with torch.no_grad():
        out2 = G(LR.to(DEV), Z.to(DEV))
    assert torch.equal(out2, out.detach())


def _emulated_bf16_bounds(truth: dict, emul: dict, floor: float = 2e-2, pooled: bool = False):
    """per-tensor bf16 tolerance: floor + twice the distance the oracle's bf16-storage emulation
    (``GSpec.bf16_storage``) shows from the fp32 truth on that tensor.  ``pooled`` (the discriminator): a
    tensor's own emulated distance is ONE draw of a heavy-tailed quantity there - a single LeakyReLU branch flip
    among the 100 hidden units of the classifier, or in a BatchNorm population of 64, moves every gradient
    upstream of it by ~10 % (measured: forward activations of the HIP path and of the emulation agree to three
    digits layer by layer, tools/tuning/diag_d_bf16.py, while the flips fall on different units) - so the
    distance used is at least the network's median one."""
    d = {k: rel_l2(emul[k], truth[k]) for k in truth}
    med = float(np.median(list(d.values()))) if pooled else 0.0
    return {k: floor + 2.0 * max(v, med) for k, v in d.items()}


def test_generator_bf16_vs_reference(golden, hip):
    g = golden("g_small_s4.npz")
    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8)
    G, _ = build_G(spec, torch.bfloat16, 15)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 6, 5, 4, seed=9)
    out = G(LR.to(DEV), Z.to(DEV))
    assert out.dtype == torch.float32
    assert rel_l2(out, T(g["out"])) < 2e-2
    (out * T(g["gy"]).to(DEV)).sum().backward()
    # bound per parameter tensor: what a bf16-storage evaluation of the reference's graph shows on it
    sd = onets.deterministic_state(onets.g_param_shapes(spec), seed=15, scale=0.7)
    for v in sd.values():
        v.requires_grad_(True)
    em = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8,
                     bf16_storage=True)
    (onets.generator_forward(sd, LR, Z, em) * T(g["gy"])).sum().backward()
    truth = {k: T(g[f"grad.{k}"]) for k in sd}
    lim = _emulated_bf16_bounds(truth, {k: v.grad for k, v in sd.items()})
    errs = {k: rel_l2(p.grad, truth[k]) for k, p in G.named_parameters()}
    bad = {k: (v, lim[k]) for k, v in errs.items() if not v < lim[k]}
    assert not bad, bad


@pytest.mark.parametrize("in_ch", [3, 5, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_generator_input_widths_vs_reference(golden, hip, in_ch, dtype):
    """Generator input widths other than 4: in_channels = 3 + include_pressure + include_z_channel +
    include_above_ground_channel (reference wind_field_GAN_3D.py:93-96).  The feature conv's channel pieces are 4
    (fp32) / 8 (bf16) wide, so 3 / 5 / 6 run the piece padding of the forward AND of its filter gradient that 4 does
    not.  Fixtures ``g_small_s4_c{3,5,6}.npz`` come from the imported reference (make_golden.py ``Gch``)."""
    g = golden(f"g_small_s4_c{in_ch}.npz")
    spec = onets.GSpec(upscale=4, in_channels=in_ch, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8)
    G, _ = build_G(spec, dtype, 15)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 6, 5, 4, seed=9, in_ch=in_ch)
    assert LR.shape[1] == in_ch and G.state_dict()["model.0.0.weight"].shape[1] == in_ch
    out = G(LR.to(DEV), Z.to(DEV))
    assert out.shape == (2, 3, 24, 24, 5) and out.dtype == torch.float32
    truth = {k: T(g[f"grad.{k}"]) for k, _ in G.named_parameters()}
    (out * T(g["gy"]).to(DEV)).sum().backward()
    if dtype == torch.float32:
        assert rel_l2(out, T(g["out"])) < 2e-5
        for k, p in G.named_parameters():
            assert rel_l2(p.grad, truth[k]) < 2e-4, k
        return
    assert rel_l2(out, T(g["out"])) < 2e-2
    sd = onets.deterministic_state(onets.g_param_shapes(spec), seed=15, scale=0.7)
    for v in sd.values():
        v.requires_grad_(True)
    em = onets.GSpec(upscale=4, in_channels=in_ch, out_channels=3, nf=16, n_rrdb=2, hr_kern=5, gc=8, tf=8,
                     bf16_storage=True)
    (onets.generator_forward(sd, LR, Z, em) * T(g["gy"])).sum().backward()
    lim = _emulated_bf16_bounds(truth, {k: v.grad for k, v in sd.items()})
    errs = {k: rel_l2(p.grad, truth[k]) for k, p in G.named_parameters()}
    bad = {k: (v, lim[k]) for k, v in errs.items() if not v < lim[k]}
    assert not bad, bad
    # the feature conv's own filter gradient, tightly: against an fp32 evaluation of the same bf16-rounded operands
    # the emulation's gradient of model.0.0.weight is the nearest statement of that
    k0 = "model.0.0.weight"
    assert rel_l2(G.state_dict()[k0], sd[k0].detach()) < 1e-6


def test_generator_dropout_mask_and_train_mode(hip):
    """Dropout3d channel mask in the hr0 epilogue / backward == oracle with the same mask."""
    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=16, n_rrdb=1, hr_kern=5, gc=8, tf=8,
                       dropout_p=0.5)
    G, sd = build_G(spec, torch.float32, 21)
    G.train()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 5, 4, 4, seed=1)
    gen = torch.Generator().manual_seed(0)
    mask = (torch.rand((2, 24), generator=gen) > 0.5).float() * 2.0
    out = G(LR.to(DEV), Z.to(DEV), dropout_scale=mask.to(DEV))
    for v in sd.values():
        v.requires_grad_(True)
    ref = onets.generator_forward(sd, LR, Z, spec, training=True, dropout_mask=mask.view(2, 24, 1, 1, 1))
    assert rel_l2(out, ref) < 2e-5
    gy = torch.randn(ref.shape, generator=gen)
    (ref * gy).sum().backward()
    (out * gy.to(DEV)).sum().backward()
    for k, p in G.named_parameters():
        assert rel_l2(p.grad, sd[k].grad) < 2e-4, k
    # RNG-driven mask: some channels dropped, survivors scaled by 1/(1-p)
    out2 = G(LR.to(DEV), Z.to(DEV))
    assert torch.isfinite(out2).all() and not torch.equal(out2, out)


def _d_grads_fp64(spec, seed, x_seed, xy, nz):  # (spec carries the normalisation type)
    """fp64 oracle gradients of the D test graph (train-mode BN), on the CPU."""
    sd = onets.deterministic_state(onets.d_param_shapes(spec), seed=seed, scale=1.0)
    sd = {k: (v.double() if v.is_floating_point() else v).clone() for k, v in sd.items()}
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    gen = torch.Generator().manual_seed(x_seed)
    x = (torch.rand((2, 3, xy, xy, nz), generator=gen) * 2 - 1).double()
    out = onets.discriminator_forward(sd, x, spec, training=True)
    (out * torch.tensor([[1.0], [-0.5]], dtype=torch.float64)).sum().backward()
    return {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}


@pytest.mark.parametrize("slicing,xy,nz,norm", [(True, 64, 4, "batch"), (False, 128, 3, "batch"), (False, 128, 21, "batch"),
                                                (False, 128, 3, "instance"), (True, 64, 4, "instance")])
def test_discriminator_fp32_vs_reference(golden, hip, slicing, xy, nz, norm):
    """(norm = "instance": the reference's ``normalization_type="instance"``, torch_blocks.py:26-30 - nn.InstanceNorm3d
    layers in the blocks, fixtures recorded from the reference; the slicing tail keeps its BatchNorm3d layers)"""
    tag = ("slice" if slicing else "full") + f"_z{nz}" + ("" if norm == "batch" else f"_{norm}")
    g = golden(f"d_small_{tag}.npz")
    spec = onets.DSpec(bf=4, nz=nz, enable_slicing=slicing, norm=norm)
    D, _ = build_D(spec, torch.float32, 31 + nz)
    gen = torch.Generator().manual_seed(int(g["x_seed"]))
    x = (torch.rand((2, 3, xy, xy, nz), generator=gen) * 2 - 1).to(DEV).requires_grad_(True)
    D.eval()
    assert rel_l2(D(x), T(g["out_eval"])) < 2e-5
    D.train()
    out = D(x)
    assert rel_l2(out, T(g["out_train"])) < 2e-5
    (out * torch.tensor([[1.0], [-0.5]], device=DEV)).sum().backward()
    # input gradient after 10 conv + 9 train-mode BatchNorm backward stages (each a
    # g - mean(g) - xhat*mean(g*xhat) cancellation): 1e-3; the shallower cases sit at ~1e-4.
    # BatchNorm reductions are two-pass and atomic-free, so this gradient is deterministic.  The z21 case lands
    # 2.6e-3 from the reference: one near-zero pre-activation takes the other LeakyReLU branch under this
    # summation order (the reference's own fp32 result is 5.4e-4 from an fp64 evaluation for the same reason).
    tol_dx = 5e-3 if nz == 21 else 1e-3
    assert rel_l2(x.grad[:, :, ::4, ::4, :], T(g["dx_sub"])) < tol_dx
    assert abs(float(x.grad.double().abs().sum()) / float(g["dx_abs_sum"]) - 1) < tol_dx
    # The recorded fp32 reference gradients are themselves up to 5.3e-4 away from an fp64
    # evaluation of the same graph (features.0.0.0.weight of the z21 case: 9 train-mode BN
    # backward stages over tiny populations), so each key's tolerance is 2e-4 plus 1.5x the
    # reference's own fp32-vs-fp64 distance, and the HIP result must also sit within
    # 2e-4 + that distance of the fp64 oracle.
    ref64 = _d_grads_fp64(spec, 31 + nz, int(g["x_seed"]), xy, nz)
    for k, p in D.named_parameters():
        floor = rel_l2(T(g[f"grad.{k}"]).double(), ref64[k])
        flip = 1e-2 if nz == 21 else 0.0  # the branch flip above reaches the parameter gradients below it (worst: 6.5e-3 on a 4-element BatchNorm weight)
        assert rel_l2(p.grad, T(g[f"grad.{k}"])) < max(2e-4 + 1.5 * floor, flip), (k, floor)
        assert rel_l2(p.grad.double().cpu(), ref64[k]) < max(2e-4 + floor, flip), (k, floor)
    for k, v in D.state_dict().items():
        if "running_" in k or "num_batches" in k:
            assert rel_l2(v.float(), T(g[f"after.{k}"]).float()) < 1e-5, k


def test_discriminator_eval_mode_input_gradient(hip):
    """G-iteration use: D.eval(), parameters frozen, gradient w.r.t. the input only."""
    spec = onets.DSpec(bf=4, nz=4, enable_slicing=True)
    D, sd = build_D(spec, torch.float32, 5)
    D.eval()
    for p in D.parameters():
        p.requires_grad = False
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1)
    xd = x.to(DEV).requires_grad_(True)
    D(xd).sum().backward()
    xr = x.clone().requires_grad_(True)
    onets.discriminator_forward(sd, xr, spec, training=False).sum().backward()
    assert rel_l2(xd.grad, xr.grad) < 2e-4
    assert all(p.grad is None for p in D.parameters())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["train", "eval_input_grad"])
def test_discriminator_pair_equals_two_calls(hip, dt, mode):
    """D.forward_pair(a, b) - the feature pyramid run once on both inputs, BatchNorm statistics per call - against
    D(a), D(b) as the reference issues them (wind_field_GAN_3D.py:247-304): logits, running statistics, parameter
    gradients (train: both calls feed one backward pass) and the input gradient of the second input (generator
    iteration: D in eval mode, parameters frozen, first input detached).  Equal up to summation order: the batched
    filter gradient adds the two samples inside one launch (fp32 2e-5; bf16: identical roundings, 2e-3)."""
    import copy
    spec = onets.DSpec(bf=8, nz=4, enable_slicing=True)
    D1, _ = build_D(spec, dt, 23)
    D2 = copy.deepcopy(D1)
    D2.features.compute_dtype = D1.features.compute_dtype
    gen = torch.Generator().manual_seed(9)
    a = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    b = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    tol = 2e-5 if dt == torch.float32 else 2e-3
    wgt = torch.tensor([[1.0], [-0.5]], device=DEV)
    if mode == "train":
        D1.train(); D2.train()
        ya, yb = D1(a), D1(b)
        ((ya - yb.mean()) * wgt).sum().backward()
        pa, pb = D2.forward_pair(a, b)
        ((pa - pb.mean()) * wgt).sum().backward()
        assert rel_l2(pa, ya) < tol and rel_l2(pb, yb) < tol
        for (k, p1), (_, p2) in zip(D1.named_parameters(), D2.named_parameters()):
            assert rel_l2(p2.grad, p1.grad) < (2e-4 if dt == torch.float32 else 2e-2), k
        for (k, v1), (_, v2) in zip(D1.state_dict().items(), D2.state_dict().items()):
            if "running_" in k or "num_batches" in k:
                assert rel_l2(v2.float(), v1.float()) < 1e-5, k
            if "num_batches" in k:  # two BatchNorm calls, however they were batched (the reference counts per call)
                assert int(v1) == 2 and int(v2) == 2, k
    else:
        D1.eval(); D2.eval()
        for p in list(D1.parameters()) + list(D2.parameters()):
            p.requires_grad = False
        b1, b2 = b.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ya, yb = D1(a).detach(), D1(b1)
        ((yb - ya.mean()) * wgt).sum().backward()
        pa, pb = D2.forward_pair(a, b2)
        ((pb - pa.detach().mean()) * wgt).sum().backward()
        assert rel_l2(pa, ya) < tol and rel_l2(pb, yb) < tol
        assert rel_l2(b2.grad, b1.grad) < (2e-5 if dt == torch.float32 else 2e-3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_batchnorm_statistics_are_bit_identical(hip, dt, monkeypatch):
    """Round 6: the train-mode BatchNorm statistics of both batch groups of a discriminator layer in four launches
    (``wsr_bn_train_stats``, engine.FUSED_BN_STATS) against the six-launches-per-group form (``wsr_bn_stats`` / ``_mean`` /
    ``_stats`` / ``_finalize``): logits, running statistics (two updates per layer, in call order: reference
    torch_blocks.py:20-25 called twice, wind_field_GAN_3D.py:247-304) and every parameter gradient - bit for bit."""
    import copy
    from gan_sr_wind_field_amd import engine

    spec = onets.DSpec(bf=8, nz=4, enable_slicing=True)
    D1, _ = build_D(spec, dt, 23)
    D2 = copy.deepcopy(D1)
    D2.features.compute_dtype = D1.features.compute_dtype
    gen = torch.Generator().manual_seed(9)
    a = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    b = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    wgt = torch.tensor([[1.0], [-0.5]], device=DEV)
    outs = []
    for D, fused in ((D1, True), (D2, False)):
        monkeypatch.setattr(engine, "FUSED_BN_STATS", fused)
        D.train()
        pa, pb = D.forward_pair(a, b)
        ((pa - pb.mean()) * wgt).sum().backward()
        ya = D(a)  # a single-group call as well (the generator iteration's D(real) when the pair is off)
        outs.append((pa.detach().clone(), pb.detach().clone(), ya.detach().clone()))
    for u, v in zip(outs[0], outs[1]):
        assert torch.equal(u, v)
    for (k, p1), (_, p2) in zip(D1.named_parameters(), D2.named_parameters()):
        assert torch.equal(p1.grad, p2.grad), k
    for (k, v1), (_, v2) in zip(D1.state_dict().items(), D2.state_dict().items()):
        assert torch.equal(v1, v2), k
        if "num_batches" in k:
            assert int(v1) == 3, k


def test_discriminator_pair_keeps_the_order_of_random_draws(hip):
    """Dropout3d masks and the second input's instance noise are drawn in the order of two consecutive calls
    (first mask, noise, second mask): same seed -> same logits as D(a), D(b + noise())."""
    spec = onets.DSpec(bf=8, nz=4, enable_slicing=True, dropout_p=0.3)
    D, _ = build_D(spec, torch.float32, 29)
    D.train()
    for m in D.modules():  # (keep the running statistics out of the comparison: both runs start from the same state)
        if isinstance(m, torch.nn.BatchNorm3d):
            m.momentum = 0.0
    gen = torch.Generator().manual_seed(10)
    a = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    b = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1).to(DEV)
    with torch.no_grad():
        torch.manual_seed(77)
        ya = D(a)
        yb = D(b + 0.1 * torch.rand(b.shape, device=DEV))
        torch.manual_seed(77)
        pa, pb = D.forward_pair(a, lambda: b + 0.1 * torch.rand(b.shape, device=DEV))
    assert rel_l2(pa, ya) < 2e-5 and rel_l2(pb, yb) < 2e-5
    assert float((ya - D(a)).abs().max()) > 0  # (the masks do matter: another draw gives other logits)


def test_discriminator_bf16_vs_oracle(hip):
    spec = onets.DSpec(bf=8, nz=4, enable_slicing=True)
    D, _ = build_D(spec, torch.bfloat16, 8)
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand((2, 3, 64, 64, 4), generator=gen) * 2 - 1)
    D.train()
    out = D(x.to(DEV))
    wgt = torch.tensor([[1.0], [-0.5]])
    (out * wgt.to(DEV)).sum().backward()
    res = {}
    for mode in ("fp32", "emul"):  # fp32 oracle, and the oracle with bf16 storage emulation (the yard-stick)
        sd = onets.deterministic_state(onets.d_param_shapes(spec), seed=8, scale=1.0)
        params = {k: v for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
        for p in params.values():
            p.requires_grad_(True)
        ref = onets.discriminator_forward(sd, x, onets.DSpec(bf=8, nz=4, enable_slicing=True,
                                                              bf16_storage=mode == "emul"), training=True)
        (ref * wgt).sum().backward()
        res[mode] = (ref.detach(), {k: v.grad for k, v in params.items()})
    assert rel_l2(out, res["fp32"][0]) < 1e-2 + 2 * rel_l2(res["emul"][0], res["fp32"][0])
    # batch-of-2 BatchNorm backward on bf16-stored activations is the noisiest spot of the bf16 path (the
    # projection terms cancel most of g): the emulation itself is 0.1-0.3 away from fp32 on the first layers
    lim = _emulated_bf16_bounds(res["fp32"][1], res["emul"][1], pooled=True)
    errs = {k: rel_l2(p.grad, res["fp32"][1][k]) for k, p in D.named_parameters()}
    bad = {k: (v, lim[k]) for k, v in errs.items() if not v < lim[k]}
    assert not bad, bad
    for k, p in D.named_parameters():
        if k != "classifier.2.bias":
            cos = torch.nn.functional.cosine_similarity(p.grad.flatten().cpu(), res["fp32"][1][k].flatten(), dim=0)
            assert float(cos) > 0.97, (k, float(cos))


@pytest.mark.parametrize("slicing,xy,nz", [(True, 64, 10), (False, 128, 10)])
def test_discriminator_bf16_backward_layer_by_layer(hip, slicing, xy, nz):
    """The bf16 discriminator backward, STAGE BY STAGE, against an fp32 CPU evaluation of each stage fed the HIP path's
    own operands - its saved bf16 activations, its batch statistics and the bf16 gradient it handed to that stage - so
    that neither the rounding of the stages above nor a LeakyReLU branch that falls the other way can hide an error:
    BatchNorm (+ LeakyReLU) backward, input gradient, filter gradient and the BatchNorm parameter gradients of every
    layer: results the path stores in bf16 within 4e-3 (one rounding: measured 1.7e-3), fp32 results within 2e-5
    (measured 1e-7 .. 1e-6).  Full width (bf 32), train-mode batch statistics, batch
    2; the end-to-end bounds of the network-level bf16 tests are 0.5-0.7 on these tensors (conditioning), this one
    would catch a 1 % error in any single kernel of the pass."""
    import torch.nn.functional as F
    from torch.nn import grad as ngrad

    spec = onets.DSpec(bf=32, nz=nz, enable_slicing=slicing)
    D, _ = build_D(spec, torch.bfloat16, 77)
    D.train()
    prog = D.features.program()
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand((2, 3, xy, xy, nz), generator=gen) * 2 - 1).to(DEV)
    feat, saved = prog.forward(x, True, True)
    g_feat = (torch.randn(feat.shape, generator=gen) * 0.1).to(DEV).to(feat.dtype)
    prog.trace = []
    try:
        dx, flat = prog.backward(saved, g_feat, need_dx=True, need_dw=True)
    finally:
        trace, prog.trace = prog.trace, None
    torch.cuda.synchronize()
    tr = {(tag, li): t for tag, li, t in trace}
    sl, worst = prog.slope, {}

    def planar(t, c):  # NDHWC (B, X, Y, Z, Cp) -> fp32 (B, c, X, Y, Z) on the host
        return t[..., :c].permute(0, 4, 1, 2, 3).float().cpu().contiguous()

    for li, (l, r) in enumerate(zip(prog.layers, saved["recs"])):
        s = l.conv
        g = planar(tr[("g", li)], s.cout)
        a = planar(r["a"], s.cout)
        dact = g * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, sl)) if l.act else g
        if l.bn is None:
            gy_ref = dact
        else:
            y = planar(r["y"], s.cout)
            mean, invstd = r["mean"][0].float().cpu().view(1, -1, 1, 1, 1), r["invstd"][0].float().cpu().view(1, -1, 1, 1, 1)
            gamma = l.bn.weight.detach().float().cpu().view(1, -1, 1, 1, 1)
            xhat = (y - mean) * invstd
            n = float(y.numel() // y.shape[1])
            dbeta, dgamma = dact.sum((0, 2, 3, 4)), (dact * xhat).sum((0, 2, 3, 4))
            gy_ref = gamma * invstd * (dact - dbeta.view(1, -1, 1, 1, 1) / n - xhat * dgamma.view(1, -1, 1, 1, 1) / n)
            worst[f"{li}.bn.bias"] = rel_l2(prog.space.view(flat, l.bn.bias), dbeta)
            worst[f"{li}.bn.weight"] = rel_l2(prog.space.view(flat, l.bn.weight), dgamma)
            assert worst[f"{li}.bn.bias"] < 2e-5 and worst[f"{li}.bn.weight"] < 2e-5, (li, worst)
        gy_hip = planar(tr[("gy", li)], s.cout)
        worst[f"{li}.gy"] = rel_l2(gy_hip, gy_ref)
        assert worst[f"{li}.gy"] < 4e-3, (li, worst)   # ONE bf16 rounding of the stored result (measured 1.7e-3)
        # the two conv gradients from the HIP path's own gy (bf16) and saved input; the filter as the kernels see it
        inp = planar(r["inp"], s.cin)
        w = s.weight.detach().float().cpu()
        dw_ref = ngrad.conv3d_weight(inp, w.shape, gy_hip, stride=s.stride, padding=s.pad)
        worst[f"{li}.dw"] = rel_l2(prog.space.view(flat, s.weight), dw_ref)
        assert worst[f"{li}.dw"] < 2e-5, (li, worst)   # fp32 sums of the same bf16 products: only the order differs (1e-6)
        w16 = w.to(torch.bfloat16).float()
        gin_ref = ngrad.conv3d_input(inp.shape, w16, gy_hip, stride=s.stride, padding=s.pad)
        if li > 0:
            worst[f"{li}.gin"] = rel_l2(planar(tr[("gin", li)], s.cin), gin_ref)
            assert worst[f"{li}.gin"] < 4e-3, (li, worst)
        else:
            worst["0.dx"] = rel_l2(dx.cpu(), gin_ref)
            assert worst["0.dx"] < 2e-5, worst     # planar fp32 output of the first layer's input gradient
    try:
        import json
        import os
        from conftest import REPO
        os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
        with open(os.path.join(REPO, "gpurun_out", f"parity_d_bf16_layerwise_{'slice' if slicing else 'full'}.json"), "w") as f:
            json.dump(worst, f, indent=1, sort_keys=True)
    except OSError:
        pass


def test_generator_bf16_backward_stage_by_stage(hip, monkeypatch):
    """The bf16 generator backward, STAGE BY STAGE, against fp32 CPU evaluations fed the HIP path's own operands (its saved
    bf16 activations, the bf16 gradient it handed to the stage - ``ProgramBase.trace``): the z-folded last conv's masked input
    gradient, the 5x5x5 conv over the two-tensor concat (input gradient to both tensors, filter gradient), the terrain
    branch, the sub-pixel up-convs (parity input gradients with the mask of the conv below, parity filter gradients
    folded back), lr_conv, and every residual dense block (LFF input gradient in place, stacked growth windows with their
    LeakyReLU masks, stacked filter gradients, LFF filter / bias gradients).  Full width (nf 128, gc 32, tf 16), one
    RRDB; HR 32 x 64 x 32 = 65 536 voxels, so the HR stages run the 512-voxel production tiles and the split concat.
    Results the path stores in bf16: within 4e-3 of the fp32 evaluation per stage (measured 1.66e-3: ONE rounding; the dense
    block's windows accumulate through bf16 once more: 2.35e-3 = sqrt(2) x that, bound 5e-3; the parity filters of the up-convs
    are rounded sums of taps: 3.1e-3, bound 6e-3); fp32 results (every filter / bias gradient): 2e-5 (measured 1e-7 .. 4e-6).  The network-
    level bounds on these tensors are 0.1-0.26 (test_hip_fullsize_parity): this is the test that sees a 1 % error in one kernel."""
    import torch.nn.functional as F
    from torch.nn import grad as ngrad
    from gan_sr_wind_field_amd import engine

    monkeypatch.setattr(engine, "GD_PINGPONG", False)  # (the in-place form: one gradient buffer, block by block)
    spec = onets.GSpec(n_rrdb=1)
    G, _ = build_G(spec, torch.bfloat16, 91, scale=0.5)
    G.eval()
    prog = G.program()
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 8, 32, 4, seed=6)
    LR, Z = LR[:, :, :, :, :], Z
    # (LR 8 x 16 x 32: a non-square patch)
    LR = torch.cat([LR, LR.flip(3)], dim=3)
    Z = torch.cat([Z, Z.flip(3) + 3.0], dim=3)
    out, saved = prog.forward(LR.to(DEV), Z.to(DEV), False, True, None)
    gen = torch.Generator().manual_seed(8)
    g_out = torch.randn(out.shape, generator=gen).to(DEV)
    prog.trace = []
    try:
        flat = prog.backward(saved, g_out)
    finally:
        trace, prog.trace = prog.trace, None
    torch.cuda.synchronize()
    tr = {(tag, i): t for tag, i, t in trace}
    nf, gc, tf, sl = prog.nf, prog.gc, prog.tf, prog.slope
    worst = {}

    def planar(t, c0=0, c1=None):
        c1 = t.shape[-1] if c1 is None else c1
        return t[..., c0:c1].permute(0, 4, 1, 2, 3).float().cpu().contiguous()

    def w16(site):
        return site.weight.detach().to(torch.bfloat16).float().cpu()

    def mask(a):
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, sl))

    def gradw(site):
        return prog.space.view(flat, site.weight).float().cpu()

    def hold(name, got, want, tol):
        worst[name] = rel_l2(got, want)
        assert worst[name] < tol, (name, worst)

    # ---- last conv in z-folded form: input gradient with the mask of the 5x5x5 conv's output
    h = planar(saved["h"])
    g3 = planar(tr[("g3", 0)], 0, prog.hr1z.cout)
    wz = prog.hr1z.weight.detach().to(torch.bfloat16).float().cpu()
    gh_ref = ngrad.conv3d_input(h.shape, wz, g3, padding=prog.hr1z.pad) * mask(h)
    gh = planar(tr[("gh", 0)])
    hold("hr1.dgrad", gh, gh_ref, 4e-3)
    # ---- the 5x5x5 conv over the concat (two tensors): input gradient to both, filter gradient from both
    hcat = torch.cat([planar(saved["hcat"], 0, nf), planar(saved["tfeat"])], dim=1) if saved.get("tfeat") is not None \
        else planar(saved["hcat"], 0, nf + tf)
    assert saved.get("tfeat") is not None  # (this size runs the split form)
    dcat_ref = ngrad.conv3d_input(hcat.shape, w16(prog.hr0), gh, padding=prog.hr0.pad)
    hold("hr0.dgrad.up", planar(tr[("ghcat", 0)], 0, nf), dcat_ref[:, :nf], 4e-3)
    hold("hr0.dgrad.terrain", planar(tr[("gterrain", 0)], 0, tf), dcat_ref[:, nf:], 4e-3)
    hold("hr0.wgrad", gradw(prog.hr0), ngrad.conv3d_weight(hcat, prog.hr0.weight.shape, gh, padding=prog.hr0.pad), 2e-5)
    # ---- terrain branch
    t0, gter = planar(saved["t0"], 0, tf), planar(tr[("gterrain", 0)], 0, tf)
    gt0_ref = ngrad.conv3d_input(t0.shape, w16(prog.terrain1), gter, padding=1) * mask(t0)
    gt0 = planar(tr[("gt0", 0)], 0, tf)
    hold("terrain1.dgrad", gt0, gt0_ref, 4e-3)
    hold("terrain1.wgrad", gradw(prog.terrain1), ngrad.conv3d_weight(t0, prog.terrain1.weight.shape, gter, padding=1), 2e-5)
    hold("terrain0.wgrad", gradw(prog.terrain0),
         ngrad.conv3d_weight(planar(saved["z_nd"], 0, 1), prog.terrain0.weight.shape, gt0, padding=1), 2e-5)
    # ---- up-convs (nearest x(2,2,1) + 3x3x3 conv + LeakyReLU), last to first
    for u in reversed(range(len(prog.ups))):
        site, (inp, outp) = prog.ups[u], saved["up_io"][u]
        gy = planar(tr[("gup_out", u)], 0, nf)                    # (already carries the LeakyReLU derivative of outp)
        xin = planar(inp, 0, nf)
        xup = xin.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        hold(f"up{u}.wgrad", gradw(site), ngrad.conv3d_weight(xup, site.weight.shape, gy, padding=1), 2e-5)
        dfine = ngrad.conv3d_input(xup.shape, site.weight.detach().float().cpu(), gy, padding=1)
        B_, C_, X2, Y2, Z_ = dfine.shape
        gin_ref = dfine.view(B_, C_, X2 // 2, 2, Y2 // 2, 2, Z_).sum((3, 5))
        if u > 0:  # the mask of up-conv u-1's output rides on the last parity launch
            gin_ref = gin_ref * mask(xin)
        # (parity filters are sums of fp32 master taps rounded to bf16 once: a different rounding of the filter than
        # tap-by-tap - the fp32 master filter is the reference)
        hold(f"up{u}.dgrad", planar(tr[("gup_in", u)], 0, nf), gin_ref, 6e-3)
    # ---- lr_conv
    gs, tl = planar(tr[("gs", 0)], 0, nf), planar(saved["t_last"], 0, nf)
    hold("lr_conv.dgrad", planar(tr[("g_lr", 0)], 0, nf), ngrad.conv3d_input(tl.shape, w16(prog.lr_conv), gs, padding=1), 4e-3)
    hold("lr_conv.wgrad", gradw(prog.lr_conv), ngrad.conv3d_weight(tl, prog.lr_conv.weight.shape, gs, padding=1), 2e-5)
    # ---- residual dense blocks, last to first (in-place form)
    bufs = saved["bufs"]
    bi = len(bufs)
    for rdbs in reversed(prog.rrdbs):
        for convs, lff, rdb_scale in reversed(rdbs):
            bi -= 1
            buf = planar(bufs[bi])                                # all nf + 4 gc channels as saved (bf16)
            go = planar(tr[("rdb_go", bi)], 0, nf)
            gd = planar(tr[("rdb_gd", bi)])                       # the gradient buffer after the block
            lw = lff.weight.detach().to(torch.bfloat16).float().cpu()[:, :, 0, 0, 0]
            d = rdb_scale * torch.einsum("bnxyz,nc->bcxyz", go, lw)
            d[:, :nf] += go
            for i in reversed(range(len(convs))):
                win = slice(nf + i * gc, nf + (i + 1) * gc)
                d[:, win] = d[:, win] * mask(buf[:, win])
                # the filter gradient of conv i from the HIP path's OWN final window (bf16) and saved input
                hold(f"rdb{bi}.conv{i}.wgrad", gradw(convs[i]),
                     ngrad.conv3d_weight(buf[:, :nf + i * gc], convs[i].weight.shape, gd[:, win], padding=1), 2e-5)
                d[:, :nf + i * gc] += ngrad.conv3d_input(buf[:, :nf + i * gc].shape, w16(convs[i]), d[:, win].contiguous(),
                                                         padding=1)
            for i in range(len(convs)):
                win = slice(nf + i * gc, nf + (i + 1) * gc)
                hold(f"rdb{bi}.window{i + 1}", gd[:, win], d[:, win], 5e-3)
            hold(f"rdb{bi}.input", gd[:, :nf], d[:, :nf], 5e-3)
            hold(f"rdb{bi}.lff.wgrad", gradw(lff)[:, :, 0, 0, 0], rdb_scale * torch.einsum("bnxyz,bcxyz->nc", go, buf), 2e-5)
            hold(f"rdb{bi}.lff.bias", prog.space.view(flat, lff.bias).float().cpu(), rdb_scale * go.sum((0, 2, 3, 4)), 2e-5)
    try:
        import json
        import os
        from conftest import REPO
        os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
        with open(os.path.join(REPO, "gpurun_out", "parity_g_bf16_stagewise.json"), "w") as f:
            json.dump(worst, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _gpu_gan(dtype="fp32", use_noise=False, dropout=0.0, feature_cost=False):
    import os
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    import gan_sr_wind_field_amd

    ini = os.path.join(os.path.dirname(gan_sr_wind_field_amd.__file__), "config", "wind_field_GAN_3D_config_local.ini")
    cfg = Config(ini)
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id = 0
    cfg.device = torch.device(DEV)
    cfg.compute_dtype = dtype
    cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 16, 1, 8
    cfg.generator.terrain_number_of_features = 4 if dtype == "fp32" else 8
    cfg.generator.dropout_probability = dropout
    cfg.discriminator.num_features = 4 if dtype == "fp32" else 8
    cfg.discriminator.dropout_probability = dropout
    cfg.gan_config.number_of_z_layers = 4
    cfg.training.use_instance_noise = use_noise
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = 2
    if feature_cost:
        cfg.gan_config.use_D_feature_extractor_cost = True
        cfg.training.feature_D_update_period = 1
    torch.manual_seed(2001)
    return wind_field_GAN_3D(cfg), cfg


def test_gan_train_step_trace_fp32_vs_reference(golden, hip):
    """6 iterations (G, D, D, G, G, D) of the product on the GPU == the reference trace."""
    g = golden("gan_trace_plain.npz")
    gan, cfg = _gpu_gan()
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=4, hr_kern=5, upscale=4)
    ds = onets.DSpec(bf=4, nz=4, enable_slicing=True)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
    LR, HR, Z, x, y = (t.to(DEV) for t in ogan.synthetic_batch(2, 16, 4, 4, seed=2001))
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 2)
    keys = ["total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"]
    for row, it in enumerate(g["its"]):
        gan.optimize_parameters(LR, HR, Z, int(it))
        if int(it) > 4:
            gan.update_learning_rate()
        if g["kinds"][row]:
            got = [float(gan.get_G_train_loss_dict_ref()[k]) for k in keys]
            np.testing.assert_allclose(got, g["G_losses"][row], rtol=1e-3, atol=1e-7, err_msg=f"it={it}")
        else:
            np.testing.assert_allclose(float(gan.get_D_loss_dict_ref()["train_loss"]), g["D_loss"][row], rtol=1e-3,
                                       err_msg=f"it={it}")
        sdG, sdD = gan.G.state_dict(), gan.D.state_dict()
        wg = [float(sdG[k].double().abs().sum())
              for k in ("model.0.0.weight", "hr_convs.2.weight", "model.1.module.0.RDBs.1.LFF.bias")]
        wd = [float(sdD[k].double().abs().sum())
              for k in ("features.0.0.0.weight", "classifier.2.weight", "features.1.1.1.running_var")]
        np.testing.assert_allclose(wg, g["wsum_g"][row], rtol=2e-4, err_msg=f"it={it}")
        np.testing.assert_allclose(wd, g["wsum_d"][row], rtol=2e-4, err_msg=f"it={it}")
    for k in g.files:
        if k.startswith("final_G."):
            assert rel_l2(gan.G.state_dict()[k[8:]], T(g[k])) < 2e-3, k
        if k.startswith("final_D."):
            assert rel_l2(gan.D.state_dict()[k[8:]], T(g[k])) < 2e-3, k


def test_gan_train_step_noise_trace_fp32_vs_reference(golden, hip, monkeypatch):
    """The instance-noise / noisy-label / Dropout3d branch (reference GAN_models/wind_field_GAN_3D.py:221-304, 627-678,
    tools/trainingtricks.py:18-59) ON THE HIP PATH against the reference trace ``gan_trace_noise.npz``: every random
    draw of the branch is routed to the CPU generator in the reference's order and shapes - the instance noise as
    ``torch.rand(shape)``, a Dropout3d mask as ATen's feature dropout draws it (one Bernoulli per (sample, channel) on
    a (B, C, 1, 1, 1) tensor; the generator's through the injectable ``dropout_scale``), the labels already are CPU
    ``torch.normal`` draws - and everything else (G, D, losses, both Adam steps) runs through the HIP programs."""
    import torch.nn.functional as F
    from gan_sr_wind_field_amd.tools import trainingtricks

    g = golden("gan_trace_noise.npz")
    p = float(g["dropout"])
    gan, cfg = _gpu_gan(use_noise=bool(g["use_noise"]), dropout=p)
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=4, hr_kern=5, upscale=4, dropout_p=p)
    ds = onets.DSpec(bf=4, nz=4, enable_slicing=True, dropout_p=p)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))

    draws = {"noise": 0, "g_mask": 0, "d_mask": 0}

    def cpu_instance_noise(sigma_base, shape, it, niter, device=torch.device("cpu")):
        draws["noise"] += 1
        scale = torch.sqrt(sigma_base.cpu() * (1 - (it.cpu() - 1) / niter.cpu()))
        return (torch.rand(shape) * scale).to(device)

    monkeypatch.setattr(trainingtricks, "instance_noise", cpu_instance_noise)

    def cpu_feature_mask(b, c, prob):  # what nn.Dropout3d multiplies a (b, c, X, Y, Z) CPU tensor by
        return F.dropout3d(torch.ones(b, c, 1, 1, 1), prob, True)

    g_forward = gan.G.forward

    def forward_with_cpu_mask(x, Z, dropout_scale=None):
        if dropout_scale is None and gan.G.training and p > 0:
            draws["g_mask"] += 1
            c = gan.G.hr_convs[0][0].out_channels
            dropout_scale = cpu_feature_mask(x.shape[0], c, p).reshape(x.shape[0], c).to(x.device)
        return g_forward(x, Z, dropout_scale)

    monkeypatch.setattr(gan.G, "forward", forward_with_cpu_mask)

    class CpuDropout3d(torch.nn.Dropout3d):
        def forward(self, x):
            if not self.training or self.p == 0:
                return x
            draws["d_mask"] += 1
            return x * cpu_feature_mask(x.shape[0], x.shape[1], self.p).to(x.device)

    gan.D.dropout = CpuDropout3d(p=p)

    LR, HR, Z, x, y = (t.to(DEV) for t in ogan.synthetic_batch(2, 16, 4, 4, seed=2001))
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), cfg.training.d_g_train_ratio,
                      cfg.training.d_g_train_period)
    torch.manual_seed(4242)  # RNG state at the first optimize_parameters call of the recorded trace
    keys = ["total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"]
    for row, it in enumerate(g["its"]):
        gan.optimize_parameters(LR, HR, Z, int(it))
        if int(it) > 2 * cfg.training.d_g_train_period:
            gan.update_learning_rate()
        if g["kinds"][row]:
            got = [float(gan.get_G_train_loss_dict_ref()[k]) for k in keys]
            np.testing.assert_allclose(got, g["G_losses"][row], rtol=1e-3, atol=1e-7, err_msg=f"it={it}")
        else:
            np.testing.assert_allclose(float(gan.get_D_loss_dict_ref()["train_loss"]), g["D_loss"][row], rtol=1e-3,
                                       err_msg=f"it={it}")
        sdG, sdD = gan.G.state_dict(), gan.D.state_dict()
        wg = [float(sdG[k].double().abs().sum())
              for k in ("model.0.0.weight", "hr_convs.2.weight", "model.1.module.0.RDBs.1.LFF.bias")]
        wd = [float(sdD[k].double().abs().sum())
              for k in ("features.0.0.0.weight", "classifier.2.weight", "features.1.1.1.running_var")]
        np.testing.assert_allclose(wg, g["wsum_g"][row], rtol=2e-4, err_msg=f"it={it}")
        np.testing.assert_allclose(wd, g["wsum_d"][row], rtol=2e-4, err_msg=f"it={it}")
        assert abs(gan.optimizer_G.param_groups[0]["lr"] - g["lr"][row]) < 1e-12
    # the branch really ran: noise for every D input (+ the reference's one debug draw), a generator mask per
    # G-iteration (the D-iteration's generator pass runs in eval mode), two discriminator masks per D-iteration
    n_g, n_d = int(np.sum(g["kinds"])), int(np.sum(1 - g["kinds"]))
    assert draws == {"noise": 2 * (n_g + n_d) + 1, "g_mask": n_g, "d_mask": 2 * n_d}, draws
    for k in g.files:
        if k.startswith("final_G."):
            assert rel_l2(gan.G.state_dict()[k[8:]], T(g[k])) < 2e-3, k
        if k.startswith("final_D."):
            assert rel_l2(gan.D.state_dict()[k[8:]], T(g[k])) < 2e-3, k


def test_discriminator_feature_extractor_loss(hip):
    """``use_D_feature_extractor_cost`` (reference GAN_models/wind_field_GAN_3D.py:372-375, 577-583: a frozen deep copy
    of D.features, MSE between its features of HR and of the generated field): the loss entry against the oracle's
    feature pyramid on the same weights, and its gradient reaching the generator."""
    import copy
    import torch.nn.functional as F

    outs = {}
    for fc in (False, True):
        gan, cfg = _gpu_gan(feature_cost=fc)
        gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=4, hr_kern=5, upscale=4)
        ds = onets.DSpec(bf=4, nz=4, enable_slicing=True)
        gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
        gan.D.load_state_dict(onets.deterministic_state(onets.d_param_shapes(ds), seed=43, scale=1.0))
        LR, HR, Z, x, y = (t.to(DEV) for t in ogan.synthetic_batch(2, 16, 4, 4, seed=2001))
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 2)
        gan.G.train()
        with torch.no_grad():
            fake = gan.G(LR, Z).cpu()
        mode = gan.D.features.training  # the copy inherits the mode D.features is in when it is taken
        sd = {k: v.detach().clone().cpu() for k, v in gan.D.state_dict().items()}
        f_hr = onets.discriminator_features(copy.deepcopy(sd), HR.cpu(), ds, mode)
        f_sr = onets.discriminator_features(copy.deepcopy(sd), fake, ds, mode)
        want = float(F.mse_loss(f_sr, f_hr)) * cfg.training.feature_D_loss_weight
        gan.optimize_parameters(LR, HR, Z, 0)  # it = 0: a generator iteration
        L = {k: float(v) for k, v in gan.get_G_train_loss_dict_ref().items()}
        outs[fc] = (L, gan.G.state_dict()["hr_convs.2.weight"].clone())
        if fc:
            assert want > 0 and abs(L["feature_D"] - want) <= 2e-3 * want, (L["feature_D"], want)
            assert gan.feature_extractor is not None and not any(p.requires_grad for p in gan.feature_extractor.parameters())
        else:
            assert L["feature_D"] == 0.0
    (L0, w0), (L1, w1) = outs[False], outs[True]
    assert abs((L1["total"] - L1["feature_D"]) - L0["total"]) <= 1e-4 * abs(L0["total"])  # the other terms are unchanged
    assert not torch.equal(w0, w1)  # the feature loss reached the generator's update


def test_gan_train_step_bf16_noise_dropout_runs(hip):
    """bf16 compute with instance noise + Dropout3d + validation: finite losses, weights move."""
    gan, cfg = _gpu_gan("bf16", use_noise=True, dropout=0.1)
    LR, HR, Z, x, y = (t.to(DEV) for t in ogan.synthetic_batch(2, 16, 4, 4, seed=2001))
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=DEV), 1, 2)
    w0 = gan.G.state_dict()["hr_convs.2.weight"].clone()
    d0 = gan.D.state_dict()["classifier.2.weight"].clone()
    for it in (1, 2, 3, 4):
        gan.optimize_parameters(LR, HR, Z, it)
    gan.validation(LR, HR, Z, 4)
    for d in (gan.get_G_train_loss_dict_ref(), gan.get_G_val_loss_dict_ref(), gan.get_D_loss_dict_ref(),
              gan.get_metrics_dict_ref()):
        for k, v in d.items():
            assert np.isfinite(float(v)), k
    assert not torch.equal(w0, gan.G.state_dict()["hr_convs.2.weight"])
    assert not torch.equal(d0, gan.D.state_dict()["classifier.2.weight"])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_generator_stacks_are_callable_and_sliceable(hip, dt):
    """``G.model[:2](LR)``, ``G.model(LR)``, ``G.terrain_convs(Z)``, ``G.hr_convs[:-2](t)``, ``G.hr_convs[:-3](t)`` - what the
    reference's ``plot_data.get_feature_maps`` (plot_data.py:770-793) calls - run through the HIP program and equal the
    oracle's intermediate features; chained together with ``hr_convs[-1]`` they reproduce ``G(LR, Z)``."""
    import torch.nn.functional as F

    spec = onets.GSpec(in_channels=4, nf=16, n_rrdb=2, gc=8, tf=8, hr_kern=5, upscale=4)
    G, sd = build_G(spec, dt, 21, scale=0.5)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 6, 5, 4, seed=3)
    LRd, Zd = LR.to(DEV), Z.to(DEV)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    # oracle intermediates (reference Generator_3D_Resnet_ESRGAN.py:198-229)
    f = F.conv3d(LR, sd["model.0.0.weight"], None, 1, 1)
    t = f
    for r in range(spec.n_rrdb):
        t = onets.rrdb_forward(sd, f"model.1.module.{r}", t, spec)
    lr_feat = f + F.conv3d(t, sd[f"model.1.module.{spec.n_rrdb}.0.weight"], None, 1, 1)
    up_feat = onets.generator_trunk(sd, LR, spec)
    ter = onets.terrain_features(sd, Z, spec)
    pre = torch.cat((up_feat, ter), dim=1)
    act = F.leaky_relu(F.conv3d(pre, sd["hr_convs.0.0.weight"], None, 1, 2), spec.slope)
    with torch.no_grad():
        got_lr = G.model[:2](LRd)
        got_up = G.model(LRd)
        got_ter = G.terrain_convs(Zd)
        got_pre = torch.cat((got_up, got_ter), dim=1)
        got_act = G.hr_convs[:-2](got_pre)
        got_id = G.hr_convs[:-3](got_pre)
        sr = G.hr_convs[-1:](G.hr_convs[1:2](got_act))
        full = G(LRd, Zd)
    assert got_lr.shape == lr_feat.shape and rel_l2(got_lr, lr_feat) < tol
    assert got_up.shape == up_feat.shape and rel_l2(got_up, up_feat) < tol
    assert rel_l2(G.model[2:](got_lr), up_feat) < tol       # a slice that starts in the middle
    assert got_ter.shape == ter.shape and rel_l2(got_ter, ter) < tol
    assert rel_l2(got_act, act) < tol
    assert got_id is got_pre or torch.equal(got_id, got_pre)  # the empty slice is the identity, as for nn.Sequential
    assert rel_l2(sr, full) < (1e-5 if dt == torch.float32 else 2e-2)
    assert not got_lr.requires_grad and list(G.state_dict().keys()) == list(sd.keys())
    with pytest.raises(RuntimeError):
        G.model[:2](LR)  # CPU tensors: no fallback


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_generator_substacks_are_differentiable(hip, dt):
    """The reference's ``G.model`` / ``G.terrain_convs`` / ``G.hr_convs`` are plain ``nn.Sequential``s: a slice called with
    gradients enabled is differentiable (reference Generator_3D_Resnet_ESRGAN.py:220-229).  Here such a call runs layer by
    layer on the HIP conv kernels (layerwise.py): chained as the reference's forward chains them (:225-229) the slices
    reproduce ``G(LR, Z)``, and their gradients - parameters AND the input - equal the oracle's."""
    spec = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=8, hr_kern=5, upscale=4)
    G, sd = build_G(spec, dt, 23, scale=0.5)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 5, 4, 4, seed=6)
    LRd = LR.to(DEV).requires_grad_(True)
    Zd = Z.to(DEV)
    feat = G.model(LRd)
    assert feat.requires_grad and feat.is_cuda
    out = G.hr_convs(torch.cat((feat, G.terrain_convs(Zd)), dim=1))
    with torch.no_grad():
        fused = G(LRd.detach(), Zd)
    tol_o, tol_g = (2e-5, 2e-4) if dt == torch.float32 else (2e-2, 6e-2)
    assert out.shape == fused.shape and rel_l2(out, fused) < tol_o
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (out * gy.to(DEV)).sum().backward()
    # the oracle on the same inputs (fp32 on the CPU)
    for v in sd.values():
        v.requires_grad_(True)
    LRc = LR.clone().requires_grad_(True)
    ref = onets.generator_forward(sd, LRc, Z, spec)
    assert rel_l2(out, ref) < tol_o
    (ref * gy).sum().backward()
    truth = dict({k: v.grad for k, v in sd.items()}, LR=LRc.grad)
    got = dict({k: p.grad for k, p in G.named_parameters()}, LR=LRd.grad)
    if dt == torch.float32:
        lim = {k: tol_g for k in truth}
    else:  # per tensor: what a bf16-storage evaluation of the same graph shows on it (as in test_generator_bf16_vs_reference)
        sd2 = onets.deterministic_state(onets.g_param_shapes(spec), seed=23, scale=0.5)
        for v in sd2.values():
            v.requires_grad_(True)
        LR2 = LR.clone().requires_grad_(True)
        em = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=8, hr_kern=5, upscale=4, bf16_storage=True)
        (onets.generator_forward(sd2, LR2, Z, em) * gy).sum().backward()
        lim = _emulated_bf16_bounds(truth, dict({k: v.grad for k, v in sd2.items()}, LR=LR2.grad))
    bad = {k: (rel_l2(got[k], truth[k]), lim[k]) for k in truth if got[k] is None or not rel_l2(got[k], truth[k]) < lim[k]}
    assert not bad, bad
    # a slice in the middle, a frozen slice (no parameter gradients wanted: the fused stages run) and the no-grad form agree
    mid = G.model[1:2](G.model[:1](LRd))
    for p in G.parameters():
        p.requires_grad_(False)
    frozen = G.model[:2](LRd.detach())
    assert not frozen.requires_grad and rel_l2(mid, frozen) < tol_o


def test_dense_forward_grouped_by_produced_window(hip):
    """At large volumes the growth-channel part of a dense block's bf16 forward runs one 16-wide launch per produced
    window (engine.conv_dense; the grouping by source window was measured slower and removed).  Same arithmetic as the
    reference's RDB (torch_blocks.py:202-214, 278-290): the trunk stage of a generator with 16-channel growth at
    32 x 32 x 64 (>= 128 tiles of 512 voxels) against the oracle."""
    import torch.nn.functional as F

    spec = onets.GSpec(in_channels=4, nf=32, n_rrdb=1, gc=16, tf=8, hr_kern=5, upscale=4)
    G, sd = build_G(spec, torch.bfloat16, 29, scale=0.5)
    G.eval()
    g = torch.Generator().manual_seed(3)
    f = torch.randn((1, 32, 32, 32, 64), generator=g) * 0.5
    seen = []
    prog = G.program()
    prog.launch_probe = lambda tag, fn: (seen.append(tag.split(":")[0]), fn())[1]
    with torch.no_grad():
        out = G.model[1:2](f.to(DEV)).cpu()
    prog.launch_probe = None
    assert sum(t.startswith("fwd_dense_grow") for t in seen) == 3 * 3
    assert not any(t.startswith("fwd_dense_src") for t in seen)
    t = f
    t = onets.rrdb_forward(sd, "model.1.module.0", t, spec)
    ref = f + F.conv3d(t, sd["model.1.module.1.0.weight"], None, 1, 1)
    assert rel_l2(out, ref) < 2e-2


def test_full_size_generator_properties(hip):
    """Shipped-config G (34.77 M parameters) at 16x16x10 -> 64x64x10: linear response of the
    output to the last conv's bias, bf16 close to fp32, parameter gradients finite."""
    spec = onets.GSpec()
    outs = {}
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 16, 10, 4, seed=4)
    for dt in (torch.float32, torch.bfloat16):
        G, _ = build_G(spec, dt, 77, scale=0.3)
        G.eval()
        with torch.no_grad():
            a = G(LR.to(DEV), Z.to(DEV))
            G.hr_convs[2].bias += 1.0
            b = G(LR.to(DEV), Z.to(DEV))
        assert rel_l2(b - a, torch.ones_like(a)) < 1e-4
        outs[dt] = a
        if dt == torch.float32:
            G.train()
            G(LR.to(DEV), Z.to(DEV)).square().mean().backward()
            assert all(torch.isfinite(p.grad).all() for p in G.parameters())
            assert sum(float(p.grad.abs().sum()) > 0 for p in G.parameters()) == len(list(G.parameters()))
        del G
    assert rel_l2(outs[torch.bfloat16], outs[torch.float32]) < 3e-2


@pytest.mark.parametrize("nf,gc,n_rrdb", [(32, 16, 2), (128, 32, 1)])
def test_generator_bf16_stacked_dense_input_gradient(hip, monkeypatch, nf, gc, n_rrdb):
    """The dense blocks' input gradients grouped by produced window (one conv over the stacked output
    gradients per window, engine.dgrad_dense) against one launch per conv: both must sit at the bf16
    distance from the fp32 program (itself pinned to the reference above), and the stacked filters must
    be rebuilt after a parameter update."""
    from gan_sr_wind_field_amd import engine

    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=nf, n_rrdb=n_rrdb, hr_kern=5, gc=gc, tf=8)
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 8, 6, 4, seed=31)
    gy = torch.randn(1, 3, 32, 32, 6, generator=torch.Generator().manual_seed(3)).to(DEV)
    grads, tags = {}, {}
    for mode in ("fp32", "fp32_perconv", "stacked", "perconv"):
        monkeypatch.setattr(engine, "STACK_DGRAD", not mode.endswith("perconv"))
        G, _ = build_G(spec, torch.float32 if mode.startswith("fp32") else torch.bfloat16, 21)
        G.eval()
        seen = []
        G.program().launch_probe = lambda tag, fn: (seen.append(tag.split(":")[0]), fn())
        (G(LR.to(DEV), Z.to(DEV)) * gy).sum().backward()
        grads[mode] = {k: p.grad.clone() for k, p in G.named_parameters()}
        tags[mode] = list(seen)
        if mode == "stacked":  # second step with changed filters: stale stacked copies would show here
            with torch.no_grad():
                for p in G.parameters():
                    p.mul_(1.25)
            G.zero_grad()
            (G(LR.to(DEV), Z.to(DEV)) * gy).sum().backward()
            g2 = {k: p.grad.clone() for k, p in G.named_parameters()}
            monkeypatch.setattr(engine, "STACK_DGRAD", False)
            G.zero_grad()
            (G(LR.to(DEV), Z.to(DEV)) * gy).sum().backward()
            for k, p in G.named_parameters():
                assert rel_l2(g2[k], p.grad) < 3e-2, k
    n_rdb = 3 * n_rrdb
    assert sum(t.startswith("dgrad_dense") for t in tags["stacked"]) == 4 * n_rdb
    assert sum(t.startswith("dgrad_dense") for t in tags["fp32"]) == 4 * n_rdb  # (fp32 tile kernels stack as well)
    assert not any(t.startswith("dgrad_dense") for t in tags["perconv"] + tags["fp32_perconv"])
    for k in grads["fp32"]:  # fp32: the two groupings differ by summation order only
        assert rel_l2(grads["fp32"][k], grads["fp32_perconv"][k]) < 1e-4, k
    for k in grads["fp32"]:
        e_s, e_p = rel_l2(grads["stacked"][k], grads["fp32"][k]), rel_l2(grads["perconv"][k], grads["fp32"][k])
        assert e_s < max(1.5 * e_p, 2e-2), (k, e_s, e_p)


def test_generator_bf16_zfolded_last_conv(hip, monkeypatch):
    """hr_convs.2 (144 -> 3, 5x5x5) as a (5,5,1) conv with 15 outputs + z-fold against the plain kernel:
    same outputs and gradients up to the bf16 rounding of the operands (the partial sums stay fp32)."""
    from gan_sr_wind_field_amd import engine

    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=16, n_rrdb=1, hr_kern=5, gc=8, tf=8)
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 6, 5, 4, seed=12)
    gy = torch.randn(2, 3, 24, 24, 5, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for zf in (True, "stated", False):
        monkeypatch.setattr(engine, "ZFOLD", bool(zf))
        # (the folded conv's filter gradient: operands' roles exchanged by default, "stated": x the halo image)
        monkeypatch.setattr(engine, "SWAP_THIN_WGRAD", zf is True)
        G, _ = build_G(spec, torch.bfloat16, 33)
        G.eval()
        seen = []
        G.program().launch_probe = lambda tag, fn: (seen.append(tag), fn())
        out = G(LR.to(DEV), Z.to(DEV))
        (out * gy).sum().backward()
        assert any("zfold" in t for t in seen) == bool(zf)
        assert ("wgrad:hr_convs.2.zfold.T" in seen) == (zf is True)
        res[zf] = (out.detach(), {k: p.grad.clone() for k, p in G.named_parameters()})
        if zf is True:  # the folded filter follows a parameter update
            with torch.no_grad():
                G.hr_convs[2].weight.mul_(2.0)
            assert rel_l2(G(LR.to(DEV), Z.to(DEV)) - G.hr_convs[2].bias.view(1, 3, 1, 1, 1),
                          2.0 * (out.detach() - G.hr_convs[2].bias.view(1, 3, 1, 1, 1))) < 1e-5
    assert rel_l2(res[True][0], res[False][0]) < 1e-5
    for k in res[True][1]:
        assert rel_l2(res[True][1][k], res[False][1][k]) < 2e-2, k
    # exchanged vs stated: the same bf16 products, another summation order
    assert rel_l2(res[True][1]["hr_convs.2.weight"], res["stated"][1]["hr_convs.2.weight"]) < 1e-5


@pytest.mark.parametrize("nf,gc,n_rrdb", [(32, 16, 1), (128, 32, 1)])
def test_generator_bf16_split_dense_forward(hip, monkeypatch, nf, gc, n_rrdb):
    """Growth convs of a dense block as one conv over the block input + narrow second stages
    (engine.conv_dense) against one launch per conv: outputs and gradients at the bf16 distance from the
    fp32 program, and the stacked filters follow a parameter update."""
    from gan_sr_wind_field_amd import engine

    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=nf, n_rrdb=n_rrdb, hr_kern=5, gc=gc, tf=8)
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 8, 6, 4, seed=41)
    gy = torch.randn(1, 3, 32, 32, 6, generator=torch.Generator().manual_seed(6)).to(DEV)
    res, tags = {}, {}
    for mode in ("fp32", "fp32_perconv", "split", "perconv"):
        monkeypatch.setattr(engine, "STACK_FWD", not mode.endswith("perconv"))
        G, _ = build_G(spec, torch.float32 if mode.startswith("fp32") else torch.bfloat16, 27)
        G.eval()
        seen = []
        G.program().launch_probe = lambda tag, fn: (seen.append(tag.split(":")[0]), fn())
        out = G(LR.to(DEV), Z.to(DEV))
        (out * gy).sum().backward()
        tags[mode] = list(seen)
        res[mode] = (out.detach(), {k: p.grad.clone() for k, p in G.named_parameters()})
        if mode == "split":
            with torch.no_grad():
                for p in G.parameters():
                    p.mul_(0.8)
            o2 = G(LR.to(DEV), Z.to(DEV)).detach()
            monkeypatch.setattr(engine, "STACK_FWD", False)
            assert rel_l2(o2, G(LR.to(DEV), Z.to(DEV)).detach()) < 2e-2
    n_rdb = 3 * n_rrdb
    assert sum(t == "fwd_dense_pre" for t in tags["split"]) == n_rdb
    assert sum(t.startswith("fwd_dense_grow") for t in tags["split"]) == 3 * n_rdb
    assert sum(t == "fwd_dense_pre" for t in tags["fp32"]) == n_rdb  # (the fp32 tile kernels split as well)
    assert not any(t.startswith("fwd_dense") for t in tags["perconv"] + tags["fp32_perconv"])
    # fp32: the split form differs by summation order only (the partial sums stay in fp32): outputs to 2e-5; the
    # gradients of the first layers see the few LeakyReLU branches that the last bit flips (measured 1.2e-3 on the
    # feature conv at nf = 128 with these 0.7-scale weights; the reference's own fp32 sits up to 9e-4 from fp64 there)
    assert rel_l2(res["fp32"][0], res["fp32_perconv"][0]) < 2e-5
    for k in res["fp32"][1]:
        assert rel_l2(res["fp32"][1][k], res["fp32_perconv"][1][k]) < 5e-3, k
    e_s, e_p = rel_l2(res["split"][0], res["fp32"][0]), rel_l2(res["perconv"][0], res["fp32"][0])
    assert e_s < max(1.5 * e_p, 1e-2), (e_s, e_p)
    for k in res["fp32"][1]:
        e_s = rel_l2(res["split"][1][k], res["fp32"][1][k])
        e_p = rel_l2(res["perconv"][1][k], res["fp32"][1][k])
        assert e_s < max(1.5 * e_p, 2e-2), (k, e_s, e_p)


def test_generator_bf16_inplace_block_gradient(hip, monkeypatch):
    """Running block-output gradient kept in channels [0, nf) of the dense gradient buffer (LFF input
    gradient in place, partial accumulation) against the separate-tensor form."""
    from gan_sr_wind_field_amd import engine

    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=128, n_rrdb=2, hr_kern=5, gc=32, tf=8)
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 8, 6, 4, seed=51)
    gy = torch.randn(1, 3, 32, 32, 6, generator=torch.Generator().manual_seed(8)).to(DEV)
    grads = {}
    for inplace in (True, False):
        monkeypatch.setattr(engine, "GD_INPLACE", inplace)
        G, _ = build_G(spec, torch.bfloat16, 29)
        G.eval()
        (G(LR.to(DEV), Z.to(DEV)) * gy).sum().backward()
        grads[inplace] = {k: p.grad.clone() for k, p in G.named_parameters()}
    for k in grads[True]:
        assert torch.isfinite(grads[True][k]).all(), k
        assert rel_l2(grads[True][k], grads[False][k]) < 2e-2, k


def test_full_size_c3_generator_properties(hip, monkeypatch):
    """BASELINE's headline size (LR 32x32x128 -> HR 128^3, full 34.77 M-parameter G, bf16): size-independent
    properties - the output is linear in the last conv's bias, the forward pass is deterministic, the split /
    stacked dense-block forms agree with the per-conv forms, and all parameter gradients are finite, non-zero."""
    from gan_sr_wind_field_amd import engine

    spec = onets.GSpec()
    G, _ = build_G(spec, torch.bfloat16, 78, scale=0.3)
    G.eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(1, 32, 128, 4, seed=14)
    LR, Z = LR.to(DEV), Z.to(DEV)
    with torch.no_grad():
        a = G(LR, Z)
        assert a.shape == (1, 3, 128, 128, 128)
        assert torch.equal(a, G(LR, Z))
        G.hr_convs[2].bias += 0.5
        b = G(LR, Z)
        G.hr_convs[2].bias -= 0.5
        assert rel_l2(b - a, torch.full_like(a, 0.5)) < 1e-4
        monkeypatch.setattr(engine, "STACK_FWD", False)
        monkeypatch.setattr(engine, "ZFOLD", False)
        c = G(LR, Z)
        assert rel_l2(c, a) < 2e-2
    monkeypatch.setattr(engine, "STACK_FWD", True)
    monkeypatch.setattr(engine, "ZFOLD", True)
    G.train()
    torch.manual_seed(321)
    G(LR, Z).square().mean().backward()
    g1 = {k: p.grad.clone() for k, p in G.named_parameters()}
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert all(float(v.abs().sum()) > 0 for v in g1.values())
    # bit-reproducible backward at the benchmark's size (no float atomics anywhere on the path)
    G.zero_grad()
    torch.manual_seed(321)
    G(LR, Z).square().mean().backward()
    assert all(torch.equal(p.grad, g1[k]) for k, p in G.named_parameters())
    # the stacked / in-place backward forms against one launch per conv, same dropout mask (seeded)
    for flag in ("STACK_DGRAD", "GD_INPLACE", "ZFOLD"):
        monkeypatch.setattr(engine, flag, False)
    G.zero_grad()
    torch.manual_seed(123)
    out_ref = G(LR, Z)
    out_ref.square().mean().backward()
    g_ref = {k: p.grad.clone() for k, p in G.named_parameters()}
    for flag in ("STACK_DGRAD", "GD_INPLACE", "ZFOLD"):
        monkeypatch.setattr(engine, flag, True)
    G.zero_grad()
    torch.manual_seed(123)
    G(LR, Z).square().mean().backward()
    worst = max(rel_l2(p.grad, g_ref[k]) for k, p in G.named_parameters())
    assert worst < 6e-2, worst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_backward_is_bit_reproducible(hip, dtype):
    """Filter gradients without float atomics (engine.DETERMINISTIC: split copies + ordered sum), two-pass
    BatchNorm / bias reductions: two backward passes over the same inputs give bit-identical gradients, for the
    generator (stacked dense-block launches, z-folded last conv) and the discriminator (strided convs, train-mode
    BatchNorm), on the tile kernels (bf16) and the generic ones (fp32)."""
    from gan_sr_wind_field_amd import engine

    assert engine.DETERMINISTIC
    spec = onets.GSpec(upscale=4, in_channels=4, out_channels=3, nf=32, n_rrdb=1, hr_kern=5, gc=16, tf=8)
    G, _ = build_G(spec, dtype, 3)
    G.train()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 8, 16, 4, seed=13)
    LR, Z = LR.to(DEV), Z.to(DEV)
    runs = []
    for _ in range(2):
        G.zero_grad(set_to_none=True)
        torch.manual_seed(5)  # same Dropout3d mask
        G(LR, Z).square().mean().backward()
        runs.append({k: p.grad.clone() for k, p in G.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    ds = onets.DSpec(bf=8, nz=16, enable_slicing=True)
    D, _ = build_D(ds, dtype, 4)
    D.train()
    xin = (torch.rand((2, 3, 64, 64, 16), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    runs = []
    for _ in range(2):
        D.zero_grad(set_to_none=True)
        xg = xin.clone().requires_grad_(True)
        D(xg).sum().backward()
        runs.append(dict({k: p.grad.clone() for k, p in D.named_parameters()}, x=xg.grad.clone()))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_full_size_c3_discriminator_properties(hip, monkeypatch):
    """Full-size D (bf 32) on 128^3 inputs, bf16: eval-mode logits are deterministic and agree between the
    strided convs on the tile kernel and on the generic kernel; train-mode input and parameter gradients are
    finite and non-zero."""
    spec = onets.DSpec(bf=32, nz=128)
    D, _ = build_D(spec, torch.bfloat16, 91)
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand((1, 3, 128, 128, 128), generator=gen) * 2 - 1).to(DEV)
    D.eval()
    with torch.no_grad():
        a = D(x)
        assert a.shape == (1, 1) and torch.isfinite(a).all()
        assert torch.equal(a, D(x))
        monkeypatch.setenv("WSR_CT_NOSTRIDE", "1")  # strided convs back on the generic implicit GEMM
        reload_wsr_env()
        b = D(x)
        monkeypatch.delenv("WSR_CT_NOSTRIDE")
        reload_wsr_env()
        assert abs(float(a - b)) < 2e-2 * max(1.0, abs(float(a)))
    D.train()
    xg = x.clone().requires_grad_(True)
    D(xg).sum().backward()
    assert torch.isfinite(xg.grad).all() and float(xg.grad.abs().sum()) > 0
    assert all(torch.isfinite(p.grad).all() for p in D.parameters())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["lff3", "convs3", "hr3", "relu", "scales"])
def test_generator_constructor_variants_vs_oracle(hip, dt, variant):
    """Constructor arguments of Generator_3D the shipped configurations leave at their values (reference
    Generator_3D_Resnet_ESRGAN.py:24-46, torch_blocks.py:270-330): a 3x3x3 local-feature-fusion conv
    (``lff_kern_size=3``), three growth convs per dense block, a 3x3x3 HR conv pair, ReLU (``act_type='relu'``: slope 0)
    and other residual scalings - forward and all parameter gradients against the oracle's functional generator.
    fp32: 2e-5 / 2e-4 as for the shipped shapes; bf16: the storage format's distance (5e-2 outputs, per-tensor bounds
    from the oracle's bf16-storage emulation for the gradients)."""
    from gan_sr_wind_field_amd.CNN_models.Generator_3D_Resnet_ESRGAN import Generator_3D

    kw = dict(upscale=4, in_channels=4, out_channels=3, nf=16, n_rrdb=1, hr_kern=5, gc=8, tf=8, n_rdb_convs=5)
    kw.update({"lff3": dict(lff_kern=3), "convs3": dict(n_rdb_convs=3), "hr3": dict(hr_kern=3), "relu": dict(slope=0.0),
               "scales": dict(rdb_scale=0.5, rrdb_scale=1.0)}[variant])
    spec = onets.GSpec(**kw)
    G = Generator_3D(spec.in_channels, spec.out_channels, spec.nf, spec.n_rrdb, upscale=spec.upscale,
                     hr_kern_size=spec.hr_kern, number_of_RDB_convs=spec.n_rdb_convs, RDB_gc=spec.gc,
                     lff_kern_size=spec.lff_kern, RDB_residual_scaling=spec.rdb_scale,
                     RRDB_residual_scaling=spec.rrdb_scale, act_type="relu" if spec.slope == 0.0 else "leakyrelu",
                     terrain_number_of_features=spec.tf, dropout_probability=0.0, use_mixed_precision=dt == torch.bfloat16)
    sd = onets.deterministic_state(onets.g_param_shapes(spec), seed=61, scale=0.7)
    assert set(sd) == set(G.state_dict())
    G.load_state_dict(sd)
    G = G.to(DEV).eval()
    LR, HR, Z, x, y = ogan.synthetic_batch(2, 6, 5, 4, seed=13)
    gy = torch.randn(2, 3, 24, 24, 5, generator=torch.Generator().manual_seed(3))

    def oracle(s):
        ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        o = onets.generator_forward(ref, LR, Z, s)
        (o * gy).sum().backward()
        return o.detach(), {k: v.grad for k, v in ref.items()}

    want, gw = oracle(spec)
    out = G(LR.to(DEV), Z.to(DEV))
    (out * gy.to(DEV)).sum().backward()
    got = {k: p.grad for k, p in G.named_parameters()}
    if dt == torch.float32:
        assert rel_l2(out, want) < 2e-5
        for k in gw:
            assert rel_l2(got[k], gw[k]) < 2e-4, k
    else:
        em_spec = onets.GSpec(**{**kw, "bf16_storage": True})
        _, ge = oracle(em_spec)
        assert rel_l2(out, want) < 5e-2
        lim = _emulated_bf16_bounds(gw, ge)
        for k in gw:
            assert rel_l2(got[k], gw[k]) < lim[k], (k, lim[k])


@pytest.mark.parametrize("variant", ["relu"])
def test_discriminator_constructor_variants_vs_oracle(hip, variant):
    """Discriminator_3D with ReLU (``act_type='relu'``, reference Discriminator_3D.py:23-38), fp32, train mode (a 5-tap
    feature kernel shrinks z by two levels per down-sampling conv in the reference and needs its own depths: not a
    variant of these shapes): logits, parameter gradients and the input gradient against the oracle's functional
    discriminator (fp64 for the gradients: train-mode BatchNorm at batch 2, see test_discriminator_fp32_vs_reference)."""
    from gan_sr_wind_field_amd.CNN_models.Discriminator_3D import Discriminator_3D

    kw = dict(bf=4, nz=4, enable_slicing=True)
    kw.update({"relu": dict(slope=0.0)}[variant])
    spec = onets.DSpec(**kw)
    D = Discriminator_3D(spec.in_channels, spec.bf, feat_kern_size=spec.feat_kern, number_of_z_layers=spec.nz,
                         enable_slicing=True, dropout_probability=0.0, use_mixed_precision=False,
                         act_type="relu" if spec.slope == 0.0 else "leakyrelu")
    sd = onets.deterministic_state(onets.d_param_shapes(spec), seed=71, scale=1.0)
    assert set(sd) == set(D.state_dict())
    D.load_state_dict(sd)
    D = D.to(DEV).train()
    x = (torch.rand((2, 3, 64, 64, spec.nz), generator=torch.Generator().manual_seed(17)) * 2 - 1)
    wgt = torch.tensor([[1.0], [-0.5]])
    ref = {k: (v.double().clone().requires_grad_("running_" not in k) if v.is_floating_point() else v.clone())
           for k, v in sd.items()}
    xr = x.double().clone().requires_grad_(True)
    want = onets.discriminator_forward(ref, xr, spec, training=True)
    (want * wgt.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = D(xd)
    (out * wgt.to(DEV)).sum().backward()
    assert rel_l2(out, want.detach().float()) < 2e-5
    assert rel_l2(xd.grad.cpu().double(), xr.grad) < 5e-3
    for k, p in D.named_parameters():
        assert rel_l2(p.grad.cpu().double(), ref[k].grad) < 5e-3, k
