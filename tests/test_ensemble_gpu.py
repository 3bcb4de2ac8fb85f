"""[ENSEMBLE] on the GPU: the two kernels of csrc/ensemble.hip against the CPU rules of tests/test_ensemble.py, their
assembly in ``ensemble.self_ensemble``, ``wind_field_GAN_3D.G_ensemble`` against eight separate generator calls, and
``run.py --train --test`` without the section, with ``members = 8`` and with ``members = 1``.  Outputs of the kernels go in
``Guarded`` buffers.

Bounds (kernel_bounds.py's convention, LAMBDA = 16 untouched).

* ``wsr_dihedral_members``: ``torch.equal`` with the CPU rules - the kernel only moves values and flips sign bits.
* ``wsr_ensemble_reduce``, mean: ``torch.equal`` with the same pairwise tree evaluated in fp32 on the CPU after the CPU
  inverse maps (IEEE additions in the same order, one exact product with 1 / K).  K identical members: the member back,
  bit for bit, and a variance of exactly zero.
* ``wsr_ensemble_reduce``, variance: per element ``LAMBDA * sqrt(K + 2) * 2^-24 * A_v + 2^-100`` against float64, with
  ``A_v = sum (|m_k| + |mean|)^2 / K``: K squares and their tree, plus the roundings of the mean and of the final product.
  The members are a common field plus noise of relative size 1 and 1e-3 (the second: the cancellation in m_k - mean).
  The fp32 tree evaluated on the CPU sits at 0.078 of this bound.
* generator: rel-L2 <= 2e-5 (the fp32 output tolerance) against eight separate ``gan.G`` calls on
  CPU-transformed inputs, CPU inverse maps and the fp32 tree: a batch of 16 may take other tile shapes than a batch of 2,
  so this one is not bit-equality.

Measured on an MI355X when the kernels were written: worst |err| / bound of the variance 0.085; ``G_ensemble`` against the
eight separate calls rel-L2 0 (at this shape the batch of 16 takes the tiles of the batch of 2); the whole file ran in
9.9 s, 8.2 s of it the end-to-end test.
"""
import csv
import math
import os
import pickle
import time

import numpy as np
import pytest
import torch

from kernel_bounds import LAMBDA, U_FP32, Guarded, assert_guards_intact, assert_within
from test_ensemble import TABLE, cpu_forward, cpu_inverse, tree

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()

# (B, C, X, Y, NZ): NZ 5 / 6 / 8 -> pieces of 1 / 2 / 4 floats; 24 x 24 x 8: more pieces in a plane than one workgroup
# moves; 6 x 10: a non-square domain (member sets without quarter turns by an odd count); B 1 and 3; C 3, 4 and 6
SHAPES = [(1, 3, 8, 8, 5), (3, 4, 8, 8, 6), (1, 6, 8, 8, 8), (3, 3, 24, 24, 8), (3, 4, 6, 10, 6)]


def _sets(shape):
    return (1, 2, 4, 8) if shape[2] == shape[3] else (1, 2, 4)


CASES = [(sh, m) for sh in SHAPES for m in _sets(sh)]
CASE_IDS = ["x".join(map(str, sh)) + f"-m{m}" for sh, m in CASES]


def _codes(members):
    from gan_sr_wind_field_amd.ensemble import member_codes

    codes = member_codes(members)
    assert codes == [k + 4 * fx for k, fx in TABLE[members]]
    return codes


def _carr(codes):
    import ctypes

    return (ctypes.c_int32 * len(codes))(*codes)


def _field(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ wsr_dihedral_members
@pytest.mark.parametrize("shape,members", CASES, ids=CASE_IDS)
def test_dihedral_members_equal_the_cpu_rules(hip, shape, members):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, C, X, Y, NZ = shape
    codes = _codes(members)
    x = _field(shape, 7 + NZ + members)
    for is_vector, src in ((1, x), (0, x[:, 2:3].contiguous())):  # the wind field, and one scalar channel (C = 1)
        Cs = src.shape[1]
        out = Guarded((members, B, Cs, X, Y, NZ), torch.float32, DEV)  # (odd k only for X == Y)
        src_d = src.to(DEV)
        check(hip.wsr_dihedral_members(hip_ops._p(src_d), B, Cs, X, Y, NZ, _carr(codes), members, is_vector,
                                       hip_ops._p(out.t), hip_ops._stream()))
        torch.cuda.synchronize()
        assert_guards_intact(out, label=f"dihedral_members {shape} {members}")
        got = out.t.cpu()
        for m, code in enumerate(codes):
            want = cpu_forward(src, code, is_vector=bool(is_vector))
            assert torch.equal(got[m], want), (shape, members, code, is_vector)
            assert got[m].view(torch.int32).equal(want.contiguous().view(torch.int32)), (code, "sign of zero / bits")
        assert torch.equal(hip_ops.dihedral_members(src_d, codes, bool(is_vector)), out.t)  # the wrapper: same launch


def test_dihedral_members_refuse_quarter_turns_on_a_non_square_domain(hip):
    from gan_sr_wind_field_amd import hip_ops

    B, C, X, Y, NZ = 3, 4, 6, 10, 6
    src_d = _field((B, C, X, Y, NZ), 3).to(DEV)
    for codes in ([1], [0, 3], [0, 2, 4, 5]):
        out = Guarded((len(codes), B, C, X, Y, NZ), torch.float32, DEV)
        before = out.base.view(torch.int32).clone()
        rc = hip.wsr_dihedral_members(hip_ops._p(src_d), B, C, X, Y, NZ, _carr(codes), len(codes), 1, hip_ops._p(out.t),
                                      hip_ops._stream())
        torch.cuda.synchronize()
        assert rc == -1, (codes, rc)  # WSR_EINVAL
        assert torch.equal(out.base.view(torch.int32), before), codes  # nothing written
        with pytest.raises(ValueError, match="X = 6, Y = 10"):
            hip_ops.dihedral_members(src_d, codes, True)
    mem = torch.zeros((1, B, 3, X, Y, NZ), device=DEV)
    mean = Guarded((B, 3, X, Y, NZ), torch.float32, DEV)
    before = mean.base.view(torch.int32).clone()
    assert hip.wsr_ensemble_reduce(hip_ops._p(mem), _carr([3]), 1, B, X, Y, NZ, hip_ops._p(mean.t), None,
                                   hip_ops._stream()) == -1
    assert hip.wsr_ensemble_reduce(hip_ops._p(mem), _carr([0, 2, 4]), 3, B, X, Y, NZ, hip_ops._p(mean.t), None,
                                   hip_ops._stream()) == -1  # K = 3
    torch.cuda.synchronize()
    assert torch.equal(mean.base.view(torch.int32), before)
    for bad in ([], [0, 2, 4], [8], [-1], list(range(8)) * 2):
        with pytest.raises(ValueError):
            hip_ops.dihedral_members(torch.zeros((1, 3, 4, 4, 4), device=DEV), bad, True)
    with pytest.raises(ValueError):
        hip_ops.dihedral_members(torch.zeros((1, 1, 4, 4, 4), device=DEV), [0], True)  # a vector field has u and v
    with pytest.raises(ValueError):
        hip_ops.dihedral_members(torch.zeros((1, 3, 4, 4, 4), device=DEV)[:, :, ::2], [0], True)  # not contiguous
    with pytest.raises(ValueError):
        hip_ops.dihedral_members(torch.zeros((1, 3, 4, 4, 4), device=DEV, dtype=torch.float64), [0], True)
    with pytest.raises(ValueError):
        hip_ops.ensemble_reduce(torch.zeros((2, 1, 3, 4, 4, 4), device=DEV), [0])  # one code for two members
    with pytest.raises(ValueError):
        hip_ops.ensemble_reduce(torch.zeros((1, 1, 4, 4, 4, 4), device=DEV), [0])  # three components


# ------------------------------------------------------------------------------------------------- wsr_ensemble_reduce
def _reduce(hip, mem_d, codes, with_var, label):
    """the raw entry point into Guarded buffers -> (mean, var or None) on the device, guards checked"""
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    K, B, _, X, Y, NZ = mem_d.shape
    mean = Guarded((B, 3, X, Y, NZ), torch.float32, DEV)
    var = Guarded((B, 3, X, Y, NZ), torch.float32, DEV) if with_var else None
    check(hip.wsr_ensemble_reduce(hip_ops._p(mem_d), _carr(codes), K, B, X, Y, NZ, hip_ops._p(mean.t),
                                  hip_ops._p(var.t) if with_var else None, hip_ops._stream()))
    torch.cuda.synchronize()
    assert_guards_intact(*([mean, var] if with_var else [mean]), label=label)
    return mean.t, (var.t if with_var else None)


_RANDOM = {}


def _random_members(shape, members, noise):
    """independent members (K, B, 3, X', Y', NZ): a common field + noise of relative size ``noise``, each in its
    member's frame; with the CPU inverse maps, the fp32 tree mean and the float64 mean / variance / A_v.  Computed
    once per case and shared (never modified)."""
    key = (shape, members, noise)
    if key not in _RANDOM:
        B, _, X, Y, NZ = shape
        codes = _codes(members)
        gen = torch.Generator().manual_seed(101 + NZ + members)
        common = torch.randn((B, 3, X, Y, NZ), generator=gen)
        mem = torch.stack([cpu_forward(common + noise * torch.randn((B, 3, X, Y, NZ), generator=gen), c) for c in codes])
        back = [cpu_inverse(mem[m], c) for m, c in enumerate(codes)]
        mean32 = tree(back) * torch.tensor(1.0 / members)
        b64 = torch.stack(back).double()
        mean64 = b64.mean(0)
        var64 = ((b64 - mean64) ** 2).mean(0)
        A_v = ((b64.abs() + mean64.abs()) ** 2).mean(0)
        _RANDOM[key] = (codes, mem.contiguous(), back, mean32, var64, A_v)
    return _RANDOM[key]


@pytest.mark.parametrize("shape,members", CASES, ids=CASE_IDS)
def test_reduce_identity_gives_the_field_back_and_zero_variance(hip, shape, members):
    from gan_sr_wind_field_amd import hip_ops

    B, _, X, Y, NZ = shape
    codes = _codes(members)
    field = _field((B, 3, X, Y, NZ), 31 + NZ)
    field_d = field.to(DEV)
    mem_d = hip_ops.dihedral_members(field_d, codes, True)
    mean, var = _reduce(hip, mem_d, codes, True, f"reduce identity {shape} {members}")
    assert mean.view(torch.int32).equal(field_d.view(torch.int32)), (shape, members)
    assert bool((var == 0).all()), (shape, members)


@pytest.mark.parametrize("shape,members", CASES, ids=CASE_IDS)
def test_reduce_mean_equals_the_cpu_tree(hip, shape, members):
    codes, mem, _, mean32, _, _ = _random_members(shape, members, 1.0)
    mean, _ = _reduce(hip, mem.to(DEV), codes, False, f"reduce mean {shape} {members}")
    assert torch.equal(mean.cpu(), mean32), (shape, members)


@pytest.mark.parametrize("noise", [1.0, 1e-3], ids=["noise1", "noise1e-3"])
@pytest.mark.parametrize("shape,members", CASES, ids=CASE_IDS)
def test_reduce_variance_within_the_bound_of_float64(hip, shape, members, noise):
    codes, mem, _, mean32, var64, A_v = _random_members(shape, members, noise)
    mean, var = _reduce(hip, mem.to(DEV), codes, True, f"reduce var {shape} {members}")
    assert torch.equal(mean.cpu(), mean32), (shape, members)
    bnd = LAMBDA * math.sqrt(members + 2) * U_FP32 * A_v + 2.0 ** -100
    assert_within(var, var64, bnd, f"ensemble variance vs float64[{shape} K={members} noise={noise}]")
    assert bool((var >= 0).all())
    if members == 1:
        assert bool((var == 0).all())


@pytest.mark.parametrize("shape,members", CASES, ids=CASE_IDS)
def test_reduce_is_reproducible_and_a_null_var_leaves_the_mean(hip, shape, members):
    from gan_sr_wind_field_amd import hip_ops

    codes, mem, _, _, _, _ = _random_members(shape, members, 1.0)
    mem_d = mem.to(DEV)
    m1, v1 = _reduce(hip, mem_d, codes, True, "first call")
    m2, v2 = _reduce(hip, mem_d, codes, True, "second call")
    assert m1.view(torch.int32).equal(m2.view(torch.int32)) and v1.view(torch.int32).equal(v2.view(torch.int32))
    m3, none = _reduce(hip, mem_d, codes, False, "var = NULL")
    assert none is None and m3.view(torch.int32).equal(m1.view(torch.int32))
    # the wrapper: same launches
    assert torch.equal(hip_ops.ensemble_reduce(mem_d, codes), m1)
    wm, wv = hip_ops.ensemble_reduce(mem_d, codes, with_var=True)
    assert torch.equal(wm, m1) and torch.equal(wv, v1)


# ---------------------------------------------------------------------------------------------------------- assembly
@pytest.mark.parametrize("shape,members", [((2, 4, 8, 8, 5), 1), ((2, 4, 8, 8, 5), 2), ((2, 4, 8, 8, 5), 4),
                                           ((2, 4, 8, 8, 5), 8), ((3, 5, 6, 6, 8), 8), ((1, 4, 3, 5, 6), 4)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"m{v}")
def test_self_ensemble_of_an_equivariant_function_is_the_function(hip, shape, members):
    """nearest x4 up-sampling in x and y of LR[:, :3] commutes with every member exactly: the ensemble must give the
    plain result bit for bit - an LR-resolution map applied at HR resolution (or the reverse), a wrong inverse or a
    wrong member order does not"""
    from gan_sr_wind_field_amd.ensemble import self_ensemble

    B, C, Xl, Yl, NZ = shape
    s = 4
    calls = []

    def fn(lr, z):
        calls.append((tuple(lr.shape), tuple(z.shape)))
        return lr[:, :3].repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)

    LR = _field(shape, 17 + members).to(DEV)
    Z = _field((B, 1, Xl * s, Yl * s, NZ), 19).to(DEV)
    mean, var = self_ensemble(fn, LR, Z, members=members, with_var=True)
    assert calls == [((members * B, C, Xl, Yl, NZ), (members * B, 1, Xl * s, Yl * s, NZ))]  # once, with batch K * B
    want = LR[:, :3].repeat_interleave(s, dim=2).repeat_interleave(s, dim=3).contiguous()
    assert mean.view(torch.int32).equal(want.view(torch.int32)), (shape, members)
    assert bool((var == 0).all())
    only = self_ensemble(fn, LR, Z, members=members)
    assert torch.is_tensor(only) and torch.equal(only, mean)


def test_self_ensemble_hands_the_terrain_over_in_each_members_frame(hip):
    """fn sees, for member m of sample b, LR and Z transformed by THAT member (Z as a scalar: never negated)"""
    from gan_sr_wind_field_amd.ensemble import self_ensemble

    B, s = 2, 4
    LR, Z = _field((B, 4, 4, 4, 6), 23), _field((B, 1, 16, 16, 6), 29)
    seen = {}

    def fn(lr, z):
        seen["lr"], seen["z"] = lr.cpu(), z.cpu()
        return torch.zeros((lr.shape[0], 3, lr.shape[2] * s, lr.shape[3] * s, lr.shape[4]), device=lr.device)

    self_ensemble(fn, LR.to(DEV), Z.to(DEV), members=8)
    for m, code in enumerate(_codes(8)):
        assert torch.equal(seen["lr"][m * B:(m + 1) * B], cpu_forward(LR, code)), code
        assert torch.equal(seen["z"][m * B:(m + 1) * B], cpu_forward(Z, code, is_vector=False)), code
    with pytest.raises(ValueError, match="X = 4, Y = 6"):
        self_ensemble(fn, torch.zeros((1, 4, 4, 6, 5), device=DEV), torch.zeros((1, 1, 16, 24, 5), device=DEV), members=8)


# --------------------------------------------------------------------------------------------------------- generator
def _gan(nz=5, ensemble_members=None):
    import gan_sr_wind_field_amd
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from oracle import nets as onets

    ini = os.path.join(os.path.dirname(gan_sr_wind_field_amd.__file__), "config", "wind_field_GAN_3D_config_local.ini")
    cfg = Config(ini)
    cfg.is_train, cfg.is_test, cfg.is_use = False, True, False
    cfg.gpu_id, cfg.device = 0, DEV
    cfg.compute_dtype = "fp32"
    cfg.generator.num_features, cfg.generator.num_RRDB, cfg.generator.RDB_growth_chan = 16, 1, 8
    cfg.generator.terrain_number_of_features = 4
    cfg.generator.dropout_probability = 0.0
    cfg.gan_config.number_of_z_layers = nz
    if ensemble_members is not None:
        cfg.ensemble.present, cfg.ensemble.members = True, ensemble_members
    torch.manual_seed(2001)
    gan = wind_field_GAN_3D(cfg)
    gs = onets.GSpec(in_channels=4, nf=16, n_rrdb=1, gc=8, tf=4, hr_kern=5, upscale=4)
    gan.G.load_state_dict(onets.deterministic_state(onets.g_param_shapes(gs), seed=41, scale=0.5))
    return gan, cfg


def test_G_ensemble_against_eight_separate_generator_calls(hip):
    from conftest import rel_l2
    from gan_sr_wind_field_amd.config.config import Config
    from oracle import gan as ogan

    try:
        gan, cfg = _gan(nz=5, ensemble_members=8)
        LR, _, Z, _, _ = ogan.synthetic_batch(2, 8, 5, 4, seed=2001)
        assert tuple(LR.shape) == (2, 4, 8, 8, 5) and tuple(Z.shape) == (2, 1, 32, 32, 5)
        gan.G.eval()
        codes = _codes(8)
        back = []
        with torch.no_grad():
            for code in codes:  # eight separate calls on CPU-transformed inputs, mapped back on the CPU
                sr = gan.G(cpu_forward(LR, code).to(DEV), cpu_forward(Z, code, is_vector=False).to(DEV)).float().cpu()
                back.append(cpu_inverse(sr, code))
        want_mean = tree(back) * torch.tensor(1.0 / 8)
        assert rel_l2(back[1], back[0]) > 1e-3, "an un-trained generator is not equivariant: the members must differ"

        rng_cpu, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state()
        for training in (False, True):  # (dropout probability 0: both modes compute the same)
            gan.G.train(training)
            mean = gan.G_ensemble(LR.to(DEV), Z.to(DEV))  # members from the config
            assert gan.G.training is training
            assert torch.is_tensor(mean) and mean.dtype == torch.float32 and tuple(mean.shape) == (2, 3, 32, 32, 5)
            assert not mean.requires_grad
            err = rel_l2(mean, want_mean)
            print(f"[ensemble] G_ensemble vs eight calls (training={training}): rel-L2 {err:.3g}")
            assert err <= 2e-5, err
        gan.G.eval()
        assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_dev)
        mean8, var8 = gan.G_ensemble(LR.to(DEV), Z.to(DEV), members=8, with_var=True)
        assert torch.equal(mean8, mean)
        # (the variance kernel is held to float64 above; here only that it is a spread of members that differ)
        assert tuple(var8.shape) == tuple(mean.shape) and bool(torch.isfinite(var8).all()) and bool((var8 >= 0).all())
        assert float(var8.max()) > 0
        # members = 1 is the generator itself, bit for bit; an argument overrides the config
        with torch.no_grad():
            plain = gan.G(LR.to(DEV), Z.to(DEV)).float()
        one = gan.G_ensemble(LR.to(DEV), Z.to(DEV), members=1)
        assert one.view(torch.int32).equal(plain.contiguous().view(torch.int32))
        assert rel_l2(gan.G_ensemble(LR.to(DEV), Z.to(DEV), members=4), tree([back[0], back[2], back[4], back[6]]) * 0.25) <= 2e-5
    finally:
        Config(os.path.join(os.path.dirname(__import__("gan_sr_wind_field_amd").__file__), "config",
                            "wind_field_GAN_3D_config_local.ini"))  # (the section objects are singletons: reset)


# ----------------------------------------------------------------------------------------------- test.py, both loops
def test_host_and_device_loops_take_sr_from_the_ensemble(hip, tmp_path):
    """the loop of ``[EVAL] device_metrics`` (batches of two fields) against the host loop (one field at a time), both
    with ``[ENSEMBLE] members = 4, write_spread = True``: same fields, SR and spread of the ensemble in both.

    Tolerances from the fp32 output tolerance eps = 2e-5 (another batch size may take other tiles): SR within
    rel-L2 eps.  The standard deviation over K members is a norm of the members' deviations scaled by 1 / sqrt(K), so
    1-Lipschitz in them: ||d sd|| <= max_k ||d m_k|| <= eps max_k ||m_k|| <= eps (||mean|| + sqrt(K) ||sd||).  The CSV
    value is uvw times the mean over V voxels of the length of sd: it moves by at most uvw ||d sd|| / sqrt(V)."""
    import io

    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd.config.config import Config
    from conftest import rel_l2
    from oracle import gan as ogan

    try:
        gan, cfg = _gan(nz=5, ensemble_members=4)
        cfg.ensemble.write_spread = True
        cfg.training.log_period = 1
        gan.G.eval()
        n, uvw = 4, 30.0
        LR, HR, Z, _, _ = ogan.synthetic_batch(n, 8, 5, 4, seed=7)
        empty = torch.zeros(0)
        fields = [(LR[i], HR[i], Z[i], f"f{i}", empty, empty) for i in range(n)]
        want = [gan.G_ensemble(LR[i:i + 1].to(DEV), Z[i:i + 1].to(DEV), with_var=True) for i in range(n)]
        with torch.no_grad():
            plain = gan.G(LR[:1].to(DEV), Z[:1].to(DEV))
        assert rel_l2(want[0][0], plain) > 1e-3  # (the ensemble is not the plain forward here)
        got = {}
        for name, loop, bs in (("host", tmod._host_loop, 1), ("device", tmod._device_loop, 2)):
            cfg.env.this_runs_folder = str(tmp_path / name)
            cfg.eval.present, cfg.eval.device_metrics, cfg.eval.batch_size = name == "device", True, bs
            loader = torch.utils.data.DataLoader(fields, batch_size=bs, shuffle=False)
            out = io.StringIO()
            with tmod._FieldMean("ensemble_spread", "mean_spread", "var", uvw, name, "", str(tmp_path)) as spread:
                loop(cfg, gan, loader, uvw, n, tmod._LevelSet(out, [spread]))
            text = open(spread.path()).read()
            assert text.startswith("field,mean_spread\n")
            rows = [r.split(",") for r in text.strip().splitlines()[1:]]
            assert [r[0] for r in rows] == [f"f{i}" for i in range(n)] == [r.split(",")[0] for r in out.getvalue().strip().splitlines()]
            got[name] = [float(r[1]) for r in rows]
            for i in range(n):
                p = pickle.load(open(os.path.join(cfg.env.this_runs_folder, "fields", f"test_fields_f{i}.pkl"), "rb"))
                mean_i, var_i = want[i]
                assert p["SR"].shape == p["SR_spread"].shape == (3, 32, 32, 5)
                assert rel_l2(torch.from_numpy(p["SR"]), mean_i[0]) <= 2e-5, (name, i)
                sd_i = torch.sqrt(var_i[0]).double().cpu()
                d_sd = 2e-5 * (float(mean_i.double().norm()) + math.sqrt(4) * float(sd_i.norm()))
                assert float((torch.from_numpy(p["SR_spread"]).double() - sd_i).norm()) <= d_sd, (name, i)
                spread_i = float(torch.sqrt(var_i.double().sum(dim=1)).mean()) * uvw
                allowed = uvw * d_sd / math.sqrt(32 * 32 * 5) + 2.0 ** -22 * spread_i  # (+ the fp32 mean's own rounding)
                assert abs(got[name][i] - spread_i) <= allowed and spread_i > 0, (name, i, got[name][i], spread_i, allowed)
            if name == "host":  # one field per forward there too: the very bits of G_ensemble
                p0 = pickle.load(open(os.path.join(cfg.env.this_runs_folder, "fields", "test_fields_f0.pkl"), "rb"))
                assert np.array_equal(p0["SR"], want[0][0][0].cpu().numpy())
    finally:
        Config(os.path.join(os.path.dirname(__import__("gan_sr_wind_field_amd").__file__), "config",
                            "wind_field_GAN_3D_config_local.ini"))  # (the section objects are singletons: reset)


# ------------------------------------------------------------------------------------------------------------ run.py
def _rows(name, suffix="metrics"):
    with open(os.path.join("test_output", f"{name}____{suffix}.csv")) as f:
        return list(csv.reader(f))


def test_run_train_and_test_without_with_eight_and_with_one_member(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import LOSS_KEYS, _write_ini

    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod
    from gan_sr_wind_field_amd.test import METRIC_NAMES

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    rec = {}
    cls = gmod.wind_field_GAN_3D
    orig_opt = cls.optimize_parameters

    def rec_opt(self, LR, HR, Z, it):
        orig_opt(self, LR, HR, Z, it)
        rec.setdefault(self.cfg.name, []).append(
            [float(self.get_G_train_loss_dict_ref()[k].detach()) for k in LOSS_KEYS]
            + [float(self.get_D_loss_dict_ref()["train_loss"].detach())])

    monkeypatch.setattr(cls, "optimize_parameters", rec_opt)
    calls = {"dihedral_members": 0, "ensemble_reduce": 0}

    def counted(name):
        orig = getattr(hip_ops, name)

        def f(*a, **kw):
            calls[name] += 1
            return orig(*a, **kw)
        return f

    for name in calls:
        monkeypatch.setattr(hip_ops, name, counted(name))

    def run(name, section):
        ini = str(tmp_path / f"{name}.ini")
        cfg = _write_ini(ini)
        cfg.name = name
        with open(ini, "w") as f:
            f.write(cfg.asINI() + section)
        runmod.main(["--train", "--test", "--cfg", ini])
        return os.path.join(str(tmp_path), "runs", name)

    dir_a = run("plain", "")
    assert calls == {"dihedral_members": 0, "ensemble_reduce": 0}  # the section absent: no new launch
    assert not os.path.exists(os.path.join("test_output", "plain____ensemble_spread.csv"))
    dir_b = run("ens8", "\n[ENSEMBLE]\nmembers = 8\nwrite_spread = True\n")
    rows_a, rows_b = _rows("plain"), _rows("ens8")
    n_test = len(rows_a) - 1
    assert n_test > 0 and calls == {"dihedral_members": 2 * n_test, "ensemble_reduce": n_test}, calls
    dir_c = run("ens1", "\n[ENSEMBLE]\nmembers = 1\n")
    assert calls == {"dihedral_members": 4 * n_test, "ensemble_reduce": 2 * n_test}, calls
    with open(os.path.join(dir_b, "config.ini")) as f:
        assert f.read().endswith("\n[ENSEMBLE]\nmembers = 8\nwrite_spread = True\n")

    # the section touches nothing in training: losses and weights bit for bit
    assert rec["plain"] == rec["ens8"] == rec["ens1"] and len(rec["plain"]) == 7
    ga, gb, gc = (torch.load(os.path.join(d, "G_6.pth"), map_location="cpu") for d in (dir_a, dir_b, dir_c))
    assert list(ga) == list(gb) == list(gc) and all(torch.equal(ga[k], gb[k]) and torch.equal(ga[k], gc[k]) for k in ga)

    # members = 8: same header, names and row order, other values
    assert rows_a[0] == rows_b[0] == ["field"] + list(METRIC_NAMES)
    assert [r[0] for r in rows_a] == [r[0] for r in rows_b]
    assert all(ra[1:] != rb[1:] for ra, rb in zip(rows_a[1:], rows_b[1:]))
    for k in ("PSNR_trilinear", "trilinear_pix", "average_wind_speed"):  # nothing that does not involve SR moved
        i = 1 + METRIC_NAMES.index(k)
        assert [r[i] for r in rows_a] == [r[i] for r in rows_b], k
    assert all(math.isfinite(float(v)) for r in rows_b[1:] for v in r[1:])
    spread = _rows("ens8", "ensemble_spread")
    assert spread[0] == ["field", "mean_spread"] and [r[0] for r in spread[1:]] == [r[0] for r in rows_a[1:]]
    vals = [float(r[1]) for r in spread[1:]]
    assert all(len(r) == 2 for r in spread) and all(math.isfinite(v) and v >= 0 for v in vals) and max(vals) > 0
    fields = sorted(f for f in os.listdir(os.path.join(dir_b, "fields")) if f.startswith("test_fields_"))
    assert fields and fields == sorted(f for f in os.listdir(os.path.join(dir_a, "fields")) if f.startswith("test_fields_"))
    for f in fields:
        pa, pb = (pickle.load(open(os.path.join(d, "fields", f), "rb")) for d in (dir_a, dir_b))
        assert set(pb) == set(pa) | {"SR_spread"}
        assert pb["SR_spread"].shape == pb["SR"].shape == pa["SR"].shape and pb["SR_spread"].dtype == np.float32
        assert np.isfinite(pb["SR_spread"]).all() and (pb["SR_spread"] >= 0).all() and pb["SR_spread"].max() > 0
        for k in ("HR", "LR", "TL", "Z"):
            assert np.array_equal(pa[k], pb[k]), k
        assert not np.array_equal(pa["SR"], pb["SR"])
    # the CSV value is the mean over voxels of the pickled spread's length, in m/s
    _, te, _, _, _ = runmod.prepare_data(_write_ini(str(tmp_path / "again.ini")))
    uvw = float(te.UVW_MAX)
    by_name = dict((r[0], float(r[1])) for r in spread[1:])
    for f in fields:
        p = pickle.load(open(os.path.join(dir_b, "fields", f), "rb"))
        want = float(np.sqrt((p["SR_spread"].astype(np.float64) ** 2).sum(0)).mean()) * uvw
        assert by_name[f[len("test_fields_"):-4]] == pytest.approx(want, rel=1e-4)

    # members = 1: the identity member alone - the plain run's file, character for character; no spread file
    with open(os.path.join("test_output", "plain____metrics.csv")) as fa, \
            open(os.path.join("test_output", "ens1____metrics.csv")) as fc:
        assert fa.read() == fc.read()
    assert not os.path.exists(os.path.join("test_output", "ens1____ensemble_spread.csv"))
    for f in fields:
        pa, pc = (pickle.load(open(os.path.join(d, "fields", f), "rb")) for d in (dir_a, dir_c))
        assert set(pa) == set(pc) and all(np.array_equal(pa[k], pc[k]) for k in pa)
    print(f"[time] tests/test_ensemble_gpu.py up to here: {time.time() - T0:.1f} s")
