"""[EVAL] on the GPU: the three kernels of csrc/eval_metrics.hip against float64 / numpy references computed here, and
``run.py --train --test`` with and without the section.  Outputs of the kernels go in ``Guarded`` buffers.

Bounds (kernel_bounds.py's convention, LAMBDA = 16 untouched; helpers shared with test_eval.py):

* ``wsr_trilinear_xy``: per element ``LAMBDA * sqrt(6) * 2^-24 * A``, A the same blend of |corners|, 6 the products of
  one element; against the float64 evaluation of the same blend (same index pairs and fp32 weights) and against
  ``F.interpolate`` on the CPU.
* ``wsr_field_metrics``: per sum ``LAMBDA * sqrt(K) * 2^-24 * A`` with A the float64 sum of the (non-negative) terms and
  K their number (3 V for the component sums, V for the vector lengths, V voxels).  The sums against the baseline made
  on the fly are compared with float64 sums against the float64 baseline, so they also carry the baseline's own bound
  delta (per element): sum (2 |HR-TL| delta + delta^2) for the squares, sum delta for the absolute values, and
  sum ||delta|| (over the three components) for the vector lengths (triangle inequality).  The on-the-fly form and the
  tensor form fed by ``wsr_trilinear_xy`` are bit-equal (the blend is evaluated without contraction in both), and so are
  two calls.
* ``wsr_column_interp``: within one fp32 ulp of ``np.interp`` (double) stored to fp32, bit-equal outside the source
  range; the share of elements that are not bit-equal is printed (the kernel evaluates numpy's expression without
  contraction, so the share is expected to be 0).
* end to end: each CSV value within ``metric_bounds`` of the host path's (the baseline sums also carry the baseline's
  bound, as a relative extra of those sums); the calls of the three wrappers are counted, so the runs with the section
  are known to have gone through the kernels, and the pickled TL is held against the host run's under the baseline's
  bound.

Measured on an MI355X when the kernels were written: worst |err| / bound 0.091 (baseline against float64), 0.107 (against
``F.interpolate``), 1.1e-3 (sums), 7.8e-4 (end to end); share of ``wsr_column_interp`` elements not bit-equal to numpy: 0 of
74 610; the whole file ran in 11.9 s.
"""
import csv
import math
import os
import pickle
import re
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import LAMBDA, U_FP32, Guarded, assert_guards_intact, assert_within
from test_eval import SUM_NAMES, baseline, baseline_bound, metric_bounds, sums_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T0 = time.time()


def _nan_extra_channels(t, keep=3):
    """channels >= keep must never be read: poison them"""
    if t.shape[1] > keep:
        t[:, keep:] = float("nan")
    return t


# ---------------------------------------------------------------------------------------------------- wsr_trilinear_xy
TL_CASES = [(4, (1, 3, 8, 8, 10)), (4, (3, 4, 6, 5, 5)), (8, (1, 5, 4, 6, 6)), (8, (3, 6, 4, 4, 8)),
            (16, (1, 4, 4, 3, 128)), (16, (3, 3, 3, 4, 10)), (4, (1, 6, 8, 8, 128))]


@pytest.mark.parametrize("s,lr_shape", TL_CASES, ids=[f"s{s}-" + "x".join(map(str, sh)) for s, sh in TL_CASES])
def test_trilinear_xy_elementwise(hip, s, lr_shape):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    gen = torch.Generator().manual_seed(11 + s)
    LR = _nan_extra_channels(torch.randn(lr_shape, generator=gen))
    B, cin, Xl, Yl, NZ = lr_shape
    out = Guarded((B, 3, Xl * s, Yl * s, NZ), torch.float32, DEV)
    LR_d = LR.to(DEV)
    check(hip.wsr_trilinear_xy(hip_ops._p(LR_d), B, cin, Xl, Yl, NZ, s, hip_ops._p(out.t), hip_ops._stream()))
    torch.cuda.synchronize()
    assert_guards_intact(out, label="trilinear_xy")
    ref, A = baseline(LR, s)
    bnd = baseline_bound(A)
    assert_within(out.t, ref, bnd, f"trilinear_xy vs float64 blend[s={s} {lr_shape}]")
    aten = F.interpolate(LR[:, :3], scale_factor=(s, s, 1), mode="trilinear", align_corners=True)
    assert_within(out.t, aten.double(), bnd, f"trilinear_xy vs F.interpolate[s={s} {lr_shape}]")
    assert torch.equal(hip_ops.trilinear_xy(LR_d, s), out.t)  # the wrapper: same launch


# ---------------------------------------------------------------------------------------------------- wsr_column_interp
def _writer_levels(tmp_path, monkeypatch):
    """source levels of the synthetic HARMONIE-SIMRA writer: (1, 1, 32, 32, 10) terrain-following altitudes"""
    import pickle
    from datetime import date

    from gan_sr_wind_field_amd import process_data as pd

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    XS, ZS = {"start": 0, "max": 32, "step": 1}, {"start": 0, "max": 10, "step": 1}
    sub = pd.write_synthetic_dataset(date(2018, 3, 1), date(2018, 3, 1), XS, XS, ZS, seed=5)
    name = pd.filenames_from_start_and_end_dates(date(2018, 3, 1), date(2018, 3, 1))[3]
    z = pickle.load(open(os.path.join(str(tmp_path / "data"), "full_dataset_files", sub, name), "rb"))[0]
    return torch.from_numpy(z.astype(np.float32))[None, None]


def _interp_case(hip, vals, z_src, z_dst, label):
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd._lib import check

    B, C, X, Y, NZ = vals.shape
    assert bool((z_src[..., 1:] > z_src[..., :-1]).all())  # strictly increasing: numpy leaves equal knots undefined
    out = Guarded(vals.shape, torch.float32, DEV)
    v_d, s_d, q_d = vals.to(DEV), z_src.to(DEV), z_dst.to(DEV)
    check(hip.wsr_column_interp(hip_ops._p(v_d), hip_ops._p(s_d), hip_ops._p(q_d), B, C, X * Y, NZ, hip_ops._p(out.t),
                                hip_ops._stream()))
    torch.cuda.synchronize()
    assert_guards_intact(out, label=label)
    got = out.t.cpu().numpy()
    assert torch.equal(hip_ops.column_interp(v_d, s_d, q_d), out.t)
    v, zs, zq = vals.numpy(), z_src.numpy(), z_dst.numpy()
    ref = np.empty_like(v)
    for b in range(B):
        for c in range(C):
            for i in range(X):
                for j in range(Y):
                    ref[b, c, i, j] = np.interp(zq[b, 0, i, j], zs[b, 0, i, j], v[b, c, i, j])
    ulp = np.spacing(np.abs(ref))
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp).all(), label
    outside = np.broadcast_to((zq < zs[..., :1]) | (zq > zs[..., -1:]), ref.shape)
    on_knot = np.broadcast_to((zq[..., :, None] == zs[..., None, :]).any(-1), ref.shape)
    assert outside.any() and on_knot.any(), label
    same = got.view(np.int32) == ref.view(np.int32)
    assert same[outside].all() and same[on_knot].all(), label
    share = 1.0 - float(same.mean())
    print(f"[interp] {label}: {ref.size} elements, share not bit-equal to numpy {share:.3g}, outside the range "
          f"{int(outside.sum())}, on a knot {int(on_knot.sum())}")
    return share


@pytest.mark.parametrize("shape", [(2, 3, 7, 9, 5), (1, 3, 12, 10, 10), (1, 2, 5, 6, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_column_interp_vs_numpy_random_levels(hip, shape):
    B, C, X, Y, NZ = shape
    gen = torch.Generator().manual_seed(NZ)
    z_src = torch.cumsum(torch.rand((B, 1, X, Y, NZ), generator=gen) * 49 + 1, dim=-1)
    lo, hi = z_src[..., :1], z_src[..., -1:]
    z_dst = lo - 20 + (hi - lo + 40) * torch.rand((B, 1, X, Y, NZ), generator=gen)  # below, inside and above
    on = torch.rand((B, 1, X, Y, NZ), generator=gen) < 0.2                           # ... and exactly on knots
    z_dst = torch.where(on, z_src.roll(1, dims=-1), z_dst)
    vals = torch.randn(shape, generator=gen)
    _interp_case(hip, vals, z_src, z_dst, f"random levels {shape}")


def test_column_interp_vs_numpy_writer_levels(hip, tmp_path, monkeypatch):
    z_src = _writer_levels(tmp_path, monkeypatch)
    gen = torch.Generator().manual_seed(3)
    nz = z_src.shape[-1]
    flat = torch.linspace(float(z_src.min()) - 5, float(z_src.max()) + 5, nz).expand_as(z_src).contiguous()
    z_dst = torch.where(torch.rand(z_src.shape, generator=gen) < 0.2, z_src, flat)
    vals = torch.randn((1, 3) + tuple(z_src.shape[2:]), generator=gen)
    _interp_case(hip, vals, z_src, z_dst, "writer levels -> flat levels")
    # and the way test.py uses it: from the flat (interpolated) levels back onto the raw ones
    flat_inc = torch.linspace(float(z_src.min()) + 30, float(z_src.max()) - 30, nz).expand_as(z_src)
    flat_inc = flat_inc + torch.rand(z_src.shape, generator=gen)  # (steps of tens of metres: still strictly increasing)
    z_back = torch.where(torch.rand(z_src.shape, generator=gen) < 0.2, flat_inc, z_src)
    _interp_case(hip, vals, flat_inc, z_back, "flat levels -> writer levels")


# ---------------------------------------------------------------------------------------------------- wsr_field_metrics
def _sum_bounds(HR, TL64, sums, delta=None):
    """(B, 7) bound of the seven sums: LAMBDA sqrt(K) 2^-24 A, + the propagated baseline bound on the TL sums"""
    B = HR.shape[0]
    V = HR.shape[2] * HR.shape[3] * HR.shape[4]
    K = torch.tensor([3 * V, 3 * V, 3 * V, 3 * V, V, V, V], dtype=torch.float64)
    bnd = LAMBDA * torch.sqrt(K) * U_FP32 * sums + 2.0 ** -100
    if delta is not None:
        d = (HR[:, :3].double() - TL64).abs()
        bnd[:, 1] += (2 * d * delta + delta ** 2).flatten(1).sum(1)
        bnd[:, 3] += delta.flatten(1).sum(1)
        bnd[:, 5] += torch.sqrt((delta ** 2).sum(dim=1)).flatten(1).sum(1)
    assert bnd.shape == (B, 7)
    return bnd


MET_CASES = [(4, 3, 3, (3, 16, 12, 10)), (8, 4, 5, (1, 32, 32, 128)), (4, 5, 3, (2, 8, 12, 5)), (16, 3, 6, (2, 16, 32, 6)),
             (4, 3, 4, (1, 128, 128, 10))]


@pytest.mark.parametrize("s,hr_c,lr_c,dims", MET_CASES, ids=[f"s{c[0]}-" + "x".join(map(str, c[3])) for c in MET_CASES])
def test_field_metrics_sums(hip, s, hr_c, lr_c, dims):
    from gan_sr_wind_field_amd import hip_ops

    B, X, Y, NZ = dims
    gen = torch.Generator().manual_seed(X + NZ)
    LR = _nan_extra_channels(torch.randn((B, lr_c, X // s, Y // s, NZ), generator=gen) * 0.4)
    TL64, A = baseline(LR, s)
    HR = _nan_extra_channels(torch.cat([TL64.float() + 0.1 * torch.randn((B, 3, X, Y, NZ), generator=gen),
                                        torch.zeros((B, hr_c - 3, X, Y, NZ))], dim=1))
    SR = HR[:, :3] + 0.03 * torch.randn((B, 3, X, Y, NZ), generator=gen)
    HR_d, SR_d, LR_d = HR.to(DEV), SR.to(DEV).contiguous(), LR.to(DEV)
    buf = torch.full((B + 2, 7), -7.0, dtype=torch.float64, device=DEV)  # guard rows before and after the output
    fly = hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=s, out=buf[1:B + 1])
    assert fly.data_ptr() == buf[1].data_ptr() and bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
    want = sums_f64(HR, SR, TL64)
    label = f"s={s} hr_c={hr_c} lr_c={lr_c} {dims}"
    assert_within(fly, want, _sum_bounds(HR, TL64, want, baseline_bound(A)), f"field_metrics on the fly[{label}]")
    # the tensor form, fed by wsr_trilinear_xy: bit-equal to the on-the-fly form; against float64 sums of ITS inputs
    TL_d = hip_ops.trilinear_xy(LR_d, s)
    ten = hip_ops.field_metrics(HR_d, SR_d, TL=TL_d)
    assert torch.equal(ten, fly), label
    want_t = sums_f64(HR, SR, TL_d.cpu())
    assert_within(ten, want_t, _sum_bounds(HR, None, want_t), f"field_metrics tensor form[{label}]")
    # two calls: the same bits
    assert torch.equal(hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=s), fly), label
    assert torch.equal(hip_ops.field_metrics(HR_d, SR_d, TL=TL_d), ten), label
    with pytest.raises(ValueError):
        hip_ops.field_metrics(HR_d, SR_d)
    with pytest.raises(ValueError):
        hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=s, TL=TL_d)


# ---------------------------------------------------------------------------------------------------- run.py
def _rows(name, suffix=""):
    with open(os.path.join("test_output", f"{name}____metrics{suffix}.csv")) as f:
        return list(csv.reader(f))


def _val_lines(path):
    """the validation averages the status log holds: [{key: value}] per validation epoch"""
    out = []
    with open(path) as f:
        for line in f:
            m = re.search(r"train\.py: it: (\d+) (.*)$", line)
            if m:
                out.append({k: float(v) for k, v in re.findall(r"(\w+): (\S+)", m.group(2))})
    return out


def _tl_extra(HR, LR, s):
    """relative extra of the three baseline sums of one field when the baseline moves by its bound"""
    TL64, A = baseline(LR, s)
    delta = baseline_bound(A)
    zero = sums_f64(HR, HR[:, :3], TL64)
    b = _sum_bounds(HR, TL64, zero, delta) - _sum_bounds(HR, TL64, zero)
    return {k: float(b[0, i] / zero[0, i]) for i, k in enumerate(SUM_NAMES) if k.endswith("_tl")}


def _assert_rows_within(a, b, nvox, extras, label):
    from gan_sr_wind_field_amd.test import METRIC_NAMES

    assert a[0] == b[0] == ["field"] + list(METRIC_NAMES), label
    assert [r[0] for r in a] == [r[0] for r in b] and len(a) > 1, label
    worst = 0.0
    for ra, rb, extra in zip(a[1:], b[1:], extras):
        ma = dict(zip(METRIC_NAMES, map(float, ra[1:])))
        mb = dict(zip(METRIC_NAMES, map(float, rb[1:])))
        bnd = metric_bounds(ma, nvox, extra)
        for k in METRIC_NAMES:
            allowed = bnd[k] + 2.0 ** -22 * abs(ma[k])  # (+ the host path's fp32 rounding of the value itself)
            worst = max(worst, abs(ma[k] - mb[k]) / allowed)
            assert abs(ma[k] - mb[k]) <= allowed, (label, ra[0], k, ma[k], mb[k], allowed)
    print(f"[e2e] {label}: worst |difference| / bound {worst:.3g}")


def _run(tmp_path, name, flags, section, interpolate_z=False, **env):
    """``run.py`` with ``flags`` on the e2e configuration named ``name`` plus the text ``section`` -> (cfg, run folder)"""
    from test_hip_train_e2e import _write_ini

    from gan_sr_wind_field_amd import run as runmod

    ini = str(tmp_path / f"{name}.ini")
    cfg = _write_ini(ini)
    cfg.name = name
    cfg.gan_config.interpolate_z = interpolate_z
    for k, v in env.items():
        setattr(cfg.env, k, v)
    with open(ini, "w") as f:
        f.write(cfg.asINI() + section)
    runmod.main(flags + ["--cfg", ini])
    return cfg, os.path.join(str(tmp_path), "runs", name)


def test_run_train_and_test_with_and_without_the_section(hip, tmp_path, monkeypatch):
    from test_hip_train_e2e import LOSS_KEYS

    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    rec = {}
    cls = gmod.wind_field_GAN_3D
    orig_opt, orig_val = cls.optimize_parameters, cls.validation

    def rec_opt(self, LR, HR, Z, it):
        orig_opt(self, LR, HR, Z, it)
        rec.setdefault(self.cfg.name, {"train": [], "val": []})["train"].append(
            [float(self.get_G_train_loss_dict_ref()[k].detach()) for k in LOSS_KEYS]
            + [float(self.get_D_loss_dict_ref()["train_loss"].detach())])

    def rec_val(self, LR, HR, Z, it):
        orig_val(self, LR, HR, Z, it)
        rec.setdefault(self.cfg.name, {"train": [], "val": []})["val"].append(
            {k: float(v) for k, v in self.get_metrics_dict_ref().items()})

    monkeypatch.setattr(cls, "optimize_parameters", rec_opt)
    monkeypatch.setattr(cls, "validation", rec_val)

    from gan_sr_wind_field_amd import hip_ops
    calls = {"field_metrics": 0, "trilinear_xy": 0, "column_interp": 0}
    val_types = {}

    def counted(name):
        orig = getattr(hip_ops, name)

        def f(*a, **kw):
            calls[name] += 1
            return orig(*a, **kw)
        return f

    for name in calls:
        monkeypatch.setattr(hip_ops, name, counted(name))

    def rec_val_typed(self, LR, HR, Z, it):
        orig_val(self, LR, HR, Z, it)
        v = self.get_metrics_dict_ref()["val_PSNR"]
        val_types.setdefault(self.cfg.name, set()).add((torch.is_tensor(v) and v.is_cuda, getattr(v, "dtype", None)))
        rec.setdefault(self.cfg.name, {"train": [], "val": []})["val"].append(
            {k: float(v) for k, v in self.get_metrics_dict_ref().items()})

    monkeypatch.setattr(cls, "validation", rec_val_typed)

    def run(*a, **kw):
        return _run(tmp_path, *a, **kw)

    cfg_a, dir_a = run("plain", ["--train", "--test"], "")
    assert calls == {"field_metrics": 0, "trilinear_xy": 0, "column_interp": 0}  # the section absent: no new launch
    cfg_b, dir_b = run("dev", ["--train", "--test"], "\n[EVAL]\nbatch_size = 2\n")
    # the run with the section went through the kernels: one metrics launch per validation batch and per test batch,
    # one baseline per validation image sample and per pickled test batch, float64 device tensors in metrics_dict
    n_val, n_test = len(rec["dev"]["val"]), len(_rows("dev")) - 1
    assert calls["field_metrics"] == n_val + -(-n_test // 2) and calls["column_interp"] == 0, calls
    assert calls["trilinear_xy"] == 2 + -(-n_test // 2), calls
    assert val_types["dev"] == {(True, torch.float64)} and val_types["plain"] != val_types["dev"]
    with open(os.path.join(dir_b, "config.ini")) as f:
        assert "[EVAL]\ndevice_metrics = True\nbatch_size = 2\nreverse_interpolate = False\n" in f.read()
    # the section touches nothing in the step: losses and weights bit for bit
    assert rec["plain"]["train"] == rec["dev"]["train"] and len(rec["plain"]["train"]) == 7
    ga, gb = (torch.load(os.path.join(d, "G_6.pth"), map_location="cpu") for d in (dir_a, dir_b))
    assert list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)

    _, te, va, _, _ = runmod.prepare_data(cfg_a)
    s = cfg_a.scale
    nvox = te[0][1].shape[1] * te[0][1].shape[2] * te[0][1].shape[3]
    extras = [_tl_extra(te[i][1][None], te[i][0][None], s) for i in range(len(te))]
    _assert_rows_within(_rows("plain"), _rows("dev"), nvox, extras, "metrics.csv")
    av = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert av[1].startswith("plain,") and av[2].startswith("dev,") and len(av) == 3
    fields = sorted(f for f in os.listdir(os.path.join(dir_b, "fields")) if f.startswith("test_fields_"))
    assert fields and fields == sorted(f for f in os.listdir(os.path.join(dir_a, "fields")) if f.startswith("test_fields_"))[:len(fields)]

    for f in fields:  # the pickled baseline: wsr_trilinear_xy against the host run's F.interpolate, and the same SR source
        pa, pb = (pickle.load(open(os.path.join(d, "fields", f), "rb")) for d in (dir_a, dir_b))
        assert set(pa) == set(pb) and pa["TL"].shape == pb["TL"].shape == pa["HR"].shape
        lr = torch.from_numpy(pa["LR"])[None]
        assert np.array_equal(pa["LR"], pb["LR"]) and np.array_equal(pa["HR"], pb["HR"])
        ref, A = baseline(lr, s)
        bnd = baseline_bound(A)[0].numpy()
        for p in (pa, pb):
            assert (np.abs(p["TL"].astype(np.float64) - ref[0].numpy()) <= bnd).all(), f
        assert (np.abs(pa["TL"].astype(np.float64) - pb["TL"].astype(np.float64)) <= bnd).all(), f

    # validation: metrics_dict per batch and the epoch averages
    db = 10.0 / math.log(10.0)
    va_a, va_b = rec["plain"]["val"], rec["dev"]["val"]
    assert len(va_a) == len(va_b) > 0
    nv = math.prod(va[0][1].shape[1:])  # (K of ONE field: the tighter bound, whatever the size of a batch)
    r = LAMBDA * math.sqrt(3 * nv) * U_FP32
    ex = max(e[k] for i in range(len(va)) for e in [_tl_extra(va[i][1][None], va[i][0][None], s)] for k in e)
    for ma, mb in zip(va_a, va_b):
        assert set(ma) == set(mb)
        assert ma["pix_loss_unscaled"] == mb["pix_loss_unscaled"]
        assert abs(ma["val_PSNR"] - mb["val_PSNR"]) <= db * r / (1 - r) + 2.0 ** -22 * abs(ma["val_PSNR"])
        assert abs(ma["Trilinear_PSNR"] - mb["Trilinear_PSNR"]) <= db * (r + ex) / (1 - r - ex) + 2.0 ** -22 * abs(ma["Trilinear_PSNR"])
        assert abs(ma["trilinear_pix_loss"] - mb["trilinear_pix_loss"]) <= (r + ex + 2.0 ** -22) * abs(ma["trilinear_pix_loss"])
    la = _val_lines(os.path.join(str(tmp_path), "log", "plain.log"))
    lb = _val_lines(os.path.join(str(tmp_path), "log", "dev.log"))
    assert len(lb) == 2 and len(la) >= 2
    for ea, eb in zip(la[:2], lb):
        assert list(ea) == list(eb)
        for k in ea:
            if k in ("val_PSNR", "Trilinear_PSNR"):
                assert abs(ea[k] - eb[k]) <= db * (r + ex) / (1 - r - ex) + 2.0 ** -22 * abs(ea[k]), k
            elif k == "trilinear_pix_loss":
                assert abs(ea[k] - eb[k]) <= (r + ex + 2.0 ** -22) * abs(ea[k]), k
            else:
                assert ea[k] == eb[k], k

    # the raw terrain-following levels: host re-levelling and metrics against the kernels, from the same checkpoint
    load = dict(generator_load_path=os.path.join(dir_a, "G_6.pth"), discriminator_load_path=os.path.join(dir_a, "D_6.pth"),
                state_load_path=os.path.join(dir_a, "state_6.pth"))
    rev = "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n"
    cfg_h, _ = run("rev_host", ["--test"], rev + "device_metrics = False\n", interpolate_z=True, **load)
    before = dict(calls)
    run("rev_dev", ["--test"], rev, interpolate_z=True, **load)
    nb = -(-n_test // 2)  # per batch: two metrics launches, SR and TL re-levelled, one stored baseline
    assert {k: calls[k] - before[k] for k in calls} == {"field_metrics": 2 * nb, "trilinear_xy": nb, "column_interp": 2 * nb}
    cfg_h.gan_config.interpolate_z = True
    _, te_z, _, _, _ = runmod.prepare_data(cfg_h)
    extras_z = [_tl_extra(te_z[i][1][None], te_z[i][0][None], s) for i in range(len(te_z))]
    _assert_rows_within(_rows("rev_host"), _rows("rev_dev"), nvox, extras_z, "metrics.csv on interpolated levels")
    # (re-levelled values differ by at most one fp32 ulp per element, 2^-23 of a term: far inside r(K); the baseline's
    #  bound passes through np.interp, a convex combination of two levels, without growing)
    _assert_rows_within(_rows("rev_host", "_reverse_interpolate"), _rows("rev_dev", "_reverse_interpolate"), nvox, extras_z,
                        "metrics_reverse_interpolate.csv")
    for name in ("rev_host", "rev_dev"):
        assert any(r.startswith(name + ",") for r in open("test_output/averages_reverse_interpolate.csv").read().splitlines())
    print(f"[time] tests/test_eval_gpu.py up to here: {time.time() - T0:.1f} s")


# ------------------------------------------------------------------------------- the extra outputs of the device loop
def _counted(monkeypatch, names):
    """counting wrappers around ``hip_ops.<name>`` -> the counts"""
    from gan_sr_wind_field_amd import hip_ops

    calls = dict.fromkeys(names, 0)

    def counted(name):
        orig = getattr(hip_ops, name)

        def f(*a, **kw):
            calls[name] += 1
            return orig(*a, **kw)
        return f

    for name in names:
        monkeypatch.setattr(hip_ops, name, counted(name))
    return calls


def _lines(path):
    with open(path) as f:
        return [r.split(",") for r in f.read().strip().splitlines()]


def test_device_loop_with_a_remainder_batch_and_a_flush_in_mid_run(hip, tmp_path, monkeypatch):
    """three fields in batches of two with ``log_period = 2``: a flush after the first batch, a last batch of one field.
    [DIAGNOSTICS], [SPECTRUM] and [SSIM] on, every file of theirs asked for: each field once and in the loader's order in
    every per-field file, every whole-set file complete, one launch per output, baseline and metrics per batch.  Exact
    counts and orders, no tolerance."""
    import contextlib
    import io

    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd.diagnostics import PROFILE_COLUMNS
    from gan_sr_wind_field_amd.spectra import SPECTRUM_COLUMNS, n_bins
    from gan_sr_wind_field_amd.ssim import SSIM_COLUMNS
    from test_ensemble_gpu import _gan
    from test_tiling_gpu import _inputs, _reset_config

    try:
        gan, cfg = _gan(nz=5)
        cfg.name, cfg.env.this_runs_folder = "loop", str(tmp_path / "run")
        cfg.eval.present, cfg.eval.device_metrics, cfg.eval.batch_size = True, True, 2
        cfg.training.log_period = 2
        cfg.diagnostics.present = cfg.diagnostics.per_field = True
        cfg.spectrum.present = cfg.spectrum.per_level = True
        cfg.ssim.present = cfg.ssim.per_level = True
        gan.G.eval()
        n, uvw, NZ = 3, 30.0, 5
        LR, HR, Z = _inputs(n)
        X, Y = HR.shape[2:4]
        assert (X, Y, HR.shape[4]) == (48, 40, NZ)
        gan.x, gan.y = (200.0 * torch.arange(k, dtype=torch.float32, device=DEV) for k in (X, Y))
        empty = torch.zeros(0)
        names = [f"f{i}" for i in range(n)]
        loader = torch.utils.data.DataLoader([(LR[i], HR[i], Z[i], names[i], empty, empty) for i in range(n)], batch_size=2,
                                             shuffle=False)
        calls = _counted(monkeypatch, ("level_diagnostics", "level_spectra", "level_ssim", "trilinear_xy", "field_metrics"))
        out = io.StringIO()
        with contextlib.ExitStack() as stack:
            flat = tmod._LevelSet(out, (stack.enter_context(o)
                                        for o in tmod._outputs(cfg, gan, uvw, 200.0, "", True, str(tmp_path))))
            assert [type(o).__name__ for o in flat.outputs] == ["_LevelProfile", "_Spectrum", "_Ssim"]
            tmod._device_loop(cfg, gan, loader, uvw, n, flat)
        assert calls == dict.fromkeys(calls, 2), calls  # (two batches: one launch each per batch)
        assert [r.split(",")[0] for r in out.getvalue().strip().splitlines()] == names
        assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".csv")) == sorted(
            ["averages_ssim.csv"] + [f"loop____{stem}.csv" for stem in (
                "level_profile", "level_profile_fields", "energy_spectrum", "energy_spectrum_levels", "ssim", "ssim_levels")])
        NK = n_bins(X, Y)
        levels = [str(k) for k in range(NZ)]
        rows = _lines(tmp_path / "loop____level_profile_fields.csv")
        assert rows[0] == ["field", "level"] + list(PROFILE_COLUMNS)
        assert [r[:2] for r in rows[1:]] == [[nm, lvl] for nm in names for lvl in levels]
        rows = _lines(tmp_path / "loop____ssim.csv")
        assert rows[0] == ["field"] + list(SSIM_COLUMNS) and [r[0] for r in rows[1:]] == names
        rows = _lines(tmp_path / "loop____level_profile.csv")
        assert rows[0] == ["level"] + list(PROFILE_COLUMNS) and [r[0] for r in rows[1:]] == levels
        rows = _lines(tmp_path / "loop____ssim_levels.csv")
        assert rows[0] == ["level"] + list(SSIM_COLUMNS) and [r[0] for r in rows[1:]] == levels
        rows = _lines(tmp_path / "loop____energy_spectrum.csv")
        assert rows[0] == ["bin"] + list(SPECTRUM_COLUMNS) and [r[0] for r in rows[1:]] == [str(k) for k in range(NK)]
        rows = _lines(tmp_path / "loop____energy_spectrum_levels.csv")
        assert rows[0] == ["level", "bin"] + list(SPECTRUM_COLUMNS)
        assert [r[:2] for r in rows[1:]] == [[lvl, str(k)] for lvl in levels for k in range(NK)]
        rows = _lines(tmp_path / "averages_ssim.csv")
        assert len(rows) == 2 and rows[1][0] == "loop"
        assert sorted(os.listdir(tmp_path / "run" / "fields")) == ["test_fields_f0.pkl", "test_fields_f1.pkl"]  # batch 0
    finally:
        _reset_config()


def test_all_sections_together_write_each_sections_own_files_on_the_device(hip, tmp_path, monkeypatch):
    """the device-loop form of test_eval.py's test of the same name: from one checkpoint, ``[EVAL] batch_size = 2`` with
    ``reverse_interpolate``, the run with [DIAGNOSTICS], [SPECTRUM] and [SSIM] writes 14 files, each the bytes of the run
    with only its own section, the metrics files those of every run.  Exact - it rests on the kernels giving the same bits
    on every call and on the generator forward giving the same bits for the same batch shape."""
    from gan_sr_wind_field_amd import process_data as pd
    from test_eval import STEMS, _files

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    ev = "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n"
    text = {"diagnostics": "\n[DIAGNOSTICS]\nper_field = True\n", "spectrum": "\n[SPECTRUM]\nper_level = True\n",
            "ssim": "\n[SSIM]\nper_level = True\nwindow_size = 7\nsigma = 1.0\n"}
    _, folder = _run(tmp_path, "ckpt", ["--train"], "", interpolate_z=True)
    load = {k + "_load_path": os.path.join(folder, f"{v}_6.pth")
            for k, v in (("generator", "G"), ("discriminator", "D"), ("state", "state"))}
    runs = {"plain": ev, **{k: ev + v for k, v in text.items()}, "all": ev + "".join(text.values())}
    for name, section in runs.items():
        _run(tmp_path, name, ["--test"], section, interpolate_z=True, **load)
    got = {name: _files(name) for name in runs}
    metrics = {"metrics.csv", "metrics_reverse_interpolate.csv"}
    assert set(got["plain"]) == metrics and len(got["all"]) == 14, sorted(got["all"])
    for sec, stem in STEMS.items():
        own = {f for f in got[sec] if f.startswith(stem)}
        assert len(own) == 4 and set(got[sec]) == metrics | own, (sec, sorted(got[sec]))
        for f in own:
            assert got["all"][f] == got[sec][f], f
    for f in metrics:
        assert len(got["plain"][f].splitlines()) > 1 and all(got[name][f] == got["plain"][f] for name in runs), f
