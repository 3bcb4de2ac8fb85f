#!/usr/bin/env python
"""Cost of evaluation with and without [EVAL] (one device), at the shipped test shape (128 x 128 x 10, x4, fp32) and at
C3' (128^3, x4, bf16 generator).

Per shape, one model from the seed and ``--fields`` synthetic fields:

* the loop of ``run.py --test`` (``test._host_loop`` against ``test._device_loop``; the parent commit's path is the
  build with the section absent): wall time per field, host clock around a synchronised pass over the fields.  Both
  paths pickle the same number of fields per pass (the device path its first batch, the host path every
  ``fields / batch_size``-th field; the count is checked), and the time inside ``write_fields`` is taken separately and
  reported beside the figure without it (the device path's copy of SR and TL of the pickled batch to the host stays in
  both figures, as the host path's copy of every SR does);
* a validation epoch (``train._validate`` without its image sample): wall time per batch, dictionary reads included;
* ``process_data.reverse_interpolate_z_axis`` on the host (one field, three channels, timed once) against
  ``hip_ops.column_interp`` (device events);
* the kernels alone from device events: ``field_metrics`` in both forms and ``trilinear_xy``, with the bytes the
  algorithm needs (HR + SR [+ TL or LR] read once; TL written once) over that time.

Blocks alternate between the two paths (``--reps`` blocks each, medians reported).  One JSON line:

    python tools/bench_eval.py --out profiles/eval.json
"""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"test_128x128x10": dict(lr=32, nz=10, dtype="fp32", val_batch=2), "c3_128x128x128": dict(lr=32, nz=128, dtype="bf16", val_batch=1)}


def make(dev, nz, dtype, folder):
    import torch
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    cfg = Config(os.path.join(ROOT, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = dev.index, dev
    cfg.compute_dtype = dtype
    cfg.gan_config.enable_slicing = False
    cfg.gan_config.number_of_z_layers = nz
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = 1
    cfg.training.log_period = 10 ** 9  # (set per pass in test_pass)
    cfg.env.this_runs_folder = folder
    torch.manual_seed(cfg.env.fixed_seed)
    return wind_field_GAN_3D(cfg), cfg


def section(cfg, on, batch_size):
    cfg.eval.present, cfg.eval.device_metrics, cfg.eval.batch_size, cfg.eval.reverse_interpolate = on, True, batch_size, False


def events_ms(fn, n=30, warm=3):
    import torch
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def bench_shape(tag, spec, args, dev):
    import numpy as np
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd import train as trmod
    from gan_sr_wind_field_amd.process_data import reverse_interpolate_z_axis, synthetic_batch

    folder = tempfile.mkdtemp(prefix="bench_eval_")
    gan, cfg = make(dev, spec["nz"], spec["dtype"], folder)
    LR, HR, Z, x, y = synthetic_batch(args.fields, spec["lr"], spec["nz"], cfg.scale, seed=2001)
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    gan.G.eval()
    empty = torch.zeros(0)
    fields = [(LR[i], HR[i], Z[i], f"f{i}", empty, empty) for i in range(args.fields)]
    uvw = 30.0
    out = {"LR": list(LR.shape[1:]), "HR": list(HR.shape[1:]), "compute_dtype": spec["dtype"], "fields": args.fields}

    assert args.fields % args.batch_size == 0 and args.fields > args.batch_size
    real_write = tmod.write_fields
    pickled = {"n": 0, "ms": 0.0}

    def timed_write(*a, **kw):
        t = time.perf_counter()
        real_write(*a, **kw)
        pickled["ms"] += (time.perf_counter() - t) * 1e3
        pickled["n"] += 1

    tmod.write_fields = timed_write

    def test_pass(on):
        """(ms per field, ms per field without the time inside write_fields, averages); batch_size fields pickled"""
        section(cfg, on, args.batch_size)
        # device: batch 0 only = batch_size fields; host (one field per batch): every (fields / batch_size)-th field
        cfg.training.log_period = 10 ** 9 if on else args.fields // args.batch_size
        loader = torch.utils.data.DataLoader(fields, batch_size=args.batch_size if on else 1, shuffle=False)
        loop = tmod._device_loop if on else tmod._host_loop
        pickled["n"], pickled["ms"] = 0, 0.0
        with open(os.devnull, "w") as o:
            flat = tmod._LevelSet(o)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(cfg, gan, loader, uvw, args.fields, flat)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        assert pickled["n"] == args.batch_size, pickled
        return ms / args.fields, (ms - pickled["ms"]) / args.fields, flat.avg, pickled["ms"] / pickled["n"]

    vb = spec["val_batch"]
    batches = [(LR[i:i + vb], HR[i:i + vb], Z[i:i + vb]) for i in range(0, args.fields - vb + 1, vb)]
    log = logging.getLogger("bench_eval")

    class Train:  # (what _validate reads of the training dataset)
        UVW_MAX = uvw

    def val_pass(on):
        section(cfg, on, args.batch_size)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trmod._validate(cfg, gan, batches, Train, 1, None, log, False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)

    for on in (False, True):  # warm-up of every shape the timed blocks use
        test_pass(on)
        val_pass(on)
    t_ms, t_nw, w_ms, v_ms = ({False: [], True: []} for _ in range(4))
    avgs = {}
    for _ in range(args.reps):
        for on in (False, True):
            ms, ms_nw, avgs[on], ms_w = test_pass(on)
            t_ms[on].append(ms)
            t_nw[on].append(ms_nw)
            w_ms[on].append(ms_w)
        for on in (False, True):
            v_ms[on].append(val_pass(on))
    section(cfg, False, 1)
    for on, name in ((False, "host"), (True, "device")):
        out[f"test_ms_per_field_{name}"] = round(statistics.median(t_ms[on]), 3)
        out[f"test_ms_per_field_{name}_blocks"] = [round(v, 3) for v in t_ms[on]]
        out[f"test_ms_per_field_{name}_without_write_fields"] = round(statistics.median(t_nw[on]), 3)
        out[f"write_fields_ms_per_pickled_field_{name}"] = round(statistics.median(w_ms[on]), 3)
        out[f"val_ms_per_batch_{name}"] = round(statistics.median(v_ms[on]), 3)
        out[f"val_ms_per_batch_{name}_blocks"] = [round(v, 3) for v in v_ms[on]]
    out["val_batch"] = vb
    out["test_batch_size_device"] = args.batch_size
    out["fields_pickled_per_pass"] = args.batch_size
    tmod.write_fields = real_write
    out["largest_relative_difference_of_the_averages"] = max(
        abs(avgs[True][k] - avgs[False][k]) / max(abs(avgs[False][k]), 1e-30) for k in tmod.METRIC_NAMES)

    # the kernels alone
    b = min(args.batch_size, args.fields)
    LR_d, HR_d = LR[:b].to(dev).contiguous(), HR[:b].to(dev).contiguous()
    with torch.no_grad():
        SR_d = gan.G(LR_d, Z[:b].to(dev)).float().contiguous()
    TL_d = hip_ops.trilinear_xy(LR_d, cfg.scale)
    vox_bytes = 3 * HR_d[:, :3].numel() // 3 * 4
    for name, fn, nbytes in (
            ("field_metrics_fly", lambda: hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=cfg.scale), 2 * vox_bytes + LR_d[:, :3].numel() * 4),
            ("field_metrics_tensor", lambda: hip_ops.field_metrics(HR_d, SR_d, TL=TL_d), 3 * vox_bytes),
            ("trilinear_xy", lambda: hip_ops.trilinear_xy(LR_d, cfg.scale), vox_bytes + LR_d[:, :3].numel() * 4)):
        ms = events_ms(fn)
        out[f"{name}_us_batch{b}"] = round(ms * 1e3, 2)
        out[f"{name}_MB"] = round(nbytes / 1e6, 2)
        out[f"{name}_TBps"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
    if b > 1:
        one = (HR_d[:1].contiguous(), SR_d[:1].contiguous(), LR_d[:1].contiguous())
        out["field_metrics_fly_us_batch1"] = round(events_ms(lambda: hip_ops.field_metrics(one[0], one[1], LR=one[2], scale=cfg.scale)) * 1e3, 2)

    # back onto raw levels: the host loop of np.interp against the kernel (one field, three channels)
    z_flat = Z[:1].contiguous()
    z_raw = (z_flat + 3.0 * torch.rand(z_flat.shape, generator=torch.Generator().manual_seed(1))).contiguous()
    z_raw = torch.sort(z_raw, dim=-1).values
    sr1 = SR_d[:1].cpu()
    t0 = time.perf_counter()
    host = reverse_interpolate_z_axis(sr1.numpy(), z_raw.numpy(), z_flat.numpy())
    out["reverse_interpolate_host_ms_per_field"] = round((time.perf_counter() - t0) * 1e3, 1)
    a, zs, zq = SR_d[:1].contiguous(), z_flat.to(dev), z_raw.to(dev)
    out["column_interp_us_per_field"] = round(events_ms(lambda: hip_ops.column_interp(a, zs, zq)) * 1e3, 2)
    got = hip_ops.column_interp(a, zs, zq).cpu()
    out["column_interp_share_not_bit_equal_to_host"] = float((got.view(torch.int32) != host.view(torch.int32)).float().mean())
    out["column_interp_max_abs_difference"] = float((got - host).abs().max())
    assert np.isfinite(got.numpy()).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=4, help="[EVAL] batch_size of the device path")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gan_sr_wind_field_amd import _lib

    _lib.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"device": torch.cuda.get_device_name(dev), "blocks": args.reps}
    for tag in args.shapes.split(","):
        out[tag] = bench_shape(tag, SHAPES[tag], args, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
