#!/usr/bin/env python
"""Cost of [EMA] at C3' (bench.py's default workload: full G + D step, bf16, batch 1, one device).

Two models from the same seed, one without the section and one with ``[EMA] decay = 0.999`` (so the shadow update of
every generator step is the averaging form, not the copy).  Each is warmed up, then timed in ``--reps`` alternating
blocks of ``--steps`` G + D iteration pairs (host clock around a synchronised block, as bench.py times its steps).  The
generator's optimizer step alone is timed from device events around ``optimizer_G.step()`` (``--steps`` pairs, after
the blocks).  The estimate the measurement is held against is the traffic alone: one read and one write of the shadows
per generator step at the 5 TB/s DESIGN 12 observed for this access pattern.  One JSON line:

    python tools/bench_ema.py --out profiles/ema.json
    rocprofv3 --kernel-trace --stats -d DIR -o ema -- python tools/bench_ema.py --steps 5 --warmup 1 --reps 1
    python tools/bench_ema.py --kernel-stats DIR > profiles/ema_kernel_stats.txt
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TBPS_OBSERVED = 5.0  # adam_multi_kernel, 0.83 GB in 163 us


def kernel_stats(folder: str) -> None:
    """durations (us) of the optimizer kernels out of a rocprofv3 kernel trace, per kernel and grid size"""
    files = [folder] if os.path.isfile(folder) else glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {folder}")
    rows = {}
    for path in files:
        with open(path) as f:
            for r in csv.DictReader(f):
                hit = re.search(r"\b(adam_multi\w*|grad_sqnorm\w*)", r["Kernel_Name"])
                if hit is None:
                    continue
                short = hit.group(1)
                wgs = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
                rows.setdefault((short, wgs), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':<30}{'jobs (= workgroups)':>20}{'calls':>8}{'mean':>9}{'min':>9}{'max':>9}   (microseconds)")
    for (short, wgs), us in sorted(rows.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
        print(f"{short:<30}{wgs:>20}{len(us):>8}{statistics.mean(us):>9.1f}{min(us):>9.1f}{max(us):>9.1f}")


def make(dev, ema: bool):
    import torch
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    cfg = Config(os.path.join(ROOT, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = dev.index, dev
    cfg.compute_dtype = "bf16"
    cfg.gan_config.enable_slicing = False
    cfg.gan_config.number_of_z_layers = 128
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = 1
    cfg.ema.present, cfg.ema.decay, cfg.ema.start_iter = ema, 0.999, 0
    torch.manual_seed(cfg.env.fixed_seed)
    return wind_field_GAN_3D(cfg), cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR_OR_CSV",
                    help="summarise the optimizer kernels of a rocprofv3 --kernel-trace output folder and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import torch
    from gan_sr_wind_field_amd import _lib
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    _lib.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    runs = {}
    for tag, ema in (("off", False), ("ema", True)):
        gan, cfg = make(dev, ema)
        LR, HR, Z, x, y = (t.to(dev) for t in synthetic_batch(1, 32, 128, cfg.scale, seed=2001))
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=dev), 1, 1)
        runs[tag] = dict(gan=gan, data=(LR, HR, Z), it=0, ms=[], opt_ms=[])
    assert runs["ema"]["gan"].optimizer_G.ema_decay == 0.999 and runs["off"]["gan"].optimizer_G.ema_decay is None

    def pairs(r, k):
        LR, HR, Z = r["data"]
        for _ in range(k):
            r["gan"].optimize_parameters(LR, HR, Z, r["it"])      # G-iteration
            r["gan"].optimize_parameters(LR, HR, Z, r["it"] + 1)  # D-iteration
            r["gan"].update_learning_rate()
            r["it"] += 2

    for r in runs.values():
        pairs(r, args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for r in runs.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pairs(r, args.steps)
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) * 1e3 / args.steps)
    # the generator's optimizer step on its own (device time between events around step())
    for r in runs.values():
        opt, pending, ev = r["gan"].optimizer_G, [], []

        def pre(*_):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev[:] = [e]

        def post(*_):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            pending.append((ev[0], e))
        opt.register_step_pre_hook(pre)
        opt.register_step_post_hook(post)
        pairs(r, args.steps)
        torch.cuda.synchronize()
        r["opt_ms"] = [a.elapsed_time(b) for a, b in pending]
    gan = runs["ema"]["gan"]
    n_par = sum(p.numel() for p in gan.G.parameters())
    assert sum(e.numel() for e in gan.ema_shadows) == n_par
    assert any(not torch.equal(e, p.detach()) for e, p in zip(gan.ema_shadows, gan.G.parameters()))
    traffic = 2 * 4 * n_par
    out = {"workload": "C3' G+D step, bf16, batch 1, LR 32x32x128", "device": torch.cuda.get_device_name(dev),
           "steps_per_block": args.steps, "blocks": args.reps, "generator_parameters": n_par,
           "generator_tensors": len(gan.ema_shadows), "shadow_traffic_MB_per_G_step": round(traffic / 1e6, 1),
           "estimate_us_per_G_step": round(traffic / (TBPS_OBSERVED * 1e12) * 1e6, 1)}
    for tag, r in runs.items():
        out[f"ms_per_step_{tag}"] = round(statistics.median(r["ms"]), 3)
        out[f"ms_per_step_{tag}_blocks"] = [round(v, 3) for v in r["ms"]]
        out[f"opt_step_G_ms_{tag}"] = round(statistics.median(r["opt_ms"]), 4)
    out["delta_ms_per_step"] = round(out["ms_per_step_ema"] - out["ms_per_step_off"], 3)
    out["delta_opt_step_G_us"] = round((out["opt_step_G_ms_ema"] - out["opt_step_G_ms_off"]) * 1e3, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
