#!/usr/bin/env python
"""Cost of [GRAD_CLIP] at C3' (bench.py's default workload: full G + D step, bf16, batch 1, one device).

Two models from the same seed, one without the section and one with ``clip_generator``, ``clip_discriminator`` and
``log_grad_norms`` on (bounds 1.0, as the shipped inis' [GENERATOR] max_norm).  Each is warmed up, then timed in
``--reps`` alternating blocks of ``--steps`` G + D iteration pairs (host clock around a synchronised block, as
bench.py times its steps).  The optimizer steps alone are timed from device events around ``optimizer.step()``
(``--steps`` pairs, after the blocks).  One JSON line:

    python tools/bench_grad_clip.py --out profiles/grad_clip.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def make(dev, clip: bool):
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
    gc = cfg.grad_clip
    gc.clip_generator = gc.clip_discriminator = gc.log_grad_norms = clip
    cfg.generator.max_norm = gc.max_norm_discriminator = 1.0
    torch.manual_seed(cfg.env.fixed_seed)
    return wind_field_GAN_3D(cfg), cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gan_sr_wind_field_amd import _lib
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    _lib.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    runs = {}
    for tag, clip in (("off", False), ("clip", True)):
        gan, cfg = make(dev, clip)
        LR, HR, Z, x, y = (t.to(dev) for t in synthetic_batch(1, 32, 128, cfg.scale, seed=2001))
        gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=dev), 1, 1)
        runs[tag] = dict(gan=gan, data=(LR, HR, Z), it=0, ms=[], opt_ms={"G": [], "D": []})
    assert runs["clip"]["gan"].optimizer_G.max_grad_norm == 1.0

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
    # the optimizer steps on their own (device time between events around step())
    for r in runs.values():
        gan = r["gan"]
        ev = {}
        for w, opt in (("G", gan.optimizer_G), ("D", gan.optimizer_D)):
            def pre(*_, w=w):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev[w] = [e]

            def post(*_, w=w):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev[w].append(e)
                r["_pending"].append((w, ev[w]))
            # (pre-hooks run in registration order: this one after the model's own, right in front of the update)
            opt.register_step_pre_hook(pre)
            opt.register_step_post_hook(post)
        r["_pending"] = []
        pairs(r, args.steps)
        torch.cuda.synchronize()
        for w, (e0, e1) in r["_pending"]:
            r["opt_ms"][w].append(e0.elapsed_time(e1))
        del r["_pending"]
    out = {"workload": "C3' G+D step, bf16, batch 1, LR 32x32x128", "device": torch.cuda.get_device_name(dev),
           "steps_per_block": args.steps, "blocks": args.reps}
    for tag, r in runs.items():
        out[f"ms_per_step_{tag}"] = round(statistics.median(r["ms"]), 3)
        out[f"ms_per_step_{tag}_blocks"] = [round(v, 3) for v in r["ms"]]
        for w in ("G", "D"):
            out[f"opt_step_{w}_ms_{tag}"] = round(statistics.median(r["opt_ms"][w]), 4) if r["opt_ms"][w] else None
    out["delta_ms_per_step"] = round(out["ms_per_step_clip"] - out["ms_per_step_off"], 3)
    norms = runs["clip"]["gan"].get_grad_norms()
    out["last_grad_norms"] = {k: float(v) for k, v in norms.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
