#!/usr/bin/env python
"""Cost of the wind-speed distribution loss ([DISTRIBUTION_LOSS]; one device).

The kernel pair beside the composed path, at 128 x 128 x 128 and at 64 x 64 x 10 with batch 32, 32 bins: forward and
backward of ``L = sum(H(HR, SR)[1][..., :NS] * G)`` for a fixed random G - ``hip_ops.speed_soft_counts``
(csrc/distribution_loss.hip: a zero pass, one counting launch for both sources and a convert pass forward, one backward
that recomputes, workspace allocation included) against ``distribution_loss.soft_counts_reference`` with fp32 weights on
the device (the path of ``WSR_FUSED_DISTRIBUTION_LOSS=0``: torch element-wise ops, ``index_add`` and autograd).  The two
are checked against each other before anything is timed (tables within 1e-4 of the voxels of a row; gradients within 1e-3
of the largest element at all but 1e-3 of the elements, the derivative being piecewise constant in the bin).  Between
device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls, medians and the blocks themselves reported).

The train step of bench.py's presets C3' (full G + D step, bf16, batch 1, LR 32 x 32 x 128) and C1c (the cluster file as
shipped: batch 32, LR 16 x 16 x 10, D with slicing) without and with the section on ONE model - the section is read at
every generator pass - in a child process, host clock around synchronised blocks of ``--steps`` steps, alternating,
medians and the blocks themselves.  With ``--parent-tree DIR`` (a built checkout of the parent commit) a second child
runs the parent's step on the same device, its blocks in turn with the others: the gate is that the step without the
section lies within the parent's block-to-block spread of the parent's step.

One JSON line:

    python tools/bench_distribution_loss.py --parent-tree ../parent --out profiles/distribution_loss.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {"128x128x128_B1": (1, 128, 128, 128), "64x64x10_B32": (32, 64, 64, 10)}
UVW_MAX, BIN_WIDTH, NS = 20.0, 1.0, 32


def events_ms(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def bench_case(dims, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_reference, soft_tables

    B, X, Y, NZ = dims
    g = torch.Generator(device=dev).manual_seed(2001)
    HR = torch.rand((B, 3, X, Y, NZ), device=dev, generator=g) * 2 - 1
    SR = (HR + 0.1 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)).requires_grad_(True)
    G = torch.randn((B, NZ, NS), device=dev, generator=g, dtype=torch.float64)
    tables = soft_tables(UVW_MAX, BIN_WIDTH, NS)

    def run(sums):
        SR.grad = None
        p = sums()
        (p[1][..., :NS] * G).sum().backward()
        return p.detach(), SR.grad

    def hip_fn():
        return run(lambda: hip_ops.speed_soft_counts(HR, SR, tables))

    def ref_fn():
        return run(lambda: soft_counts_reference(HR, SR, tables, dtype=torch.float32))

    def hip_fwd():
        with torch.no_grad():
            return hip_ops.speed_soft_counts(HR, SR, tables)

    p, d = hip_fn()
    p_ref, d_ref = ref_fn()  # the comparison computes what the kernels compute
    rel_p = float((p - p_ref.double()).abs().max() / (X * Y))
    off = float(((d - d_ref).abs() > 1e-3 * d.abs().max()).double().mean())
    assert rel_p < 1e-4 and off < 1e-3, (rel_p, off)
    L = hip_ops._lib.lib()
    res = {"shape": [B, 3, X, Y, NZ], "speed_bins": NS, "geometry": list(hip_ops.speed_soft_counts_geometry(B, X, Y, NZ, NS)),
           "max_table_difference_over_row": rel_p, "gradient_elements_off_by_more_than_1e-3_of_scale": off}
    fns = {"hip": hip_fn, "hip_forward_only": hip_fwd, "reference": ref_fn}
    for fn in fns.values():  # warm-up (allocator, code objects, convolution plans)
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(events_ms(fn, args.calls))
    h = statistics.median(ms["hip"])
    vox = B * X * Y * NZ
    # what each launch must move: the forward reads u and v of HR and SR once, the backward reads u and v of SR and
    # writes all three channels of dsr
    res.update({"forward_must_move_MB": round(16 * vox / 1e6, 2), "backward_must_move_MB": round(20 * vox / 1e6, 2),
                "workspace_MB": round(4 * int(L.wsr_speed_soft_counts_workspace_floats(B, X, Y, NZ, NS)) / 1e6, 3)})
    for k, v in ms.items():
        res[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
        res[f"{k}_us_blocks"] = [round(t * 1e3, 2) for t in v]
    res["hip_backward_us"] = round(res["hip_us"] - res["hip_forward_only_us"], 2)
    res["reference_over_hip"] = round(statistics.median(ms["reference"]) / h, 2)
    return res


STEPS = {  # bench.py's presets of the same names: (ini, LR n, levels, batch, D slicing, what)
    "C3p": ("local", 32, 128, 1, False, "C3' G+D step, bf16, batch 1, LR 32x32x128"),
    "C1c": ("cluster", 16, 10, 32, True, "C1c G+D step, bf16, batch 32, LR 16x16x10, D with slicing"),
}


def step_worker(tree, preset):
    """one model of ``preset`` built from the checkout ``tree`` (this one, or a built checkout of the parent commit),
    timing one block of train steps per line of standard input: ``off K`` / ``on K`` -> one line, ms per step"""
    reply = os.fdopen(os.dup(1), "w")  # (whatever else the model prints goes to standard error)
    os.dup2(2, 1)
    sys.path.insert(0, tree)
    import torch
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    ini, n, nz, batch, slicing, _ = STEPS[preset]
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = Config(os.path.join(tree, "gan_sr_wind_field_amd", "config", f"wind_field_GAN_3D_config_{ini}.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = True, False, False
    cfg.gpu_id, cfg.device = dev.index, dev
    cfg.compute_dtype = "bf16"
    cfg.gan_config.enable_slicing = slicing
    cfg.gan_config.number_of_z_layers = nz
    cfg.training.niter = 150000
    cfg.training.d_g_train_period = 1
    torch.manual_seed(cfg.env.fixed_seed)
    gan = wind_field_GAN_3D(cfg)
    LR, HR, Z, x, y = (t.to(dev) for t in synthetic_batch(batch, n, nz, cfg.scale, seed=2001))
    gan.feed_xy_niter(x, y, torch.tensor(cfg.training.niter, device=dev), 1, 1)
    sl = getattr(cfg, "distribution_loss", None)  # (the parent commit has no such section: it is only ever asked for ``off``)
    if sl is not None:
        gan.set_wind_scale(UVW_MAX)
    it = 0
    print("ready", file=reply, flush=True)
    for line in sys.stdin:
        mode, k = line.split()
        if sl is not None:
            sl.present = mode == "on"  # (read at every generator pass)
            sl.weight, sl.bin_width = (0.1, BIN_WIDTH) if sl.present else (None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(int(k)):
            gan.optimize_parameters(LR, HR, Z, it)      # G-iteration
            gan.optimize_parameters(LR, HR, Z, it + 1)  # D-iteration
            gan.update_learning_rate()
            it += 2
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / int(k)
        term = float(gan.get_G_train_loss_dict_ref()["distribution"].detach()) if mode == "on" else None
        print(json.dumps({"ms": ms, "distribution": term}), file=reply, flush=True)


class Worker:
    """a ``step_worker`` in a fresh child process (the workers stay alive side by side; one of them runs at a time)"""

    def __init__(self, tree, preset):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, preset],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self.p.stdout.readline().strip() == "ready", f"the worker of {tree} did not start"

    def block(self, mode, k):
        self.p.stdin.write(f"{mode} {k}\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        assert line, "a worker ended early"
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def bench_step(args, preset):
    """ms per train step of ``preset`` without and with the section and, given ``--parent-tree``, of the parent commit's
    build: one block of each in turn, ``--reps`` times, medians and the blocks themselves.  The gate: without the section
    the median is within the parent's block-to-block spread (max - min of its blocks) of the parent's median."""
    trees = {"this": ROOT}
    if args.parent_tree:
        trees["parent"] = os.path.abspath(args.parent_tree)
    workers = {k: Worker(t, preset) for k, t in trees.items()}
    order = [(k, "off") for k in sorted(trees)] + [("this", "on")]  # parent off, this off, this on
    try:
        for k, mode in order:
            workers[k].block(mode, args.warmup)
        ms = {o: [] for o in order}
        term = None
        for _ in range(args.reps):
            for o in order:
                r = workers[o[0]].block(o[1], args.steps)
                ms[o].append(r["ms"])
                term = r["distribution"] if r["distribution"] is not None else term
    finally:
        for w in workers.values():
            w.close()
    off, on_ = ms[("this", "off")], ms[("this", "on")]
    a, b = statistics.median(off), statistics.median(on_)
    res = {"workload": STEPS[preset][5], "steps_per_block": args.steps, "ms_per_step_without": round(a, 3),
           "ms_per_step_with": round(b, 3), "delta_ms": round(b - a, 3), "increase": round(b / a - 1, 4),
           "without_blocks": [round(v, 3) for v in off], "with_blocks": [round(v, 3) for v in on_],
           "without_spread_ms": round(max(off) - min(off), 3), "with_spread_ms": round(max(on_) - min(on_), 3),
           "last_weighted_distribution_term": term}
    if "parent" in trees:
        par = ms[("parent", "off")]
        c = statistics.median(par)
        res.update({"parent_ms_per_step": round(c, 3), "parent_blocks": [round(v, 3) for v in par],
                    "parent_spread_ms": round(max(par) - min(par), 3), "without_minus_parent_ms": round(a - c, 3),
                    "gate_without_within_parent_spread": bool(abs(a - c) <= max(par) - min(par))})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--reps", type=int, default=5, help="alternating blocks per measurement")
    ap.add_argument("--calls", type=int, default=10, help="calls per block of the kernel measurements")
    ap.add_argument("--steps", type=int, default=5, help="train steps per block")
    ap.add_argument("--warmup", type=int, default=3, help="train steps before the first block, each way")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-step", action="store_true", help="leave the train steps out")
    ap.add_argument("--step-presets", default=",".join(STEPS), help="train steps to measure")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its step beside this one's")
    ap.add_argument("--worker", nargs=2, metavar=("TREE", "PRESET"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return step_worker(*args.worker)
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_distribution_loss.py measures on the GPU: no device found")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in [t for t in args.cases.split(",") if t]:
        res[tag] = bench_case(CASES[tag], args, dev)
        torch.cuda.empty_cache()
    # the shapes at which the pair takes longer than the composition
    res["pair_slower_than_reference_at"] = [t for t in CASES if res.get(t, {}).get("reference_over_hip", 1.0) < 1.0]
    if not args.no_step:
        torch.cuda.empty_cache()
        for preset in [t for t in args.step_presets.split(",") if t]:
            res[f"step_{preset}"] = bench_step(args, preset)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
