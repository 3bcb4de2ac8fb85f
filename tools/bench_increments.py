#!/usr/bin/env python
"""Cost of the structure functions ([INCREMENTS]; one device): ``hip_ops.level_increments`` (the two kernels of
csrc/increments.hip and the wrapper's workspace allocation) at 128 x 128 x 128 and at 128 x 128 x 10, one and eight fields
per call, with the default separations (1, 2, 4, 8, 16) on gaussian wind of standard deviation 0.3.

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the wrapper, with the bytes it must read (u, v and w of three fields, once) over that time as a share of 8 TB/s;
* ``increments.level_increments_reference`` in fp32 on the device: the composed path (per source, separation, direction
  and kind two sliced copies, three products and three reductions).  Its sums are checked against the kernel's before
  anything is timed: orders 2 and 4 within 1e-4 of the sum, order 3 within 1e-4 of sqrt(S2 S4) (both paths add fp32 terms,
  in different orders).

The requirement of the feature: the kernel's median below the composed path's at all four shapes, with no block of one
overlapping a block of the other (``blocks_do_not_overlap``).

And the loop of ``run.py --test`` under ``[EVAL]`` (``test._device_loop``, model and synthetic fields as in
tools/bench_eval.py) without and with the section - without it the loop is the parent commit's - at the shipped test shape
(128 x 128 x 10, fp32) and at C3' (128^3, bf16 generator): wall time per field, host clock around a synchronised pass,
alternating blocks, medians; the spread of the blocks stands beside them.  The files go to a temporary folder.

One JSON line:

    python tools/bench_increments.py --out profiles/increments.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fss import CASES, HBM_BYTES_PER_S, UVW, events_ms  # noqa: E402  (the four shapes of bench_fss.py)

SEPARATIONS = (1, 2, 4, 8, 16)


def bench_case(dims, args, dev):
    import ctypes

    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.increments import level_increments_reference

    B, X, Y, NZ = dims
    g = torch.Generator(device=dev).manual_seed(2001)
    HR = 0.3 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    SR = HR + 0.02 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    TL = HR + 0.05 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)

    def hip_fn():
        return hip_ops.level_increments(HR, SR, TL, SEPARATIONS)

    def ref_fn():
        return level_increments_reference(HR, SR, TL, SEPARATIONS, dtype=torch.float32)

    got, ref = hip_fn(), ref_fn()  # the comparison computes what the kernel computes
    scale = ref[..., [0, 0, 2]].clone()
    scale[..., 1] = (ref[..., 0] * ref[..., 2]).sqrt()
    worst = float(((got - ref).abs() / scale).max())
    assert worst <= 1e-4, worst
    fns = (hip_fn, ref_fn)
    for fn in fns:  # warm-up (allocator, code objects)
        for _ in range(3):
            fn()
    ms = [[] for _ in fns]
    for _ in range(args.reps):
        for acc, fn in zip(ms, fns):
            acc.append(events_ms(fn, args.calls))
    h, r = statistics.median(ms[0]), statistics.median(ms[1])
    nbytes = 3 * 3 * B * X * Y * NZ * 4
    sep = (ctypes.c_int32 * len(SEPARATIONS))(*SEPARATIONS)
    return {"shape": [B, 3, X, Y, NZ], "separations": list(SEPARATIONS),
            "level_chunk": hip_ops.increments_level_chunk(NZ, SEPARATIONS),
            "worst_relative_difference_to_reference": worst, "hip_us": round(h * 1e3, 2), "bytes_read_once": nbytes,
            "hip_share_of_8TBps": round(nbytes / (h * 1e-3) / HBM_BYTES_PER_S, 4),
            "workspace_MB": round(4 * int(hip_ops._lib.lib().wsr_level_increments_workspace_floats(
                B, X, Y, NZ, sep, len(SEPARATIONS))) / 1e6, 3),
            "reference_us": round(r * 1e3, 2), "reference_over_hip": round(r / h, 2),
            "blocks_do_not_overlap": max(ms[0]) < min(ms[1]),
            "hip_us_blocks": [round(v * 1e3, 2) for v in ms[0]], "reference_us_blocks": [round(v * 1e3, 2) for v in ms[1]]}


def bench_loop(spec, args, dev):
    import tempfile
    import time

    import torch

    import bench_eval as be
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    folder = tempfile.mkdtemp(prefix="bench_increments_")
    gan, cfg = be.make(dev, spec["nz"], spec["dtype"], folder)
    LR, HR, Z, x, y = synthetic_batch(args.fields, spec["lr"], spec["nz"], cfg.scale, seed=2001)
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    gan.G.eval()
    empty = torch.zeros(0)
    fields = [(LR[i], HR[i], Z[i], f"f{i}", empty, empty) for i in range(args.fields)]
    be.section(cfg, True, args.batch_size)

    def loop_pass(on):
        acc = [tmod._Increments(lambda HR, SR, TL, Z: hip_ops.level_increments(HR, SR, TL, SEPARATIONS), SEPARATIONS, UVW,
                                200.0, False, cfg.name, "", folder)] if on else []
        loader = torch.utils.data.DataLoader(fields, batch_size=args.batch_size, shuffle=False)
        with open(os.devnull, "w") as o:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tmod._device_loop(cfg, gan, loader, UVW, args.fields, tmod._LevelSet(o, acc))
            for a in acc:
                a.close()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.fields

    for on in (False, True):  # warm-up
        loop_pass(on)
    off_ms, on_ms = [], []
    for _ in range(args.reps):
        off_ms.append(loop_pass(False))
        on_ms.append(loop_pass(True))
    a, b = statistics.median(off_ms), statistics.median(on_ms)
    return {"HR": list(HR.shape[1:]), "compute_dtype": spec["dtype"], "fields": args.fields, "batch_size": args.batch_size,
            "ms_per_field_without": round(a, 3), "ms_per_field_with": round(b, 3), "increase": round(b / a - 1, 4),
            "spread_without": round((max(off_ms) - min(off_ms)) / a, 4), "spread_with": round((max(on_ms) - min(on_ms)) / b, 4),
            "without_blocks": [round(v, 3) for v in off_ms], "with_blocks": [round(v, 3) for v in on_ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--reps", type=int, default=5, help="alternating blocks per measurement")
    ap.add_argument("--calls", type=int, default=10, help="calls per block")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--loops", default="test_128x128x10,c3_128x128x128", help="run.py --test loops to time ('' for none)")
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=4, help="[EVAL] batch_size of the loops")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_increments.py measures on the GPU: no device found")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in args.cases.split(","):
        res[tag] = bench_case(CASES[tag], args, dev)
        print(f"{tag}: {res[tag]['hip_us']} us, reference {res[tag]['reference_us']} us", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if args.loops:
        import bench_eval as be

        for tag in args.loops.split(","):
            res["loop_" + tag] = bench_loop(be.SHAPES[tag], args, dev)
            print(f"loop {tag}: {res['loop_' + tag]['ms_per_field_without']} -> {res['loop_' + tag]['ms_per_field_with']} ms "
                  f"per field", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
