#!/usr/bin/env python
"""Cost of the per-level diagnostics ([DIAGNOSTICS]; one device): ``hip_ops.level_diagnostics`` (the two kernels of
csrc/diagnostics.hip and the wrapper's workspace allocation) at 128 x 128 x 128 and at the shipped test shape
128 x 128 x 10, for one and for four fields per call.

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the wrapper, with the bytes the algorithm needs - 10 floats read per voxel (three components of HR, SR and the
  baseline, and the altitude; the neighbours of the divergence are other voxels' own reads) - over that time, and that
  rate as a fraction of 8 TB/s;
* ``diagnostics.level_sums_reference`` in fp32 on the device, the composed path (ATen reductions and the fused
  ``wsr_wind_gradient``); no earlier path exists in the project.  Its sums are checked against the kernel's before
  anything is timed: every sum within 1e-4 of the largest level of that sum (the signed speed biases: of the speed sum).

One JSON line:

    python tools/bench_diagnostics.py --out profiles/diagnostics.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"128x128x128": (128, 128, 128), "test_128x128x10": (128, 128, 10)}
HBM_BYTES_PER_S = 8e12
FLOATS_PER_VOXEL = 10


def events_ms(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def bench_shape(dims, B, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.diagnostics import level_sums_reference

    X, Y, NZ = dims
    g = torch.Generator(device=dev).manual_seed(2001)
    HR = torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    SR = HR + 0.1 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    TL = HR + 0.3 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    x = torch.arange(X, device=dev, dtype=torch.float32) * 200.0
    y = torch.arange(Y, device=dev, dtype=torch.float32) * 200.0
    Z = (300 * torch.rand((B, 1, X, Y, 1), device=dev, generator=g)
         + torch.cumsum(5 + 40 * torch.rand((B, 1, X, Y, NZ), device=dev, generator=g), -1)).contiguous()

    def hip_fn():
        return hip_ops.level_diagnostics(HR, SR, TL, x, y, Z)

    def ref_fn():
        return level_sums_reference(HR, SR, TL, x, y, Z, dtype=torch.float32)

    # the comparison computes what the kernel computes
    got, ref = hip_fn(), ref_fn().double()
    scale = got.abs().amax(dim=(0, 1))  # per sum: its largest level
    scale[3] = scale[4] = scale[0]  # (the signed speed biases cancel: the size of their terms)
    rel = float(((got - ref).abs().amax(dim=(0, 1)) / scale).max())
    assert rel < 1e-4, rel
    nbytes = B * X * Y * NZ * FLOATS_PER_VOXEL * 4
    for fn in (hip_fn, ref_fn):  # warm-up (allocator, code objects)
        for _ in range(3):
            fn()
    hip_ms, ref_ms = [], []
    for _ in range(args.reps):
        hip_ms.append(events_ms(hip_fn, args.calls))
        ref_ms.append(events_ms(ref_fn, args.calls))
    h, r = statistics.median(hip_ms), statistics.median(ref_ms)
    return {"shape": [B, 3, X, Y, NZ], "hip_us": round(h * 1e3, 2), "reference_us": round(r * 1e3, 2),
            "reference_over_hip": round(r / h, 2), "bytes": nbytes, "hip_TB_per_s": round(nbytes / (h * 1e-3) / 1e12, 3),
            "hip_share_of_8_TB_per_s": round(nbytes / (h * 1e-3) / HBM_BYTES_PER_S, 3),
            "max_difference_to_reference_over_scale": rel,
            "hip_us_blocks": [round(v * 1e3, 2) for v in hip_ms], "reference_us_blocks": [round(v * 1e3, 2) for v in ref_ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--reps", type=int, default=5, help="alternating blocks per measurement")
    ap.add_argument("--calls", type=int, default=20, help="calls per block")
    ap.add_argument("--batches", default="1,4", help="fields per call")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_diagnostics.py measures on the GPU: no device found")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in args.shapes.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            res[f"{tag}_B{B}"] = bench_shape(SHAPES[tag], B, args, dev)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
