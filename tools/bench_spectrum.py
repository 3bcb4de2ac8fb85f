#!/usr/bin/env python
"""Cost of the horizontal energy spectra ([SPECTRUM]; one device): ``hip_ops.level_spectra`` (the five kernels of
csrc/spectra.hip and the wrapper's workspace allocation) at 128 x 128 x 128 for one and for four fields per call and at
64 x 64 x 10 for four fields.

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the wrapper, with the multiply-adds of its two transform loops computed from the shape - per sample
  9 X (Y/2 + 1) Y NZ * 2 in the row pass and 9 (Y/2 + 1) X X NZ * 4 in the column pass - over that time, and that rate as
  a fraction of the fp32 vector peak (157.3 TFLOP/s = 78.65 T multiply-adds/s);
* ``spectra.level_spectra_reference`` in fp32 on the device: ``torch.fft.rfft2`` and ``index_add_``, the composed path.
  Its sums are checked against the kernel's before anything is timed: every sum within 1e-4 of the largest bin of that
  sum.  Where the device build has no FFT the tool says so and reports the kernel alone.

And the loop of ``run.py --test`` under ``[EVAL]`` (``test._device_loop``, model and synthetic fields as in
tools/bench_eval.py) without and with the section - without it the loop is the parent commit's - at the shipped test shape
(128 x 128 x 10, fp32) and at C3' (128^3, bf16 generator): wall time per field, host clock around a synchronised pass,
alternating blocks, medians.

One JSON line:

    python tools/bench_spectrum.py --out profiles/spectrum.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"128x128x128_B1": (1, 128, 128, 128), "128x128x128_B4": (4, 128, 128, 128), "64x64x10_B4": (4, 64, 64, 10)}
FP32_VECTOR_FMA_PER_S = 157.3e12 / 2


def events_ms(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def multiply_adds(B, X, Y, NZ):
    ky = Y // 2 + 1
    return B * 9 * (X * ky * Y * NZ * 2 + ky * X * X * NZ * 4)


def bench_case(dims, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.spectra import level_spectra_reference

    B, X, Y, NZ = dims
    g = torch.Generator(device=dev).manual_seed(2001)
    HR = torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    SR = HR + 0.1 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    TL = HR + 0.3 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)

    def hip_fn():
        return hip_ops.level_spectra(HR, SR, TL, args.window)

    def ref_fn():
        return level_spectra_reference(HR, SR, TL, args.window, dtype=torch.float32)

    got = hip_fn()
    res = {"shape": [B, 3, X, Y, NZ], "window": args.window}
    try:  # the comparison computes what the kernel computes
        ref = ref_fn().double()
        rel = float(((got - ref).abs().amax(dim=(0, 1, 2)) / got.abs().amax(dim=(0, 1, 2))).max())
        assert rel < 1e-4, rel
        res["max_difference_to_reference_over_scale"] = rel
        fns = (hip_fn, ref_fn)
    except RuntimeError as e:
        res["reference"] = f"torch.fft is not available on this device build: {str(e).splitlines()[0]}"
        print(res["reference"], file=sys.stderr)
        fns = (hip_fn,)
    for fn in fns:  # warm-up (allocator, code objects, FFT plans)
        for _ in range(3):
            fn()
    ms = [[] for _ in fns]
    for _ in range(args.reps):
        for acc, fn in zip(ms, fns):
            acc.append(events_ms(fn, args.calls))
    h = statistics.median(ms[0])
    fma = multiply_adds(B, X, Y, NZ)
    res.update({"hip_us": round(h * 1e3, 2), "multiply_adds": fma, "hip_T_multiply_adds_per_s": round(fma / (h * 1e-3) / 1e12, 3),
                "hip_share_of_fp32_vector_peak": round(fma / (h * 1e-3) / FP32_VECTOR_FMA_PER_S, 4),
                "workspace_MB": round(4 * int(hip_ops._lib.lib().wsr_level_spectra_workspace_floats(B, X, Y, NZ)) / 1e6, 1),
                "hip_us_blocks": [round(v * 1e3, 2) for v in ms[0]]})
    if len(fns) == 2:
        r = statistics.median(ms[1])
        res.update({"reference_us": round(r * 1e3, 2), "reference_over_hip": round(r / h, 2),
                    "reference_us_blocks": [round(v * 1e3, 2) for v in ms[1]]})
    return res


def bench_loop(spec, args, dev):
    import tempfile
    import time

    import torch

    import bench_eval as be
    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    folder = tempfile.mkdtemp(prefix="bench_spectrum_")
    gan, cfg = be.make(dev, spec["nz"], spec["dtype"], folder)
    LR, HR, Z, x, y = synthetic_batch(args.fields, spec["lr"], spec["nz"], cfg.scale, seed=2001)
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    gan.G.eval()
    empty = torch.zeros(0)
    fields = [(LR[i], HR[i], Z[i], f"f{i}", empty, empty) for i in range(args.fields)]
    be.section(cfg, True, args.batch_size)
    cfg.spectrum.window = args.window
    uvw = 30.0

    def loop_pass(on):
        from gan_sr_wind_field_amd import hip_ops

        acc = [tmod._Spectrum(lambda HR, SR, TL, Z: hip_ops.level_spectra(HR, SR, TL, args.window), uvw, 200.0, False,
                              cfg.name, "", folder)] if on else []
        loader = torch.utils.data.DataLoader(fields, batch_size=args.batch_size, shuffle=False)
        with open(os.devnull, "w") as o:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tmod._device_loop(cfg, gan, loader, uvw, args.fields, tmod._LevelSet(o, acc))
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
            "without_blocks": [round(v, 3) for v in off_ms], "with_blocks": [round(v, 3) for v in on_ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--reps", type=int, default=5, help="alternating blocks per measurement")
    ap.add_argument("--calls", type=int, default=10, help="calls per block")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--window", default="hann", choices=("hann", "none"))
    ap.add_argument("--loops", default="test_128x128x10,c3_128x128x128", help="run.py --test loops to time ('' for none)")
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=4, help="[EVAL] batch_size of the loops")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectrum.py measures on the GPU: no device found")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in args.cases.split(","):
        res[tag] = bench_case(CASES[tag], args, dev)
        torch.cuda.empty_cache()
    if args.loops:
        import bench_eval as be

        for tag in args.loops.split(","):
            res["loop_" + tag] = bench_loop(be.SHAPES[tag], args, dev)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
