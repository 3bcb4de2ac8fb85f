#!/usr/bin/env python
"""Cost of the hub-height evaluation ([HUB_HEIGHT]; one device): ``hip_ops.hub_height`` (the two kernels of
csrc/hub_height.hip and the wrapper's workspace allocation) at 128 x 128 x 128 and at 128 x 128 x 10, one and four fields
per call, for the heights 50, 100 and 150 m in log mode with the default power curve, without and with the per-column
planes.  Columns reach 120 .. 600 m above a rolling terrain from 2 m, the levels stretched quadratically.

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the wrapper, with the bytes it must read (u and v of three fields and the altitudes, once) over that time as a share of
  8 TB/s;
* ``hub_height.hub_height_reference`` on the device in fp32: the composed path (a count along z, gathers, element-wise
  maps and about twenty reductions per height).  Its counts must equal the kernel's and its sums agree to 1e-4 before
  anything is timed.

And the loop of ``run.py --test`` under ``[EVAL]`` (``test._device_loop``, model and synthetic fields as in
tools/bench_eval.py) without and with the section - without it the loop is the parent commit's - at the shipped test shape
(128 x 128 x 10, fp32) and at C3' (128^3, bf16 generator): wall time per field, host clock around a synchronised pass,
alternating blocks, medians; the spread of the blocks stands beside them.  The files go to a temporary folder.

One JSON line:

    python tools/bench_hub_height.py --out profiles/hub_height.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"128x128x128_B1": (1, 128, 128, 128), "128x128x10_B1": (1, 128, 128, 10),
         "128x128x128_B4": (4, 128, 128, 128), "128x128x10_B4": (4, 128, 128, 10)}
HBM_BYTES_PER_S = 8e12
UVW = 30.0
HEIGHTS = (50.0, 100.0, 150.0)
INTERP = "log"


def events_ms(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def make_tables(uvw, heights=HEIGHTS):
    from gan_sr_wind_field_amd.config.config import default_power_curve
    from gan_sr_wind_field_amd.hub_height import hub_height_tables

    return hub_height_tables(uvw, heights, *default_power_curve())


def bench_case(dims, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    B, X, Y, NZ = dims
    g = torch.Generator(device=dev).manual_seed(2001)
    i, j = torch.arange(X, device=dev)[:, None] / X, torch.arange(Y, device=dev)[None, :] / Y
    terrain = (200.0 + 200.0 * torch.sin(6.2832 * (1.3 * i + 0.2)) * torch.cos(6.2832 * (0.9 * j + 0.1))).contiguous()
    top = 120.0 + 480.0 * torch.rand((B, X, Y, 1), device=dev, generator=g)
    h = 2.0 + (top - 2.0) * (torch.arange(NZ, device=dev) / (NZ - 1)) ** 2
    Z = (terrain[None, :, :, None] + h)[:, None].contiguous()
    prof = (0.3 * torch.log(h / 0.05) / 9.39)[:, None]
    HR = (prof * torch.tensor([0.8, 0.6, 0.0], device=dev).view(1, 3, 1, 1, 1)
          + 0.03 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)).contiguous()
    SR = HR + 0.02 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    TL = HR + 0.05 * torch.randn((B, 3, X, Y, NZ), device=dev, generator=g)
    tables = make_tables(UVW)

    def hip_fn():
        return hip_ops.hub_height(HR, SR, TL, Z, terrain, tables, INTERP)

    def hip_cols_fn():
        return hip_ops.hub_height(HR, SR, TL, Z, terrain, tables, INTERP, True)

    def ref_fn():
        return hub_height_reference(HR, SR, TL, Z, terrain, tables, INTERP, dtype=torch.float32)

    got, ref = hip_fn(), ref_fn()  # the comparison computes what the kernel computes
    assert torch.equal(got[..., 0], ref[..., 0]), "validity counts differ"
    rel = float(((got - ref).abs() / ref.abs().clamp(min=1e-30))[..., 1:].max())
    assert rel < 1e-4, rel
    fns = (hip_fn, hip_cols_fn, ref_fn)
    for fn in fns:  # warm-up (allocator, code objects)
        for _ in range(3):
            fn()
    ms = [[] for _ in fns]
    for _ in range(args.reps):
        for acc, fn in zip(ms, fns):
            acc.append(events_ms(fn, args.calls))
    k, c, r = (statistics.median(m) for m in ms)
    nbytes = 7 * B * X * Y * NZ * 4
    return {"shape": [B, 3, X, Y, NZ], "heights": list(HEIGHTS), "interp": INTERP,
            "columns_per_chunk": hip_ops.hub_height_columns_per_chunk(NZ, len(HEIGHTS)),
            "valid_fraction": [round(v, 4) for v in (got[..., 0].sum(dim=0) / (B * X * Y)).tolist()],
            "max_rel_diff_to_fp32_reference": rel, "hip_us": round(k * 1e3, 2), "hip_with_planes_us": round(c * 1e3, 2),
            "bytes_read_once": nbytes, "hip_share_of_8TBps": round(nbytes / (k * 1e-3) / HBM_BYTES_PER_S, 4),
            "workspace_MB": round(4 * int(hip_ops._lib.lib().wsr_hub_height_workspace_floats(B, X, Y, NZ, len(HEIGHTS))) / 1e6, 3),
            "reference_us": round(r * 1e3, 2), "reference_over_hip": round(r / k, 2),
            "blocks_do_not_overlap": max(ms[0]) < min(ms[2]),
            "hip_us_blocks": [round(v * 1e3, 2) for v in ms[0]], "reference_us_blocks": [round(v * 1e3, 2) for v in ms[2]]}


def bench_loop(spec, args, dev):
    import tempfile
    import time

    import torch

    import bench_eval as be
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd import test as tmod
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    folder = tempfile.mkdtemp(prefix="bench_hub_height_")
    gan, cfg = be.make(dev, spec["nz"], spec["dtype"], folder)
    LR, HR, Z, x, y = synthetic_batch(args.fields, spec["lr"], spec["nz"], cfg.scale, seed=2001)
    gan.feed_xy_niter(x.to(dev), y.to(dev), torch.tensor(cfg.training.niter, device=dev), 1, 1)
    gan.G.eval()
    empty = torch.zeros(0)
    fields = [(LR[i], HR[i], Z[i], f"f{i}", empty, empty) for i in range(args.fields)]
    be.section(cfg, True, args.batch_size)
    uvw = UVW
    # a ground 2 m below the lowest level of any field, and three heights every column holds
    terrain = (Z[:, 0, :, :, 0].amin(dim=0) - 2.0).float().contiguous()
    h = Z[:, 0] - terrain[None, :, :, None]
    lo, hi = float(h[..., 0].max()), float(h[..., -1].min())
    heights = [round(lo + f * (hi - lo), 3) for f in (0.1, 0.5, 0.9)]
    tables, terrain_d = make_tables(uvw, heights), terrain.to(dev)

    def loop_pass(on):
        acc = [tmod._HubHeight(lambda HR, SR, TL, Z: hip_ops.hub_height(HR, SR, TL, Z, terrain_d, tables, INTERP), tables,
                               1.225, False, False, (x, y), cfg.name, "", folder)] if on else []
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
            "heights": heights, "ms_per_field_without": round(a, 3), "ms_per_field_with": round(b, 3),
            "increase": round(b / a - 1, 4),
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
        raise SystemExit("bench_hub_height.py measures on the GPU: no device found")
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in args.cases.split(","):
        res[tag] = bench_case(CASES[tag], args, dev)
        print(f"{tag}: {res[tag]['hip_us']} us ({res[tag]['hip_with_planes_us']} us with planes), reference "
              f"{res[tag]['reference_us']} us", file=sys.stderr, flush=True)
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
