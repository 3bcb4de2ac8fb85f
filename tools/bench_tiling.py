#!/usr/bin/env python
"""Cost of tiled whole-domain inference ([TILE], tile = 16, overlap = 4; one device) at C3' (LR 32 x 32 x 128, x4, bf16
generator) and at the shipped test shape (LR 32 x 32 x 10, fp32 generator), which the plain forward handles with room to
spare.

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the two kernels: ``hip_ops.tile_gather`` on LR and on the terrain tensor Z, and ``hip_ops.tile_stitch`` without and
  with the seam map, with the bytes the algorithm needs (tiles read and written for the gather; tiles read once and the
  output [and the seam] written for the stitch) over that time, and that rate as a fraction of 8 TB/s;
* a device-side ATen composition of the same work, written here: slice copies stacked for the gather; a loop of
  weighted adds into a zeroed output plus a divide by the accumulated weights for the stitch (and a second loop for the
  seam).  Its results are checked against the kernels' before anything is timed;
* a whole ``gan.G_tiled`` call beside one plain generator forward of the whole domain.

One JSON line:

    python tools/bench_tiling.py --out profiles/tiling.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c3_128x128x128": dict(lr=32, nz=128, dtype="bf16"), "test_128x128x10": dict(lr=32, nz=10, dtype="fp32")}
HBM_BYTES_PER_S = 8e12


def make(dev, nz, dtype):
    import torch
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.GAN_models.wind_field_GAN_3D import wind_field_GAN_3D

    cfg = Config(os.path.join(ROOT, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_local.ini"))
    cfg.is_train, cfg.is_test, cfg.is_use = False, True, False
    cfg.gpu_id, cfg.device = dev.index, dev
    cfg.compute_dtype = dtype
    cfg.gan_config.enable_slicing = False
    cfg.gan_config.number_of_z_layers = nz
    torch.manual_seed(cfg.env.fixed_seed)
    return wind_field_GAN_3D(cfg), cfg


def events_ms(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def axis_weight_rows(starts, T, N, R, dev):
    """(n, N) fp32 on the device: the integer ramp of every tile of an axis (include/windsr_hip.h), 0 outside the tile"""
    import torch
    i = torch.arange(N, device=dev)[None, :]
    a = torch.tensor(starts, device=dev)[:, None]
    p = i - a
    left = torch.where(a == 0, torch.full_like(p, R + 1), torch.clamp(p + 1, max=R + 1))
    right = torch.where(a + T == N, torch.full_like(p, R + 1), torch.clamp(T - p, max=R + 1))
    return torch.where((p >= 0) & (p < T), torch.minimum(left, right), torch.zeros_like(p)).float()


def aten_gather(src, x0, y0, tx, ty):
    import torch
    return torch.stack([src[:, :, a:a + tx, b:b + ty] for a, b in zip(x0, y0)])


def aten_stitch(tiles, xs, ys, X, Y, wx, wy, with_seam):
    """weighted adds into a zeroed output, then a divide; the seam from a second loop"""
    import torch
    n, B, C, Tx, Ty, NZ = tiles.shape
    out = torch.zeros((B, C, X, Y, NZ), device=tiles.device)
    norm = (wx.sum(0)[:, None] * wy.sum(0)[None, :])[None, None, :, :, None]
    each = [(ix * len(ys) + iy, a, b, (wx[ix, a:a + Tx, None] * wy[iy, None, b:b + Ty])[None, None, :, :, None])
            for ix, a in enumerate(xs) for iy, b in enumerate(ys)]
    for k, a, b, w in each:
        out[:, :, a:a + Tx, b:b + Ty] += w * tiles[k]
    out /= norm
    if not with_seam:
        return out
    seam = torch.zeros_like(out)
    for k, a, b, w in each:
        seam[:, :, a:a + Tx, b:b + Ty] += w * (tiles[k] - out[:, :, a:a + Tx, b:b + Ty]) ** 2
    seam /= norm
    return out, seam


def bench_shape(tag, spec, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.process_data import synthetic_batch
    from gan_sr_wind_field_amd.tiling import tile_starts

    B, tile, overlap = args.batch, args.tile, args.overlap
    gan, cfg = make(dev, spec["nz"], spec["dtype"])
    gan.G.eval()
    s = cfg.scale
    LR, HR, Z, _, _ = synthetic_batch(B, spec["lr"], spec["nz"], s, seed=2001)
    LR_d, Z_d = LR.to(dev).contiguous(), Z.to(dev).contiguous()
    Xl, Yl, NZ = LR.shape[2], LR.shape[3], LR.shape[4]
    xs, ys = tile_starts(Xl, tile, overlap), tile_starts(Yl, tile, overlap)
    tx, ty = min(tile, Xl), min(tile, Yl)
    x0, y0 = [a for a in xs for _ in ys], [b for _ in xs for b in ys]
    hx, hy, hx0, hy0 = [a * s for a in xs], [b * s for b in ys], [a * s for a in x0], [b * s for b in y0]
    X, Y, Tx, Ty, R = Xl * s, Yl * s, tx * s, ty * s, overlap * s
    n = len(x0)
    tiles = torch.randn((n, B, 3, Tx, Ty, NZ), device=dev)  # stand-in generator outputs
    wx, wy = axis_weight_rows(hx, Tx, X, R, dev), axis_weight_rows(hy, Ty, Y, R, dev)
    out = {"LR": list(LR.shape), "HR": list(HR.shape), "tile": tile, "overlap": overlap, "tiles": n,
           "compute_dtype": spec["dtype"]}

    # the baseline computes what the kernels compute
    assert torch.equal(aten_gather(LR_d, x0, y0, tx, ty), hip_ops.tile_gather(LR_d, x0, y0, tx, ty))
    assert torch.equal(aten_gather(Z_d, hx0, hy0, Tx, Ty), hip_ops.tile_gather(Z_d, hx0, hy0, Tx, Ty))
    ko, ks = hip_ops.tile_stitch(tiles, hx, hy, X, Y, R, R, with_seam=True)
    ao, asm = aten_stitch(tiles, hx, hy, X, Y, wx, wy, True)
    out["blend_max_abs_difference_to_aten"] = float((ko - ao).abs().max())
    out["seam_max_abs_difference_to_aten"] = float((ks - asm).abs().max())
    assert out["blend_max_abs_difference_to_aten"] < 1e-5 and out["seam_max_abs_difference_to_aten"] < 1e-4
    del ko, ks, ao, asm

    fb = 4  # bytes per float
    timed = {
        "gather_LR": (lambda: hip_ops.tile_gather(LR_d, x0, y0, tx, ty), lambda: aten_gather(LR_d, x0, y0, tx, ty),
                      2 * n * B * LR.shape[1] * tx * ty * NZ * fb),
        "gather_Z": (lambda: hip_ops.tile_gather(Z_d, hx0, hy0, Tx, Ty), lambda: aten_gather(Z_d, hx0, hy0, Tx, Ty),
                     2 * n * B * Tx * Ty * NZ * fb),
        "stitch": (lambda: hip_ops.tile_stitch(tiles, hx, hy, X, Y, R, R),
                   lambda: aten_stitch(tiles, hx, hy, X, Y, wx, wy, False), (tiles.numel() + HR.numel()) * fb),
        "stitch_seam": (lambda: hip_ops.tile_stitch(tiles, hx, hy, X, Y, R, R, with_seam=True),
                        lambda: aten_stitch(tiles, hx, hy, X, Y, wx, wy, True), (tiles.numel() + 2 * HR.numel()) * fb),
    }
    for name, (hip_fn, aten_fn, nbytes) in timed.items():
        for fn in (hip_fn, aten_fn):  # warm-up (allocator, code objects)
            for _ in range(3):
                fn()
        hip_ms, aten_ms = [], []
        for _ in range(args.reps):
            hip_ms.append(events_ms(hip_fn, args.calls))
            aten_ms.append(events_ms(aten_fn, args.calls))
        h, a = statistics.median(hip_ms), statistics.median(aten_ms)
        out[name] = {"hip_us": round(h * 1e3, 2), "aten_us": round(a * 1e3, 2), "aten_over_hip": round(a / h, 2),
                     "bytes": nbytes, "hip_TB_per_s": round(nbytes / (h * 1e-3) / 1e12, 3),
                     "hip_share_of_8_TB_per_s": round(nbytes / (h * 1e-3) / HBM_BYTES_PER_S, 3),
                     "hip_us_blocks": [round(v * 1e3, 2) for v in hip_ms], "aten_us_blocks": [round(v * 1e3, 2) for v in aten_ms]}
    del tiles

    # the whole call beside the plain forward of the whole domain
    def plain():
        with torch.no_grad():
            return gan.G(LR_d, Z_d)

    whole = {"G_tiled": lambda: gan.G_tiled(LR_d, Z_d, tile=tile, overlap=overlap, tiles_per_forward=args.tiles_per_forward,
                                            with_seam=True),
             "G_plain": plain}
    ms = {k: [] for k in whole}
    for fn in whole.values():
        fn()
    for _ in range(args.reps):
        for k, fn in whole.items():
            ms[k].append(events_ms(fn, args.g_calls))
    for k in whole:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_blocks"] = [round(v, 3) for v in ms[k]]
    out["tiles_per_forward"] = args.tiles_per_forward
    out["G_tiled_over_G_plain"] = round(out["G_tiled_ms"] / out["G_plain_ms"], 3)
    out["tiled_voxels_over_domain_voxels"] = round(n * tx * ty / (Xl * Yl), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--tile", type=int, default=16)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--tiles-per-forward", type=int, default=9, dest="tiles_per_forward")
    ap.add_argument("--batch", type=int, default=1, help="fields per call")
    ap.add_argument("--reps", type=int, default=5, help="alternating blocks per measurement")
    ap.add_argument("--calls", type=int, default=20, help="kernel calls per block")
    ap.add_argument("--g-calls", type=int, default=3, dest="g_calls", help="generator calls per block")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls": args.calls}
    for tag in args.shapes.split(","):
        res[tag] = bench_shape(tag, SHAPES[tag], args, dev)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
