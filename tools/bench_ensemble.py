#!/usr/bin/env python
"""Cost of the geometric self-ensemble ([ENSEMBLE], members = 8; one device) at the shipped test shape
(128 x 128 x 10, x4, fp32 generator) and at C3' (128^3, x4, bf16 generator).

Per shape, between device events, in alternating blocks (``--reps`` blocks of ``--calls`` calls each, medians reported):

* the two kernels: ``hip_ops.dihedral_members`` on LR (a vector field) and on the terrain tensor Z (a scalar), and
  ``hip_ops.ensemble_reduce`` without and with the variance, with the bytes the algorithm needs (source read once and K
  copies written; K members read once and the mean [and the variance] written) over that time, and that rate as a
  fraction of 8 TB/s;
* a device-side ATen composition of the same transforms and of the same reduction (``torch.rot90`` / ``flip`` / ``cat``
  / ``stack`` / ``mean`` / ``var``), written here: the baseline - there is no earlier path in the project to compare
  with.  Its results are checked against the kernels' before anything is timed;
* a whole ``gan.G_ensemble`` call, beside one plain generator forward of the same batch and one of the K-fold batch.

One JSON line:

    python tools/bench_ensemble.py --out profiles/ensemble.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"test_128x128x10": dict(lr=32, nz=10, dtype="fp32"), "c3_128x128x128": dict(lr=32, nz=128, dtype="bf16")}
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


def aten_forward(t, code, is_vector):
    """member ``code`` of (B, C, X, Y, NZ) with ATen ops on the device"""
    import torch
    k, fx = code & 3, code >> 2
    r = torch.rot90(t, k, [2, 3])
    if is_vector and k:
        u, v = r[:, 0:1], r[:, 1:2]
        u, v = {1: (-v, u), 2: (-u, -v), 3: (v, -u)}[k]
        r = torch.cat([u, v, r[:, 2:]], dim=1)
    if fx:
        r = torch.flip(r, [2])
        if is_vector:
            r = torch.cat([-r[:, 0:1], r[:, 1:]], dim=1)
    return r


def aten_members(t, codes, is_vector):
    import torch
    return torch.stack([aten_forward(t, c, is_vector) for c in codes])


def aten_reduce(members, codes, with_var):
    import torch
    back = []
    for m, code in zip(members, codes):
        k, fx = code & 3, code >> 2
        if fx:
            m = torch.flip(m, [2])
            m = torch.cat([-m[:, 0:1], m[:, 1:]], dim=1)
        back.append(aten_forward(m, (4 - k) % 4, True))
    back = torch.stack(back)
    mean = back.mean(dim=0)
    return (mean, back.var(dim=0, unbiased=False)) if with_var else mean


def bench_shape(tag, spec, args, dev):
    import torch
    from gan_sr_wind_field_amd import hip_ops
    from gan_sr_wind_field_amd.ensemble import member_codes
    from gan_sr_wind_field_amd.process_data import synthetic_batch

    K, B = args.members, args.batch
    codes = member_codes(K)
    gan, cfg = make(dev, spec["nz"], spec["dtype"])
    gan.G.eval()
    LR, HR, Z, _, _ = synthetic_batch(B, spec["lr"], spec["nz"], cfg.scale, seed=2001)
    LR_d, Z_d = LR.to(dev).contiguous(), Z.to(dev).contiguous()
    SR_m = torch.randn((K,) + tuple(HR.shape), device=dev)  # stand-in member outputs (K, B, 3, X, Y, NZ)
    out = {"LR": list(LR.shape), "HR": list(HR.shape), "members": K, "compute_dtype": spec["dtype"]}

    # the baseline computes what the kernels compute
    assert torch.equal(aten_members(LR_d, codes, True), hip_ops.dihedral_members(LR_d, codes, True))
    assert torch.equal(aten_members(Z_d, codes, False), hip_ops.dihedral_members(Z_d, codes, False))
    km, kv = hip_ops.ensemble_reduce(SR_m, codes, with_var=True)
    am, av = aten_reduce(SR_m, codes, True)
    out["mean_max_abs_difference_to_aten"] = float((km - am).abs().max())
    out["var_max_abs_difference_to_aten"] = float((kv - av).abs().max())
    assert out["mean_max_abs_difference_to_aten"] < 1e-5 and out["var_max_abs_difference_to_aten"] < 1e-4
    del km, kv, am, av

    fb = 4  # bytes per float
    timed = {
        "members_LR": (lambda: hip_ops.dihedral_members(LR_d, codes, True), lambda: aten_members(LR_d, codes, True),
                       (1 + K) * LR_d.numel() * fb),
        "members_Z": (lambda: hip_ops.dihedral_members(Z_d, codes, False), lambda: aten_members(Z_d, codes, False),
                      (1 + K) * Z_d.numel() * fb),
        "reduce_mean": (lambda: hip_ops.ensemble_reduce(SR_m, codes), lambda: aten_reduce(SR_m, codes, False),
                        (K + 1) * HR.numel() * fb),
        "reduce_mean_var": (lambda: hip_ops.ensemble_reduce(SR_m, codes, with_var=True),
                            lambda: aten_reduce(SR_m, codes, True), (K + 2) * HR.numel() * fb),
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
    del SR_m

    # the whole call, beside the generator alone on B and on K * B samples
    LR_k = hip_ops.dihedral_members(LR_d, codes, True).flatten(0, 1)
    Z_k = hip_ops.dihedral_members(Z_d, codes, False).flatten(0, 1)

    def plain(lr, z):
        with torch.no_grad():
            return gan.G(lr, z)

    whole = {"G_ensemble": lambda: gan.G_ensemble(LR_d, Z_d, members=K, with_var=True),
             "G_batch": lambda: plain(LR_d, Z_d), "G_K_fold_batch": lambda: plain(LR_k, Z_k)}
    ms = {k: [] for k in whole}
    for fn in whole.values():
        fn()
    for _ in range(args.reps):
        for k, fn in whole.items():
            ms[k].append(events_ms(fn, args.g_calls))
    for k in whole:
        out[k + "_ms"] = round(statistics.median(ms[k]), 3)
        out[k + "_ms_blocks"] = [round(v, 3) for v in ms[k]]
    out["G_ensemble_minus_K_fold_forward_ms"] = round(out["G_ensemble_ms"] - out["G_K_fold_batch_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--members", type=int, default=8)
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
