#!/usr/bin/env python
"""The cost of ``[DEGRADATION]`` (degradation.py, csrc/data_gather.hip) at the C1c data shape, one process, one device.

Shape: the cluster ini as shipped (batch 32, 128x128x10 samples, ``interpolate_z``, z channel - 4 input channels -,
``enable_slicing`` with 64x64 slices, x4, rotation and mirrors on), on five days of synthetic HARMONIE-SIMRA-format data
written from a seed into a scratch directory (tools/bench_input_pipeline.py has the same set-up).  One JSON line:

* ``gather_us``: ``wsr_gather_batch`` and ``wsr_gather_batch_filtered`` under ``box`` and ``gaussian`` sigma 2
  (``channels = all``), each launch timed by its own pair of device events, the three alternating over ``--launches``
  different batches of draws after a warm-up: the median, and the 10th / 90th percentile as the spread;
* ``gather_bytes``: per variant, ``unique`` - every output float written once, every store float the launch needs read
  once (the filtered LR planes need the whole tap footprint inside the slice), descriptors and tables - and ``loaded``,
  the bytes the load instructions ask for (one store float per tap and output float);
* ``cpu_loader_ms_per_batch``: ``DataLoader(pin_memory=True)`` without the section and with ``gaussian`` sigma 2, at 0
  and 4 workers (``--batches`` batches after the prefetch has drained);
* ``train_ms_per_it``: ``run.py --train`` with ``[DATA] device_resident = True``, wall time per iteration after
  ``--warm`` iterations, ``--reps`` runs without the section and with ``gaussian`` sigma 2, alternating; bf16 compute,
  ``d_g_train_period`` 1, no validation or checkpoints.

    python tools/bench_degradation.py --out profiles/degradation.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CLUSTER_INI = os.path.join(ROOT, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_cluster.ini")
START, END = [2018, 4, 1], [2018, 4, 5]
GAUSS = "\n[DEGRADATION]\nkernel = gaussian\nsigma = 2.0\n"


def write_ini(path, name, niter, workers, extra=""):
    from gan_sr_wind_field_amd.config.config import Config

    cfg = Config(CLUSTER_INI)
    cfg.name = name
    cfg.also_log_to_terminal = cfg.use_tensorboard_logger = False
    cfg.compute_dtype = "bf16"
    cfg.gan_config.start_date, cfg.gan_config.end_date = START, END
    cfg.dataset_train.num_workers = cfg.dataset_val.num_workers = workers
    cfg.training.niter, cfg.training.d_g_train_period = niter, 1
    cfg.training.val_period = cfg.training.save_model_period = cfg.training.log_period = 10 ** 9
    with open(path, "w") as f:
        f.write(cfg.asINI() + extra)
    return Config(path)


def cpu_loader_ms(ds, workers, batches, batch, dev):
    warm = 2 * workers + 1  # (prefetch_factor 2: batches the workers may have ready before the clock starts)
    sampler = torch.utils.data.RandomSampler(ds, replacement=True, num_samples=batch * (batches + warm))
    dl = torch.utils.data.DataLoader(ds, batch_size=batch, sampler=sampler, num_workers=workers, pin_memory=True,
                                     drop_last=True)
    for i, (LR, HR, Z) in enumerate(dl):
        LR, HR, Z = (t.to(dev, non_blocking=True) for t in (LR, HR, Z))
        torch.cuda.synchronize(dev)
        if i == warm - 1:
            t0 = time.perf_counter()
    return (time.perf_counter() - t0) / batches * 1e3


def gather_bytes(B, cin, s, S, NZ, R, n_filt):
    """algorithmic bytes of one launch on S x S slices: (unique, loaded)"""
    Sc = -(-S // s)
    outs = B * (cin * Sc * Sc + 4 * S * S) * NZ
    copied = B * ((cin - n_filt) * Sc * Sc + 4 * S * S) * NZ
    # taps of one axis inside the slice: the union of [s i - R, s i + R] over the Sc samples, and their count
    cover = len({p for i in range(Sc) for p in range(s * i - R, s * i + R + 1) if 0 <= p < S})
    taps = sum(1 for i in range(Sc) for p in range(s * i - R, s * i + R + 1) if 0 <= p < S)
    tables = 2 * Sc * (2 * R + 1) if n_filt else 0
    unique = 4 * (outs + copied + B * n_filt * cover * cover * NZ + tables + 6 * B)
    loaded = 4 * (copied + B * n_filt * taps * taps * NZ + 6 * B)
    return unique, loaded


def train_ms_per_it(run_name, its, warm, workers, repeat, extra):
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod

    cls = gmod.wind_field_GAN_3D
    orig = cls.optimize_parameters
    stamps = []

    def timed(self, LR, HR, Z, it):
        stamps.append(time.perf_counter())
        return orig(self, LR, HR, Z, it)

    prepare = runmod.prepare_data

    def repeated(cfg):
        tr, te, va, x, y = prepare(cfg)
        tr.filenames = tr.filenames * repeat
        return tr, te, va, x, y

    ini = os.path.abspath(run_name + ".ini")
    write_ini(ini, run_name, warm + its, workers, "\n[DATA]\ndevice_resident = True\n" + extra)
    cls.optimize_parameters, runmod.prepare_data = timed, repeated
    try:
        runmod.main(["--train", "--cfg", ini])
        torch.cuda.synchronize()
    finally:
        cls.optimize_parameters, runmod.prepare_data = orig, prepare
    return (stamps[-1] - stamps[warm]) / (len(stamps) - 1 - warm) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=300, help="timed launches per gather variant")
    ap.add_argument("--batches", type=int, default=16, help="timed batches per CPU loader measurement")
    ap.add_argument("--its", type=int, default=50, help="timed iterations per run.py --train run")
    ap.add_argument("--warm", type=int, default=10, help="untimed iterations at the start of each run")
    ap.add_argument("--reps", type=int, default=2, help="run.py --train runs per variant (alternating)")
    ap.add_argument("--workers", type=int, default=4, help="num_workers of the store load")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_degradation needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    from gan_sr_wind_field_amd import degradation, device_data, hip_ops
    from gan_sr_wind_field_amd import run as runmod

    out = {"shape": "C1c data: batch 32, 128x128x10 -> 64x64 slices, x4, interpolate_z, z channel, rot + flip",
           "device": torch.cuda.get_device_properties(dev).gcnArchName}
    work = tempfile.mkdtemp(prefix="wsr_degradation_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        cfg = write_ini("probe.ini", "probe", 1, args.workers)
        batch = cfg.dataset_train.batch_size
        tr, _, va, _, _ = runmod.prepare_data(cfg)
        for ds in (tr, va):  # (fills the z-interpolation cache, as any earlier epoch of a real run has)
            device_data.ResidentStore(ds, "cpu", num_workers=8)
        repeat = -(-(args.warm + args.its + 1) * batch // len(tr))
        specs = {"plain": None, "box": degradation.DegradationSpec("box"),
                 "gaussian_sigma2": degradation.DegradationSpec("gaussian", 2.0)}

        # ---- the launch: the three variants on the same store and the same draws, alternating
        store = device_data.ResidentStore(tr, dev, num_workers=args.workers)
        S, s, cin, NZ = store.slice_size, store.s, store.cin, store.data.shape[-1]
        descs = []
        while len(descs) < args.launches:  # different batches of draws: the store is read from HBM, not the caches
            descs += list(device_data.DeviceLoader(store, batch_size=batch, shuffle=True, drop_last=True).descriptors)
        d_dev = torch.stack(descs[:args.launches]).to(dev)
        calls, radius = {}, {}
        for name, spec in specs.items():
            if spec is None:
                calls[name] = lambda d: hip_ops.gather_batch(store.data, d, cin, s, S)
                radius[name] = (0, 0)
                continue
            wx, wy, R = degradation.tables(spec, s, S, S)
            wx, wy = (torch.from_numpy(w.copy()).to(dev) for w in (wx, wy))
            n_filt = spec.n_filt(cin)
            outs = hip_ops.gather_batch_filtered(store.data, d_dev[0], cin, s, S, wx, wy, n_filt)
            calls[name] = lambda d, wx=wx, wy=wy, n_filt=n_filt, outs=outs: hip_ops.gather_batch_filtered(
                store.data, d, cin, s, S, wx, wy, n_filt, out=outs)
            radius[name] = (R, n_filt)
        for i in range(20):
            for call in calls.values():
                call(d_dev[i])
        torch.cuda.synchronize()
        events = {name: [] for name in calls}
        for i in range(args.launches):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(d_dev[i])
                e1.record()
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        out["gather_us"], out["gather_bytes"] = {}, {}
        for name, ev in events.items():
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
            out["gather_us"][name] = {"median": round(statistics.median(us), 2), "p10": round(us[len(us) // 10], 2),
                                      "p90": round(us[len(us) * 9 // 10], 2), "launches": len(us)}
            unique, loaded = gather_bytes(batch, cin, s, S, NZ, *radius[name])
            out["gather_bytes"][name] = {"unique": unique, "loaded": loaded, "R": radius[name][0]}
        del store, d_dev, calls, events

        # ---- the CPU loader with and without the section
        tr.filenames = tr.filenames * repeat
        out["cpu_loader_ms_per_batch"] = {}
        for name in ("plain", "gaussian_sigma2"):
            tr.degradation = specs[name]
            out["cpu_loader_ms_per_batch"][name] = {str(w): round(cpu_loader_ms(tr, w, args.batches, batch, dev), 2)
                                                    for w in (0, 4)}
        tr.degradation = None

        # ---- the training step on the device-resident path, alternating runs
        runs = {"plain": [], "gaussian_sigma2": []}
        for rep in range(args.reps):
            for name, extra in (("plain", ""), ("gaussian_sigma2", GAUSS)):
                runs[name].append(round(train_ms_per_it(f"{name}{rep}", args.its, args.warm, args.workers, repeat,
                                                        extra), 2))
        out["train_ms_per_it"] = {p: {"runs": v, "mean": round(sum(v) / len(v), 2)} for p, v in runs.items()}
        out["train_its_timed_per_run"] = args.its
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
