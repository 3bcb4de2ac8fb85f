#!/usr/bin/env python
"""Input pipeline at the C1c data shape: the CPU ``DataLoader`` against the device-resident store (device_data.py).

Shape: the cluster ini as shipped (batch 32, 128x128x10 samples, ``interpolate_z``, z channel, ``enable_slicing`` with
64x64 slices, x4, rotation and mirrors on), on five days of synthetic HARMONIE-SIMRA-format data written from a seed
into a scratch directory (96 training files).  The training split lists its files repeatedly, so that one epoch holds
every timed iteration: a real split (22 617 files at the cluster ini's dates) restarts its loader workers once per ~700
iterations, a 96-file one would restart them every third.  One JSON line:

* ``cpu_loader_ms_per_batch``: ``DataLoader(pin_memory=True)`` at 0 / 2 / 4 workers, ``--batches`` batches after the
  loader's prefetch has drained (2 x workers + 1 batches untimed), each copied to the device as train.py does;
* ``residency_s`` / ``residency_gb``: loading the (repeated) training split into device memory (4 workers);
* ``gather_us``: one ``wsr_gather_batch`` launch from device events (mean over 200), its algorithmic bytes (every output
  float read once and written once, plus the descriptors) and their share of 8 TB/s; ``gather_host_us``: a whole
  ``ResidentStore.gather`` call (descriptor check, pinned upload, launch) by the host clock;
* ``train_ms_per_it``: ``run.py --train`` wall time per iteration (between successive ``optimize_parameters`` calls,
  after ``--warm`` iterations), ``--reps`` runs of each path alternating cpu, device, cpu, device; bf16 compute as in
  bench.py's C1c preset, ``d_g_train_period`` 1 (G- and D-iterations alternate), no validation or checkpoints.

    python tools/bench_input_pipeline.py --out profiles/input_pipeline.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CLUSTER_INI = os.path.join(ROOT, "gan_sr_wind_field_amd", "config", "wind_field_GAN_3D_config_cluster.ini")
START, END = [2018, 4, 1], [2018, 4, 5]


def write_ini(path, name, niter, device_resident, workers):
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
        f.write(cfg.asINI() + ("\n[DATA]\ndevice_resident = True\n" if device_resident else ""))
    return cfg


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


def train_ms_per_it(run_name, its, warm, device_resident, workers, repeat):
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
    write_ini(ini, run_name, warm + its, device_resident, workers)
    cls.optimize_parameters, runmod.prepare_data = timed, repeated
    try:
        runmod.main(["--train", "--cfg", ini])
        torch.cuda.synchronize()
    finally:
        cls.optimize_parameters, runmod.prepare_data = orig, prepare
    return (stamps[-1] - stamps[warm]) / (len(stamps) - 1 - warm) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, default=24, help="timed batches per CPU loader measurement")
    ap.add_argument("--its", type=int, default=50, help="timed iterations per run.py --train run")
    ap.add_argument("--warm", type=int, default=10, help="untimed iterations at the start of each run")
    ap.add_argument("--reps", type=int, default=2, help="run.py --train runs per path (alternating)")
    ap.add_argument("--workers", type=int, default=4, help="num_workers of run.py's loaders and of the store load")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_input_pipeline needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    from gan_sr_wind_field_amd import device_data, hip_ops
    from gan_sr_wind_field_amd import run as runmod

    out = {"shape": "C1c data: batch 32, 128x128x10 -> 64x64 slices, x4, interpolate_z, z channel, rot + flip",
           "device": torch.cuda.get_device_properties(dev).gcnArchName}
    work = tempfile.mkdtemp(prefix="wsr_input_pipeline_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        cfg = write_ini("probe.ini", "probe", 1, False, args.workers)
        batch = cfg.dataset_train.batch_size
        t0 = time.perf_counter()
        tr, _, va, _, _ = runmod.prepare_data(cfg)
        for ds in (tr, va):  # (fills the z-interpolation cache, as any earlier epoch of a real run has)
            device_data.ResidentStore(ds, "cpu", num_workers=8)
        out["n_train_files"], out["n_val"], out["data_prep_s"] = len(tr), len(va), round(time.perf_counter() - t0, 1)
        repeat = -(-(args.warm + args.its + 1) * batch // len(tr))
        tr.filenames = tr.filenames * repeat
        out["n_train"] = len(tr)

        out["cpu_loader_ms_per_batch"] = {str(w): round(cpu_loader_ms(tr, w, args.batches, batch, dev), 2)
                                          for w in (0, 2, 4)}
        store = device_data.ResidentStore(tr, dev, num_workers=4)
        out["residency_s"], out["residency_gb"] = round(store.seconds, 2), round(store.gigabytes, 3)
        # 200 different batches of draws: the timed gathers read the store from HBM, not from the Infinity Cache
        descs = []
        while len(descs) < 200:
            descs += list(device_data.DeviceLoader(store, batch_size=batch, shuffle=True, drop_last=True).descriptors)
        descs = descs[:200]
        d_dev = torch.stack(descs).to(dev)
        for i in range(20):
            LR, HR, Z = hip_ops.gather_batch(store.data, d_dev[i], store.cin, store.s, store.slice_size)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(200):
            hip_ops.gather_batch(store.data, d_dev[i], store.cin, store.s, store.slice_size)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 200
        nbytes = 2 * 4 * (LR.numel() + HR.numel() + Z.numel()) + descs[0].numel() * 4
        t0 = time.perf_counter()
        for d in descs:
            store.gather(d)
        torch.cuda.synchronize()
        out["gather_us"], out["gather_bytes"] = round(us, 2), nbytes
        out["gather_share_of_8TBps"] = round(nbytes / (us * 1e-6) / 8e12, 3)
        out["gather_host_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 1)
        del store, LR, HR, Z, d_dev

        runs = {"cpu": [], "device": []}
        for rep in range(args.reps):
            for path in ("cpu", "device"):
                runs[path].append(round(train_ms_per_it(f"{path}{rep}", args.its, args.warm, path == "device",
                                                        args.workers, repeat), 2))
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
