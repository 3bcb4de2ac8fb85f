"""GPU tests of the device-resident input path: ``wsr_gather_batch`` against ``CustomizedDataset.__getitem__`` bit for
bit, the device loader's batch sequence against ``DataLoader(num_workers=0)`` from the same seeds, and ``run.py --train``
with ``[DATA] device_resident = True`` against the same run without it."""
import os

import numpy as np
import pytest
import torch

from test_device_data import all_augmentations, data_root, fixed_draws, make_datasets  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _equal_bits(a, b):
    return a.shape == b.shape and torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("geom", [
    dict(cin=3, s=4, slicing=True, slice_size=16, NZ=6),
    dict(cin=4, s=8, slicing=True, slice_size=24, NZ=5),
    dict(cin=5, s=4, slicing=False, NZ=8),
    dict(cin=6, s=8, slicing=False, NZ=6),
    dict(cin=4, s=4, slicing=False, rot=False, X=40, Y=36, NZ=6),
], ids=["c3_s4_sliced", "c4_s8_sliced_nz5", "c5_s4_full_nz8", "c6_s8_full", "c4_s4_nonsquare_flip"])
def test_gather_kernel_equals_getitem_bitwise(hip, data_root, geom):
    """one launch for all four rotations x four mirror combinations (slice origins not multiples of s) == the CPU
    sample of each, bit for bit (signed zeros included)"""
    from gan_sr_wind_field_amd import device_data

    g = dict(geom)
    S = g["slice_size"] if g["slicing"] else 0
    tr, _ = make_datasets(**g)
    store = device_data.ResidentStore(tr, DEV)
    X, Y = store.data.shape[2:4]
    x0s, y0s = ([0], [0]) if not S else ([1, X - S, 5, 0, 13], [0, 7, Y - S, 2, 9])
    augs = [a for a in all_augmentations(x0s, y0s) if g.get("rot", True) or a[2] == 0]
    desc = torch.tensor([((5 * m) % len(tr),) + a for m, a in enumerate(augs)], dtype=torch.int32)
    LR, HR, Z = (t.cpu() for t in store.gather(desc))
    for b, (n, *aug) in enumerate(desc.tolist()):
        fixed_draws(tr, tuple(aug))
        want = tr[n]
        for name, got, w in zip(("LR", "HR", "Z"), (LR[b], HR[b], Z[b]), want):
            assert _equal_bits(got, w), (aug, name)


def test_device_loader_batch_sequence_equals_cpu_loader(hip, data_root):
    """two epochs of shuffled training, the unshuffled validation set with a partial last batch and the two ranks of a
    DistributedSampler (no process group): the same batches as DataLoader(num_workers=0) from the same torch / numpy
    seeds, and the random streams end in the same state"""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    from gan_sr_wind_field_amd import device_data

    tr, va = make_datasets(slicing=True, slice_size=16, cin=4)
    stores = {id(tr): device_data.ResidentStore(tr, DEV), id(va): device_data.ResidentStore(va, DEV, num_workers=2)}

    def run(make, ds, device):
        torch.manual_seed(7)
        np.random.seed(7)
        out, sampler, kw = [], None, make()
        if isinstance(kw.get("sampler"), DistributedSampler):
            sampler = kw["sampler"]
        loader = device_data.DeviceLoader(stores[id(ds)], **kw) if device else DataLoader(ds, num_workers=0, **kw)
        for epoch in range(2):
            if sampler is not None:
                sampler.set_epoch(epoch)
            for LR, HR, Z in loader:
                out.append(tuple(t.cpu() for t in (LR, HR, Z)))
            out.append(float(torch.rand(())))  # a draw of the step between epochs sees the same stream
        return out, torch.get_rng_state(), np.random.get_state()[1].copy()

    cases = {
        "train": (tr, lambda: dict(batch_size=4, shuffle=True)),
        "val": (va, lambda: dict(batch_size=2, shuffle=False)),
        **{f"rank{r}": (tr, lambda r=r: dict(batch_size=3, drop_last=True, sampler=DistributedSampler(
            tr, num_replicas=2, rank=r, shuffle=True, drop_last=True))) for r in (0, 1)},
    }
    assert len(va) % 2 == 1  # (the validation loader ends in a partial batch)
    for name, (ds, make) in cases.items():
        want, want_t, want_n = run(make, ds, device=False)
        got, got_t, got_n = run(make, ds, device=True)
        assert len(got) == len(want), name
        for i, (a, b) in enumerate(zip(got, want)):
            if isinstance(b, float):
                assert a == b, (name, i)
            else:
                assert all(_equal_bits(x, y) for x, y in zip(a, b)), (name, i)
        assert torch.equal(got_t, want_t) and np.array_equal(got_n, want_n), name


def test_run_train_device_resident_equals_cpu_loader(hip, tmp_path, monkeypatch):
    """``run.py --train`` with ``[DATA] device_resident = True`` == the same ini without it (num_workers 0, slicing,
    rotation and mirrors on): every logged G / D loss entry, the learning rates and the saved G weights"""
    from test_hip_train_e2e import LOSS_KEYS, _write_ini

    from gan_sr_wind_field_amd import process_data as pd
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.GAN_models import wind_field_GAN_3D as gmod

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(pd, "DATA_ROOT", str(tmp_path / "data"))
    cls = gmod.wind_field_GAN_3D
    orig_opt = cls.optimize_parameters
    runs = {}
    for tag, extra in (("cpu", ""), ("dev", "\n[DATA]\ndevice_resident = True\n")):
        ini = str(tmp_path / f"{tag}.ini")
        cfg = _write_ini(ini)
        cfg.name = f"e2e_{tag}"
        cfg.dataset_train.data_aug_rot = cfg.dataset_train.data_aug_flip = True
        with open(ini, "w") as f:
            f.write(cfg.asINI() + extra)
        calls = []

        def rec_opt(self, LR, HR, Z, it, calls=calls):
            orig_opt(self, LR, HR, Z, it)
            calls.append(dict(it=int(it), batch=[t.cpu().clone() for t in (LR, HR, Z)],
                              G=[float(self.get_G_train_loss_dict_ref()[k].detach()) for k in LOSS_KEYS],
                              D=float(self.get_D_loss_dict_ref()["train_loss"].detach()),
                              lr=(self.optimizer_G.param_groups[0]["lr"], self.optimizer_D.param_groups[0]["lr"])))

        monkeypatch.setattr(cls, "optimize_parameters", rec_opt)
        runmod.main(["--train", "--cfg", ini])
        G = torch.load(os.path.join(str(tmp_path), "runs", cfg.name, "G_6.pth"), map_location="cpu")
        runs[tag] = (calls, G)
    (cpu, G_cpu), (dev, G_dev) = runs["cpu"], runs["dev"]
    assert [c["it"] for c in dev] == [c["it"] for c in cpu] == list(range(1, 8))
    for a, b in zip(dev, cpu):
        assert all(_equal_bits(x, y) for x, y in zip(a["batch"], b["batch"])), a["it"]
        assert a["G"] == b["G"] and a["D"] == b["D"] and a["lr"] == b["lr"], (a["it"], a["G"], b["G"], a["D"], b["D"])
    assert G_dev.keys() == G_cpu.keys()
    for k in G_cpu:
        assert torch.equal(G_dev[k], G_cpu[k]), k
