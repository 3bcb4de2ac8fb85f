"""Device-resident training data: a split of ``CustomizedDataset`` loaded into device memory once, then every batch
out of ONE HIP launch (``wsr_gather_batch``), bit-identical to what ``DataLoader(dataset, num_workers=0)`` yields from
the same ``torch`` / ``np.random`` seeds.  Opt-in through ``[DATA] device_resident = True`` (train.py).

    store = ResidentStore(dataset_train, cfg.device, num_workers=4)
    loader = DeviceLoader(store, batch_size=32, shuffle=True)      # same arguments as the CPU DataLoader
    for LR, HR, Z in loader: ...                                    # planar fp32 device tensors

The store holds, per sample, ``reformat_to_torch`` of the FULL field at coarseness 1 - the LR channels at full
resolution (channels 0..2 are the HR wind) - and the raw altitude Z: fp32 (N, Cin + 1, X, Y, NZ).  Normalising is
elementwise, so doing it before the slice gives the slice's fp32 bits; coarsening is not done here (its phase depends
on the slice origin; with ``dataset.degradation`` set - [DEGRADATION], degradation.py - the gather also filters the LR
channels before it samples them, ``wsr_gather_batch_filtered``).  The random part of ``__getitem__`` (``CustomizedDataset.draw_augmentation``) runs on the host in
a ``DataLoader`` over descriptors ``(sample, x0, y0, k, flip_x, flip_y)``: the sampler, its torch seeds and the
``np.random`` draws happen exactly where the CPU loader makes them, so every later draw of the step sees the same
streams.
"""
from __future__ import annotations

import logging
import time
from typing import Optional, Tuple

import numpy as np
import torch

from . import hip_ops


def check_supported(dataset) -> None:
    """Refuse the datasets the device path does not batch: evaluation sets (``is_test`` / ``for_plotting`` samples
    carry ``HR_raw`` / ``Z_raw`` or pressure in HR), and rotation of a non-square domain without slicing (the CPU
    collate cannot stack those either)."""
    if dataset.is_test or dataset.for_plotting:
        raise ValueError("device-resident data serves training and validation sets only (not is_test / for_plotting)")
    if dataset.data_aug_rot and not dataset.enable_slicing and dataset.x.size != dataset.y.size:
        raise ValueError(f"data_aug_rot on a non-square {dataset.x.size} x {dataset.y.size} domain without slicing: "
                         "the rotated samples cannot be batched")


def check_fits(need: int, free: int) -> None:
    if need > free:
        raise RuntimeError(f"device-resident data needs {need} bytes of device memory, {free} bytes are free: "
                           "turn [DATA] device_resident off or shorten the date range")


def store_entry(dataset, index: int) -> torch.Tensor:
    """(Cin + 1, X, Y, NZ) fp32: ``reformat_to_torch`` of sample ``index`` at coarseness 1, LR channels then Z."""
    (z, z_above_ground, u, v, w, pressure), _, _ = dataset.load_fields(index)
    LR, _, Z = dataset._tensors(u, v, w, pressure, z, z_above_ground, coarseness_factor=1)
    return torch.cat((LR, Z))


class _Entries(torch.utils.data.Dataset):
    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self) -> int:
        return len(self.dataset)

    def __getitem__(self, index):
        return store_entry(self.dataset, index)


class ResidentStore:
    """Every sample of ``dataset`` in one fp32 (N, Cin + 1, X, Y, NZ) tensor on ``device``, loaded by ``num_workers``
    processes in chunks of ``chunk`` samples.  ``free_bytes`` overrides the ``torch.cuda.mem_get_info`` reading the
    size is checked against."""

    def __init__(self, dataset, device, num_workers: int = 0, chunk: int = 8, free_bytes: Optional[int] = None):
        check_supported(dataset)
        if len(dataset) == 0:
            raise ValueError("device-resident data: empty dataset")
        device = torch.device(device)
        self.dataset = dataset
        self.slice_size = dataset.slice_size if dataset.enable_slicing else 0
        self.s = dataset.coarseness_factor
        first = store_entry(dataset, 0)
        self.cin = first.shape[0] - 1
        shape = (len(dataset),) + tuple(first.shape)
        need = int(np.prod(shape)) * 4
        if free_bytes is None and device.type == "cuda":
            free_bytes = torch.cuda.mem_get_info(device)[0]
        if free_bytes is not None:
            check_fits(need, free_bytes)
        t0 = time.perf_counter()
        self.data = torch.empty(shape, dtype=torch.float32, device=device)
        # (an own generator: the loader's base seed must not come out of the global torch stream the run is seeded by)
        loader = torch.utils.data.DataLoader(_Entries(dataset), batch_size=chunk, num_workers=num_workers,
                                             generator=torch.Generator())
        off = 0
        for part in loader:
            self.data[off:off + part.shape[0]].copy_(part)
            off += part.shape[0]
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        self.seconds = time.perf_counter() - t0
        self.gigabytes = need / 1e9
        # [DEGRADATION]: the dataset's LR is filtered, then sampled - the gather does the same from the two weight
        # tables the CPU path reads (degradation.tables), built and uploaded once
        self.degradation = getattr(dataset, "degradation", None)
        if self.degradation is not None:
            from . import degradation
            X, Y = shape[2:4]
            W, H = (self.slice_size, self.slice_size) if self.slice_size else (X, Y)
            wx, wy, _ = degradation.tables(self.degradation, int(self.s), W, H)
            self.wx, self.wy = (torch.from_numpy(w.copy()).to(device) for w in (wx, wy))
            self.n_filt = self.degradation.n_filt(self.cin)
        logging.getLogger("status").info(f"device-resident data: {len(dataset)} samples, {self.gigabytes:.3f} GB "
                                         f"loaded in {self.seconds:.1f} s ({num_workers} workers)")

    def __len__(self) -> int:
        return self.data.shape[0]

    def gather(self, desc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(B, 6) host descriptors -> the batch ``(LR, HR, Z)`` the CPU collate would stack from the same draws."""
        d = desc.to(torch.int32).contiguous()
        _, _, X, Y, _ = self.data.shape
        W, H = (self.slice_size, self.slice_size) if self.slice_size else (X, Y)
        n, x0, y0, k = (d[:, i] for i in range(4))
        if not bool(((n >= 0) & (n < len(self)) & (x0 >= 0) & (x0 + W <= X) & (y0 >= 0) & (y0 + H <= Y) & (k >= 0)
                     & (k <= 3) & ((k % 2 == 0) | (W == H))).all()):
            raise ValueError(f"descriptor outside the store {tuple(self.data.shape)}: {d.tolist()}")
        d_dev = d.pin_memory().to(self.data.device, non_blocking=True)
        if self.degradation is not None:
            return hip_ops.gather_batch_filtered(self.data, d_dev, self.cin, self.s, self.slice_size, self.wx, self.wy,
                                                 self.n_filt)
        return hip_ops.gather_batch(self.data, d_dev, self.cin, self.s, self.slice_size)


class _Draws(torch.utils.data.Dataset):
    """Item ``i``: the descriptor ``(i, x0, y0, k, flip_x, flip_y)``, drawn as ``dataset[i]`` would draw it."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self) -> int:
        return len(self.dataset)

    def __getitem__(self, index):
        return torch.tensor((index, *self.dataset.draw_augmentation()), dtype=torch.int32)


class DeviceLoader:
    """Drop-in for ``torch.utils.data.DataLoader(store.dataset, batch_size, shuffle, sampler, drop_last,
    num_workers=0)``: the same batch order and the same random draws, batches gathered on the device."""

    def __init__(self, store: ResidentStore, batch_size: int = 1, shuffle: bool = False, sampler=None,
                 drop_last: bool = False):
        self.store = store
        self.descriptors = torch.utils.data.DataLoader(_Draws(store.dataset), batch_size=batch_size, shuffle=shuffle,
                                                       sampler=sampler, drop_last=drop_last, num_workers=0)

    def __len__(self) -> int:
        return len(self.descriptors)

    def __iter__(self):
        for desc in self.descriptors:
            yield self.store.gather(desc)
