"""Evaluation of a trained generator (``run.py --test``): per-field PSNR / error metrics of the
super-resolved wind field against HR and against the trilinear baseline, written to the same CSV files
and pickles as the reference's ``test.py:22-374``; the generator forward is the HIP path.

Artefacts (relative to the working directory / the run folder, as in the reference):
    ./test_output/<cfg.name>____metrics.csv                       one row per field
    ./test_output/averages.csv                                     one appended row per run
    ./test_output/<cfg.name>____metrics_reverse_interpolate.csv    (+ averages_reverse_interpolate.csv)
        when ``interpolate_z`` and ``reverse_interpolate``: metrics on the raw terrain-following levels
    <run folder>/fields/test_fields_<name>.pkl                     HR / SR / TL / LR / Z every log_period-th batch

With ``[EVAL] device_metrics = True`` on a GPU the loop runs ``batch_size`` fields per generator forward and takes the
seven error sums of every field from ONE ``hip_ops.field_metrics`` launch per batch (the trilinear baseline is blended
on the fly inside it); the rows stay in a device table that is read once per ``log_period`` batches and at the end, and
``metrics_from_sums`` turns them into the nine metrics on the host, in double.  SR and the baseline leave the device only
for the pickled fields (``log_period`` counts batches: every ``log_period``-th batch pickles all of its fields, a larger
set than without the section).  With ``reverse_interpolate`` the re-levelling is ``hip_ops.column_interp``.  Same CSV files,
headers and row order; the values differ in their low digits (another summation order).  On a CPU device the section keeps the
composed torch path below.

With an ``[ENSEMBLE]`` section on a GPU both loops take SR from ``gan.G_ensemble`` (the generator averaged over
``members`` symmetries of the square, ``ensemble.py``); everything downstream is as without it.  ``write_spread`` adds
    ./test_output/<cfg.name>____ensemble_spread.csv               one row ``field,mean_spread`` per field
(the mean over voxels of ``sqrt(var_u + var_v + var_w) * UVW_MAX``, var the variance between the members) and the key
``SR_spread`` (the standard deviation per component, normalised units) in the pickled fields.

With a ``[TILE]`` section on a GPU both loops take SR from ``gan.G_tiled`` (the generator on overlapping tiles of the
size it was trained on, blended; ``tiling.py``), with ``[ENSEMBLE]`` as well every tile averaged over its ``members``;
``write_spread`` then blends the per-tile variances with the tiles' weights (a blend of per-tile variances, not the
variance of blended members).  ``write_seam`` adds
    ./test_output/<cfg.name>____tile_seam.csv                     one row ``field,mean_seam`` per field
(the mean over voxels of ``sqrt(seam_u + seam_v + seam_w) * UVW_MAX``, seam the weighted squared distance of the tiles
from their blend) and the key ``SR_seam`` (``sqrt(seam)`` per component) in the pickled fields.

With a ``[DIAGNOSTICS]`` section both loops also add the fifteen per-level sums of every batch (``diagnostics.py``) into
one (NZ, 15) table - the device loop with ONE ``hip_ops.level_diagnostics`` launch per batch on the stored baseline
(which it then builds for every batch), its table a device tensor read once after the last batch; the host loop with
``diagnostics.level_sums_reference`` on the host tensors - and write
    ./test_output/<cfg.name>____level_profile.csv                 one row ``level,`` + ``PROFILE_COLUMNS`` per z level
    ./test_output/<cfg.name>____level_profile_fields.csv          (``per_field``) one row ``field,level,...`` per field and level
    ./test_output/<cfg.name>____level_profile_reverse_interpolate.csv   (+ ``..._fields_reverse_interpolate.csv``)
        with ``reverse_interpolate``: the same on the raw truth, the re-levelled SR and baseline and the raw altitudes

With a ``[SPECTRUM]`` section both loops also add the five spectral sums per level and horizontal wavenumber bin of every
batch (``spectra.py``) into one (NZ, NK, 5) table - the device loop with ONE ``hip_ops.level_spectra`` launch per batch
on the stored baseline (which it then builds for every batch), its table a device tensor read once after the last batch;
the host loop with ``spectra.level_spectra_reference`` on the host tensors - and write
    ./test_output/<cfg.name>____energy_spectrum.csv               one row ``bin,`` + ``SPECTRUM_COLUMNS`` per bin, summed
                                                                   over fields and levels
    ./test_output/<cfg.name>____energy_spectrum_levels.csv        (``per_level``) one row ``level,bin,...`` per level and bin
    ./test_output/<cfg.name>____energy_spectrum_reverse_interpolate.csv   (+ ``..._levels_reverse_interpolate.csv``)
        with ``reverse_interpolate``: the same on the raw truth and the re-levelled SR and baseline

With an ``[SSIM]`` section both loops also take the four SSIM sums per level and wind component of every field
(``ssim.py``) - the device loop with ONE ``hip_ops.level_ssim`` launch per batch on the stored baseline (which it then
builds for every batch), the (B, NZ, 3, 4) rows kept on the device and read at the flush points of the metrics; the host
loop with ``ssim.level_ssim_reference`` on the host tensors - and write
    ./test_output/<cfg.name>____ssim.csv                          one row ``field,`` + ``SSIM_COLUMNS`` per field
    ./test_output/averages_ssim.csv                               one appended row per run: the means over the fields
                                                                   of the first four columns
    ./test_output/<cfg.name>____ssim_levels.csv                   (``per_level``) one row ``level,...`` per z level,
                                                                   summed over the fields
    ./test_output/<cfg.name>____ssim_reverse_interpolate.csv      (+ ``averages_ssim_reverse_interpolate.csv``,
        ``..._ssim_levels_reverse_interpolate.csv``) with ``reverse_interpolate``: the same on the raw truth and the
        re-levelled SR and baseline

With a ``[DISTRIBUTION]`` section both loops also add the count table speed bin x (direction sector, calm) per level and
source (HR, SR, baseline) of every batch (``distribution.py``) into one (NZ, 3, NS, ND + 1) table - the device loop with
ONE ``hip_ops.level_distribution`` launch per batch on the stored baseline (which it then builds for every batch), its
table a device tensor read once after the last batch; the host loop with ``distribution.level_distribution_reference``
on the host tensors - and write
    ./test_output/<cfg.name>____wind_distribution.csv             one row ``bin,`` + ``SPEED_COLUMNS`` per speed bin,
                                                                   summed over fields and levels
    ./test_output/<cfg.name>____wind_rose.csv                     one row ``sector,`` + ``ROSE_COLUMNS`` per sector and
                                                                   a last row ``calm``
    ./test_output/<cfg.name>____wind_distribution_levels.csv      (``per_level``) one row ``level,`` + ``SUMMARY_COLUMNS``
                                                                   per z level, summed over the fields
    ./test_output/averages_distribution.csv                       one appended row per run: ``SUMMARY_COLUMNS`` of the
                                                                   whole set
    ./test_output/<cfg.name>____wind_distribution_reverse_interpolate.csv   (+ ``..._wind_rose_reverse_interpolate.csv``,
        ``..._wind_distribution_levels_reverse_interpolate.csv``, ``averages_distribution_reverse_interpolate.csv``) with
        ``reverse_interpolate``: the same on the raw truth and the re-levelled SR and baseline

With an ``[FSS]`` section both loops also add the five window sums per level, threshold and neighbourhood of every batch
(``fss.py``) into one (NZ, NT, NN, 5) table - the device loop with ONE ``hip_ops.level_fss`` launch per batch on the stored
baseline, its table a device tensor read once after the last batch; the host loop with ``fss.level_fss_reference`` on
the host tensors - and write
    ./test_output/<cfg.name>____fss.csv                           one row ``threshold,scale,`` + ``FSS_COLUMNS`` per
                                                                   threshold and scale, pooled over fields and levels
    ./test_output/<cfg.name>____exceedance.csv                    one row ``threshold,`` + ``EXCEEDANCE_COLUMNS`` per
                                                                   threshold
    ./test_output/<cfg.name>____fss_levels.csv                    (``per_level``) one row ``level,threshold,scale,`` +
                                                                   ``FSS_COLUMNS`` per level, threshold and scale
    ./test_output/<cfg.name>____fss_reverse_interpolate.csv       (+ ``..._exceedance_reverse_interpolate.csv``,
        ``..._fss_levels_reverse_interpolate.csv``) with ``reverse_interpolate``: the same on the raw truth and the
        re-levelled SR and baseline

With a ``[HUB_HEIGHT]`` section both loops also add the 18 sums per height above ground of every batch
(``hub_height.py``) into one (NH, 18) table - the device loop with ONE ``hip_ops.hub_height`` launch per batch on the stored
baseline, the raw altitude of the batch and the ground altitude of the test domain (uploaded once), its table a device
tensor read once after the last batch; the host loop with ``hub_height.hub_height_reference`` on the host tensors - and
write
    ./test_output/<cfg.name>____hub_height.csv                    one row of ``HUB_COLUMNS`` per height
    ./test_output/<cfg.name>____hub_height_fields.csv             (``per_field``) one row ``field,`` + ``HUB_COLUMNS`` per
                                                                   field and height
    ./test_output/averages_hub_height.csv                         one appended row ``Name,`` + ``HUB_COLUMNS`` per height
    ./test_output/<cfg.name>____hub_height_maps.npz               (``write_maps``) ``heights`` (NH,), ``x``, ``y``,
        ``valid_fraction`` (NH, X, Y), ``speed`` (NH, 3, X, Y) in m/s and ``capacity_factor`` (NH, 3, X, Y) of HR, SR and
        the baseline: means over the fields in which the column was valid, nan where it never was
    ./test_output/<cfg.name>____hub_height_reverse_interpolate.csv   (+ ``..._fields_reverse_interpolate.csv``,
        ``averages_hub_height_reverse_interpolate.csv``, ``..._maps_reverse_interpolate.npz``) with
        ``reverse_interpolate``: the same on the raw truth, the re-levelled SR and baseline and the raw altitudes

With an ``[INCREMENTS]`` section both loops also add the sums of the powers of the increments per level, source,
separation, direction, kind and order of every batch (``increments.py``) into one (NZ, 3, R, 2, 3, 3) table - the device
loop with ONE ``hip_ops.level_increments`` launch per batch on the stored baseline, its table a device tensor read once
after the last batch; the host loop with ``increments.level_increments_reference`` on the host tensors - and write
    ./test_output/<cfg.name>____structure_functions.csv           one row of ``INCREMENT_COLUMNS`` per separation, pooled
                                                                   over fields and levels
    ./test_output/<cfg.name>____structure_functions_levels.csv    (``per_level``) one row ``level,`` + ``INCREMENT_COLUMNS``
                                                                   per z level and separation
    ./test_output/averages_structure_functions.csv                one appended row ``Name,`` + ``INCREMENT_COLUMNS`` per
                                                                   separation
    ./test_output/<cfg.name>____structure_functions_reverse_interpolate.csv   (+ ``..._levels_reverse_interpolate.csv``,
        ``averages_structure_functions_reverse_interpolate.csv``) with ``reverse_interpolate``: the same on the raw truth
        and the re-levelled SR and baseline
"""
from __future__ import annotations

import contextlib
import logging
import math
import os
import pickle as pkl
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .GAN_models.wind_field_GAN_3D import calculate_PSNR, wind_field_GAN_3D
from .diagnostics import PROFILE_COLUMNS, level_sums_reference, profile_from_sums
from .distribution import (ROSE_COLUMNS, SPEED_COLUMNS, SUMMARY_COLUMNS, distribution_from_counts, distribution_tables,
                           level_distribution_reference)
from .fss import EXCEEDANCE_COLUMNS, FSS_COLUMNS, fss_from_sums, fss_tables, level_fss_reference
from .hub_height import COLUMNS as HUB_COLUMNS
from .hub_height import hub_height_from_sums, hub_height_reference, hub_height_tables
from .increments import INCREMENT_COLUMNS, increments_from_sums, level_increments_reference
from .process_data import reverse_interpolate_z_axis
from .ssim import SSIM_COLUMNS, columns_from_sums, level_ssim_reference, n_positions
from .spectra import SPECTRUM_COLUMNS, grid_spacing, level_spectra_reference, mode_counts, spectrum_from_sums

METRIC_NAMES = ("PSNR", "PSNR_trilinear", "relative_error", "pix", "trilinear_pix", "relative_error_trilinear",
                "average_wind_speed", "old_pix", "old_pix_trilinear")


def field_metrics(HR: torch.Tensor, SR: torch.Tensor, trilinear: torch.Tensor, UVW_MAX: float) -> dict:
    """Metrics of one (1, 3, X, Y, Z) field in normalised units (reference ``write_metrics`` :334-374):
    PSNR, mean length of the error vector in m/s ("pix"), the same relative to the mean wind speed, and the
    component-wise L1 error ("old pix"), each for the network and for the trilinear baseline."""
    def vec_len(t):
        return torch.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2 + t[:, 2] ** 2).mean()

    err, err_tl, speed = vec_len(HR - SR), vec_len(HR - trilinear), vec_len(HR)
    l1 = nn.L1Loss()
    return {
        "PSNR": float(calculate_PSNR(HR, SR)), "PSNR_trilinear": float(calculate_PSNR(HR, trilinear)),
        "relative_error": float(err / speed), "pix": float(err * UVW_MAX), "trilinear_pix": float(err_tl * UVW_MAX),
        "relative_error_trilinear": float(err_tl / speed), "average_wind_speed": float(speed * UVW_MAX),
        "old_pix": float(l1(HR, SR) * UVW_MAX), "old_pix_trilinear": float(l1(HR, trilinear) * UVW_MAX),
    }


def metrics_from_sums(sums_row, nvox, UVW_MAX, max_diff_squared=4.0, eps=1e-8) -> dict:
    """The nine ``METRIC_NAMES`` from the seven sums of ``hip_ops.field_metrics`` over ``nvox`` voxels (X * Y * Z times
    the number of fields summed): ``sums_row`` = sum (HR-SR)^2, sum (HR-TL)^2, sum |HR-SR|, sum |HR-TL| over the three
    components, sum ||HR-SR||, sum ||HR-TL||, sum ||HR|| over voxels.  The formulas of ``field_metrics`` above and of
    ``calculate_PSNR``, defined once for the evaluation loop and the validation batches: Python floats (double) in,
    Python floats out; 0-d tensors in (a validation batch, which must not synchronise), 0-d tensors out."""
    sq, sq_tl, ab, ab_tl, ln, ln_tl, ln_hr = sums_row
    log10 = torch.log10 if torch.is_tensor(sq) else math.log10

    def psnr(s):
        return 10.0 * log10(max_diff_squared / (s / nvox + eps))

    return {
        "PSNR": psnr(sq), "PSNR_trilinear": psnr(sq_tl),
        "relative_error": ln / ln_hr, "pix": ln / nvox * UVW_MAX, "trilinear_pix": ln_tl / nvox * UVW_MAX,
        "relative_error_trilinear": ln_tl / ln_hr, "average_wind_speed": ln_hr / nvox * UVW_MAX,
        "old_pix": ab / (3 * nvox) * UVW_MAX, "old_pix_trilinear": ab_tl / (3 * nvox) * UVW_MAX,
    }


def write_metrics(HR, SR, trilinear, field_name, dest_file, UVW_MAX):
    m = field_metrics(HR, SR, trilinear, UVW_MAX)
    dest_file.write(f"{field_name}," + ",".join(str(m[k]) for k in METRIC_NAMES) + "\n")
    return tuple(m[k] for k in METRIC_NAMES)


def write_fields(LR, HR, SR, interpolated_LR, Z, folder_path, field_name, rawHR=None, Z_raw=None, SR_orig=None,
                 SR_spread=None, SR_seam=None):
    fields = {"HR": HR, "SR": SR, "TL": interpolated_LR, "LR": LR, "Z": Z}
    if SR_spread is not None:
        fields["SR_spread"] = SR_spread
    if SR_seam is not None:
        fields["SR_seam"] = SR_seam
    if rawHR is not None and torch.is_tensor(rawHR) and rawHR.numel() > 0:
        fields.update({"HR_orig": rawHR, "Z_orig": Z_raw, "SR_orig": SR_orig})
    fields = {k: (v.squeeze().cpu().numpy() if torch.is_tensor(v) else v) for k, v in fields.items() if v is not None}
    os.makedirs(os.path.join(folder_path, "fields"), exist_ok=True)
    with open(os.path.join(folder_path, "fields", f"test_fields_{field_name}.pkl"), "wb") as f:
        pkl.dump(fields, f)


def _header(path: str, line: str) -> None:
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(line + "\n")


def _generate_fields(cfg, gan, LR_d, Z_d):
    """-> (SR, var, seam) of a device batch - the single point where both loops obtain SR: the variance between the
    ensemble members (None unless ``[ENSEMBLE] write_spread``) and the seam map of the tiles (None unless ``[TILE]
    write_seam``); without either section, or on a CPU device, the plain generator forward"""
    ens, tile = cfg.ensemble, cfg.tile
    on_gpu = torch.device(cfg.device).type == "cuda"
    if tile.present and on_gpu:
        with_var = bool(ens.present and ens.write_spread)
        res = gan.G_tiled(LR_d, Z_d, members=ens.members if ens.present else 1, with_var=with_var,
                          with_seam=tile.write_seam)
        res = list(res) if isinstance(res, tuple) else [res]
        return res[0], (res[1] if with_var else None), (res[-1] if tile.write_seam else None)
    if not (ens.present and on_gpu):
        with torch.no_grad():
            return gan.G(LR_d, Z_d), None, None
    if ens.write_spread:
        return gan.G_ensemble(LR_d, Z_d, with_var=True) + (None,)
    return gan.G_ensemble(LR_d, Z_d), None, None


def _mean_spread(var: torch.Tensor, uvw: float) -> torch.Tensor:
    """per field: the mean over voxels of sqrt(var_u + var_v + var_w) in m/s -> (B,)"""
    return torch.sqrt(var.sum(dim=1)).flatten(1).mean(dim=1) * uvw


OUT_DIR = "./test_output"
RAW = "_reverse_interpolate"  # the suffix of the files about the raw levels


class _Output:
    """One family of extra CSV files about one set of levels (``suffix`` "" for the flat levels, ``RAW`` for the raw ones),
    named ``<folder>/<name>____<stem><part><suffix>.csv``.  ``add(names, b)`` takes what it needs of the batch ``b`` (HR,
    SR, TL, Z, var, seam of the fields ``names``) and queues it, ``flush`` writes the per-field rows that wait on the
    device (the loops call it at the flush points of the metrics), ``close`` writes the whole-set files.  The object owns
    its files: as a context manager it closes them, and writes the whole-set files only after a clean run."""

    stem = ""
    needs_baseline = False  # the stored baseline ``b.TL``

    def __init__(self, name, suffix="", folder=OUT_DIR):
        self.name, self.suffix, self.folder = name, suffix, folder
        self.fields, self.pending = None, []  # the open per-field file; (names, rows (B, ...)) not yet written

    def path(self, part=""):
        return os.path.join(self.folder, f"{self.name}____{self.stem}{part}{self.suffix}.csv")

    def open_fields(self, part, header):
        self.fields = open(self.path(part), "w")
        self.fields.write(header + "\n")

    def flush(self):
        if self.pending:
            rows = torch.cat([r for _, r in self.pending]).cpu().tolist()
            for name, row in zip([nm for names, _ in self.pending for nm in names], rows):
                self.write_field(name, row)
            self.pending.clear()

    def close(self):
        self.flush()
        if self.fields is not None:
            self.fields.close()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self.fields is not None:
            self.fields.close()


class _FieldMean(_Output):
    """[ENSEMBLE] write_spread (``key`` "var") and [TILE] write_seam ("seam"): one row ``field,<column>`` per field"""

    def __init__(self, stem, column, key, uvw, *where):
        super().__init__(*where)
        self.stem, self.key, self.uvw = stem, key, uvw
        self.open_fields("", "field," + column)

    def add(self, names, b):
        self.pending.append((list(names), _mean_spread(getattr(b, self.key), self.uvw)))

    def write_field(self, name, v):
        self.fields.write(f"{name},{v}\n")


class _LevelSums(_Output):
    """The per-level sums ``fn(HR, SR, TL, Z)`` -> float64 (B, NZ, ...) of every batch - the host reference or the
    ``hip_ops`` launch it was built with - and their total over the test set, which stays on the device of the sums
    until ``close``"""

    needs_baseline = True

    def __init__(self, fn, *where):
        super().__init__(*where)
        self.fn, self.total, self.nfields, self.shape = fn, None, 0, None

    def add(self, names, b):
        sums = self.fn(b.HR, b.SR, b.TL, b.Z)
        t = sums.sum(dim=0)
        self.total = t if self.total is None else self.total + t
        self.nfields += len(names)
        self.shape = (b.HR.shape[2], b.HR.shape[3])  # X, Y
        if self.fields is not None:
            self.pending.append((list(names), sums))


class _LevelProfile(_LevelSums):
    """[DIAGNOSTICS]: sums (B, NZ, 15); the profile of the test set and, with ``per_field``, of every field"""

    stem = "level_profile"

    def __init__(self, fn, uvw, per_field, *where):
        super().__init__(fn, *where)
        self.uvw = uvw
        if per_field:
            self.open_fields("_fields", "field,level," + ",".join(PROFILE_COLUMNS))

    def write_field(self, name, table):
        _write_rows(self.fields, profile_from_sums(table, self.shape[0] * self.shape[1], self.uvw), PROFILE_COLUMNS,
                    name + ",")

    def close(self):
        super().close()
        with open(self.path(), "w") as f:
            f.write("level," + ",".join(PROFILE_COLUMNS) + "\n")
            if self.total is not None:
                ncols = self.shape[0] * self.shape[1] * self.nfields
                _write_rows(f, profile_from_sums(self.total.cpu(), ncols, self.uvw), PROFILE_COLUMNS, "")  # the ONE read


def _write_rows(f, table, columns, prefix):
    """``table``: a list per column; one line ``<prefix><row>,<values>`` per row"""
    for row in range(len(table[columns[0]])):
        f.write(f"{prefix}{row}," + ",".join(str(table[c][row]) for c in columns) + "\n")


class _Spectrum(_LevelSums):
    """[SPECTRUM]: sums (B, NZ, NK, 5); the spectrum summed over the levels and, with ``per_level``, of every level.
    ``d``: the mean grid spacing in metres."""

    stem = "energy_spectrum"

    def __init__(self, fn, uvw, d, per_level, *where):
        super().__init__(fn, *where)
        self.uvw, self.d, self.per_level = uvw, d, per_level

    def close(self):
        super().close()
        table = None if self.total is None else self.total.cpu()  # the ONE read
        if table is not None:
            N, counts = max(self.shape), mode_counts(*self.shape)
        with open(self.path(), "w") as f:
            f.write("bin," + ",".join(SPECTRUM_COLUMNS) + "\n")
            if table is not None:
                spec = spectrum_from_sums(table.sum(dim=0), self.nfields * table.shape[0], self.uvw, N, self.d, counts)
                _write_rows(f, spec, SPECTRUM_COLUMNS, "")
        if self.per_level:
            with open(self.path("_levels"), "w") as f:
                f.write("level,bin," + ",".join(SPECTRUM_COLUMNS) + "\n")
                for lvl in range(0 if table is None else table.shape[0]):
                    _write_rows(f, spectrum_from_sums(table[lvl], self.nfields, self.uvw, N, self.d, counts),
                                SPECTRUM_COLUMNS, f"{lvl},")


class _Ssim(_LevelSums):
    """[SSIM]: sums (B, NZ, 3, 4); one row per field, the row of ``averages_ssim<suffix>.csv`` and, with ``per_level``,
    the rows per level summed over the fields.  ``win``: the window size."""

    stem = "ssim"

    def __init__(self, fn, win, per_level, *where):
        super().__init__(fn, *where)
        self.win, self.per_level, self.col_sums = win, per_level, [0.0] * 4
        self.averages_path = os.path.join(self.folder, f"averages_ssim{self.suffix}.csv")
        self.open_fields("", "field," + ",".join(SSIM_COLUMNS))
        _header(self.averages_path, "Name," + ",".join("Average " + k for k in SSIM_COLUMNS[:4]))

    def write_field(self, name, table):
        row = columns_from_sums(table, n_positions(*self.shape, self.win))
        self.fields.write(f"{name}," + ",".join(str(v) for v in row) + "\n")
        self.col_sums = [a + v for a, v in zip(self.col_sums, row)]

    def close(self):
        super().close()
        if self.nfields:
            with open(self.averages_path, "a") as f:
                f.write(self.name + "," + ",".join(str(v / self.nfields) for v in self.col_sums) + "\n")
        if self.per_level:
            with open(self.path("_levels"), "w") as f:
                f.write("level," + ",".join(SSIM_COLUMNS) + "\n")
                table = [] if self.total is None else self.total.cpu().tolist()  # the ONE read
                for lvl, t in enumerate(table):
                    row = columns_from_sums([t], n_positions(*self.shape, self.win) * self.nfields)
                    f.write(f"{lvl}," + ",".join(str(v) for v in row) + "\n")


class _Distribution(_LevelSums):
    """[DISTRIBUTION]: counts (B, NZ, 3, NS, ND + 1); the speed distribution and the wind rose of the test set, the row
    of ``averages_distribution<suffix>.csv`` and, with ``per_level``, the summary scalars of every level.  No per-field
    file.  ``bin_width``: in m/s."""

    stem = "wind_"

    def __init__(self, fn, bin_width, per_level, *where):
        super().__init__(fn, *where)
        self.bin_width, self.per_level = bin_width, per_level
        self.averages_path = os.path.join(self.folder, f"averages_distribution{self.suffix}.csv")
        _header(self.averages_path, "Name," + ",".join(SUMMARY_COLUMNS))

    def close(self):
        super().close()
        table = None if self.total is None else self.total.cpu()  # the ONE read
        dist = None if table is None else distribution_from_counts(table.sum(dim=0), self.bin_width)
        for part, first, key, columns in (("distribution", "bin", "speed", SPEED_COLUMNS),
                                          ("rose", "sector", "rose", ROSE_COLUMNS)):
            with open(self.path(part), "w") as f:
                f.write(first + "," + ",".join(columns) + "\n")
                if dist is not None:
                    n = len(dist[key][columns[0]])
                    for row in range(n):
                        label = "calm" if key == "rose" and row == n - 1 else str(row)
                        f.write(label + "," + ",".join(str(dist[key][c][row]) for c in columns) + "\n")
        if dist is not None:
            with open(self.averages_path, "a") as f:
                f.write(self.name + "," + ",".join(str(dist["summary"][k]) for k in SUMMARY_COLUMNS) + "\n")
        if self.per_level:
            with open(self.path("distribution_levels"), "w") as f:
                f.write("level," + ",".join(SUMMARY_COLUMNS) + "\n")
                for lvl in range(0 if table is None else table.shape[0]):
                    summary = distribution_from_counts(table[lvl], self.bin_width)["summary"]
                    f.write(f"{lvl}," + ",".join(str(summary[k]) for k in SUMMARY_COLUMNS) + "\n")


class _Fss(_LevelSums):
    """[FSS]: sums (B, NZ, NT, NN, 5); the scores per threshold and scale and the contingency scores per threshold of
    the test set, pooled over fields and levels, and, with ``per_level``, the scores of every level.  No per-field file.
    ``d``: the mean grid spacing in metres."""

    stem = ""

    def __init__(self, fn, thresholds, scales, d, per_level, *where):
        super().__init__(fn, *where)
        self.thresholds, self.scales, self.d, self.per_level = thresholds, scales, d, per_level

    def columns(self, table, levels):
        return fss_from_sums(table, self.scales, self.thresholds, self.d,
                             self.shape[0] * self.shape[1] * levels * self.nfields)

    def close(self):
        super().close()
        table = None if self.total is None else self.total.cpu()  # the ONE read
        col = None if table is None else self.columns(table.sum(dim=0), table.shape[0])
        for part, key, first, columns in (("fss", "fss", ("threshold", "scale"), FSS_COLUMNS),
                                          ("exceedance", "exceedance", ("threshold",), EXCEEDANCE_COLUMNS)):
            with open(self.path(part), "w") as f:
                f.write(",".join(first + columns) + "\n")
                for row in range(0 if col is None else len(col[key]["threshold"])):
                    f.write(",".join(str(col[key][c][row]) for c in first + columns) + "\n")
        if self.per_level:
            with open(self.path("fss_levels"), "w") as f:
                first = ("threshold", "scale")
                f.write("level," + ",".join(first + FSS_COLUMNS) + "\n")
                for lvl in range(0 if table is None else table.shape[0]):
                    rows = self.columns(table[lvl], 1)["fss"]
                    for row in range(len(rows["threshold"])):
                        f.write(f"{lvl}," + ",".join(str(rows[c][row]) for c in first + FSS_COLUMNS) + "\n")


class _HubHeight(_LevelSums):
    """[HUB_HEIGHT]: sums (B, NH, 18), with ``write_maps`` also the planes (B, NH, 7, X, Y); one row per height for the
    test set, the rows of ``averages_hub_height<suffix>.csv``, with ``per_field`` the rows of every field and with
    ``write_maps`` the per-column means.  ``xy``: the coordinates of the domain."""

    stem = "hub_height"

    def __init__(self, fn, tables, air_density, per_field, write_maps, xy, *where):
        def sums(*batch):
            if not write_maps:
                return fn(*batch)
            table, cols = fn(*batch)
            m = cols.double().sum(dim=0)  # (NH, 7, X, Y), on the device of the sums
            self.maps = m if self.maps is None else self.maps + m
            return table

        super().__init__(sums, *where)
        self.tables, self.air_density, self.write_maps, self.xy, self.maps = tables, air_density, write_maps, xy, None
        self.averages_path = os.path.join(self.folder, f"averages_hub_height{self.suffix}.csv")
        _header(self.averages_path, "Name," + ",".join(HUB_COLUMNS))
        if per_field:
            self.open_fields("_fields", "field," + ",".join(HUB_COLUMNS))

    def rows(self, table, nfields):
        col = hub_height_from_sums(table, self.tables, self.air_density, self.shape[0] * self.shape[1] * nfields)
        return [",".join(str(col[c][k]) for c in HUB_COLUMNS) for k in range(len(col["height_m"]))]

    def write_field(self, name, table):
        for row in self.rows(table, 1):
            self.fields.write(f"{name},{row}\n")

    def close(self):
        super().close()
        rows = [] if self.total is None else self.rows(self.total.cpu(), self.nfields)  # the ONE read
        with open(self.path(), "w") as f:
            f.write(",".join(HUB_COLUMNS) + "\n")
            f.writelines(row + "\n" for row in rows)
        with open(self.averages_path, "a") as f:
            f.writelines(f"{self.name},{row}\n" for row in rows)
        if self.write_maps and self.maps is not None:
            m = self.maps.cpu()
            n = m[:, 6]  # (NH, X, Y): the fields in which the column was valid
            mean = torch.where(n[:, None] > 0, m[:, :6] / n[:, None].clamp(min=1), torch.full_like(m[:, :6], math.nan))
            np.savez(os.path.join(self.folder, f"{self.name}____{self.stem}_maps{self.suffix}.npz"),
                     heights=np.asarray(self.tables.heights_m), x=np.asarray(self.xy[0]), y=np.asarray(self.xy[1]),
                     valid_fraction=(n / max(self.nfields, 1)).numpy(), speed=(mean[:, :3] * self.tables.UVW_MAX).numpy(),
                     capacity_factor=mean[:, 3:6].numpy())


class _Increments(_LevelSums):
    """[INCREMENTS]: sums (B, NZ, 3, R, 2, 3, 3); one row per separation for the test set, pooled over fields and levels,
    the rows of ``averages_structure_functions<suffix>.csv`` and, with ``per_level``, the rows of every level.  No
    per-field file.  ``d``: the mean grid spacing in metres."""

    stem = "structure_functions"

    def __init__(self, fn, separations, uvw, d, per_level, *where):
        super().__init__(fn, *where)
        self.separations, self.uvw, self.d, self.per_level = separations, uvw, d, per_level
        self.averages_path = os.path.join(self.folder, f"averages_structure_functions{self.suffix}.csv")
        _header(self.averages_path, "Name," + ",".join(INCREMENT_COLUMNS))

    def rows(self, table, levels):
        col = increments_from_sums(table, self.separations, self.nfields * levels, *self.shape, self.uvw, self.d)
        return [",".join(str(col[c][k]) for c in INCREMENT_COLUMNS) for k in range(len(self.separations))]

    def close(self):
        super().close()
        table = None if self.total is None else self.total.cpu()  # the ONE read
        rows = [] if table is None else self.rows(table.sum(dim=0), table.shape[0])
        with open(self.path(), "w") as f:
            f.write(",".join(INCREMENT_COLUMNS) + "\n")
            f.writelines(row + "\n" for row in rows)
        with open(self.averages_path, "a") as f:
            f.writelines(f"{self.name},{row}\n" for row in rows)
        if self.per_level:
            with open(self.path("_levels"), "w") as f:
                f.write("level," + ",".join(INCREMENT_COLUMNS) + "\n")
                for lvl in range(0 if table is None else table.shape[0]):
                    f.writelines(f"{lvl},{row}\n" for row in self.rows(table[lvl], 1))


def _outputs(cfg, gan, uvw, d, suffix, on_device, folder=OUT_DIR):
    """The extra outputs of one set of levels that ``cfg`` asks for, each yielded as soon as its files are open; the
    sums come from ``hip_ops`` with ``on_device`` (the device loop), else from the host references.  ``d``: the mean grid
    spacing in metres ([SPECTRUM]); [DIAGNOSTICS] reads the coordinates ``gan.x``, ``gan.y``."""
    where = (cfg.name, suffix, folder)
    if on_device:
        from . import hip_ops
    if suffix == "" and torch.device(cfg.device).type == "cuda":  # (what only the GPU paths of _generate_fields return)
        if cfg.ensemble.present and cfg.ensemble.write_spread:
            yield _FieldMean("ensemble_spread", "mean_spread", "var", uvw, *where)
        if cfg.tile.present and cfg.tile.write_seam:
            yield _FieldMean("tile_seam", "mean_seam", "seam", uvw, *where)
    if cfg.diagnostics.on:
        fn, x, y = (hip_ops.level_diagnostics, gan.x, gan.y) if on_device else (level_sums_reference, gan.x.cpu(), gan.y.cpu())
        yield _LevelProfile(lambda HR, SR, TL, Z: fn(HR, SR, TL, x, y, Z), uvw, cfg.diagnostics.per_field, *where)
    if cfg.spectrum.on:
        spectra = hip_ops.level_spectra if on_device else level_spectra_reference
        yield _Spectrum(lambda HR, SR, TL, Z: spectra(HR, SR, TL, cfg.spectrum.window), uvw, d, cfg.spectrum.per_level,
                        *where)
    if cfg.ssim.on:
        ssim, par = hip_ops.level_ssim if on_device else level_ssim_reference, (cfg.ssim.window_size, cfg.ssim.sigma,
                                                                                 cfg.ssim.data_range)
        yield _Ssim(lambda HR, SR, TL, Z: ssim(HR, SR, TL, *par), par[0], cfg.ssim.per_level, *where)
    if cfg.distribution.on:
        dc = cfg.distribution
        dist, tables = (hip_ops.level_distribution if on_device else level_distribution_reference,
                        distribution_tables(uvw, dc.bin_width, dc.speed_bins, dc.sectors, dc.calm))
        yield _Distribution(lambda HR, SR, TL, Z: dist(HR, SR, TL, tables), dc.bin_width, dc.per_level, *where)
    if cfg.fss.on:
        fc = cfg.fss
        score, thr = hip_ops.level_fss if on_device else level_fss_reference, fss_tables(uvw, fc.thresholds)
        yield _Fss(lambda HR, SR, TL, Z: score(HR, SR, TL, thr, fc.scales), fc.thresholds, fc.scales, d, fc.per_level,
                   *where)
    if cfg.hub_height.on:
        hc = cfg.hub_height
        hub, terrain = (hip_ops.hub_height, gan.terrain) if on_device else (hub_height_reference, gan.terrain.cpu())
        tab = hub_height_tables(uvw, hc.heights, hc.curve_speeds, hc.curve_power)
        yield _HubHeight(lambda HR, SR, TL, Z: hub(HR, SR, TL, Z, terrain, tab, hc.interp, hc.write_maps), tab,
                         hc.air_density, hc.per_field, hc.write_maps, gan.xy, *where)
    if cfg.increments.on:
        inc, sp = hip_ops.level_increments if on_device else level_increments_reference, tuple(cfg.increments.separations)
        yield _Increments(lambda HR, SR, TL, Z: inc(HR, SR, TL, sp), sp, uvw, d, cfg.increments.per_level, *where)


class _LevelSet:
    """What is written about one set of levels: the open metrics file ``out``, the running averages ``avg`` of its
    nine columns and the extra ``outputs``"""

    def __init__(self, out, outputs=()):
        self.out, self.outputs, self.avg = out, list(outputs), {k: 0.0 for k in METRIC_NAMES}


def _host_loop(cfg, gan, loader, uvw, n, flat, raw=None):
    """one field at a time; baseline, re-levelling and metrics on the host (the reference's loop).  ``flat``, ``raw``: the
    ``_LevelSet`` of the flat levels and, with ``reverse_interpolate``, of the raw ones."""
    dev = cfg.device
    for j, (LR, HR, Z, names, HR_raw, Z_raw) in enumerate(loader):
        TL = nn.functional.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear",
                                       align_corners=True)
        for i in range(LR.shape[0]):
            SR_i, var_i, seam_i = _generate_fields(cfg, gan, LR[i:i + 1].to(dev, non_blocking=True),
                                                   Z[i:i + 1].to(dev, non_blocking=True))
            SR_i = SR_i.cpu()
            sets = [(flat, SimpleNamespace(HR=HR[i:i + 1, :3], SR=SR_i, TL=TL[i:i + 1], Z=Z[i:i + 1], var=var_i,
                                           seam=seam_i))]
            if raw is not None:  # back onto the raw terrain-following levels of every column
                SR_r, TL_r = (reverse_interpolate_z_axis(t.numpy(), Z_raw[i:i + 1].numpy(), Z[i:i + 1].numpy())
                              for t in (SR_i, TL[i:i + 1]))
                sets.insert(0, (raw, SimpleNamespace(HR=HR_raw[i:i + 1], SR=SR_r, TL=TL_r, Z=Z_raw[i:i + 1])))
            for ls, b in sets:
                vals = write_metrics(b.HR[:, :3], b.SR, b.TL, names[i], ls.out, uvw)
                for k, v in zip(METRIC_NAMES, vals):
                    ls.avg[k] += v / n
                for o in ls.outputs:
                    o.add(names[i:i + 1], b)
                    o.flush()
            if j % cfg.training.log_period == 0:
                write_fields(LR[i], HR[i], SR_i[0], TL[i], Z[i], cfg.env.this_runs_folder, names[i],
                             None if raw is None else HR_raw[i], None if raw is None else Z_raw[i], None,
                             None if var_i is None else torch.sqrt(var_i[0]),
                             None if seam_i is None else torch.sqrt(seam_i[0]))


def _device_loop(cfg, gan, loader, uvw, n, flat, raw=None):
    """[EVAL] device_metrics: one generator forward and one metrics launch per batch; the (B, 7) rows wait in a device
    table and are read once per ``log_period`` batches and at the end.  ``flat``, ``raw``: as in ``_host_loop``; every
    output makes one launch per batch."""
    from . import hip_ops

    dev, s, rev = cfg.device, cfg.scale, raw is not None
    sets = (flat, raw) if rev else (flat,)
    store_baseline = rev or any(o.needs_baseline for o in flat.outputs)
    pending = []  # (names, nvox, sums (B, 7), sums on the raw levels (B, 7) or None) of the batches not yet written

    def flush():
        if pending:
            table = torch.cat([t for p in pending for t in p[2:] if t is not None]).cpu().tolist()  # the ONE read
            at = 0
            for names, nvox, *_ in pending:  # (per batch: all rows of the flat levels, then all of the raw ones)
                for ls in sets:
                    for name in names:
                        m = metrics_from_sums(table[at], nvox, uvw)
                        at += 1
                        ls.out.write(f"{name}," + ",".join(str(m[k]) for k in METRIC_NAMES) + "\n")
                        for k in METRIC_NAMES:
                            ls.avg[k] += m[k] / n
            pending.clear()
        for ls in sets:
            for o in ls.outputs:
                o.flush()

    for j, (LR, HR, Z, names, HR_raw, Z_raw) in enumerate(loader):
        LR_d, HR_d, Z_d = (t.to(dev, non_blocking=True).contiguous() for t in (LR, HR, Z))
        SR_d, var_d, seam_d = _generate_fields(cfg, gan, LR_d, Z_d)
        SR_d = SR_d.float().contiguous()
        nvox = HR.shape[2] * HR.shape[3] * HR.shape[4]
        sums = hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=s)  # (the baseline is blended inside, never stored)
        keep = j % cfg.training.log_period == 0
        # (the stored baseline: the outputs' kernels read it, the divergence needs the neighbouring columns)
        TL_d = hip_ops.trilinear_xy(LR_d, s) if store_baseline or keep else None
        b = SimpleNamespace(HR=HR_d, SR=SR_d, TL=TL_d, Z=Z_d, var=var_d, seam=seam_d)
        for o in flat.outputs:
            o.add(names, b)
        sums_raw = None
        if rev:  # back onto the raw terrain-following levels of every column, metrics against the raw truth
            raw_d, zraw_d = (t.to(dev, non_blocking=True).contiguous() for t in (HR_raw, Z_raw))
            SR_r, TL_r = hip_ops.column_interp(SR_d, Z_d, zraw_d), hip_ops.column_interp(TL_d, Z_d, zraw_d)
            sums_raw = hip_ops.field_metrics(raw_d, SR_r, TL=TL_r)
            for o in raw.outputs:
                o.add(names, SimpleNamespace(HR=raw_d, SR=SR_r, TL=TL_r, Z=zraw_d))
        pending.append((list(names), nvox, sums, sums_raw))
        if keep:
            SR_h, TL_h = SR_d.cpu(), TL_d.cpu()
            sd_h = None if var_d is None else torch.sqrt(var_d).cpu()
            seam_h = None if seam_d is None else torch.sqrt(seam_d).cpu()
            for i in range(LR.shape[0]):
                write_fields(LR[i], HR[i], SR_h[i], TL_h[i], Z[i], cfg.env.this_runs_folder, names[i],
                             HR_raw[i] if rev else None, Z_raw[i] if rev else None, None,
                             None if sd_h is None else sd_h[i], None if seam_h is None else seam_h[i])
            flush()
    flush()


def test(cfg, dataset_test, reverse_interpolate: bool = False):
    log = logging.getLogger("status")
    if cfg.dataset_test is None:
        raise ValueError("Test dataset not supplied")
    loader = torch.utils.data.DataLoader(dataset_test, batch_size=cfg.eval.batch_size if cfg.eval.present else 1,
                                         shuffle=False,
                                         num_workers=min(8, os.cpu_count() or 1), pin_memory=True)
    if cfg.model.lower() != "wind_field_gan_3d":
        raise NotImplementedError(f"only wind_field_GAN_3D is supported - not {cfg.model}")
    gan = wind_field_GAN_3D(cfg)
    log.info(f"loading model from from saves. G: {cfg.env.generator_load_path}")
    gan.load_model(generator_load_path=cfg.env.generator_load_path, discriminator_load_path=None, state_load_path=None)
    gan.G.eval()
    if not reverse_interpolate:
        cfg.gan_config.interpolate_z = False
    rev = bool(cfg.gan_config.interpolate_z)
    uvw = float(dataset_test.UVW_MAX)
    os.makedirs(OUT_DIR, exist_ok=True)
    os.makedirs(os.path.join(cfg.env.this_runs_folder, "fields"), exist_ok=True)
    n = max(len(dataset_test), 1)
    dev = cfg.device
    log.info("beginning test")
    if cfg.diagnostics.on:  # (the coordinates of the whole test domain)
        gan.x, gan.y = (torch.from_numpy(np.asarray(v)).float().contiguous().to(dev) for v in (dataset_test.x, dataset_test.y))
    if cfg.hub_height.on:  # (the ground altitude and the coordinates of the whole test domain; one upload)
        gan.terrain = torch.from_numpy(np.asarray(dataset_test.terrain)).float().contiguous().to(dev)
        gan.xy = (np.asarray(dataset_test.x), np.asarray(dataset_test.y))
    d = grid_spacing(np.asarray(dataset_test.x), np.asarray(dataset_test.y)) if cfg.spectrum.on or cfg.fss.on or cfg.increments.on else None
    on_device = cfg.eval.on and torch.device(dev).type == "cuda"
    with contextlib.ExitStack() as stack:  # (an exception in any batch closes every file)
        sets = []
        for suffix in ("", RAW) if rev else ("",):
            _header(f"{OUT_DIR}/averages{suffix}.csv", "Name," + ",".join("Average " + k for k in METRIC_NAMES))
            out = stack.enter_context(open(os.path.join(OUT_DIR, f"{cfg.name}____metrics{suffix}.csv"), "w"))
            out.write("field," + ",".join(METRIC_NAMES) + "\n")
            sets.append(_LevelSet(out, (stack.enter_context(o) for o in _outputs(cfg, gan, uvw, d, suffix, on_device))))
        (_device_loop if on_device else _host_loop)(cfg, gan, loader, uvw, n, *sets)
    for ls, suffix in zip(sets, ("", RAW)):
        with open(f"{OUT_DIR}/averages{suffix}.csv", "a") as f:
            f.write(cfg.name + "," + ",".join(str(ls.avg[k]) for k in METRIC_NAMES) + "\n")
    for k in METRIC_NAMES:
        log.info(f"Average {k}: {sets[0].avg[k]}")
    return sets[0].avg
