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
"""
from __future__ import annotations

import contextlib
import logging
import math
import os
import pickle as pkl

import numpy as np
import torch
import torch.nn as nn

from .GAN_models.wind_field_GAN_3D import calculate_PSNR, wind_field_GAN_3D
from .diagnostics import PROFILE_COLUMNS, level_sums_reference, profile_from_sums
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
    ens, tile = cfg.ensemble, getattr(cfg, "tile", None)
    on_gpu = torch.device(cfg.device).type == "cuda"
    if tile is not None and tile.present and on_gpu:
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


def _generate(cfg, gan, LR_d, Z_d):
    """SR and the variance between the ensemble members of ``_generate_fields``"""
    return _generate_fields(cfg, gan, LR_d, Z_d)[:2]


def _mean_spread(var: torch.Tensor, uvw: float) -> torch.Tensor:
    """per field: the mean over voxels of sqrt(var_u + var_v + var_w) in m/s -> (B,)"""
    return torch.sqrt(var.sum(dim=1)).flatten(1).mean(dim=1) * uvw


class _LevelProfile:
    """[DIAGNOSTICS]: the per-level sums of the whole test set, (NZ, 15) float64 on the device of the sums it is given,
    and the two files made of them.  ``fields``: the open per-field file or None; its rows wait in ``pending`` until
    ``flush`` (the flush points of the metrics)."""

    def __init__(self, path, uvw, fields=None):
        self.path, self.uvw, self.fields = path, uvw, fields
        self.total, self.ncols, self.pending = None, 0, []
        if fields is not None:
            fields.write("field,level," + ",".join(PROFILE_COLUMNS) + "\n")

    def add(self, names, sums, ncols_per_field):
        """``sums`` (B, NZ, 15) of the fields ``names`` with ``ncols_per_field`` = X * Y columns each"""
        t = sums.sum(dim=0)
        self.total = t if self.total is None else self.total + t
        self.ncols += ncols_per_field * len(names)
        if self.fields is not None:
            self.pending.append((list(names), sums, ncols_per_field))

    def flush(self):
        for names, sums, ncols in self.pending:
            for name, table in zip(names, sums.cpu().tolist()):
                _write_profile_rows(self.fields, profile_from_sums(table, ncols, self.uvw), name + ",")
        self.pending.clear()

    def close(self):
        self.flush()
        with open(self.path, "w") as f:
            f.write("level," + ",".join(PROFILE_COLUMNS) + "\n")
            if self.total is not None:
                _write_profile_rows(f, profile_from_sums(self.total.cpu(), self.ncols, self.uvw), "")  # the ONE read


def _write_profile_rows(f, prof, prefix):
    for lvl in range(len(prof[PROFILE_COLUMNS[0]])):
        f.write(f"{prefix}{lvl}," + ",".join(str(prof[k][lvl]) for k in PROFILE_COLUMNS) + "\n")


class _Spectrum:
    """[SPECTRUM]: the spectral sums of the whole test set, (NZ, NK, 5) float64 on the device of the sums it is given,
    and the files made of them: ``path`` (summed over the levels) and, unless None, ``levels_path`` (per level).
    ``d``: the mean grid spacing in metres."""

    def __init__(self, path, levels_path, uvw, d):
        self.path, self.levels_path, self.uvw, self.d = path, levels_path, uvw, d
        self.total, self.nfields, self.shape = None, 0, None

    def add(self, sums, X, Y):
        """``sums`` (B, NZ, NK, 5) of B fields of X x Y columns"""
        t = sums.sum(dim=0)
        self.total = t if self.total is None else self.total + t
        self.nfields += sums.shape[0]
        self.shape = (X, Y)

    def close(self):
        table = None if self.total is None else self.total.cpu()  # the ONE read
        if table is not None:
            N, counts = max(self.shape), mode_counts(*self.shape)
        with open(self.path, "w") as f:
            f.write("bin," + ",".join(SPECTRUM_COLUMNS) + "\n")
            if table is not None:
                spec = spectrum_from_sums(table.sum(dim=0), self.nfields * table.shape[0], self.uvw, N, self.d, counts)
                _write_spectrum_rows(f, spec, "")
        if self.levels_path is not None:
            with open(self.levels_path, "w") as f:
                f.write("level,bin," + ",".join(SPECTRUM_COLUMNS) + "\n")
                for lvl in range(0 if table is None else table.shape[0]):
                    _write_spectrum_rows(f, spectrum_from_sums(table[lvl], self.nfields, self.uvw, N, self.d, counts),
                                         f"{lvl},")


def _write_spectrum_rows(f, spec, prefix):
    for k in range(len(spec[SPECTRUM_COLUMNS[0]])):
        f.write(f"{prefix}{k}," + ",".join(str(spec[c][k]) for c in SPECTRUM_COLUMNS) + "\n")


class _Ssim:
    """[SSIM]: the per-field file (rows wait in ``pending`` until ``flush``, the flush points of the metrics), the sums
    of the whole test set, (NZ, 3, 4) float64 on the device of the sums it is given, for the per-level file
    (``levels_path``, unless None), and the row of ``averages_path``."""

    def __init__(self, path, levels_path, averages_path, name, win):
        self.levels_path, self.averages_path, self.name, self.win = levels_path, averages_path, name, win
        self.total, self.nfields, self.npos, self.pending = None, 0, 0, []
        self.col_sums = [0.0] * 4
        self.fields = open(path, "w")
        self.fields.write("field," + ",".join(SSIM_COLUMNS) + "\n")
        _header(averages_path, "Name," + ",".join("Average " + k for k in SSIM_COLUMNS[:4]))

    def add(self, names, sums, X, Y):
        """``sums`` (B, NZ, 3, 4) of the fields ``names`` of X x Y columns each"""
        t = sums.sum(dim=0)
        self.total = t if self.total is None else self.total + t
        self.npos = n_positions(X, Y, self.win)
        self.pending.append((list(names), sums))

    def flush(self):
        for names, sums in self.pending:
            for name, table in zip(names, sums.cpu().tolist()):
                row = columns_from_sums(table, self.npos)
                self.fields.write(f"{name}," + ",".join(str(v) for v in row) + "\n")
                self.col_sums = [a + v for a, v in zip(self.col_sums, row)]
                self.nfields += 1
        self.pending.clear()

    def close(self):
        self.flush()
        self.fields.close()
        if self.nfields:
            with open(self.averages_path, "a") as f:
                f.write(self.name + "," + ",".join(str(v / self.nfields) for v in self.col_sums) + "\n")
        if self.levels_path is not None:
            with open(self.levels_path, "w") as f:
                f.write("level," + ",".join(SSIM_COLUMNS) + "\n")
                table = [] if self.total is None else self.total.cpu().tolist()  # the ONE read
                for lvl, t in enumerate(table):
                    f.write(f"{lvl}," + ",".join(str(v) for v in columns_from_sums([t], self.npos * self.nfields)) + "\n")


def _host_loop(cfg, gan, loader, rev, uvw, n, out, out_rev, avg, avg_rev, spread=None, seam=None, diag=None,
               diag_rev=None, spec=None, spec_rev=None, ssim=None, ssim_rev=None):
    """one field at a time; baseline, re-levelling and metrics on the host (the reference's loop)"""
    dev = cfg.device
    ssim_par = _ssim_par(cfg) if ssim is not None else None
    for j, (LR, HR, Z, names, HR_raw, Z_raw) in enumerate(loader):
        TL = nn.functional.interpolate(LR[:, :3], scale_factor=(cfg.scale, cfg.scale, 1), mode="trilinear",
                                       align_corners=True)
        for i in range(LR.shape[0]):
            SR_i, var_i, seam_i = _generate_fields(cfg, gan, LR[i:i + 1].to(dev, non_blocking=True),
                                                   Z[i:i + 1].to(dev, non_blocking=True))
            SR_i = SR_i.cpu()
            if var_i is not None:
                spread.write(f"{names[i]},{float(_mean_spread(var_i, uvw)[0])}\n")
            if seam_i is not None:  # (the same reduction: sqrt of the sum over components, mean over voxels)
                seam.write(f"{names[i]},{float(_mean_spread(seam_i, uvw)[0])}\n")
            HR_i, TL_i = HR[i:i + 1, :3], TL[i:i + 1]
            if rev:  # back onto the raw terrain-following levels of every column
                SR_r = reverse_interpolate_z_axis(SR_i.numpy(), Z_raw[i:i + 1].numpy(), Z[i:i + 1].numpy())
                TL_r = reverse_interpolate_z_axis(TL_i.numpy(), Z_raw[i:i + 1].numpy(), Z[i:i + 1].numpy())
                vals = write_metrics(HR_raw[i:i + 1, :3], SR_r, TL_r, names[i], out_rev, uvw)
                for k, v in zip(METRIC_NAMES, vals):
                    avg_rev[k] += v / n
                if diag_rev is not None:
                    diag_rev.add(names[i:i + 1], level_sums_reference(HR_raw[i:i + 1], SR_r, TL_r, gan.x.cpu(),
                                                                      gan.y.cpu(), Z_raw[i:i + 1]),
                                 HR.shape[2] * HR.shape[3])
                    diag_rev.flush()
                if spec_rev is not None:
                    spec_rev.add(level_spectra_reference(HR_raw[i:i + 1], torch.as_tensor(SR_r), torch.as_tensor(TL_r),
                                                         cfg.spectrum.window), HR.shape[2], HR.shape[3])
                if ssim_rev is not None:
                    ssim_rev.add(names[i:i + 1], level_ssim_reference(HR_raw[i:i + 1], torch.as_tensor(SR_r),
                                                                      torch.as_tensor(TL_r), *ssim_par),
                                 HR.shape[2], HR.shape[3])
                    ssim_rev.flush()
            vals = write_metrics(HR_i, SR_i, TL_i, names[i], out, uvw)
            for k, v in zip(METRIC_NAMES, vals):
                avg[k] += v / n
            if diag is not None:
                diag.add(names[i:i + 1], level_sums_reference(HR_i, SR_i, TL_i, gan.x.cpu(), gan.y.cpu(), Z[i:i + 1]),
                         HR.shape[2] * HR.shape[3])
                diag.flush()
            if spec is not None:
                spec.add(level_spectra_reference(HR_i, SR_i, TL_i, cfg.spectrum.window), HR.shape[2], HR.shape[3])
            if ssim is not None:
                ssim.add(names[i:i + 1], level_ssim_reference(HR_i, SR_i, TL_i, *ssim_par), HR.shape[2], HR.shape[3])
                ssim.flush()
            if j % cfg.training.log_period == 0:
                write_fields(LR[i], HR[i], SR_i[0], TL[i], Z[i], cfg.env.this_runs_folder, names[i],
                             HR_raw[i] if rev else None, Z_raw[i] if rev else None, None,
                             None if var_i is None else torch.sqrt(var_i[0]),
                             None if seam_i is None else torch.sqrt(seam_i[0]))


def _ssim_par(cfg):
    """(window size, sigma, data range) of [SSIM]"""
    return cfg.ssim.window_size, cfg.ssim.sigma, cfg.ssim.data_range


def _device_loop(cfg, gan, loader, rev, uvw, n, out, out_rev, avg, avg_rev, spread=None, seam=None, diag=None,
                 diag_rev=None, spec=None, spec_rev=None, ssim=None, ssim_rev=None):
    """[EVAL] device_metrics: one generator forward and one metrics launch per batch; the (B, 7) rows wait in a device
    table and are read once per ``log_period`` batches and at the end"""
    from . import hip_ops

    dev, s = cfg.device, cfg.scale
    ssim_par = _ssim_par(cfg) if ssim is not None else None
    pending = []  # (names, nvox, sums (B, 7), sums on the raw levels (B, 7) or None) of the batches not yet written
    spreads = []  # ([ENSEMBLE] write_spread) (names, mean spread (B,)) of the batches not yet written
    seams = []  # ([TILE] write_seam) (names, mean seam (B,)) of the batches not yet written

    def flush():
        if not pending:
            return
        table = torch.cat([t for p in pending for t in p[2:] if t is not None]).cpu().tolist()  # the ONE read
        at = 0
        for names, nvox, _, raw in pending:
            for dest, acc, present in ((out, avg, True), (out_rev, avg_rev, raw is not None)):
                if not present:
                    continue
                for name in names:
                    m = metrics_from_sums(table[at], nvox, uvw)
                    at += 1
                    dest.write(f"{name}," + ",".join(str(m[k]) for k in METRIC_NAMES) + "\n")
                    for k in METRIC_NAMES:
                        acc[k] += m[k] / n
        pending.clear()
        for rows, dest in ((spreads, spread), (seams, seam)):
            if rows:
                vals = torch.cat([t for _, t in rows]).cpu().tolist()
                for name, v in zip([nm for names, _ in rows for nm in names], vals):
                    dest.write(f"{name},{v}\n")
                rows.clear()
        for d in (diag, diag_rev, ssim, ssim_rev):
            if d is not None:
                d.flush()

    for j, (LR, HR, Z, names, HR_raw, Z_raw) in enumerate(loader):
        LR_d, HR_d, Z_d = (t.to(dev, non_blocking=True).contiguous() for t in (LR, HR, Z))
        SR_d, var_d, seam_d = _generate_fields(cfg, gan, LR_d, Z_d)
        SR_d = SR_d.float().contiguous()
        if var_d is not None:
            spreads.append((list(names), _mean_spread(var_d, uvw)))
        if seam_d is not None:
            seams.append((list(names), _mean_spread(seam_d, uvw)))
        nvox = HR.shape[2] * HR.shape[3] * HR.shape[4]
        sums = hip_ops.field_metrics(HR_d, SR_d, LR=LR_d, scale=s)  # (the baseline is blended inside, never stored)
        keep = j % cfg.training.log_period == 0
        TL_d = (hip_ops.trilinear_xy(LR_d, s) if rev or keep or diag is not None or spec is not None or ssim is not None
                else None)
        ncols = HR.shape[2] * HR.shape[3]
        if diag is not None:  # (the stored baseline: its divergence needs the neighbouring columns)
            diag.add(names, hip_ops.level_diagnostics(HR_d, SR_d, TL_d, gan.x, gan.y, Z_d), ncols)
        if spec is not None:  # (one launch per batch, on the stored baseline)
            spec.add(hip_ops.level_spectra(HR_d, SR_d, TL_d, cfg.spectrum.window), HR.shape[2], HR.shape[3])
        if ssim is not None:  # (one launch per batch, on the stored baseline; the rows wait on the device)
            ssim.add(names, hip_ops.level_ssim(HR_d, SR_d, TL_d, *ssim_par), HR.shape[2], HR.shape[3])
        sums_raw = None
        if rev:  # back onto the raw terrain-following levels of every column, metrics against the raw truth
            raw_d, zraw_d = (t.to(dev, non_blocking=True).contiguous() for t in (HR_raw, Z_raw))
            SR_r, TL_r = hip_ops.column_interp(SR_d, Z_d, zraw_d), hip_ops.column_interp(TL_d, Z_d, zraw_d)
            sums_raw = hip_ops.field_metrics(raw_d, SR_r, TL=TL_r)
            if diag_rev is not None:
                diag_rev.add(names, hip_ops.level_diagnostics(raw_d, SR_r, TL_r, gan.x, gan.y, zraw_d), ncols)
            if spec_rev is not None:
                spec_rev.add(hip_ops.level_spectra(raw_d, SR_r, TL_r, cfg.spectrum.window), HR.shape[2], HR.shape[3])
            if ssim_rev is not None:
                ssim_rev.add(names, hip_ops.level_ssim(raw_d, SR_r, TL_r, *ssim_par), HR.shape[2], HR.shape[3])
        # (per field: the sums in the order the rows are written - all of `out`, then all of `out_rev`, per batch)
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
    os.makedirs("./test_output", exist_ok=True)
    os.makedirs(os.path.join(cfg.env.this_runs_folder, "fields"), exist_ok=True)
    cols = "field," + ",".join(METRIC_NAMES)
    _header("./test_output/averages.csv", "Name," + ",".join("Average " + k for k in METRIC_NAMES))
    metrics_path = os.path.join("./test_output", cfg.name + "____metrics.csv")
    rev_path = os.path.join("./test_output", cfg.name + "____metrics_reverse_interpolate.csv")
    if rev:
        _header("./test_output/averages_reverse_interpolate.csv",
                "Name," + ",".join("Average " + k for k in METRIC_NAMES))
    n = max(len(dataset_test), 1)
    avg = {k: 0.0 for k in METRIC_NAMES}
    avg_rev = {k: 0.0 for k in METRIC_NAMES}
    dev = cfg.device
    log.info("beginning test")
    # ([ENSEMBLE] write_spread on a GPU: one more CSV, the spread between the members per field)
    with_spread = cfg.ensemble.present and cfg.ensemble.write_spread and torch.device(dev).type == "cuda"
    spread_path = os.path.join("./test_output", cfg.name + "____ensemble_spread.csv")
    # ([TILE] write_seam on a GPU: one more CSV, the disagreement of the tiles in their overlaps per field)
    with_seam = cfg.tile.present and cfg.tile.write_seam and torch.device(dev).type == "cuda"
    seam_path = os.path.join("./test_output", cfg.name + "____tile_seam.csv")
    # ([DIAGNOSTICS]: the per-level sums of every batch, one more CSV - two with per_field - per set of levels)
    dg = getattr(cfg, "diagnostics", None)
    with_diag = dg is not None and dg.on
    if with_diag:
        gan.x, gan.y = (torch.from_numpy(np.asarray(v)).float().contiguous().to(dev) for v in (dataset_test.x, dataset_test.y))

    # ([SPECTRUM]: the spectral sums of every batch, one more CSV - two with per_level - per set of levels)
    sp = getattr(cfg, "spectrum", None)
    with_spec = sp is not None and sp.on

    def spectrum_acc(suffix):
        def path(levels):
            return os.path.join("./test_output", f"{cfg.name}____energy_spectrum{'_levels' if levels else ''}{suffix}.csv")

        return _Spectrum(path(False), path(True) if sp.per_level else None, uvw,
                         grid_spacing(np.asarray(dataset_test.x), np.asarray(dataset_test.y)))

    # ([SSIM]: the SSIM sums of every field, one more CSV - two with per_level - and one averages row per set of levels)
    sm = getattr(cfg, "ssim", None)
    with_ssim = sm is not None and sm.on

    def ssim_acc(suffix):
        def path(levels):
            return os.path.join("./test_output", f"{cfg.name}____ssim{'_levels' if levels else ''}{suffix}.csv")

        return _Ssim(path(False), path(True) if sm.per_level else None, f"./test_output/averages_ssim{suffix}.csv",
                     cfg.name, sm.window_size)

    def profile_path(fields, suffix):
        return os.path.join("./test_output", f"{cfg.name}____level_profile{'_fields' if fields else ''}{suffix}.csv")

    with open(metrics_path, "w") as out, (open(rev_path, "w") if rev else open(os.devnull, "w")) as out_rev, \
            (open(spread_path, "w") if with_spread else contextlib.nullcontext()) as spread, \
            (open(seam_path, "w") if with_seam else contextlib.nullcontext()) as seam, \
            (open(profile_path(True, ""), "w") if with_diag and dg.per_field else contextlib.nullcontext()) as pf, \
            (open(profile_path(True, "_reverse_interpolate"), "w") if with_diag and dg.per_field and rev
             else contextlib.nullcontext()) as pf_rev:
        diag = _LevelProfile(profile_path(False, ""), uvw, pf) if with_diag else None
        diag_rev = _LevelProfile(profile_path(False, "_reverse_interpolate"), uvw, pf_rev) if with_diag and rev else None
        spec = spectrum_acc("") if with_spec else None
        spec_rev = spectrum_acc("_reverse_interpolate") if with_spec and rev else None
        ssim = ssim_acc("") if with_ssim else None
        ssim_rev = ssim_acc("_reverse_interpolate") if with_ssim and rev else None
        out.write(cols + "\n")
        out_rev.write(cols + "\n")
        if with_spread:
            spread.write("field,mean_spread\n")
        if with_seam:
            seam.write("field,mean_seam\n")
        if cfg.eval.on and torch.device(dev).type == "cuda":
            _device_loop(cfg, gan, loader, rev, uvw, n, out, out_rev, avg, avg_rev, spread, seam, diag, diag_rev, spec,
                         spec_rev, ssim, ssim_rev)
        else:
            _host_loop(cfg, gan, loader, rev, uvw, n, out, out_rev, avg, avg_rev, spread, seam, diag, diag_rev, spec,
                       spec_rev, ssim, ssim_rev)
        for d in (diag, diag_rev, spec, spec_rev, ssim, ssim_rev):
            if d is not None:
                d.close()
    with open("./test_output/averages.csv", "a") as f:
        f.write(cfg.name + "," + ",".join(str(avg[k]) for k in METRIC_NAMES) + "\n")
    for k in METRIC_NAMES:
        log.info(f"Average {k}: {avg[k]}")
    if rev:
        with open("./test_output/averages_reverse_interpolate.csv", "a") as f:
            f.write(cfg.name + "," + ",".join(str(avg_rev[k]) for k in METRIC_NAMES) + "\n")
    return avg
