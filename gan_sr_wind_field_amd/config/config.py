"""INI configuration, drop-in for the reference's ``config/config.py``.

Same public names (``Config`` and the per-section ``*Config`` attribute bags),
same attribute names and ``None``-for-bare-key semantics, same ``str(cfg)`` /
``asINI()`` text (reference config/config.py:18-396), so every shipped
``config/*.ini`` and ``pretrained_models/*/config.ini`` loads unchanged.
Implemented table-driven: each section is a list of ``(key, kind)`` pairs.

Extension (optional keys, defaults keep reference behaviour):
  [DEFAULT] compute_dtype = fp32 | bf16     arithmetic type of the HIP kernels
  [DIST]    backend / bucket_mb / sync_bn   data-parallel settings (see dist.py)
  [DATA]    device_resident = True | False  training / validation splits held in device memory (device_data.py)
  [GRAD_CLIP] clip_generator / clip_discriminator / max_norm_discriminator / log_grad_norms
            gradient-norm clipping of the optimizer steps (the generator's bound is [GENERATOR] max_norm)
  [EMA]     decay / start_iter / validate_with_ema / test_with_ema
            exponential moving average of the generator's weights, updated inside the optimizer step
            (tools/table_adam.py), saved as G_ema_{it}.pth, used for validation and --test
  [EVAL]    device_metrics / batch_size / reverse_interpolate
            validation and --test take the trilinear baseline and the error sums from the HIP kernels
            (csrc/eval_metrics.hip); --test runs batch_size fields per launch and can write the metrics on the raw
            terrain-following levels
  [ENSEMBLE] members / write_spread
            --test averages the generator over 1, 2, 4 or 8 symmetries of the square (ensemble.py,
            csrc/ensemble.hip) and can write the spread between the members
  [TILE] tile / overlap / tiles_per_forward / write_seam
            --test runs the generator on overlapping tiles of ``tile`` LR voxels in x and y and blends the outputs
            (tiling.py, csrc/tiling.hip): the whole domain at the geometry of training, memory following
            tiles_per_forward instead of the domain; can write how far the tiles disagree in their overlaps
  [DIAGNOSTICS] level_profile / per_field
            --test also writes, per z level, wind speed, error-vector length, speed bias, direction error and the rms
            divergence of truth, network and baseline (diagnostics.py, csrc/diagnostics.hip), for the whole test set
            and per field
  [SPECTRUM] energy_spectrum / per_level / window
            --test also writes the horizontal kinetic-energy spectrum of truth, network and baseline and their
            coherence with the truth per wavenumber bin (spectra.py, csrc/spectra.hip), for the whole test set and
            per z level
  [SPECTRAL_LOSS] weight / window / k_min / k_max / rel_floor
            the generator loss gains an energy-spectrum term: the mean squared log ratio of the binned horizontal
            kinetic-energy spectra of SR and HR (spectral_loss.py, csrc/spectral_loss.hip), logged as ``spectral``
  [DEGRADATION] kernel / sigma / channels
            the LR inputs of training, validation and --test are a box- or gaussian-filtered, then sampled copy of the
            full-resolution channels instead of every scale-th column (degradation.py, csrc/data_gather.hip)
  [SSIM_LOSS] weight / window_size / sigma / data_range
            absent = off; present, the generator loss carries weight * (1 - mean SSIM) of SR against HR on horizontal
            planes (ssim_loss.py, csrc/ssim_loss.hip), logged as ``ssim``
  [SSIM] window_size / sigma / data_range / per_level / validation
            --test also writes the structural similarity of network and baseline with the truth on horizontal planes,
            per field, per wind component and per z level (ssim.py, csrc/ssim.hip); validation epochs add val_SSIM and
            Trilinear_SSIM to the metrics
  [DISTRIBUTION] bin_width / speed_bins / sectors / calm / per_level
            --test also writes the frequency distribution of the horizontal wind speed and the wind rose of the truth,
            the network and the baseline, with the scores between them (distribution.py, csrc/distribution.hip)
  [FSS] thresholds / scales / per_level
            --test also writes the fractions skill score of network and baseline against the truth per wind-speed
            threshold and neighbourhood size, the useful scale and the contingency-table scores (fss.py, csrc/fss.hip)
  [HUB_HEIGHT] heights / interp / air_density / curve_speeds / curve_power / per_field / write_maps
            --test also writes the wind speed, the wind power density and a turbine's capacity factor at fixed heights
            above ground for the truth, the network and the baseline
            (hub_height.py, csrc/hub_height.hip)
  [INCREMENTS] separations / per_level
            --test also writes the structure functions of truth, network and baseline: second-order structure function
            (twice the semivariogram), skewness and flatness of the velocity increments per separation
            (increments.py, csrc/increments.hip)
  [DISTRIBUTION_LOSS] weight / bin_width / speed_bins / pool
            absent = off; present, the generator loss carries weight * the 1-D Wasserstein distance (m/s) between the
            soft horizontal-speed histograms of SR and HR (distribution_loss.py, csrc/distribution_loss.hip), logged as
            ``distribution``
  [CONSISTENCY_LOSS] weight / kernel / sigma / factor / norm
            absent = off; present, the generator loss carries weight * the mean |r| (l1) or r^2 (l2) of the
            coarse-grained difference r = D(SR - HR), D the anti-aliased coarse-graining of [DEGRADATION]
            (consistency_loss.py, csrc/consistency_loss.hip), logged as ``consistency``
"""
from __future__ import annotations

import ast
import math
from configparser import ConfigParser
from typing import Any, List, Optional, Sequence, Tuple

_B, _I, _F, _S, _W = "bool", "int", "float", "str", "word"  # (word: a lower-cased string)
_L = "list"  # (a list literal of numbers; a single number is a list of one)


def safe_list_from_string(text, target_type: type) -> list:
    """``ast.literal_eval`` a list literal; anything unparsable gives ``[]``
    (reference config/config.py:384-396)."""
    try:
        val = ast.literal_eval(text)
    except Exception:
        return []
    if val is None:
        return []
    return val if isinstance(val, list) else [val]


def _read(section, key: str, kind: str):
    if section.get(key) is None:
        # missing key or bare key.  (The reference crashes on a bare bool/int key, which
        # makes its own asINI() dump unloadable whenever a value was None; returning
        # None keeps every loadable file identical and makes the round trip total.)
        return [] if kind == "intlist" else None
    if kind == _B:
        return section.getboolean(key)
    if kind == _I:
        return section.getint(key)
    if kind == _F:
        return section.getfloat(key)
    if kind == "intlist":
        return safe_list_from_string(section.get(key), int)
    if kind == _L:
        try:
            val = ast.literal_eval(section.get(key))
        except Exception:
            raise ValueError(f"{key}: not a list literal") from None
        return list(val) if isinstance(val, (list, tuple)) else [val]
    if kind == _W:
        return section.get(key).strip().lower()
    return section.get(key)


class IniConfig:
    """Attribute bag that prints itself back as an INI section."""

    _schema: Sequence[Tuple[str, str]] = ()

    def _load(self, section) -> None:
        for key, kind in self._schema:
            setattr(self, key, _read(section, key, kind))

    def __str__(self) -> str:
        head = "[" + type(self).__name__.upper().replace("CONFIG", "") + "]\n"
        body = "".join(f"{k}\n" if v is None else f"{k} = {v}\n" for k, v in vars(self).items())
        return head + body


class GANConfig(IniConfig):
    include_pressure: bool = True
    include_z_channel: bool = True
    include_above_ground_channel: bool = False
    number_of_z_layers: int = 10
    conv_mode: str = "3D"
    start_date = [2018, 4, 1]
    end_date = [2018, 4, 4]
    interpolate_z: bool = False
    use_D_feature_extractor_cost = False
    enable_slicing = False
    slice_size = 64
    _schema = (
        ("include_pressure", _B), ("include_z_channel", _B), ("include_above_ground_channel", _B),
        ("number_of_z_layers", _I), ("conv_mode", _S), ("start_date", "intlist"), ("end_date", "intlist"),
        ("interpolate_z", _B), ("use_D_feature_extractor_cost", _B), ("enable_slicing", _B), ("slice_size", _I),
    )

    def setGANConfig(self, section):
        self._load(section)


class EnvConfig(IniConfig):
    root_path: str = "~/GAN_SR_wind_field_"
    log_subpath: str = "/log"
    tensorboard_subpath: str = "/tensorboard_log"
    runs_subpath: str = "/runs"
    generator_load_path: str = None
    discriminator_load_path: str = None
    state_load_path: str = None
    fixed_seed: int = 2001
    this_runs_folder: str = None
    this_runs_tensorboard_folder: str = None
    _schema = (
        ("root_path", _S), ("log_subpath", _S), ("tensorboard_subpath", _S), ("runs_subpath", _S),
        ("generator_load_path", _S), ("discriminator_load_path", _S), ("state_load_path", _S), ("fixed_seed", _I),
    )

    def setEnvConfig(self, section):
        self._load(section)


class GeneratorConfig(IniConfig):
    norm_type: str = "none"
    act_type: str = "leakyrelu"
    layer_mode: str = "CNA"
    num_features: int = 64
    num_RRDB: int = 23
    num_RDB_convs: int = 5
    RDB_res_scaling: float = 0.2
    RRDB_res_scaling: float = 0.2
    in_num_ch: int = 3
    out_num_ch: int = 3
    RDB_growth_chan: int = 32
    hr_kern_size: int = 3
    weight_init_scale: float = 1.0
    lff_kern_size: int = 3
    conv_mode: str = "2D"
    use_mixed_precision: bool = True
    terrain_number_of_features: int = 16
    dropout_probability: float = 0.0
    max_norm: float = 1.0
    _schema = (
        ("norm_type", _S), ("act_type", _S), ("layer_mode", _S), ("num_features", _I), ("num_RRDB", _I),
        ("num_RDB_convs", _I), ("RDB_res_scaling", _F), ("RRDB_res_scaling", _F), ("in_num_ch", _I),
        ("out_num_ch", _I), ("RDB_growth_chan", _I), ("hr_kern_size", _I), ("weight_init_scale", _F),
        ("lff_kern_size", _I), ("conv_mode", _S), ("use_mixed_precision", _B), ("terrain_number_of_features", _I),
        ("dropout_probability", _F), ("max_norm", _F),
    )

    def setGeneratorConfig(self, section):
        self._load(section)


class DiscriminatorConfig(IniConfig):
    norm_type: str = "batch"
    act_type: str = "leakyrelu"
    layer_mode: str = "CNA"
    num_features: int = 64
    in_num_ch: int = 3
    feat_kern_size: int = 3
    weight_init_scale: float = 1.0
    conv_mode: str = "3D"
    use_mixed_precision: bool = True
    dropout_probability: float = 0.2
    _schema = (
        ("norm_type", _S), ("act_type", _S), ("layer_mode", _S), ("num_features", _I), ("in_num_ch", _I),
        ("feat_kern_size", _I), ("weight_init_scale", _F), ("conv_mode", _S), ("use_mixed_precision", _B),
        ("dropout_probability", _F),
    )

    def setDiscriminatorConfig(self, section):
        self._load(section)


class FeatureExtractorConfig(IniConfig):
    low_level_feat_layer: int = 1
    high_level_feat_layer: int = 34
    _schema = (("low_level_feat_layer", _I), ("high_level_feat_layer", _I))

    def setFeatureExtractorConfig(self, section):
        self._load(section)


class DatasetConfig(IniConfig):
    name: str = "default_dataset_name"
    mode: str = "downsampler"
    dataroot_hr: str = "default_path"
    dataroot_lr: str = "default_lr_path"
    num_workers: int = 0
    batch_size: int = 16
    data_aug_flip: bool = True
    data_aug_rot: bool = True
    _schema = (
        ("name", _S), ("mode", _S), ("dataroot_hr", _S), ("dataroot_lr", _S), ("num_workers", _I),
        ("batch_size", _I), ("data_aug_flip", _B), ("data_aug_rot", _B),
    )

    def setDatasetConfig(self, section):
        self._load(section)


class DatasetTrainConfig(DatasetConfig):
    pass


class DatasetValConfig(DatasetConfig):
    pass


class DatasetTestConfig(DatasetConfig):
    pass


class TrainingConfig(IniConfig):
    resume_training_from_save: bool = False
    learning_rate_g: float = 1e-4
    learning_rate_d: float = 1e-4
    adam_weight_decay_g: float = 0
    adam_weight_decay_d: float = 0
    adam_beta1_g: float = 0.9
    adam_beta1_d: float = 0.9
    multistep_lr: bool = True
    multistep_lr_steps: list = [50000, 100000, 200000, 300000]
    lr_gamma: float = 0.5
    train_eval_test_ratio: float = 0.8
    gan_type: str = "relativistic"
    adversarial_loss_weight: float = 5e-3
    d_g_train_ratio: int = 1
    d_g_train_period: int = 50
    pixel_criterion: str = "l1"
    pixel_loss_weight: float = 1e-1
    gradient_xy_loss_weight: float = 1e-1
    gradient_z_loss_weight: float = 1e-1
    divergence_loss_weight: float = 1e-1
    xy_divergence_loss_weight: float = 1e-1
    feature_D_loss_weight: float = 0.1
    feature_D_update_period: int = 1
    use_noisy_labels: bool = False
    use_one_sided_label_smoothing: bool = False
    flip_labels: bool = False
    use_instance_noise: bool = False
    niter: int = 25
    val_period: int = 2e3
    save_model_period: int = 2e3
    log_period: int = 1e2
    # order = the order in which the reference assigns them (it decides str(cfg))
    _schema = (
        ("resume_training_from_save", _B), ("learning_rate_g", _F), ("learning_rate_d", _F),
        ("adam_weight_decay_g", _F), ("adam_weight_decay_d", _F), ("adam_beta1_g", _F), ("adam_beta1_d", _F),
        ("multistep_lr", _B), ("multistep_lr_steps", "intlist"), ("lr_gamma", _F), ("gan_type", _S),
        ("adversarial_loss_weight", _F), ("d_g_train_ratio", _I), ("d_g_train_period", _I),
        ("pixel_criterion", _S), ("pixel_loss_weight", _F), ("gradient_xy_loss_weight", _F),
        ("gradient_z_loss_weight", _F), ("divergence_loss_weight", _F), ("xy_divergence_loss_weight", _F),
        ("feature_D_loss_weight", _F), ("use_noisy_labels", _B), ("use_one_sided_label_smoothing", _B),
        ("use_instance_noise", _B), ("flip_labels", _B), ("niter", _I), ("val_period", _I),
        ("save_model_period", _I), ("log_period", _I), ("conv_mode", _S), ("train_eval_test_ratio", _F),
        ("feature_D_update_period", _I),
    )

    def setTrainingConfig(self, section):
        self._load(section)


class DistConfig(IniConfig):
    """[DIST] (extension): data-parallel settings; absent section = defaults."""

    backend: str = "nccl"
    bucket_mb: float = 32.0
    sync_bn: bool = True
    _schema = (("backend", _S), ("bucket_mb", _F), ("sync_bn", _B))

    def setDistConfig(self, section):
        for key, kind in self._schema:
            val = _read(section, key, kind)
            if val is not None:
                setattr(self, key, val)


class OptionalSection(IniConfig):
    """An extension section.  Absent from the file = the class defaults with ``present`` False, and no text in
    ``asINI``; present = printed by ``asINI`` unless ``_printed`` is False."""

    _section: str = ""
    _printed: bool = True
    present: bool = False

    def load(self, section) -> None:
        """``section`` None (not in the file) restores the defaults and switches the section off."""
        self.present = section is not None
        for key, kind in self._schema:
            try:
                val = None if section is None else _read(section, key, kind)
            except ValueError:
                what = {_B: "True or False", _I: "an integer", _F: "a number", _L: "a list of numbers"}[kind]
                raise ValueError(f"[{self._section}] {key} must be {what}, not {section.get(key)!r}") from None
            setattr(self, key, getattr(type(self), key) if val is None else val)

    def validate(self) -> None:
        pass

    def __str__(self) -> str:
        return f"[{self._section}]\n" + "".join(f"{k} = {getattr(self, k)}\n" for k, _ in self._schema)


class DataConfig(OptionalSection):
    """[DATA] (extension): input-pipeline settings; absent section = defaults (not printed by ``asINI``)."""

    device_resident: bool = False
    _section, _printed = "DATA", False
    _schema = (("device_resident", _B),)

    setDataConfig = OptionalSection.load


class GradClipConfig(OptionalSection):
    """[GRAD_CLIP] (extension): gradient-norm clipping in the optimizer steps (tools/table_adam.py); absent section =
    defaults, all off, and not printed by ``asINI``.  The generator's bound is [GENERATOR] max_norm."""

    clip_generator: bool = False
    clip_discriminator: bool = False
    max_norm_discriminator: float = 1.0
    log_grad_norms: bool = False
    _section = "GRAD_CLIP"
    _schema = (("clip_generator", _B), ("clip_discriminator", _B), ("max_norm_discriminator", _F),
               ("log_grad_norms", _B))

    setGradClipConfig = OptionalSection.load

    def validate(self, max_norm_generator) -> None:
        """every bound that clips must be > 0 and finite"""
        for on, key, bound in ((self.clip_generator, "[GENERATOR] max_norm", max_norm_generator),
                               (self.clip_discriminator, "[GRAD_CLIP] max_norm_discriminator", self.max_norm_discriminator)):
            if on and not (bound is not None and bound > 0 and math.isfinite(bound)):
                raise ValueError(f"{key} must be > 0 and finite when clipping is on, not {bound}")


class EmaConfig(OptionalSection):
    """[EMA] (extension): moving average ``e <- decay * e + (1 - decay) * w`` of the generator's weights after every
    generator step; absent section = off, and not printed by ``asINI``.  Generator steps at iterations before
    ``start_iter`` copy (``e = w``)."""

    decay: float = 0.999
    start_iter: int = 0
    validate_with_ema: bool = True
    test_with_ema: bool = True
    _section = "EMA"
    _schema = (("decay", _F), ("start_iter", _I), ("validate_with_ema", _B), ("test_with_ema", _B))

    setEmaConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if not 0.0 < self.decay < 1.0:  # (NaN fails both)
            raise ValueError(f"[EMA] decay must be > 0 and < 1, not {self.decay}")
        if self.start_iter < 0:
            raise ValueError(f"[EMA] start_iter must be >= 0, not {self.start_iter}")

    def decay_at(self, it: int) -> float:
        """the factor of the generator step of iteration ``it``"""
        return self.decay if int(it) >= self.start_iter else 0.0


class EvalConfig(OptionalSection):
    """[EVAL] (extension): device-side evaluation (csrc/eval_metrics.hip); absent section = off, and not printed by
    ``asINI``.  ``device_metrics``: the validation batches and ``run.py --test`` take the trilinear baseline and the
    error sums from the HIP kernels; ``batch_size``: fields per generator forward / metrics launch of ``--test``;
    ``reverse_interpolate``: ``--test`` also writes the ``*_reverse_interpolate.csv`` files."""

    device_metrics: bool = True
    batch_size: int = 8
    reverse_interpolate: bool = False
    _section = "EVAL"
    _schema = (("device_metrics", _B), ("batch_size", _I), ("reverse_interpolate", _B))

    setEvalConfig = OptionalSection.load

    def validate(self, interpolate_z) -> None:
        if not self.present:
            return
        if self.batch_size < 1:
            raise ValueError(f"[EVAL] batch_size must be >= 1, not {self.batch_size}")
        if self.reverse_interpolate and not interpolate_z:
            raise ValueError("[EVAL] reverse_interpolate = True needs [GAN] interpolate_z = True: the metrics on the "
                             "raw levels exist only for data that was interpolated onto flat levels")

    @property
    def on(self) -> bool:
        """the device kernels replace the host evaluation"""
        return bool(self.present and self.device_metrics)


class EnsembleConfig(OptionalSection):
    """[ENSEMBLE] (extension): geometric self-ensemble of ``run.py --test`` (ensemble.py, csrc/ensemble.hip); absent
    section = off, and not printed by ``asINI``.  ``members``: 1, 2, 4 or 8 symmetries of the square the generator is
    averaged over; ``write_spread``: ``--test`` also writes ``<name>____ensemble_spread.csv`` and pickles ``SR_spread``."""

    members: int = 8
    write_spread: bool = False
    _section = "ENSEMBLE"
    _schema = (("members", _I), ("write_spread", _B))

    setEnsembleConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if self.members not in (1, 2, 4, 8):
            raise ValueError(f"[ENSEMBLE] members must be 1, 2, 4 or 8, not {self.members}")


class TileConfig(OptionalSection):
    """[TILE] (extension): tiled whole-domain inference of ``run.py --test`` (tiling.py, csrc/tiling.hip); absent section =
    off, and not printed by ``asINI``.  ``tile`` (required): LR voxels per tile side in x and y, an axis shorter than
    this is one tile; ``overlap``: LR voxels neighbouring tiles share at least, 0 .. tile // 2; ``tiles_per_forward``:
    tiles stacked into one generator forward; ``write_seam``: ``--test`` also writes ``<name>____tile_seam.csv`` and
    pickles ``SR_seam``."""

    tile: int = None
    overlap: int = 4
    tiles_per_forward: int = 8
    write_seam: bool = False
    _section = "TILE"
    _schema = (("tile", _I), ("overlap", _I), ("tiles_per_forward", _I), ("write_seam", _B))

    setTileConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if self.tile is None:
            raise ValueError("[TILE] tile is required: LR voxels per tile side")
        if self.tile < 1:
            raise ValueError(f"[TILE] tile must be >= 1, not {self.tile}")
        if not 0 <= self.overlap <= self.tile // 2:
            raise ValueError(f"[TILE] overlap must be in 0 .. tile // 2 = {self.tile // 2}, not {self.overlap}")
        if self.tiles_per_forward < 1:
            raise ValueError(f"[TILE] tiles_per_forward must be >= 1, not {self.tiles_per_forward}")


class DiagnosticsConfig(OptionalSection):
    """[DIAGNOSTICS] (extension): per-level evaluation diagnostics of ``run.py --test`` (diagnostics.py,
    csrc/diagnostics.hip); absent section = off, and not printed by ``asINI``.  ``level_profile``: ``--test`` also writes
    ``<name>____level_profile.csv``, one row per z level; ``per_field``: ... and ``<name>____level_profile_fields.csv``,
    one row per field and level."""

    level_profile: bool = True
    per_field: bool = False
    _section = "DIAGNOSTICS"
    _schema = (("level_profile", _B), ("per_field", _B))

    setDiagnosticsConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if self.per_field and not self.level_profile:
            raise ValueError("[DIAGNOSTICS] per_field = True needs level_profile = True: the per-field rows are the "
                             "terms of the level profile")

    @property
    def on(self) -> bool:
        """``--test`` takes the per-level sums and writes the profile"""
        return bool(self.present and self.level_profile)


class SpectrumConfig(OptionalSection):
    """[SPECTRUM] (extension): horizontal energy spectra of ``run.py --test`` (spectra.py, csrc/spectra.hip); absent
    section = off, and not printed by ``asINI``.  ``energy_spectrum``: ``--test`` also writes
    ``<name>____energy_spectrum.csv``, one row per wavenumber bin; ``per_level``: ... and
    ``<name>____energy_spectrum_levels.csv``, one row per z level and bin; ``window``: ``hann`` or ``none``, the taper
    of the detrended planes."""

    energy_spectrum: bool = True
    per_level: bool = False
    window: str = "hann"
    _section = "SPECTRUM"
    _schema = (("energy_spectrum", _B), ("per_level", _B), ("window", _W))

    setSpectrumConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if self.window not in ("hann", "none"):
            raise ValueError(f"[SPECTRUM] window must be hann or none, not {self.window!r}")
        if self.per_level and not self.energy_spectrum:
            raise ValueError("[SPECTRUM] per_level = True needs energy_spectrum = True: the per-level rows are the "
                             "terms of the spectrum")

    @property
    def on(self) -> bool:
        """``--test`` takes the spectral sums and writes the spectrum"""
        return bool(self.present and self.energy_spectrum)


class SpectralLossConfig(OptionalSection):
    """[SPECTRAL_LOSS] (extension): an energy-spectrum term of the generator loss (spectral_loss.py,
    csrc/spectral_loss.hip); absent section = off, and not printed by ``asINI``.  ``weight`` (required, > 0: there is no
    reference default to inherit) multiplies ``L_spec``, the mean over samples, levels and wavenumber bins of
    log^2((e_sr + floor) / (e_hr + floor)); ``window``: ``hann`` or ``none``, the taper of the detrended planes;
    ``k_min`` >= 1 (bin 0 is empty after the detrend, bar rounding) and ``k_max`` (0: the last bin; else
    k_min <= k_max < NK of the training patch, checked at the first batch) select the bins; ``rel_floor`` >= 0: the floor
    is that fraction of the level's total e_hr."""

    weight: float = None
    window: str = "hann"
    k_min: int = 1
    k_max: int = 0
    rel_floor: float = 1e-6
    _section = "SPECTRAL_LOSS"
    _schema = (("weight", _F), ("window", _W), ("k_min", _I), ("k_max", _I), ("rel_floor", _F))

    setSpectralLossConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        if self.weight is None:
            raise ValueError("[SPECTRAL_LOSS] weight is required: the weight of the spectral term in the generator loss")
        if not (self.weight > 0 and math.isfinite(self.weight)):
            raise ValueError(f"[SPECTRAL_LOSS] weight must be a finite number > 0, not {self.weight}")
        if self.window not in ("hann", "none"):
            raise ValueError(f"[SPECTRAL_LOSS] window must be hann or none, not {self.window!r}")
        if self.k_min < 1:
            raise ValueError(f"[SPECTRAL_LOSS] k_min must be >= 1, not {self.k_min}")
        if self.k_max != 0 and self.k_max < self.k_min:
            raise ValueError(f"[SPECTRAL_LOSS] k_max must be 0 (the last bin) or >= k_min = {self.k_min}, not {self.k_max}")
        if not (self.rel_floor >= 0 and math.isfinite(self.rel_floor)):
            raise ValueError(f"[SPECTRAL_LOSS] rel_floor must be a finite number >= 0, not {self.rel_floor}")

    @property
    def on(self) -> bool:
        """the generator loss carries the spectral term"""
        return bool(self.present)


class SsimLossConfig(OptionalSection):
    """[SSIM_LOSS] (extension): a structural-similarity term of the generator loss (ssim_loss.py, csrc/ssim_loss.hip);
    absent section = off, and not printed by ``asINI``.  ``weight`` (required, > 0: there is no reference default to
    inherit) multiplies ``L_ssim`` = 1 - the mean over samples, levels, components and valid positions of l cs;
    ``window_size``: the side of the gaussian window, odd, 3 .. 15 (at most the training patch, checked at the first
    batch); ``sigma`` > 0: its standard deviation in HR grid cells; ``data_range`` > 0: the range of one normalised wind
    component, behind C1 and C2.  The keys are independent of ``[SSIM]``, whose defaults the last three share."""

    weight: float = None
    window_size: int = 11
    sigma: float = 1.5
    data_range: float = 2.0
    _section = "SSIM_LOSS"
    _schema = (("weight", _F), ("window_size", _I), ("sigma", _F), ("data_range", _F))

    setSsimLossConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..ssim import MAX_WIN
        if self.weight is None:
            raise ValueError("[SSIM_LOSS] weight is required: the weight of the SSIM term in the generator loss")
        if not (self.weight > 0 and math.isfinite(self.weight)):
            raise ValueError(f"[SSIM_LOSS] weight must be a finite number > 0, not {self.weight}")
        if self.window_size % 2 == 0 or not 3 <= self.window_size <= MAX_WIN:
            raise ValueError(f"[SSIM_LOSS] window_size must be odd and 3 .. {MAX_WIN}, not {self.window_size}")
        if not (self.sigma > 0 and math.isfinite(self.sigma)):
            raise ValueError(f"[SSIM_LOSS] sigma must be a finite number > 0, not {self.sigma}")
        if not (self.data_range > 0 and math.isfinite(self.data_range)):
            raise ValueError(f"[SSIM_LOSS] data_range must be a finite number > 0, not {self.data_range}")

    @property
    def on(self) -> bool:
        """the generator loss carries the SSIM term"""
        return bool(self.present)


class DegradationConfig(OptionalSection):
    """[DEGRADATION] (extension): anti-aliased LR inputs (degradation.py, csrc/data_gather.hip); absent section = off -
    LR is every ``scale``-th HR column, as in the reference - and never printed by ``asINI``.  ``kernel`` (required):
    ``box`` (a width-``scale`` mean centred on the sample point) or ``gaussian``; ``sigma`` (gaussian only, required
    there: no reference default to inherit): in HR grid cells, 0 < sigma <= 10; ``channels``: ``all`` LR channels, or
    ``wind`` - channels 0..2 only, the others stay point-sampled."""

    kernel: str = None
    sigma: float = None
    channels: str = "all"
    _section, _printed = "DEGRADATION", False
    _schema = (("kernel", _W), ("sigma", _F), ("channels", _W))

    setDegradationConfig = OptionalSection.load

    def validate(self, scale) -> None:
        if not self.present:
            return
        from ..degradation import CHANNELS, KERNELS, MAX_RADIUS, taps
        if self.kernel is None:
            raise ValueError("[DEGRADATION] kernel is required: box or gaussian")
        if self.kernel not in KERNELS:
            raise ValueError(f"[DEGRADATION] kernel must be box or gaussian, not {self.kernel!r}")
        if self.kernel == "gaussian":
            if self.sigma is None:
                raise ValueError("[DEGRADATION] sigma is required with kernel = gaussian: the width in HR grid cells")
            if not 0.0 < self.sigma <= 10.0:  # (NaN fails both)
                raise ValueError(f"[DEGRADATION] sigma must be > 0 and <= 10, not {self.sigma}")
        if self.channels not in CHANNELS:
            raise ValueError(f"[DEGRADATION] channels must be all or wind, not {self.channels!r}")
        if scale is None or scale < 1:
            raise ValueError(f"[DEGRADATION] needs [DEFAULT] scale >= 1, not {scale}")
        try:
            taps(self.kernel, scale, self.sigma)
        except ValueError:
            raise ValueError(f"[DEGRADATION] kernel = {self.kernel} at scale {scale} needs a tap radius above "
                             f"{MAX_RADIUS}") from None

    def spec(self):
        """what the datasets take (``preprosess(degradation=...)``): a ``degradation.DegradationSpec``, None when off"""
        if not self.present:
            return None
        from ..degradation import DegradationSpec
        return DegradationSpec(self.kernel, self.sigma if self.kernel == "gaussian" else None, self.channels)


class SsimConfig(OptionalSection):
    """[SSIM] (extension): structural similarity on horizontal planes in ``run.py --test`` and in validation epochs
    (ssim.py, csrc/ssim.hip); absent section = off, and never printed by ``asINI``.  ``window_size``: the side of the
    gaussian window, odd, 3 .. 15; ``sigma`` > 0: its standard deviation in HR grid cells; ``data_range`` > 0: the range
    of one normalised wind component, behind C1 and C2; ``per_level``: ``--test`` also writes
    ``<name>____ssim_levels.csv``; ``validation``: validation epochs add ``val_SSIM`` and ``Trilinear_SSIM`` to the
    metrics."""

    window_size: int = 11
    sigma: float = 1.5
    data_range: float = 2.0
    per_level: bool = False
    validation: bool = True
    _section, _printed = "SSIM", False
    _schema = (("window_size", _I), ("sigma", _F), ("data_range", _F), ("per_level", _B), ("validation", _B))

    setSsimConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..ssim import MAX_WIN
        if self.window_size % 2 == 0 or not 3 <= self.window_size <= MAX_WIN:
            raise ValueError(f"[SSIM] window_size must be odd and 3 .. {MAX_WIN}, not {self.window_size}")
        if not (self.sigma > 0 and math.isfinite(self.sigma)):
            raise ValueError(f"[SSIM] sigma must be a finite number > 0, not {self.sigma}")
        if not (self.data_range > 0 and math.isfinite(self.data_range)):
            raise ValueError(f"[SSIM] data_range must be a finite number > 0, not {self.data_range}")

    @property
    def on(self) -> bool:
        """``--test`` takes the SSIM sums and writes the SSIM files"""
        return bool(self.present)


class DistributionConfig(OptionalSection):
    """[DISTRIBUTION] (extension): the frequency distribution of the horizontal wind speed and the wind rose of HR, SR
    and the trilinear baseline in ``run.py --test`` (distribution.py, csrc/distribution.hip); absent section = off, and
    never printed by ``asINI``.  ``bin_width`` > 0: the width of a speed bin in m/s, required; ``speed_bins``: 2 .. 64,
    the last one open-ended; ``sectors``: even, 4 .. 36, sector 0 centred on the grid's +y, counted clockwise; ``calm``
    >= 0: horizontal speeds <= calm (m/s) have no direction and go to the calm class; ``per_level``: ``--test`` also
    writes ``<name>____wind_distribution_levels.csv``."""

    bin_width: Optional[float] = None
    speed_bins: int = 32
    sectors: int = 16
    calm: float = 0.5
    per_level: bool = False
    _section, _printed = "DISTRIBUTION", False
    _schema = (("bin_width", _F), ("speed_bins", _I), ("sectors", _I), ("calm", _F), ("per_level", _B))

    setDistributionConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..distribution import MAX_SECTORS, MAX_SPEED_BINS, MIN_SECTORS, MIN_SPEED_BINS
        if self.bin_width is None:
            raise ValueError("[DISTRIBUTION] bin_width must be given (m/s, > 0): it has no default")
        if not (self.bin_width > 0 and math.isfinite(self.bin_width)):
            raise ValueError(f"[DISTRIBUTION] bin_width must be a finite number > 0, not {self.bin_width}")
        if not MIN_SPEED_BINS <= self.speed_bins <= MAX_SPEED_BINS:
            raise ValueError(f"[DISTRIBUTION] speed_bins must be {MIN_SPEED_BINS} .. {MAX_SPEED_BINS}, not "
                             f"{self.speed_bins}")
        if self.sectors % 2 or not MIN_SECTORS <= self.sectors <= MAX_SECTORS:
            raise ValueError(f"[DISTRIBUTION] sectors must be even and {MIN_SECTORS} .. {MAX_SECTORS}, not {self.sectors}")
        if not (self.calm >= 0 and math.isfinite(self.calm)):
            raise ValueError(f"[DISTRIBUTION] calm must be a finite number >= 0, not {self.calm}")

    @property
    def on(self) -> bool:
        """``--test`` takes the count tables and writes the distribution files"""
        return bool(self.present)


class FssConfig(OptionalSection):
    """[FSS] (extension): the fractions skill score of SR and of the trilinear baseline against HR in ``run.py --test``
    (fss.py, csrc/fss.hip); absent section = off, and never printed by ``asINI``.  ``thresholds``: 1 .. 8 wind speeds in
    m/s, each > 0, strictly ascending, required; ``scales``: 1 .. 8 odd neighbourhood sizes in grid cells, strictly
    ascending, the first one 1, the last one <= 33; ``per_level``: ``--test`` also writes ``<name>____fss_levels.csv``."""

    thresholds: Optional[list] = None
    scales: tuple = (1, 3, 5, 9, 17, 33)
    per_level: bool = False
    _section, _printed = "FSS", False
    _schema = (("thresholds", _L), ("scales", _L), ("per_level", _B))

    setFssConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..fss import check_scales, check_thresholds
        if self.thresholds is None:
            raise ValueError("[FSS] thresholds must be given (a list of wind speeds in m/s): it has no default")
        self.thresholds = check_thresholds(self.thresholds, "[FSS]")
        self.scales = check_scales(self.scales, "[FSS]")

    @property
    def on(self) -> bool:
        """``--test`` takes the window sums and writes the score files"""
        return bool(self.present)


def default_power_curve():
    """The default of [HUB_HEIGHT] curve_speeds / curve_power: 0 at 3 m/s, (v^3 - 27) / (1728 - 27) at 4 .. 12 m/s, 1 at
    12 and at 25 m/s, 0 at 26 m/s -> (speeds, power)"""
    speeds = [3.0] + [float(v) for v in range(4, 13)] + [25.0, 26.0]
    power = [0.0] + [(v ** 3 - 27.0) / (1728.0 - 27.0) for v in range(4, 13)] + [1.0, 0.0]
    return speeds, power


class HubHeightConfig(OptionalSection):
    """[HUB_HEIGHT] (extension): the wind speed, the wind power density and a turbine's capacity factor at fixed heights
    above ground for HR, SR and the trilinear baseline in ``run.py --test`` (hub_height.py, csrc/hub_height.hip); absent
    section = off, and never printed by ``asINI``.  ``heights``: 1 .. 8 heights in metres above ground, each > 0,
    strictly ascending, required; ``interp``: ``linear`` (in height) or ``log`` (in ln height); ``air_density`` > 0 in
    kg/m^3; ``curve_speeds`` / ``curve_power``: the power curve, 2 .. 32 knots, speeds in m/s >= 0 and strictly
    ascending, power a fraction of rated in [0, 1], piecewise linear with the end values outside (default:
    ``default_power_curve``); ``per_field``: ``--test`` also writes ``<name>____hub_height_fields.csv``; ``write_maps``:
    ``--test`` also writes ``<name>____hub_height_maps.npz``."""

    heights: Optional[list] = None
    interp: str = "log"
    air_density: float = 1.225
    curve_speeds: Optional[list] = None
    curve_power: Optional[list] = None
    per_field: bool = False
    write_maps: bool = False
    _section, _printed = "HUB_HEIGHT", False
    _schema = (("heights", _L), ("interp", _W), ("air_density", _F), ("curve_speeds", _L), ("curve_power", _L),
               ("per_field", _B), ("write_maps", _B))

    def load(self, section) -> None:
        super().load(section)
        if self.curve_speeds is None and self.curve_power is None:
            self.curve_speeds, self.curve_power = default_power_curve()

    setHubHeightConfig = load

    def validate(self) -> None:
        if not self.present:
            return
        from ..hub_height import check_curve, check_heights, check_interp
        if self.heights is None:
            raise ValueError("[HUB_HEIGHT] heights must be given (a list of heights in metres above ground): it has no "
                             "default")
        self.heights = check_heights(self.heights, "[HUB_HEIGHT]")
        check_interp(self.interp, "[HUB_HEIGHT]")
        if not (self.air_density > 0 and math.isfinite(self.air_density)):
            raise ValueError(f"[HUB_HEIGHT] air_density must be a finite number > 0, not {self.air_density}")
        if self.curve_speeds is None or self.curve_power is None:
            raise ValueError("[HUB_HEIGHT] curve_speeds and curve_power must be given together")
        self.curve_speeds, self.curve_power = check_curve(self.curve_speeds, self.curve_power, "[HUB_HEIGHT]")

    @property
    def on(self) -> bool:
        """``--test`` takes the hub-height sums and writes the hub-height files"""
        return bool(self.present)


class IncrementsConfig(OptionalSection):
    """[INCREMENTS] (extension): the structure functions of HR, SR and the trilinear baseline in ``run.py --test``
    (increments.py, csrc/increments.hip); absent section = off, and never printed by ``asINI``.  ``separations``: 1 .. 8
    integers in HR grid cells, strictly ascending, each 1 .. 32, required; ``per_level``: ``--test`` also writes
    ``<name>____structure_functions_levels.csv``."""

    separations: Optional[list] = None
    per_level: bool = False
    _section, _printed = "INCREMENTS", False
    _schema = (("separations", _L), ("per_level", _B))

    setIncrementsConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..increments import check_separations
        if self.separations is None:
            raise ValueError("[INCREMENTS] separations must be given (a list of integers in HR grid cells): it has no "
                             "default")
        self.separations = check_separations(self.separations, "[INCREMENTS]")

    @property
    def on(self) -> bool:
        """``--test`` takes the increment sums and writes the structure-function files"""
        return bool(self.present)


class DistributionLossConfig(OptionalSection):
    """[DISTRIBUTION_LOSS] (extension): a wind-speed distribution term of the generator loss (distribution_loss.py,
    csrc/distribution_loss.hip); absent section = off, and not printed by ``asINI``.  ``weight`` (required, > 0: there is
    no reference default to inherit) multiplies ``L_dist``, the mean over the rows of the 1-D Wasserstein distance in m/s
    between the soft (linearly binned) horizontal-speed histograms of SR and HR; ``bin_width`` > 0: the distance between
    bin centres in m/s, required; ``speed_bins``: 2 .. 64, the last one open-ended; ``pool``: ``level`` (every sample and
    z level is a distribution) or ``sample`` (the levels of a sample are summed first).  The keys are independent of
    ``[DISTRIBUTION]``."""

    weight: float = None
    bin_width: float = None
    speed_bins: int = 32
    pool: str = "level"
    _section = "DISTRIBUTION_LOSS"
    _schema = (("weight", _F), ("bin_width", _F), ("speed_bins", _I), ("pool", _W))

    setDistributionLossConfig = OptionalSection.load

    def validate(self) -> None:
        if not self.present:
            return
        from ..distribution import MAX_SPEED_BINS, MIN_SPEED_BINS
        if self.weight is None:
            raise ValueError("[DISTRIBUTION_LOSS] weight is required: the weight of the distribution term in the "
                             "generator loss")
        if not (self.weight > 0 and math.isfinite(self.weight)):
            raise ValueError(f"[DISTRIBUTION_LOSS] weight must be a finite number > 0, not {self.weight}")
        if self.bin_width is None:
            raise ValueError("[DISTRIBUTION_LOSS] bin_width must be given (m/s, > 0): it has no default")
        if not (self.bin_width > 0 and math.isfinite(self.bin_width)):
            raise ValueError(f"[DISTRIBUTION_LOSS] bin_width must be a finite number > 0, not {self.bin_width}")
        if not MIN_SPEED_BINS <= self.speed_bins <= MAX_SPEED_BINS:
            raise ValueError(f"[DISTRIBUTION_LOSS] speed_bins must be {MIN_SPEED_BINS} .. {MAX_SPEED_BINS}, not "
                             f"{self.speed_bins}")
        if self.pool not in ("level", "sample"):
            raise ValueError(f"[DISTRIBUTION_LOSS] pool must be level or sample, not {self.pool!r}")

    @property
    def on(self) -> bool:
        """the generator loss carries the distribution term"""
        return bool(self.present)


class ConsistencyLossConfig(OptionalSection):
    """[CONSISTENCY_LOSS] (extension): a coarse-grained consistency term of the generator loss (consistency_loss.py,
    csrc/consistency_loss.hip); absent section = off, and not printed by ``asINI``.  ``weight`` (required, > 0: there is
    no reference default to inherit) multiplies ``L_cons``, the mean over samples, wind components, coarse cells and
    levels of ``|r|`` (``norm = l1``) or ``r^2`` (``norm = l2``) of ``r = D(SR - HR)``; ``kernel`` (required): ``box`` or
    ``gaussian``, the taps of ``degradation.taps``; ``sigma`` (gaussian only, required there): in HR grid cells,
    0 < sigma <= 10; ``factor``: the coarse-graining factor in x and y, 0 = ``[DEFAULT] scale`` (the LR grid), else
    2 .. 32.  The keys are independent of ``[DEGRADATION]``."""

    weight: float = None
    kernel: str = None
    sigma: float = None
    factor: int = 0
    norm: str = "l1"
    _section = "CONSISTENCY_LOSS"
    _schema = (("weight", _F), ("kernel", _W), ("sigma", _F), ("factor", _I), ("norm", _W))

    setConsistencyLossConfig = OptionalSection.load

    def validate(self, scale) -> None:
        if not self.present:
            return
        from ..degradation import KERNELS, MAX_RADIUS, taps
        if self.weight is None:
            raise ValueError("[CONSISTENCY_LOSS] weight is required: the weight of the consistency term in the "
                             "generator loss")
        if not (self.weight > 0 and math.isfinite(self.weight)):
            raise ValueError(f"[CONSISTENCY_LOSS] weight must be a finite number > 0, not {self.weight}")
        if self.kernel is None:
            raise ValueError("[CONSISTENCY_LOSS] kernel is required: box or gaussian")
        if self.kernel not in KERNELS:
            raise ValueError(f"[CONSISTENCY_LOSS] kernel must be box or gaussian, not {self.kernel!r}")
        if self.kernel == "gaussian":
            if self.sigma is None:
                raise ValueError("[CONSISTENCY_LOSS] sigma is required with kernel = gaussian: the width in HR grid "
                                 "cells")
            if not 0.0 < self.sigma <= 10.0:  # (NaN fails both)
                raise ValueError(f"[CONSISTENCY_LOSS] sigma must be > 0 and <= 10, not {self.sigma}")
        if self.norm not in ("l1", "l2"):
            raise ValueError(f"[CONSISTENCY_LOSS] norm must be l1 or l2, not {self.norm!r}")
        if self.factor != 0 and not 2 <= self.factor <= 32:
            raise ValueError(f"[CONSISTENCY_LOSS] factor must be 0 ([DEFAULT] scale) or 2 .. 32, not {self.factor}")
        s = self.resolved_factor(scale)
        if s is None or not 2 <= s <= 32:
            raise ValueError(f"[CONSISTENCY_LOSS] factor = 0 needs [DEFAULT] scale in 2 .. 32, not {scale}")
        try:
            taps(self.kernel, s, self.sigma)
        except ValueError:
            raise ValueError(f"[CONSISTENCY_LOSS] kernel = {self.kernel} at factor {s} needs a tap radius above "
                             f"{MAX_RADIUS}") from None

    def __str__(self) -> str:
        # (``sigma`` has no value with kernel = box: a key printed as None would not load again)
        return f"[{self._section}]\n" + "".join(f"{k} = {getattr(self, k)}\n" for k, _ in self._schema
                                                if getattr(self, k) is not None)

    def resolved_factor(self, scale):
        """the coarse-graining factor: ``factor``, or ``scale`` when it is 0"""
        return int(self.factor) if self.factor else (None if scale is None else int(scale))

    @property
    def on(self) -> bool:
        """the generator loss carries the consistency term"""
        return bool(self.present)


class Config(IniConfig):
    name: str = "default_name"
    model: str = "default_model"
    use_tensorboard_logger: bool = False
    scale: int = 4
    gpu_id: int = 0
    also_log_to_terminal: bool = True
    load_model_from_save: bool = False
    display_bar = True

    # class-level singletons, exactly like the reference (config/config.py:291-299)
    env: EnvConfig = EnvConfig()
    gan_config: GANConfig = GANConfig()
    generator: GeneratorConfig = GeneratorConfig()
    discriminator: DiscriminatorConfig = DiscriminatorConfig()
    feature_extractor: FeatureExtractorConfig = FeatureExtractorConfig()
    dataset_train: DatasetTrainConfig = DatasetTrainConfig()
    dataset_test: DatasetTestConfig = DatasetTestConfig()
    dataset_val: DatasetValConfig = DatasetValConfig()
    training: TrainingConfig = TrainingConfig()
    dist: DistConfig = DistConfig()
    data: DataConfig = DataConfig()
    grad_clip: GradClipConfig = GradClipConfig()
    ema: EmaConfig = EmaConfig()
    eval: EvalConfig = EvalConfig()
    ensemble: EnsembleConfig = EnsembleConfig()
    tile: TileConfig = TileConfig()
    diagnostics: DiagnosticsConfig = DiagnosticsConfig()
    spectrum: SpectrumConfig = SpectrumConfig()
    spectral_loss: SpectralLossConfig = SpectralLossConfig()
    degradation: DegradationConfig = DegradationConfig()
    ssim: SsimConfig = SsimConfig()
    distribution: DistributionConfig = DistributionConfig()
    fss: FssConfig = FssConfig()
    hub_height: HubHeightConfig = HubHeightConfig()
    increments: IncrementsConfig = IncrementsConfig()
    ssim_loss: SsimLossConfig = SsimLossConfig()
    distribution_loss: DistributionLossConfig = DistributionLossConfig()
    consistency_loss: ConsistencyLossConfig = ConsistencyLossConfig()
    compute_dtype: str = "fp32"
    is_train: bool
    is_use: bool
    is_test: bool
    is_param_search: bool
    is_download: bool
    slurm_array_id: int = 1

    # the optional sections in the order they load and print: (attribute, what its ``validate`` is given)
    _optional = (("data", None), ("grad_clip", lambda c: c.generator.max_norm), ("ema", None),
                 ("eval", lambda c: c.gan_config.interpolate_z), ("ensemble", None), ("tile", None),
                 ("diagnostics", None), ("spectrum", None), ("spectral_loss", None),
                 ("degradation", lambda c: c.scale), ("ssim", None))
    # (the sections above are a pinned list; later extensions load and print behind them, by the same rules)
    _optional_later = (("distribution", None), ("ssim_loss", None), ("fss", None), ("hub_height", None),
                       ("increments", None), ("distribution_loss", None))
    # ([CONSISTENCY_LOSS] loads and prints behind every other section; it needs [DEFAULT] scale, like [DEGRADATION])
    _optional_last = (("consistency_loss", lambda c: c.scale),)

    def __init__(self, ini_path):
        parser = ConfigParser(allow_no_value=True)
        parser.read(ini_path)
        self.setBaseConfig(parser["DEFAULT"])
        self.gan_config.setGANConfig(parser["GAN"])
        self.env.setEnvConfig(parser["ENV"])
        self.generator.setGeneratorConfig(parser["GENERATOR"])
        self.discriminator.setDiscriminatorConfig(parser["DISCRIMINATOR"])
        self.training.setTrainingConfig(parser["TRAINING"])
        for attr, section in (("dataset_train", "DATASETTRAIN"), ("dataset_test", "DATASETTEST"),
                              ("dataset_val", "DATASETVAL")):
            if parser.has_section(section):
                getattr(self, attr).setDatasetConfig(parser[section])
            else:
                setattr(self, attr, None)
        if parser.has_section("DIST"):
            self.dist.setDistConfig(parser["DIST"])
        for attr, given in self._optional + self._optional_later + self._optional_last:
            sec = getattr(self, attr)
            sec.load(parser[sec._section] if parser.has_section(sec._section) else None)
            sec.validate(*(() if given is None else (given(self),)))

    def setBaseConfig(self, base):
        self.name = base.get("name")
        self.model = base.get("model")
        self.use_tensorboard_logger = base.getboolean("use_tensorboard_logger")
        self.scale = base.getint("scale")
        self.also_log_to_terminal = base.getboolean("also_log_to_terminal")
        gpu = base.get("gpu_id")
        self.gpu_id = None if gpu is None or gpu.lower() == "none" else int(gpu)
        self.load_model_from_save = base.getboolean("load_model_from_save")
        self.display_bar = base.getboolean("display_bar")
        dtype = base.get("compute_dtype")
        if dtype is not None:  # optional extension key; absent -> class default, not printed
            if dtype.lower() not in ("fp32", "bf16"):
                raise ValueError(f"compute_dtype must be fp32 or bf16, not {dtype}")
            self.compute_dtype = dtype.lower()

    def asINI(self) -> str:
        return str(self)

    def __str__(self) -> str:
        out = "[DEFAULT]\n" + "".join(f"{k} = {v}\n" for k, v in vars(self).items())
        sections: List[Any] = [self.env, self.gan_config, self.generator, self.discriminator, self.training,
                               self.dataset_train, self.dataset_val, self.dataset_test]
        for sec in sections:
            if sec is not None:
                out += "\n" + str(sec)
        for attr, _ in self._optional + self._optional_later + self._optional_last:  # (absent: the text of a file without the extension, unchanged)
            sec = getattr(self, attr)
            if sec.present and sec._printed:
                out += "\n" + str(sec)
        return out
