"""[EVAL] on the CPU: the config section, the host formulas ``metrics_from_sums``, a torch restatement of the
baseline's index and weight map against ``F.interpolate``, and the evaluation loop with the section on a CPU device
(the composed torch path) and with ``reverse_interpolate`` through ``run.py``.

Bounds (the convention of kernel_bounds.py).  A sum of K non-negative terms accumulated in fp32 is within
``LAMBDA * sqrt(K) * 2^-24`` of its float64 value, relative to the sum of the term magnitudes - for the seven sums the
terms are non-negative, so that is a RELATIVE bound ``r(K)`` on the sum itself.  Carried through the formulas of
``metrics_from_sums``: a metric that is linear in one sum moves by at most ``r``; a ratio of two sums by
``(r1 + r2) / (1 - r2)``; a PSNR ``10 log10(c / (s / n + eps))`` by at most ``10 / ln 10 * r / (1 - r)`` dB (eps only
shrinks the sensitivity).  ``metric_bounds`` returns those, and the GPU tests reuse it.
"""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO
from kernel_bounds import LAMBDA, U_FP32
from test_data_and_train import _patch_oracle_nets, _small_cfg, data_root  # noqa: F401  (data_root is a fixture)

CFG_DIR = os.path.join(REPO, "gan_sr_wind_field_amd", "config")
LOCAL_INI = os.path.join(CFG_DIR, "wind_field_GAN_3D_config_local.ini")
SUM_NAMES = ("sq", "sq_tl", "abs", "abs_tl", "len", "len_tl", "len_hr")
TL_PRODUCTS = 6  # products per baseline element: four in the two y-blends, two in the x-blend


# ------------------------------------------------------------------------------------------------- shared references
def axis_map(n_in: int, n_out: int):
    """index pair and upper weight of every output index of one axis (align_corners), in fp32 as ATen computes them:
    scale = (in - 1) / (out - 1), src = scale * o, lower = trunc(src), upper weight = src - lower"""
    o = torch.arange(n_out, dtype=torch.float32)
    if n_out <= 1:
        z = torch.zeros(n_out, dtype=torch.int64)
        return z, z, torch.zeros(n_out)
    scale = torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1))
    src = scale * o
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    return i0, i1, (src - i0.float()).clamp(0, 1)


def baseline(LR: torch.Tensor, s: int, dtype=torch.float64):
    """the 4-corner blend of channels 0..2 with the weights of ``axis_map``, evaluated in ``dtype``: (TL, A) with A
    the same blend of |corners|"""
    x = LR[:, :3].detach().cpu().to(dtype)
    _, _, Xl, Yl, _ = x.shape
    i0, i1, lx = axis_map(Xl, Xl * s)
    j0, j1, ly = axis_map(Yl, Yl * s)
    lx, ly = lx.to(dtype).view(1, 1, -1, 1, 1), ly.to(dtype).view(1, 1, 1, -1, 1)

    def blend(t):
        a = (1 - ly) * t[:, :, i0][:, :, :, j0] + ly * t[:, :, i0][:, :, :, j1]
        b = (1 - ly) * t[:, :, i1][:, :, :, j0] + ly * t[:, :, i1][:, :, :, j1]
        return (1 - lx) * a + lx * b

    return blend(x), blend(x.abs())


def baseline_bound(A: torch.Tensor) -> torch.Tensor:
    return LAMBDA * math.sqrt(TL_PRODUCTS) * U_FP32 * A + 2.0 ** -100


def sums_f64(HR, SR, TL) -> torch.Tensor:
    """the seven sums per sample in float64 from the given (fp32) values: (B, 7)"""
    h, r, t = (x[:, :3].detach().cpu().double() for x in (HR, SR, TL))
    ds, dt = h - r, h - t

    def per_sample(x):
        return x.flatten(1).sum(dim=1)

    def length(x):
        return torch.sqrt((x ** 2).sum(dim=1))

    return torch.stack([per_sample(ds ** 2), per_sample(dt ** 2), per_sample(ds.abs()), per_sample(dt.abs()),
                        per_sample(length(ds)), per_sample(length(dt)), per_sample(length(h))], dim=1)


def rel_sum_bound(nvox: int) -> dict:
    """r(K) per sum: K = 3 * nvox terms for the component sums, nvox for the vector lengths"""
    rc, rv = LAMBDA * math.sqrt(3 * nvox) * U_FP32, LAMBDA * math.sqrt(nvox) * U_FP32
    return dict(zip(SUM_NAMES, (rc, rc, rc, rc, rv, rv, rv)))


def metric_bounds(m: dict, nvox: int, extra: dict = None) -> dict:
    """allowed |difference| of each of the nine metrics ``m`` (values of one field) when every sum it is made of moved
    by at most r(K) (+ ``extra[name]``, a further relative error of that sum) - see the module docstring"""
    r = rel_sum_bound(nvox)
    if extra:
        r = {k: v + extra.get(k, 0.0) for k, v in r.items()}
    db = 10.0 / math.log(10.0)

    def ratio(a, b):
        return (r[a] + r[b]) / (1.0 - r[b])

    return {
        "PSNR": db * r["sq"] / (1 - r["sq"]), "PSNR_trilinear": db * r["sq_tl"] / (1 - r["sq_tl"]),
        "relative_error": abs(m["relative_error"]) * ratio("len", "len_hr"),
        "pix": abs(m["pix"]) * r["len"], "trilinear_pix": abs(m["trilinear_pix"]) * r["len_tl"],
        "relative_error_trilinear": abs(m["relative_error_trilinear"]) * ratio("len_tl", "len_hr"),
        "average_wind_speed": abs(m["average_wind_speed"]) * r["len_hr"],
        "old_pix": abs(m["old_pix"]) * r["abs"], "old_pix_trilinear": abs(m["old_pix_trilinear"]) * r["abs_tl"],
    }


def _ini_with(tmp_path, extra: str, name="c.ini", interpolate_z=None) -> str:
    with open(LOCAL_INI) as f:
        text = f.read()
    if interpolate_z is not None:
        text, n = re.subn(r"(?m)^interpolate_z\s*=.*$", f"interpolate_z = {interpolate_z}", text)
        assert n == 1
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text + "\n" + extra)
    return path


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    plain = Config(LOCAL_INI).asINI()
    assert Config(LOCAL_INI).eval.present is False and Config(LOCAL_INI).eval.on is False
    cfg = Config(_ini_with(tmp_path, "[EVAL]\n"))
    e = cfg.eval
    assert e.present and e.on and (e.device_metrics, e.batch_size, e.reverse_interpolate) == (True, 8, False)
    assert cfg.asINI() == plain + "\n[EVAL]\ndevice_metrics = True\nbatch_size = 8\nreverse_interpolate = False\n"
    z = Config(LOCAL_INI).gan_config.interpolate_z
    cfg = Config(_ini_with(tmp_path, "[EVAL]\ndevice_metrics = False\nbatch_size = 3\nreverse_interpolate = True\n",
                           interpolate_z=True))
    e = cfg.eval
    assert (e.device_metrics, e.batch_size, e.reverse_interpolate, e.on) == (False, 3, True, False)
    text = cfg.asINI()
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.eval) == vars(e) and again.asINI() == text
    with pytest.raises(ValueError, match=r"\[EVAL\] batch_size"):
        Config(_ini_with(tmp_path, "[EVAL]\nbatch_size = 0\n"))
    with pytest.raises(ValueError, match=r"reverse_interpolate.*interpolate_z"):
        Config(_ini_with(tmp_path, "[EVAL]\nreverse_interpolate = True\n", interpolate_z=False))
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.eval.present is False and back.asINI() == plain and back.gan_config.interpolate_z == z


def test_file_without_the_section_prints_the_pinned_text():
    """every shipped ini prints the text pinned before the extension existed (the digests of test_ema.py), and the
    sections ``config_golden.json`` pins are that text's sections (a fresh interpreter: the section objects are
    class-level singletons and keep what earlier tests hung on them)"""
    import hashlib

    from test_ema import SHIPPED

    code = ("import json, os, sys\n"
            "from gan_sr_wind_field_amd.config.config import Config\n"
            "out = {}\n"
            "for name in sys.argv[2:]:\n"
            "    cfg = Config(os.path.join(sys.argv[1], name))\n"
            "    assert cfg.eval.present is False and cfg.eval.on is False and cfg.asINI() == str(cfg)\n"
            "    out[name] = cfg.asINI()\n"
            "print(json.dumps(out))\n")
    res = subprocess.run([sys.executable, "-c", code, CFG_DIR] + sorted(SHIPPED), cwd=REPO, check=True,
                         capture_output=True, text=True)
    texts = json.loads(res.stdout.strip().splitlines()[-1])
    for name, digest in SHIPPED.items():
        assert "EVAL" not in texts[name] and "device_metrics" not in texts[name], name
        assert hashlib.sha256(texts[name].encode()).hexdigest() == digest, name
    text = texts[os.path.basename(LOCAL_INI)]
    gold = json.load(open(os.path.join(GOLDEN, "config_golden.json")))["asINI"]
    assert re.findall(r"^\[(\w+)\]$", text, re.M) == re.findall(r"^\[(\w+)\]$", gold, re.M)
    for sec in ("GAN", "GENERATOR", "DISCRIMINATOR", "TRAINING", "DATASETTRAIN", "DATASETVAL", "DATASETTEST"):
        assert text.split(f"[{sec}]\n")[1].split("\n\n")[0] == gold.split(f"[{sec}]\n")[1].split("\n\n")[0], sec


# ---------------------------------------------------------------------------------------------------- 2. host formulas
@pytest.mark.parametrize("shape", [(1, 3, 16, 12, 10), (1, 3, 8, 8, 128)])
def test_metrics_from_sums_agrees_with_field_metrics(shape):
    from gan_sr_wind_field_amd.test import METRIC_NAMES, field_metrics, metrics_from_sums

    gen = torch.Generator().manual_seed(5)
    HR = torch.rand(shape, generator=gen) * 2 - 1
    SR = HR + 0.05 * torch.randn(shape, generator=gen)
    TL = HR + 0.2 * torch.randn(shape, generator=gen)
    uvw = 37.5
    nvox = shape[2] * shape[3] * shape[4]
    want = field_metrics(HR, SR, TL, uvw)  # (fp32 torch reductions)
    got = metrics_from_sums(sums_f64(HR, SR, TL)[0].tolist(), nvox, uvw)
    assert tuple(got) == METRIC_NAMES and all(isinstance(v, float) for v in got.values())
    bnd = metric_bounds(got, nvox)
    for k in METRIC_NAMES:
        assert abs(got[k] - want[k]) <= bnd[k] + 2.0 ** -22 * abs(want[k]), (k, got[k], want[k], bnd[k])
        # (the 2^-22 |value|: field_metrics rounds its means, their ratio / product and the result to fp32)
    # tensors in, tensors out (a validation batch must not synchronise), same values
    t = metrics_from_sums(sums_f64(HR, SR, TL)[0].unbind(), nvox, uvw)
    for k in METRIC_NAMES:
        assert torch.is_tensor(t[k]) and float(t[k]) == pytest.approx(got[k], rel=1e-14)


# ---------------------------------------------------------------------------------------------------- 3. the baseline's map
@pytest.mark.parametrize("s", [4, 8, 16])
@pytest.mark.parametrize("lr_shape", [(2, 3, 8, 8, 10), (1, 5, 5, 9, 6), (1, 4, 16, 12, 5)])
def test_baseline_map_restatement_agrees_with_interpolate(s, lr_shape):
    gen = torch.Generator().manual_seed(s)
    LR = torch.randn(lr_shape, generator=gen)
    want = F.interpolate(LR[:, :3], scale_factor=(s, s, 1), mode="trilinear", align_corners=True)
    ref, A = baseline(LR, s)
    assert ref.shape == want.shape == (lr_shape[0], 3, lr_shape[2] * s, lr_shape[3] * s, lr_shape[4])
    ratio = ((want.double() - ref).abs() / baseline_bound(A)).max()
    assert float(ratio) <= 1.0, float(ratio)
    # with the same weights in double, ATen's double kernel differs only by its own (double) weight rounding
    want64 = F.interpolate(LR[:, :3].double(), scale_factor=(s, s, 1), mode="trilinear", align_corners=True)
    assert float((want64 - ref).abs().max()) < 1e-5  # (fp32 weights against double weights: |lambda| error < 2^-18)
    # end points are the corner values themselves
    assert torch.equal(ref[:, :, 0, 0].float(), LR[:, :3, 0, 0]) and torch.equal(ref[:, :, -1, -1].float(), LR[:, :3, -1, -1])


# ---------------------------------------------------------------------------------------------------- 4. the loop
def _trained(tmp_path, monkeypatch, interpolate_z=False):
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.train import train

    _patch_oracle_nets(monkeypatch)
    cfg = _small_cfg(tmp_path)
    cfg.gan_config.interpolate_z = interpolate_z
    cfg.training.niter, cfg.training.val_period, cfg.training.save_model_period = 2, 2, 2
    assert runmod.safe_setup_env_and_cfg(cfg)
    runmod.save_config(cfg, cfg.env.this_runs_folder)
    dataset_train, dataset_test, dataset_val, x, y = runmod.prepare_data(cfg)
    train(cfg, dataset_train, dataset_val, x, y)
    cfg.is_train, cfg.is_test = False, True
    cfg.env.generator_load_path = os.path.join(cfg.env.this_runs_folder, "G_2.pth")
    return cfg, dataset_test


def _csv(name, suffix=""):
    with open(os.path.join("test_output", f"{name}____metrics{suffix}.csv")) as f:
        return f.read()


def test_section_on_a_cpu_device_writes_the_same_csv(data_root, tmp_path, monkeypatch):
    from gan_sr_wind_field_amd.config.config import EvalConfig
    from gan_sr_wind_field_amd.test import test as evaluate

    cfg, ds = _trained(tmp_path, monkeypatch)
    monkeypatch.setattr(cfg, "eval", EvalConfig())
    cfg.eval.setEvalConfig(None)
    cfg.name = "plain"
    avg_a = evaluate(cfg, ds)
    cfg.eval.present, cfg.eval.device_metrics, cfg.eval.batch_size = True, True, 3
    cfg.name = "section"
    avg_b = evaluate(cfg, ds)
    a, b = _csv("plain"), _csv("section")
    assert a == b and len(a.splitlines()) == 1 + len(ds) and avg_a == avg_b
    rows = open(os.path.join("test_output", "averages.csv")).read().strip().splitlines()
    assert rows[1].split(",", 1)[1] == rows[2].split(",", 1)[1]


def test_run_py_passes_reverse_interpolate(data_root, tmp_path, monkeypatch):
    from gan_sr_wind_field_amd import run as runmod
    from gan_sr_wind_field_amd.test import METRIC_NAMES

    cfg, ds = _trained(tmp_path, monkeypatch, interpolate_z=True)
    cfg.name = "rev"
    ini = str(tmp_path / "rev.ini")
    base = cfg.asINI()
    with open(ini, "w") as f:
        f.write(base + "\n[EVAL]\nbatch_size = 2\nreverse_interpolate = True\n")
    seen = {}
    import gan_sr_wind_field_amd.test as tmod
    orig = tmod.test

    def spy(cfg_, ds_, *a, **kw):
        seen["args"], seen["kw"] = a, kw
        return orig(cfg_, ds_, *a, **kw)

    monkeypatch.setattr(tmod, "test", spy)
    runmod.main(["--test", "--cfg", ini])
    assert seen["kw"].get("reverse_interpolate") is True or seen["args"][:1] == (True,)
    head = "field," + ",".join(METRIC_NAMES)
    for suffix in ("", "_reverse_interpolate"):
        rows = _csv("rev", suffix).strip().splitlines()
        assert rows[0] == head and len(rows) == 1 + len(ds), suffix
        assert all(np.isfinite([float(v) for v in r.split(",")[1:]]).all() for r in rows[1:])
    rows = open(os.path.join("test_output", "averages_reverse_interpolate.csv")).read().strip().splitlines()
    assert rows[0].startswith("Name,Average PSNR") and rows[-1].startswith("rev,")
    # without the key the reverse files are not written, as before
    with open(ini, "w") as f:
        f.write(base.replace("name = rev\n", "name = norev\n", 1) + "\n[EVAL]\n")
    runmod.main(["--test", "--cfg", ini])
    assert os.path.isfile(os.path.join("test_output", "norev____metrics.csv"))
    assert not os.path.exists(os.path.join("test_output", "norev____metrics_reverse_interpolate.csv"))


def _only(cfg, monkeypatch, **sections):
    """fresh [DIAGNOSTICS], [SPECTRUM] and [SSIM] objects on ``cfg``, absent but for ``sections`` (name -> attributes)"""
    from gan_sr_wind_field_amd.config.config import DiagnosticsConfig, SpectrumConfig, SsimConfig

    for attr, cls in (("diagnostics", DiagnosticsConfig), ("spectrum", SpectrumConfig), ("ssim", SsimConfig)):
        sec = cls()
        sec.load(None)
        for k, v in sections.get(attr, {}).items():
            setattr(sec, k, v)
        sec.present = attr in sections
        sec.validate()
        monkeypatch.setattr(cfg, attr, sec)


SECTIONS = {"diagnostics": {"per_field": True}, "spectrum": {"per_level": True},
            "ssim": {"per_level": True, "window_size": 7, "sigma": 1.0}}
STEMS = {"diagnostics": "level_profile", "spectrum": "energy_spectrum", "ssim": "ssim"}


def _files(name):
    """what a run called ``name`` wrote: file name without the run's name -> text"""
    out = {}
    for f in sorted(os.listdir("test_output")):
        if f.startswith(name + "____"):
            with open(os.path.join("test_output", f)) as fh:
                out[f[len(name) + 4:]] = fh.read()
    return out


def test_all_sections_together_write_each_sections_own_files(data_root, tmp_path, monkeypatch):
    """[DIAGNOSTICS], [SPECTRUM] and [SSIM] at once, with ``reverse_interpolate``: 14 files, each the bytes of the run
    with only its own section; the metrics files are those of every run.  Exact: no tolerance.  And a first batch that
    raises (an SSIM window larger than the domain) leaves no file of the evaluation open."""
    import gan_sr_wind_field_amd.test as tmod

    cfg, ds = _trained(tmp_path, monkeypatch, interpolate_z=True)
    runs = {"plain": {}, **{k: {k: v} for k, v in SECTIONS.items()}, "all": SECTIONS}
    for name, sections in runs.items():
        cfg.gan_config.interpolate_z = True
        _only(cfg, monkeypatch, **sections)
        cfg.name = name
        tmod.test(cfg, ds, reverse_interpolate=True)
    got = {name: _files(name) for name in runs}
    metrics = {"metrics.csv", "metrics_reverse_interpolate.csv"}
    assert set(got["plain"]) == metrics
    assert len(got["all"]) == 14, sorted(got["all"])
    for sec, stem in STEMS.items():
        own = {f for f in got[sec] if f.startswith(stem)}
        assert len(own) == 4 and set(got[sec]) == metrics | own, (sec, sorted(got[sec]))
        for f in own:
            assert got["all"][f] == got[sec][f], f
    assert set(got["all"]) == metrics | {f for sec in STEMS for f in got[sec]}
    for f in metrics:
        assert len(got["plain"][f].splitlines()) == 1 + len(ds)
        assert all(got[name][f] == got["plain"][f] for name in runs), f
    # a window larger than the domain: the ValueError of the first batch comes through, and every file is closed
    made = []
    outputs = tmod._outputs
    monkeypatch.setattr(tmod, "_outputs", lambda *a, **kw: (made.append(o) or o for o in outputs(*a, **kw)))
    X, Y = ds[0][1].shape[1:3]
    _only(cfg, monkeypatch, **SECTIONS)
    cfg.ssim.window_size, cfg.name, cfg.gan_config.interpolate_z = 2 * max(X, Y) + 1, "wide", True
    with pytest.raises(ValueError, match=str(cfg.ssim.window_size)):
        tmod.test(cfg, ds, reverse_interpolate=True)
    assert [type(o).__name__ for o in made] == ["_LevelProfile", "_Spectrum", "_Ssim"] * 2
    for o in made:
        assert o.fields is None or o.fields.closed, type(o).__name__
    ssim_files = [o.path() for o in made if type(o).__name__ == "_Ssim"]
    assert len(ssim_files) == 2
    for path in ssim_files:
        os.remove(path)
    assert not any(os.path.realpath(os.path.join("/proc/self/fd", fd)).startswith(os.path.realpath("test_output"))
                   for fd in os.listdir("/proc/self/fd"))
    # (the whole-set files are written after a clean run only)
    assert not os.path.exists(os.path.join("test_output", "wide____level_profile.csv"))


OPTIONAL = {  # attribute -> (section, a key, a value that does not parse, what the message asks for)
    "grad_clip": ("GRAD_CLIP", "clip_generator", "maybe", "True or False"),
    "ema": ("EMA", "decay", "fast", "a number"),
    "eval": ("EVAL", "batch_size", "many", "an integer"),
    "ensemble": ("ENSEMBLE", "members", "8.5", "an integer"),
    "tile": ("TILE", "tile", "wide", "an integer"),
    "diagnostics": ("DIAGNOSTICS", "per_field", "some", "True or False"),
    "spectrum": ("SPECTRUM", "per_level", "2", "True or False"),
    "spectral_loss": ("SPECTRAL_LOSS", "weight", "heavy", "a number"),
    "degradation": ("DEGRADATION", "sigma", "wide", "a number"),
    "ssim": ("SSIM", "window_size", "11.0", "an integer"),
}


@pytest.mark.parametrize("attr", sorted(OPTIONAL))
def test_every_optional_section_names_section_and_key_of_an_unparsable_value(attr, tmp_path):
    from gan_sr_wind_field_amd.config.config import Config

    section, key, bad, what = OPTIONAL[attr]
    try:
        with pytest.raises(ValueError) as err:
            Config(_ini_with(tmp_path, f"[{section}]\n{key} = {bad}\n"))
        assert str(err.value) == f"[{section}] {key} must be {what}, not {bad!r}"
        assert type(getattr(Config, attr))._section == section
    finally:
        Config(LOCAL_INI)  # (the section objects are singletons: reset)
    assert getattr(Config, attr).present is False


def test_optional_sections_print_in_their_order(tmp_path):
    """three sections present at once print as the concatenation of what the per-section tests pin, in the order
    GRAD_CLIP, EMA, EVAL, ENSEMBLE, TILE, DIAGNOSTICS, SPECTRUM, SPECTRAL_LOSS, however the file orders them; [DATA],
    [DEGRADATION] and [SSIM] load and stay unprinted"""
    from gan_sr_wind_field_amd.config.config import Config

    try:
        plain = Config(LOCAL_INI).asINI()
        cfg = Config(_ini_with(tmp_path, "[SSIM]\nper_level = True\n\n[SPECTRUM]\nwindow = None\n\n[DATA]\n"
                                         "device_resident = True\n\n[EVAL]\n\n[DEGRADATION]\nkernel = Box\n\n[ENSEMBLE]\n"
                                         "members = 2\n"))
        assert cfg.ssim.on and cfg.ssim.per_level and cfg.data.device_resident and cfg.degradation.kernel == "box"
        assert cfg.asINI() == (plain + "\n[EVAL]\ndevice_metrics = True\nbatch_size = 8\nreverse_interpolate = False\n"
                               + "\n[ENSEMBLE]\nmembers = 2\nwrite_spread = False\n"
                               + "\n[SPECTRUM]\nenergy_spectrum = True\nper_level = False\nwindow = none\n")
        order = [attr for attr, _ in Config._optional]
        assert order == ["data", "grad_clip", "ema", "eval", "ensemble", "tile", "diagnostics", "spectrum",
                         "spectral_loss", "degradation", "ssim"]
    finally:
        Config(LOCAL_INI)
    assert Config(LOCAL_INI).asINI() == plain
