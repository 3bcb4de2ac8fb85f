"""[DISTRIBUTION_LOSS] on the CPU: the config section, ``soft_counts_reference`` against a plain double loop over the
definition, the analytic properties of ``L_dist`` (zero with a zero gradient for SR = HR, NaN for a non-finite SR, equal to
the shift for a field whose every speed is shifted by d), the closed-form vector-Jacobian product against autograd and a
central difference of the float64 reference, a generator iteration with the section on a CPU device, and the names the C
ABI carries.
"""
import math
import os
import re

import pytest
import torch

from conftest import REPO
from distribution_loss_bounds import random_upstream, ref_backward, tables_for, wind_fields
from test_eval import LOCAL_INI, _ini_with

G_KEYS = {"total", "adversarial", "pix", "xy_gradient", "z_gradient", "divergence", "xy_divergence", "feature_D"}
EXPORTS_NEW = ("wsr_speed_soft_counts_workspace_floats", "wsr_speed_soft_counts", "wsr_speed_soft_counts_bwd",
               "wsr_speed_soft_counts_geometry")


class Section:
    """the attributes ``distribution_loss`` reads from a config section"""

    def __init__(self, **kw):
        self.__dict__.update(dict(dict(pool="level"), **kw))


# ---------------------------------------------------------------------------------------------------- 1. config
def test_section_parses_validates_and_round_trips(tmp_path):
    from gan_sr_wind_field_amd.config.config import Config
    from gan_sr_wind_field_amd.distribution_loss import DISTRIBUTION_LOSS

    plain = Config(LOCAL_INI).asINI()
    off = Config(LOCAL_INI).distribution_loss
    assert off.present is False and off.on is False and "DISTRIBUTION_LOSS" not in plain
    assert DISTRIBUTION_LOSS == dict(weight=None, bin_width=None, speed_bins=32, pool="level")
    assert Config._optional_later[-1][0] == "distribution_loss"
    cfg = Config(_ini_with(tmp_path, "[DISTRIBUTION_LOSS]\nweight = 0.1\nbin_width = 1.5\n"))
    s = cfg.distribution_loss
    assert s.present and s.on
    assert {k: getattr(s, k) for k in DISTRIBUTION_LOSS} == dict(DISTRIBUTION_LOSS, weight=0.1, bin_width=1.5)
    assert cfg.distribution.present is False  # (independent of [DISTRIBUTION])
    assert cfg.asINI() == plain + "\n[DISTRIBUTION_LOSS]\nweight = 0.1\nbin_width = 1.5\nspeed_bins = 32\npool = level\n"
    both = Config(_ini_with(tmp_path, "[SSIM_LOSS]\nweight = 1\n[DISTRIBUTION]\nbin_width = 2\n[DISTRIBUTION_LOSS]\n; the "
                                      "weight\nweight = 2\nbin_width = 0.5\nspeed_bins = 64\npool = Sample\n"))
    assert both.distribution.bin_width == 2 and both.distribution_loss.bin_width == 0.5
    text = both.asINI()
    assert text.endswith("[DISTRIBUTION_LOSS]\nweight = 2.0\nbin_width = 0.5\nspeed_bins = 64\npool = sample\n")
    path = str(tmp_path / "snapshot.ini")
    with open(path, "w") as f:
        f.write(text)
    again = Config(path)
    assert vars(again.distribution_loss) == vars(both.distribution_loss) and again.asINI() == text
    ok = "weight = 1\nbin_width = 1\n"
    refusals = [("bin_width = 1\n", r"weight is required"), ("weight = 0\nbin_width = 1\n", r"weight.*0"),
                ("weight = -1\nbin_width = 1\n", r"weight.*-1"), ("weight = nan\nbin_width = 1\n", r"weight.*nan"),
                ("weight = 1\n", r"bin_width must be given"), ("weight = 1\nbin_width = 0\n", r"bin_width.*0"),
                ("weight = 1\nbin_width = -2.5\n", r"bin_width.*-2\.5"), ("weight = 1\nbin_width = inf\n", r"bin_width.*inf"),
                (ok + "speed_bins = 1\n", r"speed_bins.*1"), (ok + "speed_bins = 65\n", r"speed_bins.*65"),
                (ok + "pool = column\n", r"pool.*column"), (ok + "speed_bins = many\n", r"speed_bins must be an integer")]
    for body, pattern in refusals:
        with pytest.raises(ValueError, match=r"\[DISTRIBUTION_LOSS\] " + pattern):
            Config(_ini_with(tmp_path, "[DISTRIBUTION_LOSS]\n" + body))
    for bins in (2, 64):
        assert Config(_ini_with(tmp_path, f"[DISTRIBUTION_LOSS]\n{ok}speed_bins = {bins}\n")).distribution_loss.speed_bins == bins
    back = Config(LOCAL_INI)  # (the singleton is reset)
    assert back.distribution_loss.present is False and back.distribution_loss.weight is None and back.asINI() == plain


def test_tables_are_refused_with_the_number():
    from gan_sr_wind_field_amd.distribution_loss import soft_tables

    t = soft_tables(32.0, 1.5, 32)
    assert t.c == float(torch.tensor(32.0 / 1.5, dtype=torch.float64).float()) and t.speed_bins == 32
    for args, pattern in (((32.0, 0.0), "bin_width.*0"), ((32.0, 1.0, 1), "speed_bins.*1"), ((32.0, 1.0, 65), "65"),
                          ((0.0, 1.0), "UVW_MAX.*0"), ((float("inf"), 1.0), "UVW_MAX.*inf")):
        with pytest.raises(ValueError, match=pattern):
            soft_tables(*args)


# ---------------------------------------------------------------------------------------------------- 2. the reference
def _loop_tables(F, tables):
    """the definition, voxel by voxel in Python doubles -> (B, NZ, NS + 1) nested lists"""
    B, _, X, Y, NZ = F.shape
    ns, c = tables.speed_bins, tables.c
    H = [[[0.0] * (ns + 1) for _ in range(NZ)] for _ in range(B)]
    for b in range(B):
        for x in range(X):
            for y in range(Y):
                for z in range(NZ):
                    u, v = float(F[b, 0, x, y, z]), float(F[b, 1, x, y, z])
                    hs2 = u * u + v * v
                    if not math.isfinite(hs2):
                        H[b][z][ns] += 1.0
                        continue
                    t = min(max(math.sqrt(hs2) * c - 0.5, 0.0), ns - 1.0)
                    k0 = min(math.floor(t), ns - 2)
                    H[b][z][k0] += 1.0 - (t - k0)
                    H[b][z][k0 + 1] += t - k0
    return torch.tensor(H, dtype=torch.float64)


def test_the_reference_against_a_plain_loop_over_the_definition():
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_reference, soft_tables

    tables = soft_tables(32.0, 2.0, 8)  # c = 16: centres at (k + 1/2) / 16
    c = tables.c
    special = [(0.0, 0.0), (0.2 / c, 0.0), (0.0, -0.5 / c), (3.5 / c, 0.0), (0.0, 6.5 / c), (7.5 / c, 0.0), (0.7, 0.7),
               (float("nan"), 0.1), (2.25 / c, 0.0), (-3.0 / c, 4.0 / c)]
    B, X, Y, NZ = 2, 3, 4, 2
    gen = torch.Generator().manual_seed(3)
    HR = (torch.rand((B, 3, X, Y, NZ), generator=gen) - 0.5) * (12.0 / c)
    SR = (torch.rand((B, 4, X, Y, NZ), generator=gen) - 0.5) * (12.0 / c)
    SR[:, 3] = float("nan")  # (a surplus channel is never read)
    flat = SR.view(B, 4, -1)
    for i, (u, v) in enumerate(special):
        flat[i % B, 0, i], flat[i % B, 1, i] = u, v
    H = soft_counts_reference(HR, SR, tables)
    assert H.dtype == torch.float64 and H.shape == (2, B, NZ, 9)
    for s, F in enumerate((HR, SR)):
        want = _loop_tables(F, tables)
        assert float((H[s] - want).abs().max()) <= 1e-12, s
    assert bool((H.sum(dim=-1) - X * Y).abs().max() <= 1e-12)  # every row sums to X * Y
    assert float(H[0][..., 8].sum()) == 0.0 and float(H[1][..., 8].sum()) == 1.0  # the NaN, in its own column
    # on a centre: the whole voxel in that bin; below the first and beyond the last centre: the end bins
    one = torch.zeros((1, 2, 1, 1, 1))
    for (u, v), k in (((3.5 / c, 0.0), 3), ((0.2 / c, 0.0), 0), ((0.0, 0.0), 0), ((0.7, 0.7), 7), ((0.0, 7.5 / c), 7)):
        one[0, 0], one[0, 1] = u, v
        row = soft_counts_reference(one, one, tables)[1, 0, 0]
        assert abs(float(row[k]) - 1.0) <= 1e-6 and abs(float(row.sum()) - 1.0) <= 1e-12, (u, v, row)


def test_linear_binning_preserves_the_mean_speed_when_nothing_is_clamped():
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_reference, soft_tables

    tables = soft_tables(32.0, 1.0, 16)
    gen = torch.Generator().manual_seed(4)
    speed = (0.5 + 15.0 * torch.rand((2, 6, 5, 3), generator=gen, dtype=torch.float64)) / tables.c  # centres 0.5 .. 15.5
    phi = torch.rand(speed.shape, generator=gen, dtype=torch.float64) * 2 * math.pi
    F = torch.stack([speed * torch.cos(phi), speed * torch.sin(phi)], dim=1)
    H = soft_counts_reference(F, F, tables)[1]
    centres = (torch.arange(16, dtype=torch.float64) + 0.5) * tables.bin_width
    got = (H[..., :16] * centres).sum(dim=-1) / 30.0
    want = (torch.sqrt(F[:, 0] ** 2 + F[:, 1] ** 2) * tables.UVW_MAX).mean(dim=(1, 2))
    assert float((got - want).abs().max()) <= 1e-12 * 16


# ---------------------------------------------------------------------------------------------------- 3. the loss
def test_the_loss_is_zero_with_a_zero_gradient_for_equal_fields_and_nan_for_a_nan():
    from gan_sr_wind_field_amd.distribution_loss import distribution_loss

    tables = tables_for(32)
    for pool in ("level", "sample"):
        HR, SR = wind_fields(2, 3, 9, 8, 3, tables, seed=5)
        x = HR.clone().requires_grad_(True)
        zero = distribution_loss(HR, x, Section(pool=pool), tables)
        assert zero.dtype == torch.float32 and zero.dim() == 0 and float(zero.detach()) == 0.0
        zero.backward()
        assert bool((x.grad == 0).all())
        x = SR.clone().requires_grad_(True)
        L = distribution_loss(HR, x, Section(pool=pool), tables)
        L.backward()
        assert float(L.detach()) > 0 and bool(torch.isfinite(x.grad).all()) and bool((x.grad[:, 2:] == 0).all())
        assert float(x.grad.abs().max()) > 0
        bad = SR.clone()
        bad[1, 0, 2, 3, 1] = float("nan")
        assert math.isnan(float(distribution_loss(HR, bad, Section(pool=pool), tables)))
        assert math.isnan(float(distribution_loss(bad, SR, Section(pool=pool), tables)))
        inf = SR.clone()
        inf[0, 1, 0, 0, 0] = float("inf")
        assert math.isnan(float(distribution_loss(HR, inf, Section(pool=pool), tables)))
    with pytest.raises(ValueError, match="pool.*column"):
        distribution_loss(HR, SR, Section(pool="column"), tables)


@pytest.mark.parametrize("pool", ["level", "sample"])
@pytest.mark.parametrize("d_bins", [0.3, 1.0, 2.7])
def test_a_shift_of_every_speed_by_d_costs_d(pool, d_bins):
    """SR's speed = HR's + d in the same direction, every voxel unclamped, float64: the running sum of a voxel's weights
    over k < NS - 1 is NS - 1 - t, so the sum of F_hr - F_sr over k is the mean shift in bins, and every term has one
    sign because every voxel moves up: L_dist = d to rounding, also when the shift crosses bin centres."""
    from gan_sr_wind_field_amd.distribution_loss import loss_from_counts, soft_counts_reference, soft_tables

    tables = soft_tables(40.0, 1.25, 24)
    d = d_bins * tables.bin_width
    gen = torch.Generator().manual_seed(6)
    speed = (0.5 + 20.0 * torch.rand((2, 7, 6, 3), generator=gen, dtype=torch.float64)) / tables.c  # t in [0, 20]
    phi = torch.rand(speed.shape, generator=gen, dtype=torch.float64) * 2 * math.pi
    hr = torch.stack([speed * torch.cos(phi), speed * torch.sin(phi)], dim=1)
    moved = speed + d / tables.UVW_MAX  # t + d_bins <= 22.7 < NS - 1
    sr = torch.stack([moved * torch.cos(phi), moved * torch.sin(phi)], dim=1)
    H = soft_counts_reference(hr, sr, tables)
    L = loss_from_counts(H[0], H[1], tables.bin_width, pool)
    # (c is UVW_MAX / bin_width rounded to fp32: the shift in bins is d_bins to 2^-24)
    assert abs(float(L) - d) <= 1e-6 * d, (float(L), d)


# ---------------------------------------------------------------------------------------------------- 4. the VJP
def test_the_closed_form_vjp_against_autograd_and_a_central_difference():
    from gan_sr_wind_field_amd.distribution_loss import soft_counts_reference, soft_counts_vjp

    for ns, shape in ((32, (2, 3, 5, 7, 3)), (2, (1, 4, 6, 5, 2))):
        tables = tables_for(ns)
        B, C, X, Y, NZ = shape
        HR, SR = wind_fields(B, C, X, Y, NZ, tables, seed=7)
        G = random_upstream(B, NZ, ns, 8).double()
        x = SR.double().requires_grad_(True)
        H = soft_counts_reference(HR, x, tables)
        assert H.requires_grad
        (H[1][..., :ns] * G).sum().backward()
        closed = soft_counts_vjp(SR, G, tables)
        grad, bound, keep = ref_backward(SR, G.float(), tables)
        assert torch.equal(closed, grad)
        assert bool((x.grad[:, 2:] == 0).all()) and bool((closed[:, 2:] == 0).all())
        scale = float(closed.abs().max())
        assert scale > 0 and float((x.grad[:, :2] - closed[:, :2]).abs().max()) <= 1e-12 * scale
        # planted zeros and clamped voxels: no gradient
        u, v = SR[:, 0].double(), SR[:, 1].double()
        t = torch.sqrt(u * u + v * v) * tables.c - 0.5
        dead = (t <= 0) | (t >= ns - 1)
        assert int(dead.sum()) >= 6 and bool((closed[:, 0][dead] == 0).all()) and bool((closed[:, 1][dead] == 0).all())
        assert float(keep.double().mean()) >= 0.99
        # a central difference of the float64 reference at voxels away from a bin switch: H is piecewise linear in t
        h = 1e-7
        f = lambda s: float((soft_counts_reference(HR, s, tables)[1][..., :ns] * G).sum())  # noqa: E731
        inner = ((t - t.round()).abs() > 1e-3) & ~dead
        picks = inner.nonzero()[:: max(1, int(inner.sum()) // 6)][:6]
        for b, xx, yy, zz in picks.tolist():
            for ch in (0, 1):
                e = torch.zeros_like(SR, dtype=torch.float64)
                e[b, ch, xx, yy, zz] = h
                num = (f(SR.double() + e) - f(SR.double() - e)) / (2 * h)
                assert abs(num - float(closed[b, ch, xx, yy, zz])) <= 1e-5 * scale, (ns, b, ch, xx, yy, zz)


# ---------------------------------------------------------------------------------------------------- 5. the model
def _cpu_gan(section, ssim=None):
    from test_dist_gloo import _build_gan

    gan, cfg = _build_gan()
    for sec, keys in ((cfg.distribution_loss, section), (cfg.ssim_loss, ssim)):
        sec.present = keys is not None
        for k, v in (keys or {}).items():
            setattr(sec, k, v)
    return gan, cfg


def test_update_G_on_a_cpu_device_with_and_without_the_section(monkeypatch):
    from gan_sr_wind_field_amd import distribution_loss as mod
    from gan_sr_wind_field_amd.config.config import DistributionLossConfig, SsimLossConfig
    from oracle.gan import synthetic_batch
    from test_dist_gloo import _g_iteration

    LR, HR, Z, x, y = synthetic_batch(2, 16, 4, 4, seed=2001)
    W, BW, NS, UVW = 0.1, 1.0, 32, 20.0
    seen = []
    orig = mod.soft_counts

    def recorded(hr, sr, tables):
        seen.append((hr.detach().clone(), sr.detach().clone(), tables))
        return orig(hr, sr, tables)

    monkeypatch.setattr(mod, "soft_counts", recorded)
    section = dict(weight=W, bin_width=BW, speed_bins=NS, pool="level")
    try:
        gan0, cfg0 = _cpu_gan(None)
        w0, l0 = _g_iteration(gan0, cfg0, LR, HR, Z, x, y)
        assert not seen and set(l0) == G_KEYS  # never called, exactly the old keys
        assert set(gan0.get_G_val_loss_dict_ref()) == G_KEYS
        # the scale given but no section: never read, the same bits
        gan00, cfg00 = _cpu_gan(None)
        gan00.set_wind_scale(UVW)
        w00, l00 = _g_iteration(gan00, cfg00, LR, HR, Z, x, y)
        assert not seen and l00 == l0 and all(torch.equal(w00[k], w0[k]) for k in w0)

        gan1, cfg1 = _cpu_gan(section)
        with pytest.raises(ValueError, match=r"set_wind_scale\(dataset_train\.UVW_MAX\)"):
            _g_iteration(gan1, cfg1, LR, HR, Z, x, y)
        gan1, cfg1 = _cpu_gan(section)
        gan1.set_wind_scale(UVW)
        before = {k: v.clone() for k, v in gan1.G.state_dict().items()}
        w1, l1 = _g_iteration(gan1, cfg1, LR, HR, Z, x, y)
        assert len(seen) == 1 and torch.equal(seen[0][0], HR)
        tables = seen[0][2]
        assert (tables.speed_bins, tables.bin_width, tables.UVW_MAX) == (NS, BW, UVW)
        assert gan1._distribution_tables() is tables  # built once
        H = mod.soft_counts_reference(seen[0][0], seen[0][1], tables)
        want = W * float(mod.loss_from_counts(H[0], H[1], BW, "level"))
        assert want > 0 and abs(l1["distribution"] - want) <= 1e-5 * want
        # one more entry of the core vector: the total moves by it, the other terms do not, the step differs
        assert abs((l1["total"] - l0["total"]) - l1["distribution"]) <= 1e-5 * abs(l1["total"])
        assert set(l1) == G_KEYS | {"distribution"} and all(l1[k] == l0[k] for k in l0 if k != "total")
        assert any(not torch.equal(w1[k], w0[k]) for k in w0)

        # with [SSIM_LOSS] too: ``distribution`` behind ``ssim``, each weighted by its own weight
        gan3, cfg3 = _cpu_gan(dict(section, pool="sample"), ssim=dict(weight=0.05, window_size=7, sigma=1.0))
        gan3.set_wind_scale(UVW)
        _, l3 = _g_iteration(gan3, cfg3, LR, HR, Z, x, y)
        assert list(l3)[-2:] == ["ssim", "distribution"] and l3["distribution"] > 0 and l3["ssim"] > 0
        assert abs((l3["total"] - l0["total"]) - l3["ssim"] - l3["distribution"]) <= 1e-5 * abs(l3["total"])
        cfg3.ssim_loss.present = False

        # a non-finite voxel in a table: NaN on the device side of the loss, the Adam step is skipped, the weights stay
        gan2, cfg2 = _cpu_gan(section)
        gan2.set_wind_scale(UVW)

        def poisoned(hr, sr, tables):
            H = orig(hr, sr, tables).clone()
            H[1, 0, 0, 0] -= 1.0
            H[1, 0, 0, tables.speed_bins] += 1.0
            return H

        monkeypatch.setattr(mod, "soft_counts", poisoned)
        _, l2 = _g_iteration(gan2, cfg2, LR, HR, Z, x, y)
        assert math.isnan(l2["distribution"]) and math.isnan(l2["total"])
        for k, v in gan2.G.state_dict().items():
            assert torch.equal(v, before[k]), k
        # validation logs it too
        monkeypatch.setattr(mod, "soft_counts", orig)
        gan1.update_G(LR, HR, Z, 0, False)
        assert float(gan1.get_G_val_loss_dict_ref()["distribution"]) > 0
    finally:
        for cls, sec in ((DistributionLossConfig, cfg0.distribution_loss), (SsimLossConfig, cfg0.ssim_loss)):  # (singletons)
            for k in ["present"] + [k for k, _ in cls._schema]:
                setattr(sec, k, getattr(cls, k))


# ---------------------------------------------------------------------------------------------------- 6. the C ABI
def test_exports_are_in_the_header_and_in_EXPORTS():
    from gan_sr_wind_field_amd._lib import EXPORTS

    with open(os.path.join(REPO, "include", "windsr_hip.h")) as f:
        header = f.read()
    for n in EXPORTS_NEW:
        assert n in EXPORTS and re.search(rf"\b{n}\s*\(", header), n
    assert int(re.search(r"#define\s+WSR_ABI_VERSION\s+(\d+)", header).group(1)) == 9
    assert int(re.search(r"#define\s+WSR_DISTRIBUTION_LOSS_LDS_COUNTERS\s+(\d+)", header).group(1)) == 65 * 128
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "csrc", "Makefile")) as f:
        assert "distribution_loss.hip" in f.read()
    with open(os.path.join(REPO, "gan_sr_wind_field_amd", "train.py")) as f:
        assert "gan.set_wind_scale(dataset_train.UVW_MAX)" in f.read()
