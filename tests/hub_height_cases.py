"""What tests/test_hub_height.py and tests/test_hub_height_gpu.py share: the shapes, the inputs and the special columns
(those of tools/hub_height_host_check.cpp).  Nothing here is a tolerance.

``make`` builds one case: a smooth terrain between 0 and 400 m (multiples of 0.25 m, so that terrain + height is exact
for the special columns), column tops between 120 and 600 m above ground, the lowest level at 2 m and the levels
stretched quadratically; HR, SR and TL are random around a logarithmic mean profile; every surplus channel, channel 2
(w) included, is NaN: nothing but u and v can be read.

``case`` asserts two conditions with the CPU reference, so they are checked without a GPU; the pinned seeds satisfy
them: with the heights 10, 50, 100 and 150 m every (sample, height) of every case has n_valid > 0, and in every case
marked partial at least one height has 0 < n_valid < X * Y in every sample."""
import math

import torch

UVW = 32.0
HEIGHTS = (10.0, 50.0, 100.0, 150.0)
NAN = float("nan")
#: ((B, X, Y, NZ), seed, partial).  The shapes: staged columns that do not fill the block; the reference's patch; the
#: largest NZ (two columns per chunk); several workgroups per sample; a unit axis and the minimal column; remainders on
#: every axis; more chunks than partial rows (a workgroup walks two chunks: 70 * 60 / 2 = 2100 > 2048)
CASES = (((2, 7, 6, 5), 101, True),
         ((1, 16, 16, 10), 102, True),
         ((1, 9, 5, 128), 103, True),
         ((1, 40, 40, 8), 104, True),
         ((1, 3, 1, 2), 105, False),
         ((3, 33, 17, 10), 106, True),
         ((1, 70, 60, 128), 107, True))
MODES = ("linear", "log")
KINDS = 11
#: (u, v) of HR, SR and TL on the level a height of special columns 0 and 1 lies on: multiples of 1/16 on 3-4-5 triangles,
#: so that u u, v v, their sum and its root (``KNOT_V``) are exact in fp32 - a knot that comes back one bit off shows in V
KNOT_UV = ((0.1875, 0.25), (0.25, -0.1875), (-0.375, 0.5))
KNOT_V = (0.3125, 0.3125, 0.625)

_cache = {}


def default_curve():
    from gan_sr_wind_field_amd.config.config import default_power_curve

    return default_power_curve()


def tables(heights=HEIGHTS, uvw=UVW, curve=None):
    from gan_sr_wind_field_amd.hub_height import hub_height_tables

    speeds, power = default_curve() if curve is None else curve
    return hub_height_tables(uvw, heights, speeds, power)


def terrain_of(X, Y):
    i, j = torch.arange(X, dtype=torch.float64)[:, None], torch.arange(Y, dtype=torch.float64)[None, :]
    t = 200.0 + 200.0 * torch.sin(2 * math.pi * (1.3 * i / X + 0.2)) * torch.cos(2 * math.pi * (0.9 * j / Y + 0.1))
    return (torch.floor(t * 4.0) / 4.0).float()


def wind(h, gen, channels=(4, 3, 3)):
    """HR, SR, TL (B, c, X, Y, NZ) for heights above ground ``h`` (B, X, Y, NZ): a logarithmic profile of about 0.3 at
    600 m in a direction that differs between the sources, plus noise; NaN in channel 2 and above"""
    B, X, Y, NZ = h.shape
    hh = torch.where(torch.isnan(h) | (h < 0.06), torch.full_like(h, 0.06), h).double()
    prof = 0.3 * torch.log(hh / 0.05) / math.log(600.0 / 0.05)
    out = []
    for s, c in enumerate(channels):
        d = 0.6 + 0.2 * s + 0.3 * (2 * torch.rand(h.shape, generator=gen, dtype=torch.float64) - 1)
        f = torch.full((B, c, X, Y, NZ), NAN)
        f[:, 0] = (prof * torch.cos(d) + 0.03 * (2 * torch.rand(h.shape, generator=gen, dtype=torch.float64) - 1)).float()
        f[:, 1] = (prof * torch.sin(d) + 0.03 * (2 * torch.rand(h.shape, generator=gen, dtype=torch.float64) - 1)).float()
        out.append(f.contiguous())
    return out


def make(B, X, Y, NZ, seed, channels=(4, 3, 3)):
    """-> HR, SR, TL, Z (B, 1, X, Y, NZ), terrain (X, Y)"""
    gen = torch.Generator().manual_seed(seed)
    terrain = terrain_of(X, Y)
    top = 120.0 + 480.0 * torch.rand((B, X, Y, 1), generator=gen, dtype=torch.float64)
    frac = (torch.arange(NZ, dtype=torch.float64) / (NZ - 1)) ** 2
    h = (2.0 + (top - 2.0) * frac).float()
    Z = (terrain[None, :, :, None] + h)[:, None].contiguous()
    HR, SR, TL = wind(h, gen, channels)
    return HR, SR, TL, Z, terrain


def case(k):
    """the inputs of ``CASES[k]``, made once, with the two conditions of the module docstring asserted"""
    from gan_sr_wind_field_amd.hub_height import hub_height_reference

    if k not in _cache:
        (B, X, Y, NZ), seed, partial = CASES[k]
        inputs = make(B, X, Y, NZ, seed)
        n = hub_height_reference(*inputs, tables(), "linear")[..., 0]
        assert bool((n > 0).all()), (CASES[k], n.tolist())
        if partial:
            assert bool(((n > 0) & (n < X * Y)).any(dim=1).all()), (CASES[k], n.tolist())
        _cache[k] = inputs
    return _cache[k]


def special_column(kind, q, NZ):
    """The heights above ground (fp32, NZ) of special column ``kind`` for the height ``q``, and whether its terrain has to
    be 0 for the altitude to be the height itself bit for bit (tools/hub_height_host_check.cpp: special_column)"""
    q32 = torch.tensor(q, dtype=torch.float32)
    m = NZ // 2
    step = max(math.floor(q / (2.0 * (m + 1)) * 4.0) / 4.0, 0.25)
    k = torch.arange(NZ, dtype=torch.float32)

    def spread(lo, hi):
        return torch.tensor(lo, dtype=torch.float32) + torch.tensor(hi - lo, dtype=torch.float32) * k / float(NZ - 1)

    up, down = torch.nextafter(q32, torch.tensor(1e9)), torch.nextafter(q32, torch.tensor(0.0))
    if kind == 0:                      # q on level m
        return q32 + (k - m) * step, False
    if kind == 1:                      # q on the top level
        return q32 - (NZ - 1 - k) * step, False
    if kind in (2, 3):                 # the top level one fp32 step below / above q
        h = spread(1.0, q)
        h[-1] = down if kind == 2 else up
        return h, True
    if kind in (4, 5):                 # the lowest level one fp32 step above / below q
        h = spread(q, 4.0 * q)
        h[0] = up if kind == 4 else down
        return h, True
    if kind == 6:                      # the column begins above 10 and 50 m
        return spread(60.0, 500.0), False
    if kind == 7:                      # the lowest level on the ground
        return spread(0.0, 400.0), False
    if kind == 8:                      # ... below it
        return spread(-1.0, 400.0), False
    h = spread(2.0, 400.0)             # a NaN altitude at the lowest level (9) or at an inner one (10)
    h[0 if kind == 9 else (NZ // 2 if NZ > 2 else 1)] = NAN
    return h, True


def plant_specials(inputs, cps, heights=HEIGHTS, seed=7):
    """A copy of ``inputs`` with the special columns at the first and the last column, on both sides of the first
    staging boundary (``cps`` columns per chunk) and at every fifth column, for the heights ``heights[0]`` and
    ``heights[1]`` in turn; the wind of the new columns follows their heights -> (HR, SR, TL, Z, terrain, kinds) with
    ``kinds`` (B, X * Y) the kind planted at a column, -1 for none"""
    HR, SR, TL, Z, terrain = (t.clone() for t in inputs)
    B, _, X, Y, NZ = Z.shape
    ncols = X * Y
    marks = (0, cps - 1, cps, ncols - 1)
    kinds = torch.full((B, ncols), -1, dtype=torch.long)
    for b in range(B):
        for c in range(ncols):
            if c % 5 == 0:
                kinds[b, c] = (c // 5 + b) % KINDS
            for i, mark in enumerate(marks):
                if c == mark:
                    kinds[b, c] = (b * 4 + i + (0 if c == 0 else 3)) % KINDS
    hs = {}
    h = Z[:, 0] - terrain[None, :, :, None]  # (the other samples keep their heights above a ground that moves to 0)
    tflat = terrain.view(-1)
    for b, c in (kinds >= 0).nonzero().tolist():
        hs[b, c], ground0 = special_column(int(kinds[b, c]), heights[(c + b) % 2], NZ)
        if ground0:
            tflat[c] = 0.0
    for (b, c), col in hs.items():
        h[b].view(ncols, NZ)[c] = col
    Z = (terrain[None, :, :, None] + h)[:, None].contiguous()
    W = wind(h, torch.Generator().manual_seed(seed), (HR.shape[1], SR.shape[1], TL.shape[1]))
    special = (kinds >= 0).view(B, 1, X, Y, 1)
    HR, SR, TL = (torch.where(special, w, f).contiguous() for w, f in zip(W, (HR, SR, TL)))
    for b, c in ((kinds == 0) | (kinds == 1)).nonzero().tolist():  # the level the height lies on holds ``KNOT_UV``
        level = NZ // 2 if kinds[b, c] == 0 else NZ - 1
        for f, uv in zip((HR, SR, TL), KNOT_UV):
            f[b, 0].view(ncols, NZ)[c, level], f[b, 1].view(ncols, NZ)[c, level] = uv
    return HR, SR, TL, Z, terrain, kinds
