"""Horizontal kinetic-energy spectra (``[SPECTRUM]``): what ``run.py --test`` can report per horizontal wavenumber - the
energy of the truth, the super-resolved field and the trilinear baseline, and the coherence of the latter two with the
truth, which tells recovered detail from invented detail.  Every point-wise metric favours a blurred field; the spectrum
shows whether the small scales are there.

Everything is built from five sums per sample, z level and wavenumber bin (``SPECTRUM_SUMS``): on a GPU
``hip_ops.level_spectra`` takes them with a direct separable DFT (csrc/spectra.hip), ``level_spectra_reference`` composes
the same sums from ``torch.fft.rfft2`` and ``index_add_`` on any device (the path of a CPU device, and the oracle of the
CPU tests).  ``spectrum_from_sums`` turns a table of sums into the columns of ``<name>____energy_spectrum.csv``, defined
once for both evaluation loops.

Definitions (one 2-D transform over (X, Y) per sample, field, component and level):

    g = (f - m) * w                      m the plain mean of f over the plane, w(i, j) = wx(i) wy(j);  ``hann``:
                                         wx(i) = sin^2(pi (i + 1/2) / X), likewise wy, an axis of length 1 has weight 1;
                                         ``none``: w = 1;  W2 = sum w^2
    F(kx, ky) = sum g exp(-2 pi i (kx i / X + ky j / Y)),  ky = 0 .. Y // 2 (the input is real), Hermitian weight
                                         h(ky) = 1 for ky = 0 and, Y even, for ky = Y / 2, else 2
    bin = floor(kappa + 1/2),            kappa = N sqrt((kx' / X)^2 + (ky / Y)^2), N = max(X, Y), kx' the signed
                                         frequency of kx; NK = floor(N / sqrt(2) + 1/2) + 1 bins.  Decided in exact
                                         integers: with q = (kx' Y)^2 + (ky X)^2 the bin is the k >= 0 with
                                         (2k - 1)^2 (XY)^2 <= 4 N^2 q < (2k + 1)^2 (XY)^2 (for k = 0 the right half alone)
    e_a = 1/2 sum_comp sum_modes-in-bin h |F_a|^2 / (X Y W2)
    c_b = 1/2 sum_comp sum_modes-in-bin h Re(F_HR conj F_b) / (X Y W2)

so that the sum over all bins of ``e_a`` is half the window-weighted variance of field ``a`` on that level (Parseval).
"""
from __future__ import annotations

import math

import torch

#: the five sums of one (sample, level, bin), in the order of ``wsr_level_spectra``
SPECTRUM_SUMS = ("e_hr", "e_sr", "e_tl", "c_sr", "c_tl")

#: the columns of the spectrum files, after ``bin`` (and ``level`` in the per-level file)
SPECTRUM_COLUMNS = ("wavelength_m", "n_modes", "E_HR", "E_SR", "E_trilinear", "ratio_SR", "ratio_trilinear",
                    "coherence_SR", "coherence_trilinear", "err_SR", "err_trilinear")

WINDOWS = ("none", "hann")  # the window codes of ``wsr_level_spectra``: their indices
MAX_XY = 1024  # the integer test of ``bin_index`` fits int64 up to here (WSR_SPECTRUM_MAX_XY)


def n_bins(X: int, Y: int) -> int:
    """NK = floor(N / sqrt(2) + 1/2) + 1 in exact integers: the largest k with (2k - 1)^2 <= 2 N^2, plus one"""
    N = max(int(X), int(Y))
    k = math.isqrt(2 * N * N)  # (2k - 1 <= sqrt(2) N: k <= (isqrt(2 N^2) + 1) / 2)
    return (k + 1) // 2 + 1


def bin_index(X: int, Y: int) -> torch.Tensor:
    """The bin of every mode (kx, ky), ky = 0 .. Y // 2 -> int64 (X, Y // 2 + 1), decided in exact integers (see the
    module docstring); a float guess corrected by the integer test."""
    X, Y = int(X), int(Y)
    if not (0 < X <= MAX_XY and 0 < Y <= MAX_XY):
        raise ValueError(f"bin_index wants 1 <= X, Y <= {MAX_XY} (the integer test is 64-bit), not X = {X}, Y = {Y}")
    N = max(X, Y)
    kx = torch.arange(X, dtype=torch.int64)
    kx = torch.where(kx <= X // 2, kx, kx - X).view(X, 1)
    ky = torch.arange(Y // 2 + 1, dtype=torch.int64).view(1, -1)
    q = (kx * Y) ** 2 + (ky * X) ** 2
    lhs, xy2 = 4 * N * N * q, (X * Y) ** 2
    k = torch.floor(N * torch.sqrt(q.double()) / (X * Y) + 0.5).to(torch.int64)
    for _ in range(2):  # (the guess is off by one at the most: one step either way, twice to be sure)
        k = k - ((k > 0) & (lhs < (2 * k - 1) ** 2 * xy2)).to(torch.int64)
        k = k + (lhs >= (2 * k + 1) ** 2 * xy2).to(torch.int64)
    assert bool(((lhs < (2 * k + 1) ** 2 * xy2) & ((k == 0) | (lhs >= (2 * k - 1) ** 2 * xy2))).all())
    return k


def hermitian_weight(Y: int) -> torch.Tensor:
    """h(ky), ky = 0 .. Y // 2 -> float64 (Y // 2 + 1,)"""
    h = torch.full((Y // 2 + 1,), 2.0, dtype=torch.float64)
    h[0] = 1.0
    if Y % 2 == 0:
        h[Y // 2] = 1.0
    return h


def mode_counts(X: int, Y: int) -> torch.Tensor:
    """The number of modes (kx, ky) of the full X x Y spectrum in every bin -> int64 (NK,): a function of the shape"""
    idx = bin_index(X, Y)
    h = hermitian_weight(Y).to(torch.int64).view(1, -1).expand_as(idx)
    return torch.zeros(n_bins(X, Y), dtype=torch.int64).index_add_(0, idx.flatten(), h.flatten())


def window_2d(X: int, Y: int, window: str = "hann", dtype=torch.float64) -> torch.Tensor:
    """w (X, Y) of the module docstring"""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, not {window!r}")

    def axis(n):
        if window == "none" or n == 1:
            return torch.ones(n, dtype=torch.float64)
        return torch.sin(math.pi * (torch.arange(n, dtype=torch.float64) + 0.5) / n) ** 2

    return (axis(X).view(X, 1) * axis(Y).view(1, Y)).to(dtype)


def level_spectra_reference(HR, SR, TL, window: str = "hann", dtype=torch.float64) -> torch.Tensor:
    """The five sums of ``SPECTRUM_SUMS`` per sample, level and bin, composed from ``torch.fft.rfft2`` and ``index_add_``
    in ``dtype`` on the tensors' device: HR, SR, TL (B, C >= 3, X, Y, NZ; channels 0..2) -> (B, NZ, NK, 5)."""
    B, _, X, Y, NZ = HR.shape
    dev = HR.device
    w64 = window_2d(X, Y, window)
    W2 = float((w64 ** 2).sum())
    w = w64.to(device=dev, dtype=dtype).view(1, 1, 1, X, Y)
    F = []
    for f in (HR, SR, TL):
        f = f[:, :3].to(dtype).permute(0, 1, 4, 2, 3)  # (B, 3, NZ, X, Y)
        F.append(torch.fft.rfft2((f - f.mean(dim=(-2, -1), keepdim=True)) * w))
    h = hermitian_weight(Y).to(device=dev, dtype=dtype)
    scale = 0.5 / (X * Y * W2)
    terms = [(F[a].real ** 2 + F[a].imag ** 2) for a in range(3)]
    terms += [F[0].real * F[b].real + F[0].imag * F[b].imag for b in (1, 2)]
    modes = torch.stack([(t * h).sum(dim=1) for t in terms], dim=-1)  # (B, NZ, X, KY, 5): summed over the components
    idx = bin_index(X, Y).flatten().to(dev)
    out = torch.zeros((B, NZ, n_bins(X, Y), len(SPECTRUM_SUMS)), dtype=dtype, device=dev)
    out.index_add_(2, idx, modes.reshape(B, NZ, -1, len(SPECTRUM_SUMS)))
    return out * scale


def spectrum_from_sums(sums, nplanes, UVW_MAX, N, d, counts=None) -> dict:
    """``SPECTRUM_COLUMNS`` as per-bin lists of Python floats from a table ``sums`` (NK, 5) (nested lists or a tensor)
    summed over ``nplanes`` planes (levels times fields).  ``N`` = max(X, Y) and ``d`` the mean grid spacing in metres
    give the wavelength N d / bin (inf for bin 0); ``counts`` the modes per bin (``mode_counts(X, Y)``; of the square
    N x N domain when not given).
    Energies in m^2/s^2 (times ``UVW_MAX``^2), ``err_*`` the spectrum of the error field; a zero denominator gives nan."""
    rows = sums.tolist() if torch.is_tensor(sums) else sums
    n, U2 = float(nplanes), float(UVW_MAX) ** 2
    counts = mode_counts(int(N), int(N)) if counts is None else counts
    cnt = counts.tolist() if torch.is_tensor(counts) else counts
    out = {k: [] for k in SPECTRUM_COLUMNS}

    def div(a, b):
        return a / b if b != 0 else math.nan

    for k, s in enumerate(rows):
        e_hr, e_sr, e_tl, c_sr, c_tl = (float(v) for v in s)
        E = [div(v, n) * U2 for v in (e_hr, e_sr, e_tl, c_sr, c_tl)]

        def coh(c, e):
            den = e_hr * e
            return c / math.sqrt(den) if den > 0 else math.nan

        vals = (float(N) * float(d) / k if k else math.inf, float(cnt[k]), E[0], E[1], E[2],
                div(E[1], E[0]), div(E[2], E[0]), coh(c_sr, e_sr), coh(c_tl, e_tl), E[0] + E[1] - 2 * E[3],
                E[0] + E[2] - 2 * E[4])
        for name, v in zip(SPECTRUM_COLUMNS, vals):
            out[name].append(v)
    return out


def grid_spacing(x, y) -> float:
    """the mean grid spacing of ``x``, or of ``y`` when X = 1 (1.0 for a single point)"""
    for c in (x, y):
        c = [float(v) for v in (c.tolist() if hasattr(c, "tolist") else c)]
        if len(c) > 1:
            return abs(c[-1] - c[0]) / (len(c) - 1)
    return 1.0
