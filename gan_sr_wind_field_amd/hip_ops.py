"""Thin torch-tensor front end over the C-ABI (device pointers + current stream).

Activations are ``(B, X, Y, Z, ctot)`` contiguous tensors ("NDHWC"), fp32 or
bf16; filters are packed ``[rows][taps][k]`` tensors produced by
:func:`pack_filter`.  Every function launches on the *current* torch stream and
returns immediately; nothing here allocates behind the caller's back except
where a fresh output tensor is the documented result.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, Epilogue, check

Tensor = torch.Tensor


def dtype_id(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return _lib.WSR_F32
    if dt == torch.bfloat16:
        return _lib.WSR_BF16
    raise TypeError(f"unsupported activation dtype {dt}")


def piece_elems(dt: torch.dtype) -> int:
    """Channels per 16-byte piece (granularity of channel windows on the MFMA path)."""
    return 4 if dt == torch.float32 else 8


def pad_channels(c: int, dt: torch.dtype) -> int:
    e = piece_elems(dt)
    return (c + e - 1) // e * e


# torch.cuda.current_stream() / current_device() cost ~8 us / ~1 us of Python per call (device-index normalisation,
# lazy-init checks, a Stream object); at ~2 000 launches per step that is most of the host time of the launch-bound
# real-data shapes.  The raw accessors below are what they end in.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> C.c_void_p:
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _need_cuda(*ts: Tensor) -> None:
    """Operands must live on the CURRENT device: the kernels are launched on its current stream with raw
    pointers, so a tensor of another GPU would be a wild pointer there (no CPU fallback either)."""
    cur = -1
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("windsr_hip kernels need device tensors (no CPU fallback)")
        if cur < 0:
            cur = _raw_device() if _raw_device is not None else torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(f"windsr_hip: tensor on {t.device} but the current device is cuda:{cur} "
                               "(set torch.cuda.set_device / cfg.device for this rank)")


@dataclass(frozen=True)
class ConvGeom:
    """Static description of a conv layer (reference ``nn.Conv3d`` arguments)."""

    cin: int
    cout: int
    kernel: Tuple[int, int, int]
    stride: Tuple[int, int, int] = (1, 1, 1)
    pad: Tuple[int, int, int] = (1, 1, 1)
    upsample: bool = False  # nearest x(2,2,1) in front (torch_blocks.py:345-347)

    @property
    def taps(self) -> int:
        return self.kernel[0] * self.kernel[1] * self.kernel[2]

    def out_extent(self, xi: int, yi: int, zi: int) -> Tuple[int, int, int]:
        u = 2 if self.upsample else 1
        k, s, p = self.kernel, self.stride, self.pad
        return ((xi * u + 2 * p[0] - k[0]) // s[0] + 1, (yi * u + 2 * p[1] - k[1]) // s[1] + 1,
                (zi + 2 * p[2] - k[2]) // s[2] + 1)


_desc_cache: dict = {}


def make_desc(g: ConvGeom, dt: torch.dtype, B: int, in_xyz, in_ctot: int, in_off: int, out_ctot: int,
              out_off: int, cin: Optional[int] = None, cout: Optional[int] = None, lat=None) -> ConvDesc:
    """``lat`` = (ox, oy, phases): a parity conv of the sub-pixel form of an up-sampling conv (``wsr_conv_t.lat``) -
    same-size, ``g.pad`` = the LOW pads, output voxels on the (2x + ox, 2y + oy) lattice of a tensor twice as large
    along x and y; phases = 4: all four parities in one forward launch.

    The descriptor is pure geometry: it is built once per distinct argument tuple and shared (callers pass it to
    the C side by const reference and never write to it) - filling the 30 ctypes fields cost ~10 us of the ~17 us
    of Python per launch on the launch-bound real-data shapes."""
    key = (g, dt, B, tuple(in_xyz), in_ctot, in_off, out_ctot, out_off, cin, cout, None if lat is None else tuple(lat))
    d = _desc_cache.get(key)
    if d is not None:
        return d
    if len(_desc_cache) > 8192:
        _desc_cache.clear()
    d = _desc_cache[key] = _build_desc(g, dt, B, in_xyz, in_ctot, in_off, out_ctot, out_off, cin, cout, lat)
    return d


def _build_desc(g, dt, B, in_xyz, in_ctot, in_off, out_ctot, out_off, cin, cout, lat) -> ConvDesc:
    xo, yo, zo = g.out_extent(*in_xyz)
    if lat is not None:
        xo, yo, zo = in_xyz
    d = ConvDesc()
    d.dtype = dtype_id(dt)
    d.B = B
    d.Xi, d.Yi, d.Zi = in_xyz
    d.Xo, d.Yo, d.Zo = xo, yo, zo
    d.Cin, d.in_ctot, d.in_off = (g.cin if cin is None else cin), in_ctot, in_off
    d.Cout, d.out_ctot, d.out_off = (g.cout if cout is None else cout), out_ctot, out_off
    d.KX, d.KY, d.KZ = g.kernel
    d.sx, d.sy, d.sz = g.stride
    d.px, d.py, d.pz = g.pad
    d.upsample_xy = 1 if g.upsample else 0
    if lat is not None:
        d.lat, d.lat_ox, d.lat_oy, d.lat_phases = 2, lat[0], lat[1], lat[2]
        if len(lat) > 3:  # (ox, oy, phases, mz, oz): z lattice of the output as well
            d.lat_mz, d.lat_oz = lat[3], lat[4]
        if len(lat) > 5 and lat[5]:  # (..., True): the INPUT sits on the lattice (filter gradients of strided convs)
            d.lat = 3
    return d


def conv_fwd(desc: ConvDesc, x: Tensor, w: Tensor, y: Tensor, *, bias: Optional[Tensor] = None,
             chan_scale: Optional[Tensor] = None, res: Optional[Tensor] = None, res_off: int = 0,
             alpha: float = 1.0, beta: float = 0.0, act: bool = False, slope: float = 0.2,
             out_planar: bool = False) -> Tensor:
    _need_cuda(x, w, y, bias, chan_scale, res)
    ep = Epilogue()
    ep.bias, ep.chan_scale, ep.res = _p(bias), _p(chan_scale), _p(res)
    ep.res_ctot = res.shape[-1] if res is not None else 0
    ep.res_off = res_off
    ep.alpha, ep.beta = alpha, beta
    ep.act, ep.slope = int(act), slope
    ep.out_planar = int(out_planar)
    check(_lib.lib().wsr_conv3d_fwd(C.byref(desc), _p(x), _p(w), _p(y), C.byref(ep), _stream()), "conv3d_fwd")
    return y


_tile_ws: dict = {}
TILE_WS_BYTES = 32 << 20

#: bumped by :func:`reload_env`; host-side caches of values that depend on the WSR_* tuning switches (the split counts
#: of the filter-gradient plans, unpack job tables) compare it and start over
ENV_GEN = [0]


def reload_env() -> None:
    """The process changed its WSR_* environment at run time (tests, tuning scripts): have the C side read its cached
    switches again (``wsr_reload_env``) and invalidate what the host side cached from them."""
    check(_lib.lib().wsr_reload_env(), "reload_env")
    ENV_GEN[0] += 1


def tile_workspace(dev=None):
    """(pointer, bytes) of the split-reduction workspace the tile entry points get with every call (``wsr_epilogue_t.ws``,
    ``wsr_dgrad_opts_t.ws``): launches with few workgroups and a long reduction (the discriminator's deep layers) then
    spread the reduction channels over up to 256 workgroups.  One buffer per (device, stream) - launches on one
    stream are ordered, launches on different streams may overlap and must not share partial sums; the library itself
    keeps no state.  Owned here, lives as long as the process."""
    key = (_raw_device() if _raw_device is not None else torch.cuda.current_device(), _stream().value)
    ws = _tile_ws.get(key)
    if ws is None:
        ws = _tile_ws[key] = torch.empty(TILE_WS_BYTES, dtype=torch.uint8, device=f"cuda:{key[0]}")
    return ws.data_ptr(), ws.numel()


def conv_fwd_tile(desc: ConvDesc, x: Tensor, wfrag: Tensor, y: Tensor, *, bias: Optional[Tensor] = None,
                  chan_scale: Optional[Tensor] = None, res: Optional[Tensor] = None, res_off: int = 0,
                  alpha: float = 1.0, beta: float = 0.0, act=False, slope: float = 0.2,
                  out_planar: bool = False, act_c1: int = 0, res2: Optional[Tensor] = None, res2_off: int = 0,
                  beta2: float = 0.0, use_ws: bool = True, mask=None, in2: Optional[Tensor] = None,
                  in2_c0: int = 0) -> bool:
    """LDS halo-tile forward conv (bf16, stride 1).  Returns False when the shape is outside
    the tile kernels (the caller then uses :func:`conv_fwd`).  ``act`` = 2 / ``act_c1``: the two stages of a
    split dense-block conv (see ``wsr_epilogue_t``)."""
    _need_cuda(x, wfrag, y, bias, chan_scale, res)
    ep = Epilogue()
    ep.bias, ep.chan_scale, ep.res = _p(bias), _p(chan_scale), _p(res)
    ep.res_ctot = res.shape[-1] if res is not None else 0
    ep.res_off = res_off
    ep.alpha, ep.beta = alpha, beta
    ep.act, ep.slope = int(act), slope
    ep.out_planar = int(out_planar)
    ep.act_c1 = act_c1
    if res2 is not None:
        _need_cuda(res2)
        ep.res2, ep.res2_ctot, ep.res2_off, ep.beta2 = _p(res2), res2.shape[-1], res2_off, beta2
    if use_ws:
        ep.ws, ep.ws_bytes = tile_workspace()
    if in2 is not None:  # reduction channels >= in2_c0 come from this second tensor (wsr_epilogue_t.in2: the concat as two)
        _need_cuda(in2)
        if in2.shape[:-1] != x.shape[:-1] or in2.dtype != x.dtype:
            raise ValueError("in2 must have x's extents and dtype")
        ep.in2, ep.in2_ctot, ep.in2_c0 = _p(in2), in2.shape[-1], in2_c0
    if mask is not None:  # (y, y_off, c0, c1, slope): LeakyReLU-backward mask on a forward-form launch (wsr_epilogue_t.mask)
        my, my_off, mc0, mc1, mslope = mask
        _need_cuda(my)
        mk = _lib.LreluMask()
        mk.y, mk.y_ctot, mk.y_off, mk.c0, mk.c1, mk.slope = my.data_ptr(), my.shape[-1], my_off, mc0, mc1, mslope
        ep.mask = C.addressof(mk)
    rc = _lib.lib().wsr_conv3d_fwd_tile(C.byref(desc), _p(x), _p(wfrag), _p(y), C.byref(ep), _stream())
    if rc == _lib.WSR_EUNSUPPORTED:
        return False
    check(rc, "conv3d_fwd_tile")
    return True


TILE_PLAN_FIELDS = ("TX", "TY", "TZ", "NTW", "ngroups", "ksplit", "xbufs", "TS")


def last_tile_plan() -> dict:
    """Diagnostic: the launch plan of this thread's most recent halo-tile launch (``wsr_last_tile_plan``) - spatial
    tile, workgroup width in 16-channel n-tiles, channel groups, reduction splits, activation buffers, K-steps per
    weight stage; all zero before the first one.  A declined call, or one served by another kernel, leaves it as it
    was.  For tests that assert which instantiation a case reached: nothing in the product path reads it."""
    buf = (C.c_int32 * len(TILE_PLAN_FIELDS))()
    check(_lib.lib().wsr_last_tile_plan(buf), "last_tile_plan")
    return dict(zip(TILE_PLAN_FIELDS, (int(v) for v in buf)))


TILE_INST_FIELDS = ("WM", "WN", "TM", "TN", "TPK", "MASK", "F32", "WK", "SIMPLE", "seq")


def last_tile_instantiation() -> dict:
    """Diagnostic: which ``launch_ct<WM, WN, TM, TN, TPK, MASK, T, WK, SIMPLE>`` made this thread's most recent halo-tile
    launch (``wsr_last_tile_instantiation``; ``F32`` = 1 for T = F32), and ``seq``, the number of such launches the thread
    has made.  ``seq`` stands still across a call that was declined or served by the streaming 1x1x1, sliding-window or
    generic kernels.  For tests only, like :func:`last_tile_plan`."""
    buf = (C.c_int32 * len(TILE_INST_FIELDS))()
    check(_lib.lib().wsr_last_tile_instantiation(buf), "last_tile_instantiation")
    return dict(zip(TILE_INST_FIELDS, (int(v) for v in buf)))


def conv1x1_covers(red: int, n_out: int, masked: bool) -> bool:
    """shapes the streaming 1x1x1 kernel is instantiated for (conv_1x1_v2.hip, ``wsr_conv1x1_bf16``): reduction
    channels x produced channels.  Only that kernel may run a 1x1x1 input gradient in place."""
    shapes = {(128, 256)} if masked else {(256, 128), (128, 256)}
    return (red, n_out) in shapes


def conv_dgrad_tile(desc: ConvDesc, dy: Tensor, wfrag_t: Tensor, dx: Tensor, *, alpha: float = 1.0,
                    accumulate: bool = False, dx_planar: bool = False, mask=None, acc_src: Optional[Tensor] = None,
                    use_ws: bool = True, acc_beta: float = 1.0, res2: Optional[Tensor] = None, res2_off: int = 0,
                    beta2: float = 1.0, dx2: Optional[Tensor] = None, dx2_c0: int = 0) -> bool:
    """``mask`` = (y, y_off, c0, c1, slope): fold ``leaky_relu_backward`` of produced channels [c0, c1) into
    the epilogue, the mask taken from channels [y_off, y_off + c1 - c0) of the saved output ``y``.
    ``acc_src``: with ``accumulate``, the tensor (same layout as ``dx``) whose values are added instead of dx's own."""
    _need_cuda(dy, wfrag_t, dx, acc_src)
    if acc_src is not None and acc_src.shape != dx.shape:
        raise ValueError("acc_src must have dx's layout")
    opts = _lib.DgradOpts()
    opts.acc_src = _p(acc_src)
    opts.acc_beta = acc_beta
    if res2 is not None:  # (streaming 1x1x1 kernel only: the RRDB-level gradient joining the running one)
        _need_cuda(res2)
        opts.res2, opts.res2_ctot, opts.res2_off, opts.beta2 = _p(res2), res2.shape[-1], res2_off, beta2
    if use_ws:
        opts.ws, opts.ws_bytes = tile_workspace()
    if dx2 is not None:  # produced channels >= dx2_c0 go to this second tensor (wsr_dgrad_opts_t.dx2)
        _need_cuda(dx2)
        if dx2.shape[:-1] != dx.shape[:-1] or dx2.dtype != dx.dtype:
            raise ValueError("dx2 must have dx's extents and dtype")
        opts.dx2, opts.dx2_ctot, opts.dx2_c0 = _p(dx2), dx2.shape[-1], dx2_c0
    mp = None
    if mask is not None:
        y, y_off, c0, c1, slope = mask[:5]
        cs = mask[5] if len(mask) > 5 else None
        _need_cuda(y, cs)
        m = _lib.LreluMask()
        m.y, m.y_ctot, m.y_off, m.c0, m.c1, m.slope = y.data_ptr(), y.shape[-1], y_off, c0, c1, slope
        m.chan_scale = _p(cs)
        mp = C.byref(m)
    rc = _lib.lib().wsr_conv3d_dgrad_tile(C.byref(desc), _p(dy), _p(wfrag_t), _p(dx), alpha, int(accumulate),
                                          int(dx_planar), mp, C.byref(opts), _stream())
    if rc == _lib.WSR_EUNSUPPORTED:
        return False
    check(rc, "conv3d_dgrad_tile")
    return True


def pack_filter_frag(w: Tensor, *, transpose: bool = False, out: Optional[Tensor] = None,
                     dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """fp32 master ``(Cout, Cin, KX, KY, KZ)`` -> MFMA-fragment order of ``dtype`` (bf16, or fp32 for the fp32 tile
    kernels) for the tile kernels."""
    _need_cuda(w)
    if not w.is_contiguous() or w.dtype != torch.float32 or w.dim() != 5:
        raise ValueError("pack_filter_frag wants a contiguous fp32 (Cout, Cin, KX, KY, KZ) tensor")
    cout, cin, kx, ky, kz = w.shape
    rows, red = (cin, cout) if transpose else (cout, cin)
    n = _lib.lib().wsr_frag_filter_elems(rows, red, kx * ky * kz, dtype_id(dtype))
    if out is None:
        out = torch.empty(n, dtype=dtype, device=w.device)
    check(_lib.lib().wsr_pack_filter_frag(_p(w), _p(out), cout, cin, kx, ky, kz, int(transpose), dtype_id(dtype),
                                          _stream()), "pack_filter_frag")
    return out


def frag_filter_elems(w: Tensor, transpose: bool, dtype: torch.dtype = torch.bfloat16) -> int:
    cout, cin, kx, ky, kz = w.shape
    rows, red = (cin, cout) if transpose else (cout, cin)
    return int(_lib.lib().wsr_frag_filter_elems(rows, red, kx * ky * kz, dtype_id(dtype)))


def frag_filter_elems_for(rows: int, red: int, taps: int, dtype: torch.dtype = torch.bfloat16) -> int:
    return int(_lib.lib().wsr_frag_filter_elems(rows, red, taps, dtype_id(dtype)))


def pack_job_table(jobs) -> Tensor:
    """Device table of ``wsr_pack_job_t`` records for ``jobs`` = [(master fp32 weight, out bf16 tensor, transpose)]
    or, for one source of a stacked dense-block filter, [(weight, out, transpose, c_lo, c_n, red_off, red_total,
    row_off, rows_total)].  The table only holds pointers and shapes, so it stays valid while those tensors keep
    their storage."""
    import numpy as np

    rec = np.zeros((len(jobs), 8), dtype=np.int64)  # 2 pointers + 12 int32
    for r, job in zip(rec, jobs):
        w, out, tr = job[:3]
        cout, cin, kx, ky, kz = w.shape
        r[0], r[1] = w.data_ptr(), out.data_ptr()
        r[2] = cout | (cin << 32)
        r[3] = kx | (ky << 32)
        r[4] = kz | (int(tr) << 32)
        if len(job) > 3:
            c_lo, c_n, red_off, red_total, row_off, rows_total = job[3:]
            bad = cout % 16 or red_total % 16 or c_lo < 0 or c_lo + c_n > cin
            if tr:
                bad = bad or red_off % 16 or red_off + cout > red_total or rows_total != c_n
            else:
                bad = bad or red_off or red_total != c_n or row_off % 16 or row_off + cout > rows_total
            if bad:
                raise ValueError("bad stacked filter part")
            r[5] = c_lo | (c_n << 32)
            r[6] = red_off | (red_total << 32)
            r[7] = row_off | (rows_total << 32)
    return _table_to_device(rec, jobs[0][0].device)


def _table_to_device(rec, dev) -> Tensor:
    """small host table -> device through pinned memory: a pageable copy would block the host until the stream has
    drained (one pipeline bubble per rebuilt table)"""
    t = torch.from_numpy(rec)
    return t.pin_memory().to(dev, non_blocking=True) if torch.device(dev).type == "cuda" else t.to(dev)


def pack_filter_frag_multi(table: Tensor, dtype: torch.dtype = torch.bfloat16) -> None:
    """One launch for all filters of a job table (see :func:`pack_job_table`); ``dtype`` of the fragment filters."""
    check(_lib.lib().wsr_pack_filter_frag_multi(_p(table), table.shape[0], dtype_id(dtype), _stream()),
          "pack_filter_frag_multi")


def conv_dgrad(desc: ConvDesc, dy: Tensor, wt: Tensor, dx: Tensor, *, alpha: float = 1.0,
               accumulate: bool = False, dx_planar: bool = False) -> Tensor:
    _need_cuda(dy, wt, dx)
    check(_lib.lib().wsr_conv3d_dgrad(C.byref(desc), _p(dy), _p(wt), _p(dx), alpha, int(accumulate),
                                      int(dx_planar), _stream()), "conv3d_dgrad")
    return dx


def conv_wgrad(desc: ConvDesc, x: Tensor, dy: Tensor, dw: Tensor) -> Tensor:
    """``dw`` (fp32 ``[Cout][taps][Cin]``) is accumulated into."""
    _need_cuda(x, dy, dw)
    if dw.dtype != torch.float32:
        raise TypeError("filter gradients are fp32")
    check(_lib.lib().wsr_conv3d_wgrad(C.byref(desc), _p(x), _p(dy), _p(dw), _stream()), "conv3d_wgrad")
    return dw


def conv_wgrad_tri(desc: ConvDesc, x: Tensor, dy: Tensor, dw: Tensor, tri_base: int, tri_step: int) -> Tensor:
    """Stacked filter gradient of a dense block's growth convs (see ``wsr_conv3d_wgrad_tri``)."""
    _need_cuda(x, dy, dw)
    if dw.dtype != torch.float32:
        raise TypeError("filter gradients are fp32")
    check(_lib.lib().wsr_conv3d_wgrad_tri(C.byref(desc), _p(x), _p(dy), _p(dw), tri_base, tri_step, _stream()),
          "conv3d_wgrad_tri")
    return dw


def conv_wgrad_nparts(desc: ConvDesc, tri_base: int = 0, tri_step: int = 0) -> int:
    """split copies the deterministic filter-gradient launch of this geometry writes (host-side query)"""
    n = C.c_int32(0)
    check(_lib.lib().wsr_conv3d_wgrad_nparts(C.byref(desc), tri_base, tri_step, C.byref(n)), "conv3d_wgrad_nparts")
    return int(n.value)


def conv_split_ok(desc: ConvDesc, c0: int) -> bool:
    """True when the forward, input-gradient and filter-gradient kernels all take this conv with its input channels
    split at ``c0`` over two tensors (``wsr_conv_split_ok``: host-side query)"""
    return bool(_lib.lib().wsr_conv_split_ok(C.byref(desc), c0))


def conv_wgrad_parts(desc: ConvDesc, x: Tensor, dy: Tensor, parts: Tensor, n_parts: int, tri_base: int = 0,
                     tri_step: int = 0, x2: Optional[Tensor] = None, x2_c0: int = 0) -> Tensor:
    """Deterministic filter gradient: ``parts`` (n_parts, Cout, taps, Cin) fp32 receives one partial sum per split
    (plain stores, nothing to zero); :func:`unpack_wgrad_reduce_multi` adds them in order.  ``x2``: the conv's input
    channels >= ``x2_c0`` live in this second tensor (``wsr_conv3d_wgrad_parts_x2``)."""
    _need_cuda(x, dy, parts)
    if parts.dtype != torch.float32 or not parts.is_contiguous() or parts.shape[0] != n_parts:
        raise ValueError("conv_wgrad_parts wants a contiguous fp32 (n_parts, Cout, taps, Cin) buffer")
    if x2 is not None:
        _need_cuda(x2)
        if tri_step or x2.shape[:-1] != x.shape[:-1] or x2.dtype != x.dtype:
            raise ValueError("x2 must have x's extents and dtype (no stacked form)")
        check(_lib.lib().wsr_conv3d_wgrad_parts_x2(C.byref(desc), _p(x), _p(x2), x2.shape[-1], x2_c0, _p(dy), _p(parts),
                                                   parts[0].numel(), n_parts, _stream()), "conv3d_wgrad_parts_x2")
        return parts
    check(_lib.lib().wsr_conv3d_wgrad_parts(C.byref(desc), _p(x), _p(dy), _p(parts), parts[0].numel(), n_parts, tri_base,
                                            tri_step, _stream()), "conv3d_wgrad_parts")
    return parts


def conv_wgrad_nparts_bias(desc: ConvDesc) -> int:
    """split copies of the 1x1x1 filter-gradient launch that also takes the bias gradient's partial sums
    (``wsr_conv3d_wgrad_parts_bias``); 0 when the conv is not that kernel's shape (host-side query)"""
    n = C.c_int32(0)
    rc = _lib.lib().wsr_conv3d_wgrad_nparts_bias(C.byref(desc), C.byref(n))
    if rc == _lib.WSR_EUNSUPPORTED:
        return 0
    check(rc, "conv3d_wgrad_nparts_bias")
    return int(n.value)


def conv_wgrad_parts_bias(desc: ConvDesc, x: Tensor, dy: Tensor, parts: Tensor, n_parts: int, bias_parts: Tensor) -> Tensor:
    """:func:`conv_wgrad_parts` of a 1x1x1 conv; split s also stores the channel sums of its share of ``dy`` to row s
    of ``bias_parts`` (n_parts, Cout) fp32 (added later by a ``wsr_unpack_wgrad_reduce_multi`` job of n_parts rows)"""
    _need_cuda(x, dy, parts, bias_parts)
    if parts.dtype != torch.float32 or not parts.is_contiguous() or parts.shape[0] != n_parts:
        raise ValueError("conv_wgrad_parts_bias wants a contiguous fp32 (n_parts, Cout, taps, Cin) buffer")
    if (bias_parts.dtype != torch.float32 or not bias_parts.is_contiguous()
            or tuple(bias_parts.shape) != (n_parts, desc.Cout)):
        raise ValueError("conv_wgrad_parts_bias wants a contiguous fp32 (n_parts, Cout) bias buffer")
    check(_lib.lib().wsr_conv3d_wgrad_parts_bias(C.byref(desc), _p(x), _p(dy), _p(parts), parts[0].numel(), n_parts,
                                                 _p(bias_parts), _stream()), "conv3d_wgrad_parts_bias")
    return parts


def conv_wgrad_nparts_lat4(desc: ConvDesc) -> int:
    """splits PER CLASS of the merged four-class launch of a lattice-form filter gradient (``desc``: class (0, 0),
    see ``wsr_conv3d_wgrad_parts_lat4``); 0 when the merged form declines the shape (host-side query)"""
    n = C.c_int32(0)
    rc = _lib.lib().wsr_conv3d_wgrad_nparts_lat4(C.byref(desc), C.byref(n))
    if rc == _lib.WSR_EUNSUPPORTED:
        return 0
    check(rc, "conv3d_wgrad_nparts_lat4")
    return int(n.value)


def conv_wgrad_parts_lat4(desc: ConvDesc, x: Tensor, dy: Tensor, parts: Tensor, n_parts: int) -> Tensor:
    """The four xy-parity classes of one lattice-form filter gradient in one launch: ``parts`` (4, n_parts, Cout,
    taps, Cin) fp32, class (a, b) at index 2a + b, one partial sum per split of each class (plain stores)."""
    _need_cuda(x, dy, parts)
    if parts.dtype != torch.float32 or not parts.is_contiguous() or parts.dim() != 5 or parts.shape[:2] != (4, n_parts):
        raise ValueError("conv_wgrad_parts_lat4 wants a contiguous fp32 (4, n_parts, Cout, taps, Cin) buffer")
    check(_lib.lib().wsr_conv3d_wgrad_parts_lat4(C.byref(desc), _p(x), _p(dy), _p(parts), parts[0, 0].numel(),
                                                 parts[0].numel(), n_parts, _stream()), "conv3d_wgrad_parts_lat4")
    return parts


def pack_filter(w: Tensor, dt: torch.dtype, *, transpose: bool = False, kpad: Optional[int] = None,
                out: Optional[Tensor] = None) -> Tensor:
    """fp32 master ``(Cout, Cin, KX, KY, KZ)`` -> compute copy ``[rows][taps][kpad]`` of ``dt``."""
    _need_cuda(w)
    cout, cin = w.shape[:2]
    taps = w[0, 0].numel()
    if not w.is_contiguous() or w.dtype != torch.float32:
        raise ValueError("pack_filter wants a contiguous fp32 (Cout, Cin, KX, KY, KZ) tensor")
    k = cout if transpose else cin
    kpad = pad_channels(k, dt) if kpad is None else kpad
    rows = cin if transpose else cout
    if out is None:
        out = torch.empty((rows, taps, kpad), dtype=dt, device=w.device)
    check(_lib.lib().wsr_pack_filter(_p(w), _p(out), dtype_id(dt), cout, taps, cin, int(transpose), kpad, _stream()),
          "pack_filter")
    return out


def unpack_wgrad(src: Tensor, dst: Tensor, scale: float = 1.0, accumulate: bool = True) -> None:
    """master-layout grad ``(Cout, Cin, KX, KY, KZ)`` (+)= scale * packed ``[Cout][taps][kpad]``."""
    cout, taps, kpad = src.shape
    if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.shape[0] != cout:
        raise ValueError("unpack_wgrad wants a contiguous fp32 master-layout gradient")
    check(_lib.lib().wsr_unpack_wgrad(_p(src), _p(dst), cout, taps, dst.shape[1], kpad, scale, int(accumulate),
                                      _stream()), "unpack_wgrad")


def unpack_job_table(jobs) -> Tensor:
    """Device table of ``wsr_unpack_job_t`` records for ``jobs`` = [(packed src [Cout][taps][kpad] fp32,
    master-layout dst fp32, scale[, n_parts, part_stride])] - the last two for the deterministic split copies."""
    import numpy as np

    rec = np.zeros((len(jobs), 7), dtype=np.int64)  # 2 pointers + 4 int32 + float + int32 + 2 int32 + int64
    for r, job in zip(rec, jobs):
        src, dst, scale = job[:3]
        n_parts, part_stride = job[3:5] if len(job) > 3 else (0, 0)
        cout, taps, kpad = src.shape
        r[0], r[1] = src.data_ptr(), dst.data_ptr()
        r[2] = cout | (taps << 32)
        r[3] = dst.shape[1] | (kpad << 32)
        r[4] = int(np.float32(scale).view(np.int32)) & 0xFFFFFFFF  # accumulate = 0
        r[5] = n_parts
        r[6] = part_stride
    return _table_to_device(rec, jobs[0][0].device)


def unpack_wgrad_multi(table: Tensor) -> None:
    check(_lib.lib().wsr_unpack_wgrad_multi(_p(table), table.shape[0], _stream()), "unpack_wgrad_multi")


def unpack_wgrad_reduce_multi(table: Tensor) -> None:
    """jobs with split copies (``(src, dst, scale, n_parts, part_stride)`` records): ordered sum + unpack"""
    check(_lib.lib().wsr_unpack_wgrad_reduce_multi(_p(table), table.shape[0], _stream()), "unpack_wgrad_reduce_multi")


def lrelu_bwd_(g: Tensor, g_off: int, y: Tensor, y_off: int, C_: int, slope: float,
               chan_scale: Optional[Tensor] = None) -> None:
    nvox = g.numel() // g.shape[-1]
    check(_lib.lib().wsr_lrelu_bwd_inplace(_p(g), g.shape[-1], g_off, _p(y), y.shape[-1], y_off, C_, nvox, slope,
                                           _p(chan_scale), nvox // g.shape[0], dtype_id(g.dtype), _stream()),
          "lrelu_bwd")


def chan_axpby(dst: Tensor, d_off: int, src: Tensor, s_off: int, C_: int, alpha: float = 1.0,
               beta: float = 0.0) -> None:
    nvox = dst.numel() // dst.shape[-1]
    check(_lib.lib().wsr_chan_axpby(_p(dst), dst.shape[-1], d_off, _p(src), src.shape[-1], s_off, C_, nvox, alpha,
                                    beta, dtype_id(dst.dtype), _stream()), "chan_axpby")


CHAN_SUM_ROWS = 512  # WSR_CHAN_SUM_ROWS
_chan_sum_ws: dict = {}  # per-device scratch of the two-pass channel sum (stream-ordered re-use)


def chan_sum(x: Tensor, x_off: int, C_: int, out: Tensor, scale: float = 1.0) -> bool:
    """``out[c] = scale * sum_voxels x[..., x_off + c]`` (fp32, overwritten); False when the kernel does not
    cover the shape (channel counts that are not multiples of 4)."""
    _need_cuda(x, out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != C_:
        raise ValueError("chan_sum wants a contiguous fp32 output of C elements")
    nvox = x.numel() // x.shape[-1]
    ws = _chan_sum_ws.get(x.device)
    if ws is None or ws.numel() < CHAN_SUM_ROWS * C_:
        ws = _chan_sum_ws[x.device] = torch.empty(CHAN_SUM_ROWS * max(C_, 256), dtype=torch.float32, device=x.device)
    rc = _lib.lib().wsr_chan_sum(_p(x), x.shape[-1], x_off, C_, nvox, scale, _p(out), _p(ws), dtype_id(x.dtype),
                                 _stream())
    if rc == _lib.WSR_EUNSUPPORTED:
        return False
    check(rc, "chan_sum")
    return True


def chan_sum_rows(C_: int, nvox: int) -> int:
    """partial rows the first pass of :func:`chan_sum` writes for this shape (0: shape not covered)"""
    return int(_lib.lib().wsr_chan_sum_rows(C_, nvox))


def chan_sum_partials(x: Tensor, x_off: int, C_: int, partials: Tensor) -> None:
    """first pass of :func:`chan_sum` only: ``partials`` (rows, C) fp32 gets one row of sums per workgroup; the rows
    are added later (``wsr_unpack_wgrad_reduce_multi`` job with n_parts = rows)"""
    _need_cuda(x, partials)
    nvox = x.numel() // x.shape[-1]
    if partials.dtype != torch.float32 or not partials.is_contiguous() or \
            tuple(partials.shape) != (chan_sum_rows(C_, nvox), C_):
        raise ValueError("chan_sum_partials wants a contiguous fp32 (rows, C) buffer")
    check(_lib.lib().wsr_chan_sum_partials(_p(x), x.shape[-1], x_off, C_, nvox, _p(partials), dtype_id(x.dtype),
                                           _stream()), "chan_sum_partials")


#: first classifier layer of the discriminator through the streaming row kernel (WSR_LINEAR_ROWS=0: library GEMM)
LINEAR_ROWS = __import__("os").environ.get("WSR_LINEAR_ROWS", "1") != "0"


class _LinearRows(torch.autograd.Function):
    """``F.linear(x, w, b)`` for a few rows x and a very long reduction (``wsr_linear_rows``); backward = the
    matrix products autograd would issue."""

    @staticmethod
    def forward(ctx, x, w, b):
        y = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        check(_lib.lib().wsr_linear_rows(_p(x), _p(w), _p(b), _p(y), x.shape[0], w.shape[0], x.shape[1], _stream()),
              "linear_rows")
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = g @ w if ctx.needs_input_grad[0] else None
        gw = g.t() @ x if ctx.needs_input_grad[1] else None
        gb = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb


def linear_rows(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Optional[Tensor]:
    """``x @ w.T + b`` through ``wsr_linear_rows`` when the shape is the one it is built for (fp32, <= 8 rows, long
    contiguous reduction), else None (the caller uses ``F.linear``)."""
    if not (LINEAR_ROWS and x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() == 2 and x.shape[0] <= 8
            and x.shape[1] % 4 == 0 and x.shape[1] >= 8192 and x.is_contiguous() and w.is_contiguous()
            and (b is None or (b.dtype == torch.float32 and b.is_contiguous()))):
        return None
    _need_cuda(x, w, b)
    return _LinearRows.apply(x, w, b)


def plane_sum(src: Tensor, out: Tensor) -> Tensor:
    """``out[c] = sum_{b, voxels} src[b, c]`` for a planar fp32 (B, C, ...) tensor (fp32, overwritten)"""
    _need_cuda(src, out)
    if src.dtype != torch.float32 or not src.is_contiguous() or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("plane_sum wants contiguous fp32 tensors")
    B, C_ = src.shape[:2]
    if out.numel() != C_:
        raise ValueError("plane_sum: one output element per channel")
    ws = _chan_sum_ws.get(src.device)
    if ws is None or ws.numel() < CHAN_SUM_ROWS * C_:
        ws = _chan_sum_ws[src.device] = torch.empty(CHAN_SUM_ROWS * max(C_, 256), dtype=torch.float32, device=src.device)
    check(_lib.lib().wsr_plane_sum(_p(src), B, C_, src[0, 0].numel(), _p(out), _p(ws), _stream()), "plane_sum")
    return out


def upsample2_bwd(dy: Tensor, dx: Tensor) -> Tensor:
    B, X, Y, Z, C_ = dx.shape
    check(_lib.lib().wsr_upsample2_bwd(_p(dy), _p(dx), B, X, Y, Z, C_, dtype_id(dx.dtype), _stream()),
          "upsample2_bwd")
    return dx


def strided_parity_filters(w: Tensor, out: Tensor, sz: int, zc: int) -> Tensor:
    """parity filters (4, Cin, Cout, 2, 2, KZp) of the input gradient of a stride-(2, 2, sz) 4x4x3 conv
    (``wsr_strided_parity_filters``): forward-conv filters over dy, rows = the conv's input channels"""
    _need_cuda(w, out)
    cout, cin = w.shape[:2]
    kzp = 3 if sz == 1 else (1 if zc == 0 else 2)
    if tuple(w.shape[2:]) != (4, 4, 3) or tuple(out.shape) != (4, cin, cout, 2, 2, kzp) or \
            not (w.is_contiguous() and out.is_contiguous()) or w.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError("strided_parity_filters: fp32 (Cout, Cin, 4, 4, 3) -> (4, Cin, Cout, 2, 2, KZp)")
    check(_lib.lib().wsr_strided_parity_filters(_p(w), _p(out), cout, cin, sz, zc, _stream()), "strided_parity_filters")
    return out


def strided_parity_unfold(dwp: Tensor, dw: Tensor, sz: int, zc: int) -> Tensor:
    """class gradients (4, Cout, Cin, 2, 2, KZp) of the parity form of a stride-(2, 2, sz) 4x4x3 conv's filter gradient
    -> their taps of the master gradient (Cout, Cin, 4, 4, 3) (``wsr_strided_parity_unfold``)"""
    _need_cuda(dwp, dw)
    cout, cin = dw.shape[:2]
    kzp = 3 if sz == 1 else (1 if zc == 0 else 2)
    if tuple(dw.shape[2:]) != (4, 4, 3) or tuple(dwp.shape) != (4, cout, cin, 2, 2, kzp) or \
            not (dw.is_contiguous() and dwp.is_contiguous()) or dw.dtype != torch.float32 or dwp.dtype != torch.float32:
        raise ValueError("strided_parity_unfold: fp32 (4, Cout, Cin, 2, 2, KZp) -> (Cout, Cin, 4, 4, 3)")
    check(_lib.lib().wsr_strided_parity_unfold(_p(dwp), _p(dw), cout * cin, sz, zc, _stream()), "strided_parity_unfold")
    return dw


def subpixel_fold(w: Tensor, wp: Tensor) -> Tensor:
    """master fp32 (Cout, Cin, 3, 3, KZ) -> the four parity filters (4, Cout, Cin, 2, 2, KZ) of the sub-pixel form of
    nearest x(2,2,1) + conv (``wsr_subpixel_fold``)."""
    _need_cuda(w, wp)
    cout, cin, kx, ky, kz = w.shape
    if (kx, ky) != (3, 3) or tuple(wp.shape) != (4, cout, cin, 2, 2, kz) or not (w.is_contiguous() and wp.is_contiguous()) \
            or w.dtype != torch.float32 or wp.dtype != torch.float32:
        raise ValueError("subpixel_fold: fp32 (Cout, Cin, 3, 3, KZ) -> (4, Cout, Cin, 2, 2, KZ)")
    check(_lib.lib().wsr_subpixel_fold(_p(w), _p(wp), cout * cin, kz, _stream()), "subpixel_fold")
    return wp


def subpixel_unfold(dwp: Tensor, dw: Tensor) -> Tensor:
    """adjoint of :func:`subpixel_fold`: parity filter gradients (4, Cout, Cin, 2, 2, KZ) -> (Cout, Cin, 3, 3, KZ)"""
    _need_cuda(dwp, dw)
    cout, cin, kx, ky, kz = dw.shape
    if (kx, ky) != (3, 3) or tuple(dwp.shape) != (4, cout, cin, 2, 2, kz) or not (dw.is_contiguous() and dwp.is_contiguous()) \
            or dw.dtype != torch.float32 or dwp.dtype != torch.float32:
        raise ValueError("subpixel_unfold: fp32 (4, Cout, Cin, 2, 2, KZ) -> (Cout, Cin, 3, 3, KZ)")
    check(_lib.lib().wsr_subpixel_unfold(_p(dwp), _p(dw), cout * cin, kz, _stream()), "subpixel_unfold")
    return dw


class _WindGradient(torch.autograd.Function):
    """(B, 3, X, Y, Z) -> (B, 9, X, Y, Z) derivatives of the wind field (``wsr_wind_gradient``) with the adjoint
    as backward - one launch each instead of torch.gradient + slicing arithmetic and their autograd graph."""

    @staticmethod
    def forward(ctx, f: Tensor, xs: Tensor, ys: Tensor, zc: Tensor) -> Tensor:
        B, _, X, Y, Z = f.shape
        out = torch.empty((B, 9, X, Y, Z), dtype=torch.float32, device=f.device)
        check(_lib.lib().wsr_wind_gradient(_p(f), _p(xs), _p(ys), _p(zc), _p(out), B, X, Y, Z, _stream()),
              "wind_gradient")
        ctx.save_for_backward(xs, ys, zc)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        xs, ys, zc = ctx.saved_tensors
        g = g.contiguous().float()
        B, _, X, Y, Z = g.shape
        df = torch.empty((B, 3, X, Y, Z), dtype=torch.float32, device=g.device)
        check(_lib.lib().wsr_wind_gradient_bwd(_p(g), _p(xs), _p(ys), _p(zc), _p(df), B, X, Y, Z, _stream()),
              "wind_gradient_bwd")
        return df, None, None, None


def wind_gradient(f: Tensor, xs: Tensor, ys: Tensor, zc: Tensor) -> Tensor:
    """``calculate_gradient_of_wind_field`` of the reference (process_data.py:301-313) on the device"""
    _need_cuda(f, xs, ys, zc)
    B, C_, X, Y, Z = f.shape
    if C_ != 3 or xs.numel() != X or ys.numel() != Y or zc.numel() != B * X * Y * Z:
        raise ValueError("wind_gradient wants f (B,3,X,Y,Z), x (X), y (Y), Z (B,1,X,Y,Z)")
    return _WindGradient.apply(f.contiguous().float(), xs.contiguous().float(), ys.contiguous().float(),
                               zc.contiguous().float())


_physics_ws: dict = {}  # per-device partial table of the statistics pass (stream-ordered re-use)


class _PhysicsLossStats(torch.autograd.Function):
    """``wsr_physics_loss_stats`` with ``wsr_physics_loss_bwd`` as backward: (sums[6], maxima[8]) of the content
    losses in one pass over HR, SR, Z; only the sums carry gradient, and only towards SR."""

    @staticmethod
    def forward(ctx, hr: Tensor, sr: Tensor, xs: Tensor, ys: Tensor, zc: Tensor):
        B, _, X, Y, Z = sr.shape
        dev = sr.device
        ws = _physics_ws.get(dev)
        if ws is None:
            ws = _physics_ws[dev] = torch.empty(int(_lib.lib().wsr_physics_loss_workspace_floats()),
                                                dtype=torch.float32, device=dev)
        stats = torch.empty(14, dtype=torch.float32, device=dev)
        check(_lib.lib().wsr_physics_loss_stats(_p(hr), _p(sr), _p(xs), _p(ys), _p(zc), _p(stats), _p(ws), B, X, Y, Z,
                                                _stream()), "physics_loss_stats")
        ctx.save_for_backward(hr, sr, xs, ys, zc)
        sums, maxima = stats[:6], stats[6:]
        ctx.mark_non_differentiable(maxima)
        return sums, maxima

    @staticmethod
    def backward(ctx, g_sums: Tensor, _g_max):
        hr, sr, xs, ys, zc = ctx.saved_tensors
        B, _, X, Y, Z = sr.shape
        coef = g_sums.contiguous().float()
        resid = torch.empty((B, 9, X, Y, Z), dtype=torch.float32, device=sr.device)
        dsr = torch.empty_like(sr)
        check(_lib.lib().wsr_physics_loss_bwd(_p(hr), _p(sr), _p(xs), _p(ys), _p(zc), _p(coef), _p(resid), _p(dsr), B, X,
                                              Y, Z, _stream()), "physics_loss_bwd")
        return None, dsr, None, None, None


def physics_loss_stats(hr: Tensor, sr: Tensor, xs: Tensor, ys: Tensor, zc: Tensor):
    """-> (sums[6], maxima[8]), see ``wsr_physics_loss_stats`` in windsr_hip.h.  hr, sr (B,3,X,Y,Z), zc (B,1,X,Y,Z)."""
    _need_cuda(hr, sr, xs, ys, zc)
    B, C_, X, Y, Z = sr.shape
    if C_ != 3 or hr.shape != sr.shape or xs.numel() != X or ys.numel() != Y or zc.numel() != B * X * Y * Z:
        raise ValueError("physics_loss_stats wants hr, sr (B,3,X,Y,Z), x (X), y (Y), Z (B,1,X,Y,Z)")
    f = lambda t: t.contiguous().float()  # noqa: E731
    return _PhysicsLossStats.apply(f(hr), f(sr), f(xs), f(ys), f(zc))


class _RaganLoss(torch.autograd.Function):
    """( BCEWithLogits(u - mean v, lu) + BCEWithLogits(v - mean u, lv) ) / 2 with every partial derivative from ONE launch
    (``wsr_ragan_loss``); the backward is one multiply of the saved derivative vector by the upstream scalar."""

    @staticmethod
    def forward(ctx, u: Tensor, v: Tensor, lu: Tensor, lv: Tensor, mu: Optional[Tensor], mv: Optional[Tensor]):
        B = u.numel()
        flat = [t.detach().reshape(-1).float().contiguous() for t in (u, v, lu, lv)]
        if any(t.numel() != B for t in flat):
            raise ValueError("ragan_loss: logits and labels must have one element per sample")
        sc = [None if m is None else m.detach().reshape(1).float().contiguous() for m in (mu, mv)]
        _need_cuda(*flat, *sc)
        out = torch.empty(2 * B + 3, dtype=torch.float32, device=u.device)
        check(_lib.lib().wsr_ragan_loss(_p(flat[0]), _p(flat[1]), _p(flat[2]), _p(flat[3]), _p(sc[0]), _p(sc[1]), B, _p(out),
                                        _stream()), "ragan_loss")
        ctx.save_for_backward(out)
        ctx.meta = (B, u.shape, v.shape, u.dtype, v.dtype, None if mu is None else (mu.shape, mu.dtype),
                    None if mv is None else (mv.shape, mv.dtype))
        return out[0].clone()

    @staticmethod
    def backward(ctx, g: Tensor):
        (out,) = ctx.saved_tensors
        B, us, vs, ud, vd, mum, mvm = ctx.meta
        d = out[1:] * g
        du = d[:B].reshape(us).to(ud) if ctx.needs_input_grad[0] else None
        dv = d[B:2 * B].reshape(vs).to(vd) if ctx.needs_input_grad[1] else None
        dmu = d[2 * B].reshape(mum[0]).to(mum[1]) if mum is not None and ctx.needs_input_grad[4] else None
        dmv = d[2 * B + 1].reshape(mvm[0]).to(mvm[1]) if mvm is not None and ctx.needs_input_grad[5] else None
        return du, dv, None, None, dmu, dmv


def ragan_loss(u: Tensor, v: Tensor, lu: Tensor, lv: Tensor, mean_u: Optional[Tensor] = None,
               mean_v: Optional[Tensor] = None) -> Tensor:
    """Relativistic average GAN loss of the reference (wind_field_GAN_3D.py:360-364 with u = D(fake), v = D(real);
    :552-556 with u = D(real), v = D(fake)); ``mean_u`` / ``mean_v``: batch-global means from the caller's collective
    (both or neither), else the means over these samples."""
    if (mean_u is None) != (mean_v is None):
        raise ValueError("ragan_loss takes both means or neither")
    return _RaganLoss.apply(u, v, lu, lv, mean_u, mean_v)


def zfold(t: Tensor, y: Tensor, bias: Optional[Tensor], kz: int, pz: int) -> Tensor:
    """``y[b,c,x,y,z] = bias[c] + sum_k t[b, c*kz+k, x, y, z+k-pz]`` - planar fp32 (see ``wsr_zfold``)."""
    _need_cuda(t, y)
    B, C_ = y.shape[:2]
    if t.dtype != torch.float32 or y.dtype != torch.float32 or not (t.is_contiguous() and y.is_contiguous()) \
            or t.shape[1] != C_ * kz or t.shape[2:] != y.shape[2:]:
        raise ValueError("zfold wants contiguous fp32 (B, C*kz, X, Y, Z) -> (B, C, X, Y, Z)")
    Z = y.shape[-1]
    planes = y[0, 0].numel() // Z
    check(_lib.lib().wsr_zfold(_p(t), _p(y), _p(bias) if bias is not None else None, B, C_, kz, pz, planes, Z,
                               _stream()), "zfold")
    return y


def zunfold(g: Tensor, d: Tensor, kz: int, pz: int, d_off: int = 0, c_fill: Optional[int] = None) -> Tensor:
    """adjoint of :func:`zfold` into an NDHWC window: ``d[b,x,y,z, c*kz+k] = g[b,c,x,y, z-k+pz]``"""
    _need_cuda(g, d)
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("planar tensors are contiguous fp32 (B, C, X, Y, Z)")
    B, C_ = g.shape[:2]
    Z = g.shape[-1]
    planes = g[0, 0].numel() // Z
    c_fill = C_ * kz if c_fill is None else c_fill
    check(_lib.lib().wsr_zunfold(_p(g), _p(d), B, C_, kz, pz, planes, Z, d.shape[-1], d_off, c_fill,
                                 dtype_id(d.dtype), _stream()), "zunfold")
    return d


def planar_to_ndhwc(src: Tensor, dst: Tensor, d_off: int = 0, c_fill: Optional[int] = None) -> Tensor:
    """fp32 (B, C, X, Y, Z) contiguous -> channel window of an NDHWC tensor."""
    _need_cuda(src, dst)
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("planar tensors are contiguous fp32 (B, C, X, Y, Z)")
    B, C_ = src.shape[:2]
    vpb = src[0, 0].numel()
    c_fill = C_ if c_fill is None else c_fill
    check(_lib.lib().wsr_planar_to_ndhwc(_p(src), _p(dst), B, C_, vpb, dst.shape[-1], d_off, c_fill,
                                         dtype_id(dst.dtype), _stream()), "planar_to_ndhwc")
    return dst


def ndhwc_to_planar(src: Tensor, C_: int, s_off: int = 0) -> Tensor:
    B, X, Y, Z, ctot = src.shape
    dst = torch.empty((B, C_, X, Y, Z), dtype=torch.float32, device=src.device)
    check(_lib.lib().wsr_ndhwc_to_planar(_p(src), _p(dst), B, C_, X * Y * Z, ctot, s_off, dtype_id(src.dtype),
                                         _stream()), "ndhwc_to_planar")
    return dst


def _reduce_ws(dev, C_: int) -> Optional[Tensor]:
    """scratch of the atomic-free reductions (None: the scalar kernels, which accumulate, take over)"""
    if C_ % 4 or C_ > 512:
        return None
    ws = _chan_sum_ws.get(dev)
    if ws is None or ws.numel() < CHAN_SUM_ROWS * 2 * C_:
        ws = _chan_sum_ws[dev] = torch.empty(CHAN_SUM_ROWS * max(2 * C_, 256), dtype=torch.float32, device=dev)
    return ws


def bn_stats(x: Tensor, sums: Tensor, shift: Optional[Tensor] = None) -> None:
    """sums[2C] = {sum (x - shift), sum (x - shift)^2} per channel"""
    C_ = x.shape[-1]
    ws = _reduce_ws(x.device, C_)
    if ws is None:
        sums.zero_()
    check(_lib.lib().wsr_bn_stats(_p(x), C_, x.numel() // C_, _p(shift), _p(sums), _p(ws), dtype_id(x.dtype),
                                  _stream()), "bn_stats")


_bn_group_ws: dict = {}


def bn_train_stats(x: Tensor, groups: int, work: Tensor, eps: float, momentum: float, running_mean: Optional[Tensor],
                   running_var: Optional[Tensor]) -> bool:
    """Train-mode BatchNorm statistics of ``groups`` equal batch groups of ``x`` (NDHWC) in four launches
    (``wsr_bn_train_stats``): ``work[g] = (mean | invstd)`` of group g; the running statistics are updated once per group,
    in order.  False: shape outside the vectorised kernels (the caller runs the per-group ops)."""
    _need_cuda(x, work, running_mean, running_var)
    C_ = x.shape[-1]
    if C_ % 4 or C_ > 512 or x.shape[0] % groups or not x.is_contiguous() or groups > 64:
        return False
    if work.dtype != torch.float32 or tuple(work.shape) != (groups, 2 * C_) or not work.is_contiguous():
        raise ValueError("bn_train_stats wants a contiguous fp32 (groups, 2C) work buffer")
    nvox_g = x.numel() // C_ // groups
    key = (x.device, groups)
    ws = _bn_group_ws.get(key)
    if ws is None or ws.numel() < groups * CHAN_SUM_ROWS * 2 * C_:
        ws = _bn_group_ws[key] = torch.empty(groups * CHAN_SUM_ROWS * 2 * max(C_, 128), dtype=torch.float32, device=x.device)
    check(_lib.lib().wsr_bn_train_stats(_p(x), C_, nvox_g, groups, eps, momentum, _p(work), _p(running_mean), _p(running_var),
                                        _p(ws), dtype_id(x.dtype), _stream()), "bn_train_stats")
    return True


def bn_mean(sums: Tensor, mean: Tensor, count: float, count_dev: Optional[Tensor] = None) -> None:
    check(_lib.lib().wsr_bn_mean(_p(sums), _p(count_dev), float(count), _p(mean), mean.numel(), _stream()), "bn_mean")


def bn_shard_stats(work: Tensor, s2: Tensor, count: float, send: Tensor) -> None:
    """SyncBN: this rank's record ``send`` (G, 2C) = {local mean, local centred second moment} from ``work`` (G, >= C:
    the means) and ``s2`` (G, >= 2C: the shifted sums) - rows may be strided views."""
    G_, C_ = send.shape[0], send.shape[1] // 2
    if work.stride(-1) != 1 or s2.stride(-1) != 1 or not send.is_contiguous():
        raise ValueError("bn_shard_stats wants unit-stride rows")
    check(_lib.lib().wsr_bn_shard_stats(_p(work), work.stride(0), _p(s2), s2.stride(0), float(count), _p(send), G_, C_,
                                        _stream()), "bn_shard_stats")


def bn_combine_shards(gathered: Tensor, count: float, work: Tensor, s2: Tensor) -> None:
    """SyncBN: ``gathered`` (world, G, 2C) records of all ranks -> global mean in ``work[:, :C]``, {0, M2} in
    ``s2[:, :2C]`` (what :func:`bn_finalize` reads with ``count * world``)."""
    world, G_, C2 = gathered.shape
    if work.stride(-1) != 1 or s2.stride(-1) != 1 or not gathered.is_contiguous():
        raise ValueError("bn_combine_shards wants unit-stride rows")
    check(_lib.lib().wsr_bn_combine_shards(_p(gathered), world, float(count), _p(work), work.stride(0), _p(s2),
                                           s2.stride(0), G_, C2 // 2, _stream()), "bn_combine_shards")


def bn_finalize(sums2: Tensor, mean: Tensor, invstd: Tensor, count: float, eps: float, momentum: float,
                running_mean: Optional[Tensor], running_var: Optional[Tensor],
                count_dev: Optional[Tensor] = None) -> None:
    check(_lib.lib().wsr_bn_finalize(_p(sums2), _p(count_dev), float(count), _p(mean), eps, momentum, _p(invstd),
                                     C.c_void_p(0), _p(running_mean), _p(running_var), mean.numel(), _stream()),
          "bn_finalize")


def bn_apply_lrelu(x: Tensor, y: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, act: bool,
                   slope: float) -> None:
    C_ = x.shape[-1]
    check(_lib.lib().wsr_bn_apply_lrelu(_p(x), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), C_,
                                        x.numel() // C_, int(act), slope, dtype_id(x.dtype), _stream()), "bn_apply")


def bn_bwd_reduce(dy: Tensor, y: Tensor, x: Tensor, mean: Tensor, invstd: Tensor, act: bool, slope: float,
                  sums: Tensor) -> None:
    C_ = x.shape[-1]
    ws = _reduce_ws(x.device, C_)
    if ws is None:
        sums.zero_()
    check(_lib.lib().wsr_bn_bwd_reduce(_p(dy), _p(y), _p(x), _p(mean), _p(invstd), C_, x.numel() // C_, int(act),
                                       slope, _p(sums), _p(ws), dtype_id(x.dtype), _stream()), "bn_bwd_reduce")


def bn_bwd_apply(g: Tensor, x: Tensor, dx: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor,
                 sums: Optional[Tensor], inv_n: float, act_y: Optional[Tensor] = None, slope: float = 0.2) -> bool:
    """``act_y``: fold the LeakyReLU derivative of the layer's saved output into the pass (bf16, C % 8 == 0);
    returns False when that form is not available (nothing was launched: run ``lrelu_bwd_`` and call again without)"""
    C_ = x.shape[-1]
    rc = _lib.lib().wsr_bn_bwd_apply(_p(g), _p(x), _p(dx), _p(mean), _p(invstd), _p(gamma), _p(sums), inv_n, _p(act_y),
                                     slope, C_, x.numel() // C_, dtype_id(x.dtype), _stream())
    if rc == _lib.WSR_EUNSUPPORTED and act_y is not None:
        return False
    check(rc, "bn_bwd_apply")
    return True


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float, eps: float,
              weight_decay: float, step: int) -> None:
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("adam_step wants flat contiguous fp32 buffers")
    check(_lib.lib().wsr_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                                   _stream()), "adam_step")


ADAM_CHUNK = 32768  # elements per job of wsr_adam_multi (one workgroup each)


def adam_job_table(tensors) -> Tensor:
    """Device table of ``wsr_adam_job_t`` records for ``tensors`` = [(param, grad, exp_avg, exp_avg_sq)] (contiguous fp32,
    one device), large tensors cut into chunks of :data:`ADAM_CHUNK` elements."""
    import numpy as np

    rows = []
    for quad in tensors:
        n = quad[0].numel()
        for t in quad:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.device != quad[0].device:
                raise ValueError("adam_job_table wants contiguous fp32 tensors of one size on one device")
        ptrs = [t.data_ptr() for t in quad]
        for off in range(0, n, ADAM_CHUNK):
            rows.append([q + 4 * off for q in ptrs] + [min(ADAM_CHUNK, n - off)])
    rec = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    return _table_to_device(rec, tensors[0][0].device)


def adam_multi(table: Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int) -> None:
    """torch.optim.Adam's update of every tensor in ``table`` (:func:`adam_job_table`) in ONE launch; ``step`` >= 1 is the
    step count after this update (shared by all tensors, as in one param group)."""
    check(_lib.lib().wsr_adam_multi(_p(table), table.shape[0], lr, beta1, beta2, eps, weight_decay, step, _stream()),
          "adam_multi")


def _check_partials(table: Tensor, partials: Tensor) -> None:
    if partials.dtype != torch.float32 or not partials.is_cuda or not partials.is_contiguous() \
            or partials.numel() < table.shape[0] or partials.device != table.device:
        raise ValueError("grad-norm partials want a contiguous fp32 device buffer of one float per job of the table")


def grad_sqnorm_multi(table: Tensor, partials: Tensor) -> None:
    """``partials[job]`` = sum of squares of the gradient chunk of each job of ``table`` (:func:`adam_job_table`), one
    launch, the same bits from run to run."""
    _check_partials(table, partials)
    check(_lib.lib().wsr_grad_sqnorm_multi(_p(table), table.shape[0], _p(partials), _stream()), "grad_sqnorm_multi")


def adam_multi_clip(table: Tensor, partials: Tensor, max_norm: float, lr: float, beta1: float, beta2: float,
                    eps: float, weight_decay: float, step: int, total_norm: Optional[Tensor] = None) -> None:
    """:func:`adam_multi` behind ``clip_grad_norm_(max_norm)`` over every gradient of ``table``: the coefficient comes
    from ``partials`` (:func:`grad_sqnorm_multi` of the same table) on the device, the scaled gradients are written
    back.  ``max_norm`` = inf measures only (gradients untouched, the update is :func:`adam_multi`'s).  ``total_norm``
    (0-d fp32 device tensor) receives the pre-clip norm."""
    _check_partials(table, partials)
    if not max_norm > 0:
        raise ValueError(f"adam_multi_clip: max_norm must be > 0, not {max_norm}")
    if total_norm is not None and (total_norm.dtype != torch.float32 or total_norm.device != table.device):
        raise ValueError("adam_multi_clip: total_norm wants a fp32 tensor on the table's device")
    check(_lib.lib().wsr_adam_multi_clip(_p(table), table.shape[0], _p(partials), max_norm, lr, beta1, beta2, eps,
                                         weight_decay, step, _p(total_norm), _stream()), "adam_multi_clip")


def ema_ptr_table(tensors, shadows) -> Tensor:
    """Device array of one ``float*`` per job of ``adam_job_table(tensors)``, chunk for chunk: the shadow (moving
    average) of each parameter chunk.  ``shadows``: one contiguous fp32 tensor per entry of ``tensors``, same size and
    device as its parameter."""
    import numpy as np

    if len(shadows) != len(tensors):
        raise ValueError("ema_ptr_table wants one shadow per parameter")
    rows = []
    for quad, e in zip(tensors, shadows):
        n = quad[0].numel()
        if e.dtype != torch.float32 or not e.is_contiguous() or e.numel() != n or e.device != quad[0].device:
            raise ValueError("ema_ptr_table wants contiguous fp32 shadows of their parameter's size and device")
        if e.data_ptr() == quad[0].data_ptr():
            raise ValueError("ema_ptr_table: a shadow shares its parameter's storage")
        rows += [e.data_ptr() + 4 * off for off in range(0, n, ADAM_CHUNK)]
    return _table_to_device(np.asarray(rows, dtype=np.int64).reshape(-1, 1), tensors[0][0].device)


def _check_ema(table: Tensor, ema_table: Tensor, ema_decay: float) -> None:
    if ema_table.shape[0] != table.shape[0] or ema_table.device != table.device:
        raise ValueError("the EMA pointer table wants one row per job of the Adam table, on its device")
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), not {ema_decay}")


def adam_multi_ema(table: Tensor, ema_table: Tensor, lr: float, beta1: float, beta2: float, eps: float,
                   weight_decay: float, step: int, ema_decay: float) -> None:
    """:func:`adam_multi` that also moves the shadows of ``ema_table`` (:func:`ema_ptr_table` of the same tensors)
    towards the new parameters, ``e = ema_decay * e + (1 - ema_decay) * p``, in the same launch; ``ema_decay`` = 0
    copies (``e = p``).  Parameters and optimizer state come out as :func:`adam_multi` leaves them, bit for bit."""
    _check_ema(table, ema_table, ema_decay)
    check(_lib.lib().wsr_adam_multi_ema(_p(table), _p(ema_table), table.shape[0], lr, beta1, beta2, eps, weight_decay,
                                        step, ema_decay, _stream()), "adam_multi_ema")


def adam_multi_clip_ema(table: Tensor, ema_table: Tensor, partials: Tensor, max_norm: float, lr: float, beta1: float,
                        beta2: float, eps: float, weight_decay: float, step: int, ema_decay: float,
                        total_norm: Optional[Tensor] = None) -> None:
    """:func:`adam_multi_clip` with the shadow update of :func:`adam_multi_ema` in the same launch."""
    _check_partials(table, partials)
    _check_ema(table, ema_table, ema_decay)
    if not max_norm > 0:
        raise ValueError(f"adam_multi_clip_ema: max_norm must be > 0, not {max_norm}")
    if total_norm is not None and (total_norm.dtype != torch.float32 or total_norm.device != table.device):
        raise ValueError("adam_multi_clip_ema: total_norm wants a fp32 tensor on the table's device")
    check(_lib.lib().wsr_adam_multi_clip_ema(_p(table), _p(ema_table), table.shape[0], _p(partials), max_norm, lr,
                                             beta1, beta2, eps, weight_decay, step, ema_decay, _p(total_norm),
                                             _stream()), "adam_multi_clip_ema")


def gather_batch(store: Tensor, desc: Tensor, cin: int, s: int, slice_size: int) -> Tuple[Tensor, Tensor, Tensor]:
    """One training batch ``(LR, HR, Z)`` out of a resident store (``device_data.ResidentStore``) in ONE launch:
    ``store`` fp32 (N, cin + 1, X, Y, NZ), ``desc`` int32 (B, 6) rows ``sample, x0, y0, k, flip_x, flip_y`` on the
    device; ``slice_size`` 0 = the whole domain.  -> planar LR (B, cin, S/s, S/s, NZ), HR (B, 3, S, S, NZ),
    Z (B, 1, S, S, NZ) on the current stream (``wsr_gather_batch``)."""
    _need_cuda(store, desc)
    if store.dtype != torch.float32 or store.dim() != 5 or not store.is_contiguous() or store.shape[1] != cin + 1:
        raise ValueError(f"gather_batch wants a contiguous fp32 store (N, {cin + 1}, X, Y, NZ), got {tuple(store.shape)}")
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 6 or not desc.is_contiguous():
        raise ValueError(f"gather_batch wants an int32 (B, 6) descriptor table, got {desc.dtype} {tuple(desc.shape)}")
    N, _, X, Y, NZ = store.shape
    B = desc.shape[0]
    W, H = (slice_size, slice_size) if slice_size else (X, Y)
    Wc, Hc = -(-W // s), -(-H // s)
    opts = dict(dtype=torch.float32, device=store.device)
    lr = torch.empty((B, cin, Wc, Hc, NZ), **opts)
    hr = torch.empty((B, 3, W, H, NZ), **opts)
    z = torch.empty((B, 1, W, H, NZ), **opts)
    check(_lib.lib().wsr_gather_batch(_p(store), N, _p(desc), B, cin, s, slice_size, X, Y, NZ, _p(lr), _p(hr), _p(z),
                                      _stream()), "gather_batch")
    return lr, hr, z


DEGRADE_MAX_R = 32  # WSR_DEGRADE_MAX_R


def gather_batch_filtered(store: Tensor, desc: Tensor, cin: int, s: int, slice_size: int, wx: Tensor, wy: Tensor,
                          n_filt: int, out: Optional[Tuple[Tensor, Tensor, Tensor]] = None
                          ) -> Tuple[Tensor, Tensor, Tensor]:
    """:func:`gather_batch` with the LR degradation of ``[DEGRADATION]`` (degradation.py) in the same launch: the LR
    planes read from store channels below ``n_filt`` are filtered with the fp32 weight tables ``wx`` (ceil(W / s),
    2 R + 1) and ``wy`` (ceil(H / s), 2 R + 1) of ``degradation.axis_weights`` (W x H: the slice, or the domain when
    ``slice_size`` is 0) and then sampled; the other LR planes, HR and Z are the copies of :func:`gather_batch`.
    ``out``: contiguous fp32 ``(LR, HR, Z)`` of the shapes below to write into (``wsr_gather_batch_filtered``)."""
    _need_cuda(store, desc, wx, wy)
    if store.dtype != torch.float32 or store.dim() != 5 or not store.is_contiguous() or store.shape[1] != cin + 1:
        raise ValueError(f"gather_batch_filtered wants a contiguous fp32 store (N, {cin + 1}, X, Y, NZ), got "
                         f"{tuple(store.shape)}")
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 6 or not desc.is_contiguous():
        raise ValueError(f"gather_batch_filtered wants an int32 (B, 6) descriptor table, got {desc.dtype} "
                         f"{tuple(desc.shape)}")
    N, _, X, Y, NZ = store.shape
    B = desc.shape[0]
    W, H = (slice_size, slice_size) if slice_size else (X, Y)
    Wc, Hc = -(-W // s), -(-H // s)
    T = wx.shape[-1] if wx.dim() == 2 else 0
    R = (T - 1) // 2
    for name, w, rows in (("wx", wx, Wc), ("wy", wy, Hc)):
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or tuple(w.shape) != (rows, T):
            raise ValueError(f"gather_batch_filtered wants {name} as a contiguous fp32 ({rows}, 2 R + 1) table, got "
                             f"{w.dtype} {tuple(w.shape)}")
    if T != 2 * R + 1 or R > DEGRADE_MAX_R:
        raise ValueError(f"gather_batch_filtered wants 2 R + 1 taps with 0 <= R <= {DEGRADE_MAX_R}, got {T}")
    if not 0 <= n_filt <= cin:
        raise ValueError(f"gather_batch_filtered: n_filt must be in 0 .. {cin}, not {n_filt}")
    opts = dict(dtype=torch.float32, device=store.device)
    shapes = ((B, cin, Wc, Hc, NZ), (B, 3, W, H, NZ), (B, 1, W, H, NZ))
    if out is None:
        out = tuple(torch.empty(shape, **opts) for shape in shapes)
    _need_cuda(*out)
    for name, t, shape in zip(("LR", "HR", "Z"), out, shapes):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"gather_batch_filtered wants out {name} as a contiguous fp32 {shape} tensor, got "
                             f"{t.dtype} {tuple(t.shape)}")
    lr, hr, z = out
    check(_lib.lib().wsr_gather_batch_filtered(_p(store), N, _p(desc), B, cin, s, slice_size, X, Y, NZ, _p(wx), _p(wy),
                                               R, n_filt, _p(lr), _p(hr), _p(z), _stream()), "gather_batch_filtered")
    return lr, hr, z


# ---------------------------------------------------------------------------------------------------------------------
# device-side evaluation ([EVAL] device_metrics; csrc/eval_metrics.hip)
# ---------------------------------------------------------------------------------------------------------------------
FIELD_METRICS_SUMS = 7        # WSR_FIELD_METRICS_SUMS
FIELD_METRICS_MAX_ROWS = 2048  # WSR_FIELD_METRICS_MAX_ROWS


def _planar5(name: str, what: str, t: Tensor, min_c: int = 1) -> None:
    if t.dtype != torch.float32 or t.dim() != 5 or not t.is_contiguous() or t.shape[1] < min_c or t.numel() == 0:
        raise ValueError(f"{name} wants {what} as a contiguous fp32 (B, C >= {min_c}, X, Y, NZ) tensor, got "
                         f"{t.dtype} {tuple(t.shape)}")


def _same_grid(name: str, HR: Tensor, **fields: Tensor):
    """``HR`` and ``fields`` (by name) are planar fp32 with at least 3 channels, the fields on HR's grid -> (B, X, Y, NZ)"""
    for what, t in (("HR", HR), *fields.items()):
        _planar5(name, what, t, 3)
    B, _, X, Y, NZ = HR.shape
    for what, t in fields.items():
        if (t.shape[0],) + tuple(t.shape[2:]) != (B, X, Y, NZ):
            raise ValueError(f"{name}: {what} {tuple(t.shape)} does not match HR {tuple(HR.shape)}")
    return B, X, Y, NZ


def _sums_out(name: str, out: Optional[Tensor], shape: tuple, device) -> Tensor:
    """``out`` or, for None, a new float64 tensor of ``shape``: what the reductions write their sums into"""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{name} wants out as a contiguous float64 {shape} tensor, got {out.dtype} {tuple(out.shape)}")
    return out


def _workspace(floats: int, device) -> Tensor:
    return torch.empty(int(floats), dtype=torch.float32, device=device)


def trilinear_xy(LR: Tensor, s: int) -> Tensor:
    """The trilinear baseline ``F.interpolate(LR[:, :3], scale_factor=(s, s, 1), mode="trilinear",
    align_corners=True)`` in one launch: ``LR`` fp32 (B, Cin >= 3, Xl, Yl, NZ) -> (B, 3, Xl * s, Yl * s, NZ); only
    channels 0..2 are read (``wsr_trilinear_xy``)."""
    _need_cuda(LR)
    _planar5("trilinear_xy", "LR", LR, 3)
    s = int(s)
    if s < 1:
        raise ValueError(f"trilinear_xy wants a scale >= 1, not {s}")
    B, cin, Xl, Yl, NZ = LR.shape
    out = torch.empty((B, 3, Xl * s, Yl * s, NZ), dtype=torch.float32, device=LR.device)
    check(_lib.lib().wsr_trilinear_xy(_p(LR), B, cin, Xl, Yl, NZ, s, _p(out), _stream()), "trilinear_xy")
    return out


def field_metrics(HR: Tensor, SR: Tensor, *, LR: Optional[Tensor] = None, scale: Optional[int] = None,
                  TL: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Seven sums per sample over channels 0..2 of ``HR`` and ``SR`` (B, C >= 3, X, Y, NZ) -> float64 (B, 7):
    sum (HR-SR)^2, sum (HR-TL)^2, sum |HR-SR|, sum |HR-TL| over components; sum ||HR-SR||, sum ||HR-TL||, sum ||HR||
    over voxels.  The baseline is the tensor ``TL`` (B, C >= 3, X, Y, NZ), or made on the fly from ``LR``
    (B, C >= 3, X / scale, Y / scale, NZ) and ``scale`` - the bits of ``trilinear_xy``, never written to memory.  One
    pass, no atomics: the same bits on every call.  ``out``: a float64 (B, 7) slice to write into
    (``wsr_field_metrics``)."""
    if (TL is None) == (LR is None) or (LR is not None and scale is None):
        raise ValueError("field_metrics wants either TL= or LR= and scale=")
    _need_cuda(HR, SR, LR, TL, out)
    B, X, Y, NZ = _same_grid("field_metrics", HR, SR=SR, **({} if TL is None else {"TL": TL}))
    s = 0
    if TL is None:
        _planar5("field_metrics", "LR", LR, 3)
        s = int(scale)
        if s < 1 or (LR.shape[0], LR.shape[2] * s, LR.shape[3] * s, LR.shape[4]) != (B, X, Y, NZ):
            raise ValueError(f"field_metrics: LR {tuple(LR.shape)} x{s} does not match HR {tuple(HR.shape)}")
    out = _sums_out("field_metrics", out, (B, FIELD_METRICS_SUMS), HR.device)
    partials = _workspace(B * FIELD_METRICS_MAX_ROWS * FIELD_METRICS_SUMS, HR.device)
    check(_lib.lib().wsr_field_metrics(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), 0 if TL is None else TL.shape[1],
                                       _p(LR), 0 if LR is None else LR.shape[1], s, B, X, Y, NZ, _p(partials), _p(out),
                                       _stream()), "field_metrics")
    return out


def column_interp(vals: Tensor, z_src: Tensor, z_dst: Tensor) -> Tensor:
    """``np.interp(z_dst[col], z_src[col], vals[c][col])`` for every column of ``vals`` fp32 (B, C, X, Y, NZ) with source
    and query levels (B, 1, X, Y, NZ), NZ <= 128: queries outside the source range get the end values, slope and blend
    are evaluated in double and rounded once to fp32 (``process_data.reverse_interpolate_z_axis`` in one launch;
    ``wsr_column_interp``)."""
    _need_cuda(vals, z_src, z_dst)
    _planar5("column_interp", "vals", vals)
    _planar5("column_interp", "z_src", z_src)
    _planar5("column_interp", "z_dst", z_dst)
    B, C, X, Y, NZ = vals.shape
    if tuple(z_src.shape) != (B, 1, X, Y, NZ) or tuple(z_dst.shape) != (B, 1, X, Y, NZ):
        raise ValueError(f"column_interp wants levels ({B}, 1, {X}, {Y}, {NZ}), got {tuple(z_src.shape)} and "
                         f"{tuple(z_dst.shape)}")
    if NZ > 128:
        raise ValueError(f"column_interp stages one column in LDS: at most 128 levels, not {NZ}")
    out = torch.empty_like(vals)
    check(_lib.lib().wsr_column_interp(_p(vals), _p(z_src), _p(z_dst), B, C, X * Y, NZ, _p(out), _stream()),
          "column_interp")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# geometric self-ensemble ([ENSEMBLE]; csrc/ensemble.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _member_codes(name: str, codes, X: int, Y: int):
    codes = [int(c) for c in codes]
    if len(codes) not in (1, 2, 4, 8) or any(c < 0 or c > 7 for c in codes):
        raise ValueError(f"{name} wants 1, 2, 4 or 8 member codes k + 4 * fx in 0..7, got {codes}")
    if X != Y and any(c & 1 for c in codes):
        raise ValueError(f"{name}: a member with an odd number of quarter turns needs a square domain, "
                         f"not X = {X}, Y = {Y}")
    return (C.c_int32 * len(codes))(*codes), len(codes)


def dihedral_members(src: Tensor, codes, is_vector: bool) -> Tensor:
    """The ``K = len(codes)`` transformed copies of ``src`` fp32 (B, C, X, Y, NZ) in ONE launch -> (K, B, C, X', Y', NZ).
    A code is ``k + 4 * fx``: ``k`` quarter turns as ``process_data._rotate_wind`` does them, then, if ``fx``, a mirror
    along x.  ``is_vector``: channels 0 and 1 are the horizontal wind (they turn with the grid, the mirror negates u);
    otherwise every channel is only permuted.  Bit-identical to the CPU rules (``wsr_dihedral_members``)."""
    _need_cuda(src)
    _planar5("dihedral_members", "src", src, 2 if is_vector else 1)
    B, Cn, X, Y, NZ = src.shape
    arr, K = _member_codes("dihedral_members", codes, X, Y)
    odd = any(int(c) & 1 for c in codes)
    out = torch.empty((K, B, Cn, Y if odd else X, X if odd else Y, NZ), dtype=torch.float32, device=src.device)
    check(_lib.lib().wsr_dihedral_members(_p(src), B, Cn, X, Y, NZ, arr, K, 1 if is_vector else 0, _p(out), _stream()),
          "dihedral_members")
    return out


def ensemble_reduce(members: Tensor, codes, with_var: bool = False):
    """``members`` fp32 (K, B, 3, X', Y', NZ), member ``m`` transformed by ``codes[m]`` -> the mean (B, 3, X, Y, NZ) of
    the members mapped back through their inverses, as the pairwise tree sum in member order times ``1 / K``; with
    ``with_var`` also the population variance per component, ``(mean, var)``.  One pass, no atomics: the same bits on
    every call (``wsr_ensemble_reduce``)."""
    _need_cuda(members)
    if members.dtype != torch.float32 or members.dim() != 6 or not members.is_contiguous() or members.shape[2] != 3 \
            or members.numel() == 0:
        raise ValueError(f"ensemble_reduce wants members as a contiguous fp32 (K, B, 3, X, Y, NZ) tensor, got "
                         f"{members.dtype} {tuple(members.shape)}")
    K, B, _, X, Y, NZ = members.shape
    arr, n = _member_codes("ensemble_reduce", codes, X, Y)
    if n != K:
        raise ValueError(f"ensemble_reduce: {n} codes for {K} members")
    # (odd quarter turns only on a square plane: the members' shape is the output's)
    mean = torch.empty((B, 3, X, Y, NZ), dtype=torch.float32, device=members.device)
    var = torch.empty_like(mean) if with_var else None
    check(_lib.lib().wsr_ensemble_reduce(_p(members), arr, K, B, X, Y, NZ, _p(mean), _p(var), _stream()),
          "ensemble_reduce")
    return (mean, var) if with_var else mean


# ---------------------------------------------------------------------------------------------------------------------
# tiled whole-domain inference ([TILE]; csrc/tiling.hip)
# ---------------------------------------------------------------------------------------------------------------------
#: WSR_TILE_MAX_PER_AXIS of include/windsr_hip.h: the origins of an axis travel by value in the stitch launch
TILE_MAX_PER_AXIS = 128


def _origins(name: str, what: str, vals):
    vals = [int(v) for v in vals]
    if not vals:
        raise ValueError(f"{name} wants at least one origin in {what}")
    return (C.c_int32 * len(vals))(*vals), vals


def tile_gather(src: Tensor, x0, y0, tx: int, ty: int) -> Tensor:
    """The ``n = len(x0)`` tiles ``src[:, :, x0[k]:x0[k] + tx, y0[k]:y0[k] + ty, :]`` of ``src`` fp32 (B, C, X, Y, NZ) in
    ONE launch -> (n, B, C, tx, ty, NZ); a pure copy, the bits of torch slicing (``wsr_tile_gather``)."""
    _need_cuda(src)
    _planar5("tile_gather", "src", src)
    B, Cn, X, Y, NZ = src.shape
    tx, ty = int(tx), int(ty)
    ax, xl = _origins("tile_gather", "x0", x0)
    ay, yl = _origins("tile_gather", "y0", y0)
    if len(xl) != len(yl):
        raise ValueError(f"tile_gather: {len(xl)} origins in x0 for {len(yl)} in y0")
    if not (1 <= tx <= X and 1 <= ty <= Y):
        raise ValueError(f"tile_gather wants tiles inside the domain, not tx = {tx}, ty = {ty} for X = {X}, Y = {Y}")
    for k, (a, b) in enumerate(zip(xl, yl)):
        if a < 0 or b < 0 or a + tx > X or b + ty > Y:
            raise ValueError(f"tile_gather: tile {k} at ({a}, {b}) of {tx} x {ty} leaves the domain X = {X}, Y = {Y}")
    out = torch.empty((len(xl), B, Cn, tx, ty, NZ), dtype=torch.float32, device=src.device)
    check(_lib.lib().wsr_tile_gather(_p(src), B, Cn, X, Y, NZ, ax, ay, len(xl), tx, ty, _p(out), _stream()),
          "tile_gather")
    return out


def _tile_axis(name: str, axis: str, s, T: int, N: int, R: int) -> None:
    if not 1 <= T <= N:
        raise ValueError(f"{name} wants 1 <= T{axis} <= {axis.upper()}, not T{axis} = {T}, {axis.upper()} = {N}")
    if not 0 <= R <= 32768:
        raise ValueError(f"{name} wants 0 <= R{axis} <= 32768, not {R}")
    if s[0] != 0 or s[-1] + T != N:
        raise ValueError(f"{name}: the {axis} origins must start at 0 and end at {axis.upper()} - T{axis} = {N - T}, "
                         f"got {s[0]} .. {s[-1]}")
    for a, b in zip(s, s[1:]):
        if not 0 < b - a <= T:
            raise ValueError(f"{name}: the {axis} origins must increase by 1 .. T{axis} = {T}, got {a} -> {b}")
    if len(s) > TILE_MAX_PER_AXIS:
        raise ValueError(f"{name}: {len(s)} tiles along {axis}, at most {TILE_MAX_PER_AXIS}")


def tile_stitch(tiles: Tensor, xs, ys, X: int, Y: int, Rx: int, Ry: int, with_seam: bool = False):
    """``tiles`` fp32 (nx * ny, B, C, Tx, Ty, NZ), tile ``ix * ny + iy`` at origin ``(xs[ix], ys[iy])`` -> their blend
    (B, C, X, Y, NZ): ``sum alpha_T x_T`` with the separable integer ramps of include/windsr_hip.h (``Rx``, ``Ry`` the
    ramp lengths, no ramp at a domain border), every output voxel written once; with ``with_seam`` also
    ``sum alpha_T (x_T - out)^2``, ``(out, seam)``.  Where one tile covers a voxel its value comes back bit for bit.  No
    atomics: the same bits on every call (``wsr_tile_stitch``)."""
    _need_cuda(tiles)
    if tiles.dtype != torch.float32 or tiles.dim() != 6 or not tiles.is_contiguous() or tiles.numel() == 0:
        raise ValueError(f"tile_stitch wants tiles as a contiguous fp32 (nx * ny, B, C, Tx, Ty, NZ) tensor, got "
                         f"{tiles.dtype} {tuple(tiles.shape)}")
    n, B, Cn, Tx, Ty, NZ = tiles.shape
    X, Y, Rx, Ry = int(X), int(Y), int(Rx), int(Ry)
    ax, xl = _origins("tile_stitch", "xs", xs)
    ay, yl = _origins("tile_stitch", "ys", ys)
    if len(xl) * len(yl) != n:
        raise ValueError(f"tile_stitch: {len(xl)} x {len(yl)} origins for {n} tiles")
    _tile_axis("tile_stitch", "x", xl, Tx, X, Rx)
    _tile_axis("tile_stitch", "y", yl, Ty, Y, Ry)
    out = torch.empty((B, Cn, X, Y, NZ), dtype=torch.float32, device=tiles.device)
    seam = torch.empty_like(out) if with_seam else None
    check(_lib.lib().wsr_tile_stitch(_p(tiles), ax, len(xl), ay, len(yl), B, Cn, X, Y, NZ, Tx, Ty, Rx, Ry, _p(out),
                                     _p(seam), _stream()), "tile_stitch")
    return (out, seam) if with_seam else out


# ---------------------------------------------------------------------------------------------------------------------
# per-level evaluation diagnostics ([DIAGNOSTICS]; csrc/diagnostics.hip)
# ---------------------------------------------------------------------------------------------------------------------
LEVEL_DIAG_SUMS = 15  # WSR_LEVEL_DIAG_SUMS
LEVEL_DIAG_MAX_NZ = 256


def level_diagnostics(HR: Tensor, SR: Tensor, TL: Tensor, x: Tensor, y: Tensor, Z: Tensor,
                      out: Optional[Tensor] = None) -> Tensor:
    """Fifteen sums per sample and z level over the X * Y columns of the level -> float64 (B, NZ, 15), in the order of
    ``diagnostics.SUM_NAMES``: wind speed, error-vector lengths, signed and absolute speed errors, the speed-weighted
    direction errors, squared divergences and altitudes of ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ;
    channels 0..2 are read) with the raw altitude ``Z`` (B, 1, X, Y, NZ) and the coordinates ``x`` (X), ``y`` (Y).  One
    pass, no atomics: the same bits on every call.  ``out``: a float64 (B, NZ, 15) slice to write into
    (``wsr_level_diagnostics``)."""
    _need_cuda(HR, SR, TL, x, y, Z, out)
    B, X, Y, NZ = _same_grid("level_diagnostics", HR, SR=SR, TL=TL)
    _planar5("level_diagnostics", "Z", Z)
    if tuple(Z.shape) != (B, 1, X, Y, NZ):
        raise ValueError(f"level_diagnostics wants Z ({B}, 1, {X}, {Y}, {NZ}), got {tuple(Z.shape)}")
    for name, t, n in (("x", x, X), ("y", y, Y)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"level_diagnostics wants {name} as a contiguous fp32 ({n},) tensor, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if NZ > LEVEL_DIAG_MAX_NZ or B > 65535 or X > 32768 or Y > 32768 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_diagnostics: at most {LEVEL_DIAG_MAX_NZ} levels, 65535 samples, 32768 points in x and y "
                         f"and 2^31 - 1 voxels per sample, not B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("level_diagnostics", out, (B, NZ, LEVEL_DIAG_SUMS), HR.device)
    L = _lib.lib()
    ws = _workspace(L.wsr_level_diagnostics_workspace_floats(B, X, Y, NZ), HR.device)
    check(L.wsr_level_diagnostics(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), TL.shape[1], _p(Z), _p(x), _p(y), B,
                                  X, Y, NZ, _p(ws), _p(out), _stream()), "level_diagnostics")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# horizontal energy spectra ([SPECTRUM]; csrc/spectra.hip)
# ---------------------------------------------------------------------------------------------------------------------
SPECTRUM_SUMS = 5  # WSR_SPECTRUM_SUMS
SPECTRUM_MAX_XY = 1024  # WSR_SPECTRUM_MAX_XY
SPECTRUM_WINDOWS = {"none": 0, "hann": 1}  # WSR_SPECTRUM_WINDOW_*


def level_spectra(HR: Tensor, SR: Tensor, TL: Tensor, window: str = "hann", out: Optional[Tensor] = None) -> Tensor:
    """Five sums per sample, z level and horizontal wavenumber bin -> float64 (B, NZ, NK, 5), in the order of
    ``spectra.SPECTRUM_SUMS``: the kinetic energy of ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ;
    channels 0..2 are read) and the co-spectra of HR with SR and with TL, from a direct separable 2-D DFT over (X, Y) of
    the detrended, windowed (``window``: ``hann`` or ``none``) planes; NK = ``spectra.n_bins(X, Y)``.  No atomics: the
    same bits on every call.  ``out``: a float64 (B, NZ, NK, 5) slice to write into (``wsr_level_spectra``)."""
    _need_cuda(HR, SR, TL, out)
    B, X, Y, NZ = _same_grid("level_spectra", HR, SR=SR, TL=TL)
    if window not in SPECTRUM_WINDOWS:
        raise ValueError(f"level_spectra: window must be one of {tuple(SPECTRUM_WINDOWS)} (codes 0, 1), not {window!r}")
    if X > SPECTRUM_MAX_XY or Y > SPECTRUM_MAX_XY or B > 65535 or NZ > 65535 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_spectra: at most {SPECTRUM_MAX_XY} points in x and y, 65535 samples, 65535 levels and "
                         f"2^31 - 1 voxels per sample, not B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    L = _lib.lib()
    NK = int(L.wsr_level_spectra_bins(X, Y))
    out = _sums_out("level_spectra", out, (B, NZ, NK, SPECTRUM_SUMS), HR.device)
    ws = _workspace(L.wsr_level_spectra_workspace_floats(B, X, Y, NZ), HR.device)
    check(L.wsr_level_spectra(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), TL.shape[1], B, X, Y, NZ,
                              SPECTRUM_WINDOWS[window], _p(ws), _p(out), _stream()), "level_spectra")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# energy-spectrum loss of generator training ([SPECTRAL_LOSS]; csrc/spectral_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------
class _SpectralEnergy(torch.autograd.Function):
    """``wsr_spectral_energy`` with ``wsr_spectral_energy_bwd`` as backward: E (B, NZ, NK, 2) = [e_hr, e_sr]; only e_sr
    carries gradient, and only towards SR.  F_sr is saved by the forward's column pass only when SR requires grad."""

    @staticmethod
    def forward(ctx, hr: Tensor, sr: Tensor, window: int):
        B, _, X, Y, NZ = sr.shape
        L = _lib.lib()
        NK = int(L.wsr_level_spectra_bins(X, Y))
        out = torch.empty((B, NZ, NK, 2), dtype=torch.float64, device=sr.device)
        ws = _workspace(L.wsr_spectral_energy_workspace_floats(B, X, Y, NZ), sr.device)
        saved = None
        if ctx.needs_input_grad[1]:
            saved = _workspace(L.wsr_spectral_energy_saved_floats(B, X, Y, NZ), sr.device)
        check(L.wsr_spectral_energy(_p(hr), hr.shape[1], _p(sr), sr.shape[1], B, X, Y, NZ, window, _p(ws), _p(saved),
                                    _p(out), _stream()), "spectral_energy")
        ctx.meta = (tuple(sr.shape), window)
        ctx.save_for_backward(saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable  # (the kernel's result is no graph: a double backward is refused)
    def backward(ctx, g: Tensor):
        (saved,) = ctx.saved_tensors
        if saved is None or not ctx.needs_input_grad[1]:
            return None, None, None
        (B, C_, X, Y, NZ), window = ctx.meta
        L = _lib.lib()
        gbin = g[..., 1].to(torch.float64).contiguous()
        ws = _workspace(L.wsr_spectral_energy_workspace_floats(B, X, Y, NZ), g.device)
        dsr = torch.empty((B, 3, X, Y, NZ), dtype=torch.float32, device=g.device)
        check(L.wsr_spectral_energy_bwd(_p(saved), _p(gbin), B, X, Y, NZ, window, _p(ws), _p(dsr), _stream()),
              "spectral_energy_bwd")
        if C_ > 3:  # (surplus channels are never read: their gradient is zero)
            full = torch.zeros((B, C_, X, Y, NZ), dtype=torch.float32, device=g.device)
            full[:, :3] = dsr
            dsr = full
        return None, dsr, None


def spectral_energy(HR: Tensor, SR: Tensor, window: str = "hann") -> Tensor:
    """The binned horizontal kinetic-energy spectra of ``HR`` and ``SR`` (B, C >= 3, X, Y, NZ; channels 0..2 are read,
    surplus ones never) -> float64 (B, NZ, NK, 2) = [e_hr, e_sr], the first two sums of ``level_spectra`` with the same
    arithmetic (``wsr_spectral_energy``).  Differentiable: only e_sr carries gradient, and only towards SR
    (``wsr_spectral_energy_bwd``: the inverse transform of the binned upstream gradient times the saved F_sr, minus its
    plane mean).  No atomics: the same bits on every call, forward and backward."""
    _need_cuda(HR, SR)
    for name, t in (("HR", HR), ("SR", SR)):
        if t.dim() != 5 or t.shape[1] < 3 or t.numel() == 0 or not t.is_floating_point():
            raise ValueError(f"spectral_energy wants {name} as a floating-point (B, C >= 3, X, Y, NZ) tensor, got "
                             f"{t.dtype} {tuple(t.shape)}")
    B, _, X, Y, NZ = HR.shape
    if (SR.shape[0],) + tuple(SR.shape[2:]) != (B, X, Y, NZ):
        raise ValueError(f"spectral_energy: SR {tuple(SR.shape)} does not match HR {tuple(HR.shape)}")
    if window not in SPECTRUM_WINDOWS:
        raise ValueError(f"spectral_energy: window must be one of {tuple(SPECTRUM_WINDOWS)} (codes 0, 1), not {window!r}")
    if X > SPECTRUM_MAX_XY or Y > SPECTRUM_MAX_XY or B > 65535 or NZ > 65535 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"spectral_energy: at most {SPECTRUM_MAX_XY} points in x and y, 65535 samples, 65535 levels and "
                         f"2^31 - 1 voxels per sample, not B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    return _SpectralEnergy.apply(HR.detach().contiguous().float(), SR.contiguous().float(), SPECTRUM_WINDOWS[window])


# ---------------------------------------------------------------------------------------------------------------------
# structural similarity on horizontal planes ([SSIM]; csrc/ssim.hip)
# ---------------------------------------------------------------------------------------------------------------------
SSIM_SUMS = 4  # WSR_SSIM_SUMS
SSIM_MAX_WIN = 15  # WSR_SSIM_MAX_WIN
SSIM_MAX_NZ = 256
_ssim_taps: dict = {}


def _ssim_taps_on(device, win: int, sigma: float) -> Tensor:
    """``ssim.taps(win, sigma)`` on ``device``: uploaded once per (device, win, sigma)"""
    from . import ssim

    key = (device.index, int(win), float(sigma))
    t = _ssim_taps.get(key)
    if t is None:
        if len(_ssim_taps) > 64:
            _ssim_taps.clear()
        t = _ssim_taps[key] = ssim.taps(win, sigma).to(device).contiguous()
    return t


def level_ssim(HR: Tensor, SR: Tensor, TL: Tensor, win: int = 11, sigma: float = 1.5, data_range: float = 2.0,
               out: Optional[Tensor] = None) -> Tensor:
    """Four sums per sample, z level and wind component -> float64 (B, NZ, 3, 4), in the order of ``ssim.SSIM_SUMS``: over
    the (X - win + 1) (Y - win + 1) valid positions of the separable gaussian window ``ssim.taps(win, sigma)`` on the
    horizontal plane, SSIM and its contrast-structure factor of ``HR`` with ``SR`` and of ``HR`` with the baseline ``TL``
    (B, C >= 3, X, Y, NZ; channels 0..2 are read), C1 = (0.01 ``data_range``)^2, C2 = (0.03 ``data_range``)^2.  z is never
    windowed.  No atomics: the same bits on every call, and exactly the number of positions where the two fields hold the
    same bits.  ``out``: a float64 (B, NZ, 3, 4) slice to write into (``wsr_level_ssim``)."""
    from . import ssim

    _need_cuda(HR, SR, TL, out)
    B, X, Y, NZ = _same_grid("level_ssim", HR, SR=SR, TL=TL)
    ssim.check_window(win, sigma, "level_ssim")
    ssim.check_domain(X, Y, win, "level_ssim")
    c1, c2 = ssim.constants(data_range)
    if NZ > SSIM_MAX_NZ or B > 65535 or X > 32768 or Y > 32768 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_ssim: at most {SSIM_MAX_NZ} levels, 65535 samples, 32768 points in x and y and 2^31 - 1 "
                         f"voxels per sample, not B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("level_ssim", out, (B, NZ, 3, SSIM_SUMS), HR.device)
    L = _lib.lib()
    taps = _ssim_taps_on(HR.device, win, sigma)
    ws = _workspace(L.wsr_level_ssim_workspace_floats(B, X, Y, NZ, int(win)), HR.device)
    check(L.wsr_level_ssim(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), TL.shape[1], _p(taps), int(win), c1, c2, B, X,
                           Y, NZ, _p(ws), _p(out), _stream()), "level_ssim")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# SSIM loss of generator training ([SSIM_LOSS]; csrc/ssim_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------
class _SsimPairSums(torch.autograd.Function):
    """``wsr_ssim_pair_sums`` with ``wsr_ssim_pair_sums_bwd`` as backward: P (B, NZ, 3, 2) = [sum of l cs, sum of cs];
    gradient flows only towards SR, from both columns.  Nothing is saved but the inputs: the backward recomputes."""

    @staticmethod
    def forward(ctx, hr: Tensor, sr: Tensor, taps: Tensor, win: int, c1: float, c2: float):
        B, _, X, Y, NZ = sr.shape
        L = _lib.lib()
        out = torch.empty((B, NZ, 3, 2), dtype=torch.float64, device=sr.device)
        ws = _workspace(L.wsr_ssim_pair_sums_workspace_floats(B, X, Y, NZ, win), sr.device)
        check(L.wsr_ssim_pair_sums(_p(hr), hr.shape[1], _p(sr), sr.shape[1], _p(taps), win, c1, c2, B, X, Y, NZ, _p(ws),
                                   _p(out), _stream()), "ssim_pair_sums")
        ctx.meta = (win, c1, c2)
        ctx.save_for_backward(hr, sr, taps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable  # (the kernel's result is no graph: a double backward is refused)
    def backward(ctx, g: Tensor):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        hr, sr, taps = ctx.saved_tensors
        win, c1, c2 = ctx.meta
        B, C_, X, Y, NZ = sr.shape
        L = _lib.lib()
        gout = g.to(torch.float64).contiguous()
        dsr = torch.empty((B, 3, X, Y, NZ), dtype=torch.float32, device=g.device)
        check(L.wsr_ssim_pair_sums_bwd(_p(hr), hr.shape[1], _p(sr), C_, _p(gout), _p(taps), win, c1, c2, B, X, Y, NZ,
                                       _p(dsr), _stream()), "ssim_pair_sums_bwd")
        if C_ > 3:  # (surplus channels are never read: their gradient is zero)
            full = torch.zeros((B, C_, X, Y, NZ), dtype=torch.float32, device=g.device)
            full[:, :3] = dsr
            dsr = full
        return None, dsr, None, None, None, None


def ssim_pair_sums(HR: Tensor, SR: Tensor, win: int = 11, sigma: float = 1.5, data_range: float = 2.0) -> Tensor:
    """Two sums per sample, z level and wind component of ``HR`` and ``SR`` (B, C >= 3, X, Y, NZ; channels 0..2 are read,
    surplus ones never) -> float64 (B, NZ, 3, 2) = [sum of l cs, sum of cs] over the valid positions of the window
    ``ssim.taps(win, sigma)``: the first two sums of ``level_ssim``, bit for bit (``wsr_ssim_pair_sums``).
    Differentiable: both columns carry gradient, and only towards SR (``wsr_ssim_pair_sums_bwd``: one launch that
    recomputes the moments and applies the adjoint of the valid window).  No atomics: the same bits on every call,
    forward and backward."""
    from . import ssim

    _need_cuda(HR, SR)
    for name, t in (("HR", HR), ("SR", SR)):
        if t.dim() != 5 or t.shape[1] < 3 or t.numel() == 0 or not t.is_floating_point():
            raise ValueError(f"ssim_pair_sums wants {name} as a floating-point (B, C >= 3, X, Y, NZ) tensor, got "
                             f"{t.dtype} {tuple(t.shape)}")
    B, _, X, Y, NZ = HR.shape
    if (SR.shape[0],) + tuple(SR.shape[2:]) != (B, X, Y, NZ):
        raise ValueError(f"ssim_pair_sums: SR {tuple(SR.shape)} does not match HR {tuple(HR.shape)}")
    ssim.check_window(win, sigma, "ssim_pair_sums")
    ssim.check_domain(X, Y, win, "ssim_pair_sums")
    c1, c2 = ssim.constants(data_range)
    if NZ > SSIM_MAX_NZ or B > 65535 or X > 32768 or Y > 32768 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"ssim_pair_sums: at most {SSIM_MAX_NZ} levels, 65535 samples, 32768 points in x and y and "
                         f"2^31 - 1 voxels per sample, not B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    taps = _ssim_taps_on(HR.device, win, sigma)
    return _SsimPairSums.apply(HR.detach().contiguous().float(), SR.contiguous().float(), taps, int(win), c1, c2)


# ---------------------------------------------------------------------------------------------------------------------
# wind-speed distribution and wind rose ([DISTRIBUTION]; csrc/distribution.hip)
# ---------------------------------------------------------------------------------------------------------------------
DISTRIBUTION_MAX_SPEED_BINS = 64  # WSR_DISTRIBUTION_MAX_SPEED_BINS
DISTRIBUTION_MAX_SECTORS = 36  # WSR_DISTRIBUTION_MAX_SECTORS
DISTRIBUTION_LDS_COUNTERS = 15360  # WSR_DISTRIBUTION_LDS_COUNTERS
_distribution_tables: dict = {}


def distribution_level_chunk(NZ: int, speed_bins: int, sectors: int) -> int:
    """The consecutive levels one workgroup of ``wsr_level_distribution`` counts"""
    return min(int(NZ), DISTRIBUTION_LDS_COUNTERS // (int(speed_bins) * (int(sectors) + 1)))


def _distribution_tables_on(device, tables) -> Tensor:
    """``edge2``, ``bx``, ``by`` of a ``distribution.DistributionTables`` as one fp32 tensor on ``device``: uploaded once
    per (device, parameters)"""
    key = (device.index, tables.UVW_MAX, tables.bin_width, tables.speed_bins, tables.sectors, tables.calm)
    t = _distribution_tables.get(key)
    if t is None:
        if len(_distribution_tables) > 64:
            _distribution_tables.clear()
        t = _distribution_tables[key] = torch.cat([tables.edge2, tables.bx, tables.by]).float().to(device).contiguous()
    return t


def level_distribution(HR: Tensor, SR: Tensor, TL: Optional[Tensor], tables, out: Optional[Tensor] = None) -> Tensor:
    """The count table per sample, z level and source -> float64 (B, NZ, 3, NS, ND + 1): the number of voxels of every
    horizontal plane of ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ; channels 0 and 1 are read) in every
    class (speed bin, direction sector or calm) of ``tables`` = ``distribution.distribution_tables(...)``, the classes
    those of ``distribution.py`` voxel for voxel.  ``TL`` None: zeros in its slices.  Integer counting, no floating-point
    atomics: the same bits on every call, equal to ``distribution.level_distribution_reference``.  ``out``: a float64
    (B, NZ, 3, NS, ND + 1) slice to write into (``wsr_level_distribution``)."""
    from . import distribution

    _need_cuda(HR, SR, TL, out)
    B, X, Y, NZ = _same_grid("level_distribution", HR, SR=SR, **({} if TL is None else {"TL": TL}))
    ns, nd = int(tables.speed_bins), int(tables.sectors)
    distribution.check_parameters(tables.bin_width, ns, nd, tables.calm, "level_distribution")
    if tables.edge2.numel() != ns - 1 or tables.bx.numel() != nd // 2 or tables.by.numel() != nd // 2:
        raise ValueError(f"level_distribution wants tables of {ns - 1} edges and {nd // 2} boundaries, got "
                         f"{tables.edge2.numel()}, {tables.bx.numel()} and {tables.by.numel()}")
    if B > 65535 or X * Y >= 2 ** 31 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_distribution: at most 65535 samples, 2^31 - 1 columns and 2^31 - 1 voxels per sample, not "
                         f"B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("level_distribution", out, (B, NZ, 3, ns, nd + 1), HR.device)
    L = _lib.lib()
    tab = _distribution_tables_on(HR.device, tables)
    edge2, bx, by = tab[:ns - 1], tab[ns - 1:ns - 1 + nd // 2], tab[ns - 1 + nd // 2:]
    ws = _workspace(L.wsr_level_distribution_workspace_floats(B, X, Y, NZ, ns, nd), HR.device)
    check(L.wsr_level_distribution(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), 0 if TL is None else TL.shape[1],
                                   _p(edge2), ns, _p(bx), _p(by), nd, float(tables.calm2), B, X, Y, NZ, _p(ws), _p(out),
                                   _stream()), "level_distribution")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# wind-speed distribution loss of generator training ([DISTRIBUTION_LOSS]; csrc/distribution_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------
DISTRIBUTION_LOSS_LDS_COUNTERS = 8320  # WSR_DISTRIBUTION_LOSS_LDS_COUNTERS


class _SpeedSoftCounts(torch.autograd.Function):
    """``wsr_speed_soft_counts`` with ``wsr_speed_soft_counts_bwd`` as backward: H (2, B, NZ, NS + 1), source 0 HR, 1 SR;
    gradient flows only towards SR, from the NS bin columns of its table.  Nothing is saved but SR: the backward
    recomputes."""

    @staticmethod
    def forward(ctx, hr: Tensor, sr: Tensor, c: float, ns: int):
        B, _, X, Y, NZ = sr.shape
        L = _lib.lib()
        out = torch.empty((2, B, NZ, ns + 1), dtype=torch.float64, device=sr.device)
        ws = _workspace(L.wsr_speed_soft_counts_workspace_floats(B, X, Y, NZ, ns), sr.device)
        check(L.wsr_speed_soft_counts(_p(hr), hr.shape[1], _p(sr), sr.shape[1], c, ns, B, X, Y, NZ, _p(ws), _p(out),
                                      _stream()), "speed_soft_counts")
        ctx.meta = (c, ns)
        ctx.save_for_backward(sr)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable  # (the kernel's result is no graph: a double backward is refused)
    def backward(ctx, g: Tensor):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        (sr,) = ctx.saved_tensors
        c, ns = ctx.meta
        B, C_, X, Y, NZ = sr.shape
        L = _lib.lib()
        gtab = g[1, :, :, :ns].to(torch.float32).contiguous()
        dsr = torch.empty((B, C_, X, Y, NZ), dtype=torch.float32, device=g.device)
        check(L.wsr_speed_soft_counts_bwd(_p(sr), C_, _p(gtab), c, ns, B, X, Y, NZ, _p(dsr), _stream()),
              "speed_soft_counts_bwd")
        return None, dsr, None, None


def speed_soft_counts_geometry(B: int, X: int, Y: int, NZ: int, speed_bins: int) -> Tuple[int, int, int, int]:
    """(columns per workgroup of the counting launch, its column ranges per (sample, source), elements per workgroup of
    the backward, its element ranges per sample) of ``wsr_speed_soft_counts`` at this shape"""
    geom = (C.c_int32 * 4)()
    check(_lib.lib().wsr_speed_soft_counts_geometry(int(B), int(X), int(Y), int(NZ), int(speed_bins), geom),
          "speed_soft_counts_geometry")
    return tuple(geom)


def speed_soft_counts(HR: Tensor, SR: Tensor, tables) -> Tensor:
    """The soft (linearly binned) histograms of the horizontal wind speed of ``HR`` and ``SR`` (B, C >= 2, X, Y, NZ;
    channels 0 and 1 are read, surplus ones never) -> float64 (2, B, NZ, NS + 1), source 0 HR, 1 SR, per sample and z
    level, under ``tables`` = ``distribution_loss.soft_tables(...)``: the definition of ``distribution_loss.py`` in fixed
    point, column NS the voxels whose squared speed is not finite, every row summing to X * Y exactly
    (``wsr_speed_soft_counts``).  Differentiable towards SR only (``wsr_speed_soft_counts_bwd``: one launch that
    recomputes the positions).  Integer counting, no floating-point atomics: the same bits on every call, forward and
    backward."""
    from . import distribution_loss

    _need_cuda(HR, SR)
    distribution_loss._check_pair(HR, SR, "speed_soft_counts")
    ns = int(tables.speed_bins)
    distribution_loss.check_parameters(tables.bin_width, ns, "speed_soft_counts")
    B, _, X, Y, NZ = HR.shape
    if (ns + 1) * NZ > DISTRIBUTION_LOSS_LDS_COUNTERS or B > 65535 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"speed_soft_counts: at most (speed_bins + 1) * NZ = {DISTRIBUTION_LOSS_LDS_COUNTERS}, 65535 "
                         f"samples and 2^31 - 1 voxels per sample, not speed_bins = {ns}, B = {B}, X = {X}, Y = {Y}, "
                         f"NZ = {NZ}")
    return _SpeedSoftCounts.apply(HR.detach().contiguous().float(), SR.contiguous().float(), float(tables.c), ns)


# ---------------------------------------------------------------------------------------------------------------------
# coarse-grained consistency loss of generator training ([CONSISTENCY_LOSS]; csrc/consistency_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------
CONSISTENCY_LOSS_LDS_FLOATS = 16384  # WSR_CONSISTENCY_LOSS_LDS_FLOATS


class _CoarseResidual(torch.autograd.Function):
    """``wsr_coarse_residual`` with ``wsr_coarse_residual_bwd`` as backward: r (B, 3, XL, YL, NZ) = D(fl(SR - HR));
    gradient flows only towards SR.  The operator is linear: nothing is saved but the shape and the two weight
    tables."""

    @staticmethod
    def forward(ctx, hr: Tensor, sr: Tensor, wx: Tensor, wy: Tensor, s: int, R: int):
        B, C_, X, Y, NZ = sr.shape
        L = _lib.lib()
        out = torch.empty((B, 3, wx.shape[0], wy.shape[0], NZ), dtype=torch.float32, device=sr.device)
        check(L.wsr_coarse_residual(_p(hr), hr.shape[1], _p(sr), C_, _p(wx), _p(wy), s, R, B, X, Y, NZ, _p(out),
                                    _stream()), "coarse_residual")
        ctx.meta = (s, R, (B, C_, X, Y, NZ), wx, wy)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable  # (the kernel's result is no graph: a double backward is refused)
    def backward(ctx, g: Tensor):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        s, R, (B, C_, X, Y, NZ), wx, wy = ctx.meta
        L = _lib.lib()
        gout = g.contiguous().float()
        dsr = torch.empty((B, C_, X, Y, NZ), dtype=torch.float32, device=g.device)
        check(L.wsr_coarse_residual_bwd(_p(gout), _p(wx), _p(wy), s, R, C_, B, X, Y, NZ, _p(dsr), _stream()),
              "coarse_residual_bwd")
        return None, dsr, None, None, None, None


def coarse_residual_geometry(s: int, R: int, B: int, X: int, Y: int, NZ: int) -> Tuple[int, ...]:
    """(XL, YL, coarse rows per forward workgroup, its runs, rows per backward workgroup, its runs, floats of LDS of a
    forward and of a backward workgroup) of ``wsr_coarse_residual`` at this shape"""
    geom = (C.c_int32 * 8)()
    check(_lib.lib().wsr_coarse_residual_geometry(int(s), int(R), int(B), int(X), int(Y), int(NZ), geom),
          "coarse_residual_geometry")
    return tuple(geom)


def coarse_residual(HR: Tensor, SR: Tensor, wx: Tensor, wy: Tensor, s: int) -> Tensor:
    """``r = D(fl(SR - HR))`` of ``HR`` and ``SR`` (B, C >= 3, X, Y, NZ; channels 0..2 are read, surplus ones never) ->
    fp32 (B, 3, ceil(X / s), ceil(Y / s), NZ): the coarse-graining of ``degradation.py`` with the fp32 device tables
    ``wx`` (XL, 2 R + 1) and ``wy`` (YL, 2 R + 1) of ``degradation.axis_weights``, as ``consistency_loss.py`` defines it
    (``wsr_coarse_residual``).  Differentiable towards SR only (``wsr_coarse_residual_bwd``: the adjoint, from the
    upstream gradient and the tables alone; zero in surplus channels).  No atomics: the same bits on every call, forward
    and backward."""
    from . import consistency_loss

    _need_cuda(HR, SR)
    consistency_loss._check_pair(HR, SR, "coarse_residual")
    B, _, X, Y, NZ = HR.shape
    s = int(s)
    for name, w, n in (("wx", wx, X), ("wy", wy, Y)):
        if (w.dim() != 2 or w.dtype != torch.float32 or w.device != HR.device or not w.is_contiguous()
                or w.shape[0] != -(-n // s) or w.shape[1] % 2 != 1 or w.shape[1] != wx.shape[1]):
            raise ValueError(f"coarse_residual wants {name} as a contiguous float32 ({-(-n // s)}, 2 R + 1) tensor on "
                             f"{HR.device}, got {w.dtype} {tuple(w.shape)} on {w.device}")
    R = (wx.shape[1] - 1) // 2
    geom = (C.c_int32 * 8)()
    rc = _lib.lib().wsr_coarse_residual_geometry(s, R, B, X, Y, NZ, geom)
    if rc != 0 or B * SR.shape[1] > 65535:
        raise ValueError(f"coarse_residual: a factor of 2 .. 32, a tap radius of at most 32, an LDS strip of at most "
                         f"{CONSISTENCY_LOSS_LDS_FLOATS} floats (about (2 R + s) NZ), B * C <= 65535, X <= 65535 and "
                         f"2^31 - 1 voxels per sample, not s = {s}, R = {R}, B = {B}, C = {SR.shape[1]}, X = {X}, "
                         f"Y = {Y}, NZ = {NZ}")
    return _CoarseResidual.apply(HR.detach().contiguous().float(), SR.contiguous().float(), wx, wy, s, R)


# ---------------------------------------------------------------------------------------------------------------------
# fractions skill score ([FSS]; csrc/fss.hip)
# ---------------------------------------------------------------------------------------------------------------------
FSS_TILE = 32  # FS_TILE of csrc/fss_kernels.h: the positions of a workgroup are FSS_TILE x FSS_TILE
_fss_tables: dict = {}


def fss_level_chunk(B: int, X: int, Y: int, NZ: int, scales) -> int:
    """The consecutive levels one workgroup of ``wsr_level_fss`` stages (``fs_geom`` of csrc/fss_kernels.h)"""
    S = FSS_TILE + (int(scales[-1]) - 1)
    CP = S if (S // 2) % 2 else S + 2
    zc = min(26624 // (S * CP + 2), 16, int(NZ))
    tiles = -(-int(X) // FSS_TILE) * -(-int(Y) // FSS_TILE)
    while True:
        nzc = -(-NZ // zc)
        ZC = -(-NZ // nzc)
        if ZC <= 2 or tiles * nzc * B >= 512:
            return ZC
        zc = (ZC + 1) // 2


def _fss_thr2_on(device, tables) -> Tensor:
    """``thr2`` of an ``fss.FssTables`` as an fp32 tensor on ``device``: uploaded once per (device, parameters)"""
    key = (device.index, tables.UVW_MAX, tuple(tables.thresholds))
    t = _fss_tables.get(key)
    if t is None:
        if len(_fss_tables) > 64:
            _fss_tables.clear()
        t = _fss_tables[key] = tables.thr2.float().to(device).contiguous()
    return t


def level_fss(HR: Tensor, SR: Tensor, TL: Optional[Tensor], tables, scales=(1, 3, 5, 9, 17, 33),
              out: Optional[Tensor] = None) -> Tensor:
    """The five sums of ``fss.py`` per sample, z level, threshold and neighbourhood -> float64 (B, NZ, NT, NN, 5): over
    every horizontal plane of ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ; channels 0 and 1 are read) the
    sums of the squared box-window event counts and of their squared differences, for the thresholds of ``tables`` =
    ``fss.fss_tables(...)`` and the odd neighbourhoods ``scales``.  ``TL`` None: zeros in entries 3 and 4.  Integer
    counting, no floating-point atomics: the same bits on every call, equal to ``fss.level_fss_reference``.  ``out``: a
    float64 (B, NZ, NT, NN, 5) slice to write into (``wsr_level_fss``)."""
    from . import fss

    _need_cuda(HR, SR, TL, out)
    B, X, Y, NZ = _same_grid("level_fss", HR, SR=SR, **({} if TL is None else {"TL": TL}))
    th = fss.check_thresholds(tables.thresholds, "level_fss")
    sc = fss.check_scales(scales, "level_fss")
    nt, nn = len(th), len(sc)
    if tables.thr2.numel() != nt:
        raise ValueError(f"level_fss wants a table of {nt} squared thresholds, got {tables.thr2.numel()}")
    if B > 65535 or X * Y >= 2 ** 31 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_fss: at most 65535 samples, 2^31 - 1 columns and 2^31 - 1 voxels per sample, not "
                         f"B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("level_fss", out, (B, NZ, nt, nn, 5), HR.device)
    L = _lib.lib()
    thr2 = _fss_thr2_on(HR.device, tables)
    ws = _workspace(L.wsr_level_fss_workspace_floats(B, X, Y, NZ, nt, nn, sc[-1]), HR.device)
    check(L.wsr_level_fss(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), 0 if TL is None else TL.shape[1], _p(thr2), nt,
                          (C.c_int32 * nn)(*sc), nn, B, X, Y, NZ, _p(out), _p(ws), _stream()), "level_fss")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hub-height wind resource ([HUB_HEIGHT]; csrc/hub_height.hip)
# ---------------------------------------------------------------------------------------------------------------------
HUB_HEIGHT_BLOCK = 256  # HH_BLOCK of csrc/hub_height_kernels.h
_hub_height_tables: dict = {}


def hub_height_columns_per_chunk(NZ: int, nh: int) -> int:
    """The consecutive columns one workgroup of ``wsr_hub_height`` stages at a time (``hh_geom`` of
    csrc/hub_height_kernels.h)"""
    return min(HUB_HEIGHT_BLOCK // int(NZ), HUB_HEIGHT_BLOCK // int(nh))


def _hub_height_arrays(device, tables):
    """The heights and the curve of a ``hub_height.HubHeightTables`` as the float arrays the entry reads during the call
    (they travel as kernel arguments): built once per (device, parameters)"""
    key = (device.index, tables.UVW_MAX, tuple(tables.heights_m), tuple(tables.curve_speeds), tuple(tables.curve_power))
    a = _hub_height_tables.get(key)
    if a is None:
        if len(_hub_height_tables) > 64:
            _hub_height_tables.clear()
        a = _hub_height_tables[key] = tuple((C.c_float * t.numel())(*t.float().tolist())
                                            for t in (tables.heights, tables.curve_v, tables.curve_p))
    return a


def hub_height(HR: Tensor, SR: Tensor, TL: Optional[Tensor], Z: Tensor, terrain: Tensor, tables, interp: str,
               with_columns: bool = False, out: Optional[Tensor] = None):
    """The 18 sums of ``hub_height.py`` per sample and height above ground -> float64 (B, NH, 18): every column of
    ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ; channels 0 and 1 are read) interpolated from its levels
    ``Z`` (B, 1, X, Y, NZ; raw altitude, ascending) above the ground ``terrain`` (X, Y) to the heights of ``tables`` =
    ``hub_height.hub_height_tables(...)``, ``interp`` ``linear`` or ``log``; sums over the columns the height lies
    inside.  ``TL`` None: zeros in its sums.  ``with_columns``: also the planes (B, NH, 7, X, Y) fp32 - V and P of HR,
    SR and TL and the validity - as a second result.  One pass, no atomics: the same bits on every call.  ``out``: a
    float64 (B, NH, 18) slice to write into (``wsr_hub_height``)."""
    from . import hub_height as hh

    _need_cuda(HR, SR, TL, Z, terrain, out)
    B, X, Y, NZ = _same_grid("hub_height", HR, SR=SR, **({} if TL is None else {"TL": TL}))
    _planar5("hub_height", "Z", Z)
    if tuple(Z.shape) != (B, 1, X, Y, NZ):
        raise ValueError(f"hub_height wants the levels Z as ({B}, 1, {X}, {Y}, {NZ}), got {tuple(Z.shape)}")
    if terrain.dtype != torch.float32 or tuple(terrain.shape) != (X, Y) or not terrain.is_contiguous():
        raise ValueError(f"hub_height wants terrain as a contiguous fp32 ({X}, {Y}) tensor, got {terrain.dtype} "
                         f"{tuple(terrain.shape)}")
    hh.check_interp(interp, "hub_height")
    hs = hh.check_heights(tables.heights_m, "hub_height")
    cs, _ = hh.check_curve(tables.curve_speeds, tables.curve_power, "hub_height")
    nh, nk = len(hs), len(cs)
    if tables.heights.numel() != nh or tables.curve_v.numel() != nk or tables.curve_p.numel() != nk:
        raise ValueError(f"hub_height wants tables of {nh} heights and {nk} knots, got {tables.heights.numel()}, "
                         f"{tables.curve_v.numel()} and {tables.curve_p.numel()}")
    if not 2 <= NZ <= hh.MAX_NZ:
        raise ValueError(f"hub_height stages whole columns in LDS: 2 .. {hh.MAX_NZ} levels, not {NZ}")
    if B > 65535 or X > 32768 or Y > 32768 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"hub_height: at most 65535 samples, 32768 rows and columns and 2^31 - 1 voxels per sample, not "
                         f"B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("hub_height", out, (B, nh, hh.NS), HR.device)
    cols = torch.empty((B, nh, hh.PLANES, X, Y), dtype=torch.float32, device=HR.device) if with_columns else None
    L = _lib.lib()
    heights, curve_v, curve_p = _hub_height_arrays(HR.device, tables)
    ws = _workspace(L.wsr_hub_height_workspace_floats(B, X, Y, NZ, nh), HR.device)
    check(L.wsr_hub_height(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), 0 if TL is None else TL.shape[1], _p(Z),
                           _p(terrain), heights, nh, curve_v, curve_p, nk, int(interp == "log"), B, X, Y, NZ, _p(ws),
                           _p(out), _p(cols), _stream()), "hub_height")
    return (out, cols) if with_columns else out


# ---------------------------------------------------------------------------------------------------------------------
# structure functions ([INCREMENTS]; csrc/increments.hip)
# ---------------------------------------------------------------------------------------------------------------------
INCREMENTS_TILE = 32  # INC_TILE of csrc/increments_kernels.h: the positions of a workgroup are INCREMENTS_TILE squared


def increments_level_chunk(NZ: int, separations) -> int:
    """The consecutive levels one workgroup of ``wsr_level_increments`` stages (``inc_geom`` of
    csrc/increments_kernels.h)"""
    S = INCREMENTS_TILE + int(separations[-1])
    zc = min(12288 // (S * S), 16, int(NZ))
    return -(-int(NZ) // -(-int(NZ) // zc))


def level_increments(HR: Tensor, SR: Tensor, TL: Optional[Tensor], separations=(1, 2, 4, 8, 16),
                     out: Optional[Tensor] = None) -> Tensor:
    """The sums of ``increments.py`` per sample, z level, source, separation, direction, kind and order -> float64
    (B, NZ, 3, R, 2, 3, 3): over every horizontal plane of ``HR``, ``SR`` and the baseline ``TL`` (B, C >= 3, X, Y, NZ;
    channels 0, 1 and 2 are read) the sums of the second, third and fourth powers of the increments of u, v and w over
    ``separations`` grid cells along x and along y.  ``TL`` None: zeros in its slices.  One pass, fp32 partial sums in a
    fixed order added in double, no atomics: the same bits on every call.  ``out``: a float64 (B, NZ, 3, R, 2, 3, 3)
    slice to write into (``wsr_level_increments``)."""
    from . import increments

    _need_cuda(HR, SR, TL, out)
    B, X, Y, NZ = _same_grid("level_increments", HR, SR=SR, **({} if TL is None else {"TL": TL}))
    sp = increments.check_separations(separations, "level_increments")
    nr = len(sp)
    if B > 65535 or X * Y >= 2 ** 31 or X * Y * NZ >= 2 ** 31:
        raise ValueError(f"level_increments: at most 65535 samples, 2^31 - 1 columns and 2^31 - 1 voxels per sample, not "
                         f"B = {B}, X = {X}, Y = {Y}, NZ = {NZ}")
    out = _sums_out("level_increments", out, (B, NZ, 3, nr, 2, 3, 3), HR.device)
    L = _lib.lib()
    arr = (C.c_int32 * nr)(*sp)
    ws = _workspace(L.wsr_level_increments_workspace_floats(B, X, Y, NZ, arr, nr), HR.device)
    check(L.wsr_level_increments(_p(HR), HR.shape[1], _p(SR), SR.shape[1], _p(TL), 0 if TL is None else TL.shape[1], arr,
                                 nr, B, X, Y, NZ, _p(ws), _p(out), _stream()), "level_increments")
    return out
