/*
 * windsr_hip.h - C ABI of the MI355X (gfx950) kernels behind the 3D-conv GAN
 * train-step hot path of GAN_SR_wind_field.
 *
 * The reference has no FFI layer for this path: its convolutions execute inside
 * PyTorch/ATen.  Each entry point below names the reference call site (file:line
 * under the reference tree) whose ATen work it replaces.  All pointers are DEVICE
 * pointers unless stated otherwise; the caller owns every buffer; kernels never
 * allocate, never synchronise and run on the hipStream_t passed as `stream`
 * (NULL = the default stream).  Every function returns 0 on success, a negative
 * WSR_E* code for bad arguments or the positive hipError_t of a failed launch.
 *
 * Activation layout ("NDHWC"): element (b, x, y, z, c) of a tensor with `ctot`
 * channels per voxel lives at ((((b*X + x)*Y + y)*Z + z)*ctot + c); a conv may
 * read/write a channel window [off, off+C) of such a buffer, which is how the
 * dense-block concatenations (torch_blocks.py:212-214, Generator_3D...py:228)
 * are done without a copy.  "Planar" tensors are the reference's own fp32
 * (B, C, X, Y, Z) contiguous tensors (network inputs / outputs).
 * Packed (compute) filter layout: [Cout][KX][KY][KZ][Cin] (Cin fastest), made by
 * wsr_pack_filter from the master weights, which keep nn.Conv3d's own logical
 * layout (Cout, Cin, KX, KY, KZ) so checkpoints / init / Adam are untouched.
 */
#ifndef WINDSR_HIP_H
#define WINDSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSR_ABI_VERSION 9

enum wsr_dtype { WSR_F32 = 0, WSR_BF16 = 1 };

enum wsr_error {
  WSR_OK = 0,
  WSR_EINVAL = -1,      /* inconsistent geometry / null pointer            */
  WSR_EUNSUPPORTED = -2 /* shape outside what the kernels were built for   */
};

/* Geometry of one 3-D convolution.  X/Y/Z naming follows the reference
 * (tensor dims 2,3,4; Z = vertical levels, contiguous, never up-scaled).
 *
 * Channel windows.  A kernel reads only whole 16-byte pieces (8 bf16 or 4 fp32
 * channels) that overlap the window it is given: [in_off, in_off+Cin) of the
 * input, [out_off, out_off+Cout) of dy in the gradients.  A piece may extend past
 * the window's last channel (Cout not a multiple of the piece); the buffer must
 * hold it, and those channels do not change the result.  Channels outside those
 * pieces are never read.  A kernel writes nothing outside [out_off, out_off+Cout)
 * of its output (the produced window: [in_off, in_off+Cin) of dx in an input
 * gradient), and nothing past the end of any tensor; fp32 planar outputs, packed
 * filter gradients and split copies are written only inside their extents.
 * tests/kernel_bounds.py (Guarded) checks the write rule bit for bit. */
typedef struct wsr_conv {
  int32_t dtype;                 /* wsr_dtype of activations and packed filters */
  int32_t B;                     /* batch                                         */
  int32_t Xi, Yi, Zi;            /* stored input extent                           */
  int32_t Xo, Yo, Zo;            /* output extent                                 */
  int32_t Cin, in_ctot, in_off;  /* input channel window                          */
  int32_t Cout, out_ctot, out_off;
  int32_t KX, KY, KZ;
  int32_t sx, sy, sz;            /* stride                                        */
  int32_t px, py, pz;            /* zero padding                                  */
  int32_t upsample_xy;           /* 1: input is read through nearest x(2,2,1)
                                    up-sampling (torch_blocks.py:345-347)        */
  /* Sub-pixel form of that up-sampling conv (tile entry points only; all zero = none).  Nearest x(2,2,1)
   * followed by a 3x3xKZ conv equals four 2x2xKZ convs on the un-sampled input, one per output parity (a, b):
   * 4/9 of the multiply-adds (filters from wsr_subpixel_fold).  lat = 2 marks such a parity conv: a same-size
   * conv (Xo = Xi, Yo = Yi, stride 1, low pads px / py, high pads K-1-p) whose OUTPUT voxel (x, y, z) is voxel
   * (2x + lat_ox, 2y + lat_oy, z) of a tensor of extent (2Xo, 2Yo, Zo) - y in the forward pass, dy in the
   * input / filter gradient.  lat_phases = 4 (wsr_conv3d_fwd_tile only): all four parities in ONE launch -
   * parity (a, b) runs with low pads (px - a, py - b), lattice offsets (a, b) and the fragment filter at
   * wfrag + (2a + b) * wsr_frag_filter_elems(Cout, Cin, taps).
   * The same machinery runs the INPUT gradient of the discriminator's stride-(2,2,s) 4x4x3 convs
   * (torch_blocks.py:372-521) as forward convs over dy: input voxel (2m + a, 2n + b, s*l + c) only meets the filter
   * taps of matching parity, so each parity class is a 2x2xKZ' conv on dy that writes its own lattice of dx (filters
   * from wsr_strided_parity_filters).  lat_mz = 2 puts the output on the z lattice lat_mz*z + lat_oz as well
   * (0 / 1: z is not strided); with lat set the conv is same-size along z too (Zo = Zi, low pad pz).
   * lat = 3 (filter-gradient entry points only) is the mirror image for the FILTER gradient of those down-sampling
   * convs: filter tap (2i + a, 2j + b, .) only meets input voxels of one parity, so the gradient of the taps of a
   * class is a stride-1 2x2xKZ' filter gradient in which the INPUT x is read on the lattice (2x + lat_ox,
   * 2y + lat_oy, lat_mz*z + lat_oz) of the stored tensor (Xi, Yi, Zi = the lattice's extents = Xo, Yo, Zo) and dy
   * is dense; wsr_strided_parity_unfold moves the class gradients to their taps of the master gradient.     */
  int32_t lat, lat_ox, lat_oy, lat_phases;
  int32_t lat_mz, lat_oz;
} wsr_conv_t;

struct wsr_lrelu_mask;
/* Fused epilogue:  v = conv (+ bias[c]);  v = lrelu(v, slope) if act;
 *                  v *= chan_scale[b*Cout + c] if chan_scale (Dropout3d mask);
 *                  y = alpha*v (+ beta*res[...,res_off + c] if res).          */
typedef struct wsr_epilogue {
  const float* bias;        /* [Cout] or NULL                                   */
  const float* chan_scale;  /* [B*Cout] or NULL                                 */
  const void* res;          /* NDHWC tensor of `dtype`, or NULL                 */
  int32_t res_ctot, res_off;
  float alpha, beta;
  int32_t act;              /* 0 none, 1 leaky-relu, 2 leaky-relu AFTER the residual: y = alpha*lrelu(acc + bias +
                               beta*res) (tile kernels only) - the second stage of a split dense-block conv whose
                               partial sums over the block input are already in `res` (= the output window) */
  float slope;
  int32_t out_planar;       /* 1: y is fp32 planar (B, Cout, Xo, Yo, Zo)        */
  int32_t act_c1;           /* > 0 (tile kernels only): bias and activation apply to channels < act_c1 only, the rest
                               are stored as raw sums - the first stage of a split dense-block conv            */
  /* ABI 6 - split-reduction workspace of THIS call (tile entry point only; NULL / 0 = never split): device memory the
   * caller owns.  With it, launches that would otherwise run on a few workgroups with a long reduction (the deep
   * layers of the discriminator, Discriminator_3D.py:66-169: 128..1024 voxels x 256..512 channels x 27..48 taps)
   * split the reduction channels over up to 256 workgroups; the fp32 partial sums go through the workspace and a
   * second launch on the same stream adds them in index order (bit-reproducible) and applies the epilogue.  Launches
   * that may run concurrently (different streams / threads) take different workspaces - the library keeps no
   * state between calls.  Results do not depend on its presence beyond fp32 summation order.                 */
  void* ws;
  int64_t ws_bytes;
  const void* res2;         /* second residual, y += beta2*res2[..., res2_off + c] (streaming 1x1x1 kernel only,
                               WSR_EUNSUPPORTED elsewhere): the last LFF of an RRDB adds the dense block's and the
                               RRDB's shortcut at once (torch_blocks.py:290,330)                                */
  int32_t res2_ctot, res2_off;
  float beta2;
  /* ABI 6 (tile entry point only, NULL = none): the LeakyReLU-backward mask of wsr_conv3d_dgrad_tile on a FORWARD-form
   * launch - the parity input gradients of the discriminator's strided convs are forward convs over dy (wsr_conv_t.lat):
   * with the mask of the layer below (Discriminator_3D.py:67-75: conv + LeakyReLU, no BatchNorm) in their epilogue
   * that layer's leaky_relu_backward needs no pass of its own.  bf16, <= 32 or 65..224 produced channels
   * (WSR_EUNSUPPORTED otherwise).                                                                           */
  const struct wsr_lrelu_mask* mask;
  /* ABI 8 (tile entry point only, NULL = none): the conv's input is the channel concatenation of TWO tensors
   * (torch.cat((x, Zf), 1) of Generator_3D_Resnet_ESRGAN.py:228 in front of hr_convs[0]) WITHOUT the concatenated copy
   * and without one producer writing 32-byte pieces into the other's 288-byte voxel rows (partial cache lines: 1.6 x
   * the bytes at the memory side): reduction channels [0, in2_c0) of the conv are read from `x` (window in_off of
   * in_ctot channels, as always), channels [in2_c0, Cin) from channels [0, Cin - in2_c0) of `in2` (same extents,
   * in2_ctot channels per voxel, same dtype).  in2_c0 must be a multiple of the kernel's reduction chunk (16 bf16 /
   * 8 fp32 channels).  Only the 512-voxel 129..144-output tile instantiations (the 5x5x5 144 -> 144 conv) carry it:
   * WSR_EUNSUPPORTED elsewhere - ask wsr_conv_split_ok first and keep the concatenated buffer when it says no. */
  const void* in2;
  int32_t in2_ctot, in2_c0;
} wsr_epilogue_t;

/* 1 when wsr_conv3d_fwd_tile (wsr_epilogue_t.in2), wsr_conv3d_dgrad_tile (wsr_dgrad_opts_t.dx2) and
 * wsr_conv3d_wgrad_parts_x2 all take this conv with its input channels split at `c0` into two tensors, else 0
 * (host-side query, no launch).                                                                              */
int wsr_conv_split_ok(const wsr_conv_t* c, int32_t c0);

int wsr_abi_version(void);
const char* wsr_error_string(int code);
/* The WSR_* environment switches (tuning / A-B aids, none needed for normal use) are cached per call site; a process
 * that changes its environment at run time calls this to have them read again.  Always returns 0. */
int wsr_reload_env(void);

/* ---- convolution ------------------------------------------------------------
 * aten::conv3d forward of nn.Conv3d (torch_blocks.py:17,278; Generator_3D...py:105)
 * + the LeakyReLU / cat / residual / Dropout3d / Upsample ops fused around it
 * (torch_blocks.py:35,214,290,330,46,347; Generator_3D...py:104,228).          */
int wsr_conv3d_fwd(const wsr_conv_t* c, const void* x, const void* w, void* y,
                   const wsr_epilogue_t* ep, void* stream);

/* aten::convolution_backward, input gradient.  `wt` is the filter re-packed as
 * [Cin][KX][KY][KZ][Cout] (wsr_pack_filter with transpose=1).  dx gets channel
 * window [in_off, in_off+Cin) of an `in_ctot` buffer at the conv's *stored*
 * input resolution unless upsample_xy, in which case dx is at 2Xi x 2Yi and
 * wsr_upsample2_bwd folds it.  dx = alpha*result (+ dx if accumulate; the tile entry point also takes
 * accumulate = n > 1: only the first n produced channels are added to).  dx_planar=1: dx
 * is an fp32 planar (B, Cin, X, Y, Z) tensor (gradient w.r.t. a network input).  */
int wsr_conv3d_dgrad(const wsr_conv_t* c, const void* dy, const void* wt, void* dx, float alpha,
                     int accumulate, int dx_planar, void* stream);

/* ---- LDS halo-tile path (bf16, stride 1) ------------------------------------
 * (bf16; fp32 as well for stride-1 convs - ABI 6: the same kernel on 16-byte pieces of 4 channels, exact fp32
 * products and sums through v_mfma_f32_16x16x4_f32; 1x1x1 and strided fp32 convs return WSR_EUNSUPPORTED.)
 * Same contracts as wsr_conv3d_fwd / wsr_conv3d_dgrad, but the activation tile
 * (with halo) is staged in LDS once per channel chunk and re-used by every tap,
 * and the filter comes in MFMA-fragment order from wsr_pack_filter_frag
 * (transpose = 0 for the forward pass, 1 for the input gradient; element count
 * from wsr_frag_filter_elems(rows, reduction channels, taps)).  Return
 * WSR_EUNSUPPORTED for shapes outside the tile kernels (strided convs, fp32):
 * the caller then uses the generic entry points above.                          */
int wsr_conv3d_fwd_tile(const wsr_conv_t* c, const void* x, const void* wfrag, void* y,
                        const wsr_epilogue_t* ep, void* stream);
/* leaky_relu_backward folded into the input-gradient epilogue (optional, NULL = none): after the
 * accumulation, produced channels [c0, c1) are multiplied by (y > 0 ? 1 : slope), y = channel
 * y_off + (c - c0) of the saved forward output at the same voxel (NDHWC bf16, y_ctot channels).  This is
 * the LeakyReLU of the layer whose OUTPUT gradient those channels are (dense-block growth channels). */
typedef struct wsr_lrelu_mask {
  const void* y;
  int32_t y_ctot, y_off, c0, c1;
  float slope;
  const float* chan_scale;  /* optional [B][Cin]: every produced channel is also multiplied by it - the
                               Dropout3d keep factors of that layer (Generator_3D...py:104), backward       */
} wsr_lrelu_mask_t;
/* ABI 6 - optional extras of the tile input gradient (NULL = none of them):
 *   acc_src : with `accumulate`, the tensor whose values are added (dx's own layout: in_ctot channels per voxel, the
 *             window at in_off) - NULL = dx itself.  Lets the running gradient of a residual chain move from one
 *             buffer to the next instead of being updated in place, so that a filter-gradient launch on another
 *             stream may still read the previous buffer (the dense blocks' backward pass, torch_blocks.py:256-290).
 *   ws / ws_bytes : split-reduction workspace of this call, as wsr_epilogue_t.ws.                            */
typedef struct wsr_dgrad_opts {
  const void* acc_src;
  void* ws;
  int64_t ws_bytes;
  /* The running gradient of a residual-in-residual block (torch_blocks.py:293-330: out = x + scale * chain(x)) without
   * copy / add passes - streaming 1x1x1 kernel only (WSR_EUNSUPPORTED elsewhere when res2 is set):
   *   acc_beta : weight of the accumulated values (0 = 1): dx = alpha * conv^T(dy) + acc_beta * acc_src (first n channels);
   *   res2     : a second tensor added to the same first n channels, dx += beta2 * res2[..., res2_off + c] - the gradient
   *              of the RRDB's output, which joins the chain's gradient where the chain ends.                     */
  float acc_beta;
  float beta2;
  const void* res2;
  int32_t res2_ctot, res2_off;
  /* ABI 8 - the mirror image of wsr_epilogue_t.in2: the input gradient of a conv over a two-tensor concatenation is
   * written to TWO tensors - produced channels [0, dx2_c0) to dx (window in_off of in_ctot, as always), channels
   * [dx2_c0, Cin) to channels [0, Cin - dx2_c0) of `dx2` (dx2_ctot channels per voxel).  No accumulate / mask /
   * planar output with it; same instantiations as in2 (WSR_EUNSUPPORTED elsewhere).                         */
  void* dx2;
  int32_t dx2_ctot, dx2_c0;
} wsr_dgrad_opts_t;
int wsr_conv3d_dgrad_tile(const wsr_conv_t* c, const void* dy, const void* wfrag_t, void* dx, float alpha,
                          int accumulate, int dx_planar, const wsr_lrelu_mask_t* mask, const wsr_dgrad_opts_t* opts,
                          void* stream);
/* Diagnostic (additive export): the launch plan of the calling thread's most recent halo-tile launch through the two
 * entry points above, as 8 values {TX, TY, TZ, NTW, ngroups, ksplit, xbufs, TS}: spatial tile, output-channel width of a
 * workgroup in 16-wide n-tiles, channel groups, split count of the reduction (1 = single pass), activation buffers in
 * LDS, K-steps per weight stage.  All zero before the first such launch; a call that was declined, or served by another
 * kernel (streaming 1x1x1, sliding-window), leaves the record as it was.  For tests that assert which instantiation a
 * case reached: no launch of the library reads the record.  Returns 0, WSR_EINVAL for a null pointer.           */
int wsr_last_tile_plan(int32_t* plan8);
/* Diagnostic (additive export): which instantiation of the halo-tile kernel served that launch, as 10 values
 * {WM, WN, TM, TN, TPK, MASK, F32, WK, SIMPLE, seq}: wave rows and columns of a workgroup, 16-row m-tiles and 16-channel
 * n-tiles per wave, taps per K-step, LeakyReLU-backward mask compiled in, fp32 operands, waves that share the K-steps of a
 * stage, the form with the general run-time switches folded away; `seq` counts the calling thread's halo-tile launches (a
 * split-reduction launch counts once).  Same rules as wsr_last_tile_plan: a declined call or one served by another kernel
 * changes nothing, no launch reads the record.  Returns 0, WSR_EINVAL for a null pointer.                       */
int wsr_last_tile_instantiation(int32_t* inst10);
/* ABI 6: `dtype` (wsr_dtype) of the fragment filter - bf16, or fp32 for the fp32 tile kernels (stride-1 convs in the
 * reference's own arithmetic; the 16-byte pieces then hold 4 channels instead of 8).                        */
int64_t wsr_frag_filter_elems(int32_t rows, int32_t red, int32_t taps, int32_t dtype);
int wsr_pack_filter_frag(const float* w, void* out, int32_t Cout, int32_t Cin, int32_t KX, int32_t KY, int32_t KZ,
                         int32_t transpose, int32_t dtype, void* stream);
/* The same for many filters in ONE launch (every filter changes at each optimizer step, and a
 * generator has ~300 of them): `jobs_dev` is a DEVICE array of n_jobs records.                    */
typedef struct wsr_pack_job {
  const float* w;  /* master (Cout, Cin, KX, KY, KZ) fp32 */
  void* out;       /* wsr_frag_filter_elems(...) bf16 elements */
  int32_t Cout, Cin, KX, KY, KZ, transpose;
  /* Sub-block of a stacked filter of a residual dense block (torch_blocks.py:256-267), red_total > 0: the
   * destination is the filter of ONE virtual conv with rows_total rows and red_total reduction channels,
   * several jobs fill disjoint parts of it.
   *   transpose = 1 (stacked input gradient): this conv's output channels are reduction channels
   *     [red_off, red_off + Cout) and its input channels [c_lo, c_lo + c_n) the rows (rows_total = c_n);
   *   transpose = 0 (split forward conv): this conv's output channels are rows [row_off, row_off + Cout) and
   *     its input channels [c_lo, c_lo + c_n) the whole reduction axis (red_total = c_n, red_off = 0).
   * Offsets and extents that index whole chunks / n-tiles must be multiples of 16 (fp32: 8).  red_total = 0: a plain
   * filter (the fields above).                                                                        */
  int32_t c_lo, c_n, red_off, red_total, row_off, rows_total;
} wsr_pack_job_t;
int wsr_pack_filter_frag_multi(const wsr_pack_job_t* jobs_dev, int32_t n_jobs, int32_t dtype, void* stream);

/* aten::convolution_backward, filter gradient: dw[Cout][taps][Cin] fp32 (packed
 * order) is ACCUMULATED into (caller zeroes it when a fresh gradient is wanted;
 * wsr_unpack_wgrad moves it to the master layout).                             */
int wsr_conv3d_wgrad(const wsr_conv_t* c, const void* x, const void* dy, float* dw, void* stream);
/* Deterministic (atomic-free, bit-reproducible) form of the same gradient.  The kernels split the reduction
 * over the voxels between workgroups / waves; wsr_conv3d_wgrad adds the partial sums into one buffer with float
 * atomics (order varies from launch to launch), here split s STORES its sums to parts + s*part_stride (each a
 * packed [Cout][taps][Cin] image; nothing has to be zeroed) and wsr_unpack_wgrad_reduce_multi adds the copies
 * in index order while moving them to the master layout.  n_parts must be the value wsr_conv3d_wgrad_nparts
 * reports for the same geometry (host-side query, no launch); tri_base / tri_step > 0: the stacked dense-block
 * form of wsr_conv3d_wgrad_tri.                                                                             */
int wsr_conv3d_wgrad_nparts(const wsr_conv_t* c, int32_t tri_base, int32_t tri_step, int32_t* n_parts);
int wsr_conv3d_wgrad_parts(const wsr_conv_t* c, const void* x, const void* dy, float* parts, int64_t part_stride,
                           int32_t n_parts, int32_t tri_base, int32_t tri_step, void* stream);
/* ABI 8 - the same with the conv's input split over two tensors (wsr_epilogue_t.in2): input channels [x2_c0, Cin)
 * are read from channels [0, Cin - x2_c0) of `x2` (x2_ctot channels per voxel); x2_c0 a multiple of 32.  The
 * packed [Cout][taps][Cin] image is the un-split conv's.  bf16 / fp32 tile filter-gradient kernels, stride 1, no
 * lattice (WSR_EUNSUPPORTED otherwise).                                                                        */
int wsr_conv3d_wgrad_parts_x2(const wsr_conv_t* c, const void* x, const void* x2, int32_t x2_ctot, int32_t x2_c0,
                              const void* dy, float* parts, int64_t part_stride, int32_t n_parts, void* stream);
/* The four xy-parity classes of one lattice-form filter gradient in ONE launch (lat = 2: the parity convs of a
 * sub-pixel up-sampling conv; lat = 3: one z-class of a strided conv in parity form; the classes share the tap
 * shape).  `c` describes class (0, 0): lat_ox = lat_oy = 0, (px, py) >= 1 its low pads ((1, 1) for lat = 3),
 * lat_phases 0 or 4.  Class (a, b) runs exactly as wsr_conv3d_wgrad_parts would with low pads (px - a, py - b) and
 * lattice offsets (a, b) (lat = 2) or (px - a, py - b) (lat = 3), and split s of it STORES its sums to
 * parts + (2a + b)*class_stride + s*part_stride.  n_parts = splits PER CLASS as wsr_conv3d_wgrad_nparts_lat4
 * reports them; a per-class launch with the same number of splits gives the same bits.  WSR_EUNSUPPORTED: the
 * shape does not fit the merged form - launch the classes one by one.                                           */
int wsr_conv3d_wgrad_nparts_lat4(const wsr_conv_t* c, int32_t* n_parts);
int wsr_conv3d_wgrad_parts_lat4(const wsr_conv_t* c, const void* x, const void* dy, float* parts, int64_t part_stride,
                                int64_t class_stride, int32_t n_parts, void* stream);
/* wsr_conv3d_wgrad_parts for a 1x1x1 conv with a bias (the generator's LFF convs), the bias gradient's partial sums
 * taken in the same launch: split s also STORES sum_v dy[v, n] to bias_parts[s*Cout + n] (n_parts rows of Cout
 * floats; wsr_unpack_wgrad_reduce_multi adds the rows in order as a job of one output row).  The filter gradient is
 * wsr_conv3d_wgrad_parts' bit for bit.  n_parts as wsr_conv3d_wgrad_nparts_bias reports it (the same number as
 * wsr_conv3d_wgrad_nparts); WSR_EUNSUPPORTED from either: not the bf16 1x1x1 tile kernel's shape (Cout, Cin >= 64,
 * stride 1, no lattice) - use wsr_conv3d_wgrad_parts and wsr_chan_sum_partials.                                    */
int wsr_conv3d_wgrad_nparts_bias(const wsr_conv_t* c, int32_t* n_parts);
int wsr_conv3d_wgrad_parts_bias(const wsr_conv_t* c, const void* x, const void* dy, float* parts, int64_t part_stride,
                                int32_t n_parts, float* bias_parts, void* stream);
/* Filter gradients of ALL growth convs of a residual dense block in one launch
 * (torch_blocks.py:256-267: conv i reads channels [0, tri_base + i*tri_step) of the
 * dense buffer and writes tri_step channels).  c describes the stacked conv: Cin =
 * the widest input window, Cout = n_convs*tri_step, dy = the stacked output
 * gradients.  Row n of dw belongs to conv n / tri_step; its entries with
 * c >= tri_base + (n / tri_step)*tri_step are unspecified.  bf16, stride 1 only
 * (WSR_EUNSUPPORTED otherwise).                                                 */
int wsr_conv3d_wgrad_tri(const wsr_conv_t* c, const void* x, const void* dy, float* dw, int32_t tri_base,
                         int32_t tri_step, void* stream);

/* ---- filter packing ----------------------------------------------------------
 * master fp32 (Cout, Cin, KX, KY, KZ) contiguous -> compute copy of `dtype`:
 *   transpose=0: [Cout][taps][kpad]  (channels >= Cin zero-filled)
 *   transpose=1: [Cin][taps][kpad]   (channels >= Cout zero-filled; dgrad operand)
 * kpad lets 1/3/4-channel tensors (LR fields, terrain height, D input, SR output:
 * Generator_3D...py:78-85,105-110,120-127; Discriminator_3D.py:67) use the
 * 16-byte-piece MFMA path.                                                     */
int wsr_pack_filter(const float* w, void* out, int32_t dtype, int32_t Cout, int32_t taps,
                    int32_t Cin, int32_t transpose, int32_t kpad, void* stream);
/* Filter gradient back to the master layout:
 * dst (Cout, Cin, taps) = scale * src [Cout][taps][kpad] (+ dst if accumulate).  */
int wsr_unpack_wgrad(const float* src, float* dst, int32_t Cout, int32_t taps, int32_t Cin,
                     int32_t kpad, float scale, int32_t accumulate, void* stream);

/* The same for many filter gradients in ONE launch; `jobs_dev` is a DEVICE array of n_jobs records. */
typedef struct wsr_unpack_job {
  const float* src; /* packed [Cout][taps][kpad] */
  float* dst;       /* master (Cout, Cin, taps)   */
  int32_t Cout, taps, Cin, kpad;
  float scale;
  int32_t accumulate;
  int32_t n_parts;     /* wsr_unpack_wgrad_reduce_multi: split copies to sum (src + s*part_stride), else unused */
  int32_t reserved;
  int64_t part_stride; /* elements between two copies */
} wsr_unpack_job_t;
int wsr_unpack_wgrad_multi(const wsr_unpack_job_t* jobs_dev, int32_t n_jobs, void* stream);
/* The same with the ordered sum over the split copies of wsr_conv3d_wgrad_parts folded in (taps <= 128). */
int wsr_unpack_wgrad_reduce_multi(const wsr_unpack_job_t* jobs_dev, int32_t n_jobs, void* stream);

/* ---- elementwise / normalisation ---------------------------------------------
 * leaky_relu_backward from the saved OUTPUT sign, in place on a channel window
 * (torch_blocks.py:35 autograd):  g *= (y > 0 ? 1 : slope), optionally also
 * times the Dropout3d keep factor chan_scale[b*C + c] (Generator_3D...py:104).  */
int wsr_lrelu_bwd_inplace(void* g, int32_t g_ctot, int32_t g_off, const void* y, int32_t y_ctot,
                          int32_t y_off, int32_t C, int64_t nvox, float slope,
                          const float* chan_scale, int64_t vox_per_b, int32_t dtype, void* stream);
/* copy / axpby on channel windows: dst = alpha*src (+ beta*dst)                */
int wsr_chan_axpby(void* dst, int32_t d_ctot, int32_t d_off, const void* src, int32_t s_ctot,
                   int32_t s_off, int32_t C, int64_t nvox, float alpha, float beta, int32_t dtype,
                   void* stream);
/* Bias gradient of a conv (aten::convolution_backward's third output; the LFF bias of a residual dense
 * block, torch_blocks.py:278): out[c] = scale * sum over voxels of x[v, x_off + c], fp32.  `out` is
 * overwritten.  Two passes (per-workgroup partial rows, then a column sum: float atomics on C addresses
 * serialise) through `partials`, a caller-owned scratch of WSR_CHAN_SUM_ROWS * C floats.  C must be a
 * multiple of 4 and <= 1024 (WSR_EUNSUPPORTED otherwise).                                          */
#define WSR_CHAN_SUM_ROWS 512
int wsr_chan_sum(const void* x, int32_t x_ctot, int32_t x_off, int32_t C, int64_t nvox, float scale, float* out,
                 float* partials, int32_t dtype, void* stream);
/* First pass of wsr_chan_sum alone: row r of `partials` (wsr_chan_sum_rows(C, nvox) rows of C floats, caller-owned)
 * receives the sums of workgroup r.  The rows can then be added by wsr_unpack_wgrad_reduce_multi together with the
 * filter gradients of the same backward pass (job: Cout = 1, taps = 1, Cin = kpad = C, n_parts = rows, part_stride =
 * C) - one launch less per bias gradient (48 per backward pass of the generator).                          */
int wsr_chan_sum_rows(int32_t C, int64_t nvox);
int wsr_chan_sum_partials(const void* x, int32_t x_ctot, int32_t x_off, int32_t C, int64_t nvox, float* partials,
                          int32_t dtype, void* stream);
/* backward of nearest x(2,2,1) up-sampling: dx[b,x,y,z,c] = sum of the 4 dy    */
int wsr_upsample2_bwd(const void* dy, void* dx, int32_t B, int32_t Xi, int32_t Yi, int32_t Zi,
                      int32_t C, int32_t dtype, void* stream);
/* Filters of the sub-pixel form of an up-sampling conv (wsr_conv_t.lat): master fp32 w (n, 3, 3, KZ), n =
 * Cout*Cin, -> wp (4, n, 2, 2, KZ), parity (a, b) at index 2a + b:
 *   wp[2a+b][f][i][j][kz] = sum over kx in S_a(i), ky in S_b(j) of w[f][kx][ky][kz],
 *   S_0(0) = {0}, S_0(1) = {1, 2} (input offsets -1, 0);  S_1(0) = {0, 1}, S_1(1) = {2} (offsets 0, +1)
 * - the taps of the 3x3 filter that read the same un-sampled voxel, summed in fp32 (torch_blocks.py:345-347:
 * nn.Upsample(scale_factor=(2,2,1), mode="nearest") in front of the conv).  _unfold is the adjoint:
 * dw[f][kx][ky][kz] = sum over (a, b, i, j) with kx in S_a(i), ky in S_b(j) of dwp[2a+b][f][i][j][kz]
 * (dw is overwritten).                                                                                  */
/* Parity filters of the input gradient of a stride-(2, 2, sz) conv with a 4x4x3 filter and padding 1 (the
 * discriminator's down-sampling convs): w (Cout, Cin, 4, 4, 3) fp32 -> out (4, Cin, Cout, 2, 2, KZp), parity (a, b)
 * at index 2a + b, for z parity class zc:
 *   out[2a+b][ci][co][i][j][t] = w[co][ci][kx(a,i)][ky(b,j)][kz(t)],  k(0,.) = {3, 1} (dy offsets -1, 0),
 *   k(1,.) = {2, 0} (offsets 0, +1);  sz = 1: KZp = 3, kz(t) = 2 - t (offsets -1, 0, +1);  sz = 2: zc = 0: KZp = 1,
 *   kz = 1 (offset 0); zc = 1: KZp = 2, kz = {2, 0} (offsets 0, +1).
 * Rows are the conv's INPUT channels: the result is the filter of a forward conv over dy (wsr_conv_t.lat).   */
int wsr_strided_parity_filters(const float* w, float* out, int32_t Cout, int32_t Cin, int32_t sz, int32_t zc,
                               void* stream);
/* Filter gradient of such a conv in parity form (wsr_conv_t.lat = 3): class (a, b) of the taps (2i + a, 2j + b) is a
 * (2,2,KZp) stride-1 filter gradient over the input sub-lattice (1 - a, 1 - b[, z class]) with low pads (1 - a, 1 - b);
 * sz = 1: KZp = 3, kz = kk, pad 1;  sz = 2: zc = 0: KZp = 1, kz = 1, z lattice offset 0, pad 0;  zc = 1: KZp = 2,
 * kz = 2 kk, z lattice offset 1, pad 1.  dwp (4, n = Cout*Cin, 2, 2, KZp) fp32, class (a, b) at index 2a + b ->
 * dw[f][2i + a][2j + b][kz] of the master gradient (n, 4, 4, 3); every element is written by exactly one class.   */
int wsr_strided_parity_unfold(const float* dwp, float* dw, int64_t n, int32_t sz, int32_t zc, void* stream);
int wsr_subpixel_fold(const float* w, float* wp, int64_t n, int32_t KZ, void* stream);
int wsr_subpixel_unfold(const float* dwp, float* dw, int64_t n, int32_t KZ, void* stream);
/* planar fp32 (B,C,X,Y,Z) <-> NDHWC `dtype` window; c_fill >= C channels are
 * written, those beyond C with zeros                                           */
int wsr_planar_to_ndhwc(const float* src, void* dst, int32_t B, int32_t C, int64_t vox_per_b,
                        int32_t d_ctot, int32_t d_off, int32_t c_fill, int32_t dtype, void* stream);
int wsr_ndhwc_to_planar(const void* src, float* dst, int32_t B, int32_t C, int64_t vox_per_b,
                        int32_t s_ctot, int32_t s_off, int32_t dtype, void* stream);

/* Wind-field derivatives of the physics losses (process_data.py:273-313 of the reference:
 * calculate_gradient_of_wind_field = torch.gradient over x, y with coordinate spacing + calculate_div_z on
 * the terrain-following levels): out[b, 3*a + c] = d f[b, c] / d axis_a, a = 0 (x), 1 (y), 2 (z), planar
 * fp32 (B, ., X, Y, Z).  Interior points use the second-order three-point stencil for non-uniform
 * spacing, the two ends one-sided first differences.  xs[X], ys[Y] are the horizontal coordinates, zc
 * (B, 1, X, Y, Z) the height of every level.  _bwd applies the adjoint (transpose) of that linear map to
 * g (B, 9, X, Y, Z): the gradient w.r.t. f.                                                        */
int wsr_wind_gradient(const float* f, const float* xs, const float* ys, const float* zc, float* out, int32_t B,
                      int32_t X, int32_t Y, int32_t Z, void* stream);
int wsr_wind_gradient_bwd(const float* g, const float* xs, const float* ys, const float* zc, float* df, int32_t B,
                          int32_t X, int32_t Y, int32_t Z, void* stream);

/* nn.Linear forward for a handful of rows and a very long reduction (the discriminator's first classifier layer,
 * Discriminator_3D.py:171-175: 1..8 samples x 100 outputs x 256*4*4*z features): y (B, N) = x (B, K) w^T (N, K) +
 * bias, fp32, one workgroup per output row streaming its weight row once -> aten::addmm.  B <= 8 and K a multiple
 * of 4 (WSR_EUNSUPPORTED otherwise: the caller uses the library GEMM).  Bit-reproducible.                  */
int wsr_linear_rows(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t N, int64_t K,
                    void* stream);
/* out[c] = sum over b, v of src[b][c][v] for a planar fp32 (B, C, V) tensor - the bias gradient of a conv whose
 * output gradient arrives planar (hr_convs.2, Generator_3D_Resnet_ESRGAN.py:105-110; aten: sum.dim_IntList).
 * Two passes through `partials` (WSR_CHAN_SUM_ROWS * C floats), no atomics.                                  */
int wsr_plane_sum(const float* src, int32_t B, int32_t C, int64_t V, float* out, float* partials, void* stream);

/* Fused content losses of the generator (reference GAN_models/wind_field_GAN_3D.py:377-432: pixel L1 / L2,
 * xy-gradient, z-gradient, divergence and xy-divergence MSE terms over the Jacobians of
 * calculate_gradient_of_wind_field, normalised by get_norm_factors_of_gradients :773-814).  Every normaliser is
 * a scalar, so one pass over hr, sr (B,3,X,Y,Z) and zc (B,1,X,Y,Z), planar fp32, yields everything:
 *   stats[0..5]  = sum (J_sr - J_hr)^2 over channels 0..5 | over channels 6..8 | sum (div3_hr - div3_sr)^2 |
 *                  sum (div2_hr - div2_sr)^2 | sum |hr - sr| | sum (hr - sr)^2
 *   stats[6..13] = max |J[:6]|, max J[6:] (signed, as the reference), max |div3|, max |div2| of hr, then of sr
 * (maxima propagate NaN like torch.max).  workspace: wsr_physics_loss_workspace_floats() floats; the reduction
 * is two-pass and atomic-free (bit-reproducible).  _bwd: coef[6] (DEVICE array) = d loss / d stats[0..5];
 * residual = scratch of B*9*X*Y*Z floats; dsr (B,3,X,Y,Z) = d loss / d sr (overwritten).                  */
int64_t wsr_physics_loss_workspace_floats(void);
int wsr_physics_loss_stats(const float* hr, const float* sr, const float* xs, const float* ys, const float* zc,
                           float* stats, float* workspace, int32_t B, int32_t X, int32_t Y, int32_t Z, void* stream);
int wsr_physics_loss_bwd(const float* hr, const float* sr, const float* xs, const float* ys, const float* zc,
                         const float* coef, float* residual, float* dsr, int32_t B, int32_t X, int32_t Y, int32_t Z,
                         void* stream);

/* z-folded form of a conv with very few output channels (the last conv of the generator, 144 -> 3,
 * 5x5x5, Generator_3D_Resnet_ESRGAN.py:120-127): the KZ taps along z become output channels of a
 * (KX,KY,1) conv with C*KZ outputs - 15 instead of 3 of the 16 columns of an MFMA tile do work, a fifth
 * of the K-steps - and the z taps are summed afterwards:
 *   fold  : y[b,c,p,z]        = bias[c] + sum_kz t[b, c*KZ+kz, p, z + kz - pz]      (planar fp32, p = x*Y+y)
 *   unfold: d[b,p,z, c*KZ+kz] = g[b,c,p, z - kz + pz]   (its adjoint: planar fp32 -> NDHWC `dtype`;
 *           channels [C*KZ, c_fill) are written as zeros); out-of-range z contributes 0.          */
int wsr_zfold(const float* t, float* y, const float* bias, int32_t B, int32_t C, int32_t KZ, int32_t pz,
              int64_t planes, int32_t Z, void* stream);
int wsr_zunfold(const float* g, void* d, int32_t B, int32_t C, int32_t KZ, int32_t pz, int64_t planes, int32_t Z,
                int32_t d_ctot, int32_t d_off, int32_t c_fill, int32_t dtype, void* stream);

/* BatchNorm3d (torch_blocks.py:20-25) on NDHWC tensors, fp32 statistics.
 * stats: sums[2*C] = {sum d, sum d^2}, d = x - shift[c] (shift NULL = 0).  Two calls - shift 0, then
 * shift = mean - give a cancellation-free variance.  `partials` = caller-owned scratch of
 * WSR_CHAN_SUM_ROWS * 2C floats: with it (and C a multiple of 4, <= 512) the reduction is vectorised,
 * atomic-free and OVERWRITES sums; with NULL the scalar kernel ADDS to sums (caller zeroes them).     */
int wsr_bn_stats(const void* x, int32_t C, int64_t nvox, const float* shift, float* sums, float* partials,
                 int32_t dtype, void* stream);
/* The small per-channel steps between the two statistics passes, fused (they are launch-latency bound):
 * mean = sums[0:C] / count;  then from the shifted sums: biased variance, invstd = rsqrt(var + eps) and the
 * nn.BatchNorm3d running-stat update (unbiased variance, `momentum`).  `count_dev` (device scalar, e.g. the
 * all-reduced voxel count under data parallelism) overrides `count_host` when not NULL.                  */
int wsr_bn_mean(const float* sums, const float* count_dev, float count_host, float* mean, int32_t C, void* stream);
/* ABI 5 - SyncBN around its one collective per layer (data-parallel nn.BatchNorm3d, torch_blocks.py:20-25).  G groups
 * (D(real), D(fake)) of C channels; `work` rows hold the local means at [0, C), `s2` rows the shifted sums {sum d,
 * sum d^2} at [0, 2C) (strides in floats).  _shard_stats writes this rank's record send (G, 2C) = {mean, M2};
 * _combine_shards takes the gathered (world, G, 2C) records and leaves the global mean in work[:, 0:C) and {0, M2} in
 * s2[:, 0:2C) - what wsr_bn_finalize reads with count = n * world.  Ranks are added in index order.           */
int wsr_bn_shard_stats(const float* work, int32_t work_stride, const float* s2, int32_t s2_stride, float count, float* send,
                       int32_t G, int32_t C, void* stream);
int wsr_bn_combine_shards(const float* gathered, int32_t world, float count, float* work, int32_t work_stride, float* s2,
                          int32_t s2_stride, int32_t G, int32_t C, void* stream);
int wsr_bn_finalize(const float* sums2, const float* count_dev, float count_host, const float* mean, float eps,
                    float momentum, float* invstd, float* var_out, float* running_mean, float* running_var,
                    int32_t C, void* stream);
/* y = lrelu((x-mean)*invstd*gamma + beta); mean/invstd fp32 [C]                 */
int wsr_bn_apply_lrelu(const void* x, void* y, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, int32_t C, int64_t nvox, int32_t act,
                       float slope, int32_t dtype, void* stream);
/* backward, pass 1: g = dy * lrelu'(y) (written in place into dy);
 * sums[2*C] = {sum g, sum g*xhat} (`partials` as for wsr_bn_stats).              */
int wsr_bn_bwd_reduce(void* dy, const void* y, const void* x, const float* mean, const float* invstd,
                      int32_t C, int64_t nvox, int32_t act, float slope, float* sums, float* partials,
                      int32_t dtype, void* stream);
/* pass 2 (training): dx = gamma*invstd*(g - sum_g/n - xhat*sum_gxhat/n); eval:
 * dx = gamma*invstd*g (sums == NULL).  ABI 6 - act_y != NULL: g is first multiplied by the LeakyReLU derivative
 * (act_y > 0 ? 1 : slope) of the layer's saved OUTPUT act_y (same shape) - an eval-mode layer in a pass that wants
 * no parameter gradients (D inside a generator iteration, wind_field_GAN_3D.py:570-583) needs no separate
 * leaky_relu_backward pass.                                                                                 */
int wsr_bn_bwd_apply(const void* g, const void* x, void* dx, const float* mean, const float* invstd,
                     const float* gamma, const float* sums, float inv_n, const void* act_y, float slope, int32_t C,
                     int64_t nvox, int32_t dtype, void* stream);

/* ---- optimizer ---------------------------------------------------------------
 * torch.optim.Adam single-tensor step over a flat fp32 buffer
 * (wind_field_GAN_3D.py:151-162,460,566), bias-corrected, L2 weight decay.     */
int wsr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t step, void* stream);
/* ABI 7 - the same update for MANY tensors in one launch (an optimizer's whole parameter list:
 * wind_field_GAN_3D.py:460 `optimizer_G.step()`, :566 `optimizer_D.step()`): `jobs_dev` is a DEVICE array of n_jobs
 * records, one workgroup each - the caller cuts large tensors into chunks (32 768 elements is a good size).  All
 * tensors of a call share the hyper-parameters and the step count, as the parameters of one param group do.     */
typedef struct wsr_adam_job {
  float* p;       /* parameter chunk, updated in place */
  const float* g; /* its gradient                      */
  float* m;       /* exp_avg                           */
  float* v;       /* exp_avg_sq                        */
  int64_t n;      /* elements                          */
} wsr_adam_job_t;
/* (hyper-parameters as doubles, the way torch.optim.Adam holds them: 1 - beta is taken in double and rounded once, so
 *  exp_avg / exp_avg_sq follow torch's to the last bits instead of to 1e-5)                                           */
int wsr_adam_multi(const wsr_adam_job_t* jobs_dev, int32_t n_jobs, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int32_t step, void* stream);
/* additive - gradient-norm clipping over the same job table (torch.nn.utils.clip_grad_norm_ in front of the Adam
 * step, L2 norm over every gradient of the table), two launches and no host sync:
 * wsr_grad_sqnorm_multi: partials[job] = sum of g^2 over the job's chunk (n_jobs floats; one workgroup per job, fixed
 *   summation order: the same bits from run to run).
 * wsr_adam_multi_clip: total = sqrt(sum of partials) (every workgroup sums them in the same order), coef =
 *   min(1, max_norm / (total + 1e-6)); per element g *= coef, written back to the job's gradient (the `g` of the
 *   table is updated in place), then wsr_adam_multi's update on the scaled g.  max_norm = +inf measures only: coef 1,
 *   the gradients are not written and the update is wsr_adam_multi's bit for bit.  *total_norm_out (device, may be
 *   NULL) = the pre-clip total.  A non-finite total gives a NaN / zero coefficient, as in torch.                    */
int wsr_grad_sqnorm_multi(const wsr_adam_job_t* jobs_dev, int32_t n_jobs, float* partials, void* stream);
int wsr_adam_multi_clip(const wsr_adam_job_t* jobs_dev, int32_t n_jobs, const float* partials, double max_norm,
                        double lr, double beta1, double beta2, double eps, double weight_decay, int32_t step,
                        float* total_norm_out, void* stream);
/* additive - exponential moving average (EMA) of the parameters inside the same launches: ema_dev is a DEVICE array
 * parallel to the job table, ema_dev[job] = the shadow of job's chunk (n floats; wsr_adam_job_t is unchanged).  Per
 * element, after the update has produced the new p:  e = fma(d, e, fl(omd * p))  - two roundings - with
 * d = (float)ema_decay and omd = (float)(1.0 - ema_decay) (taken in double, rounded once); ema_decay == 0 selects
 * e = p bit for bit whatever the old e holds (inf, NaN).  0 <= ema_decay < 1, else WSR_EINVAL.  p, m, v - and with
 * clipping the written-back g and *total_norm_out - are those of wsr_adam_multi / wsr_adam_multi_clip bit for bit.
 * p, g, m, v take the float4 path exactly when they do in wsr_adam_multi (all four 16-byte aligned); the shadow moves
 * as float4 there when it is aligned too, element by element otherwise - the same arithmetic either way.             */
int wsr_adam_multi_ema(const wsr_adam_job_t* jobs_dev, float* const* ema_dev, int32_t n_jobs, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t step, double ema_decay, void* stream);
int wsr_adam_multi_clip_ema(const wsr_adam_job_t* jobs_dev, float* const* ema_dev, int32_t n_jobs,
                            const float* partials, double max_norm, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int32_t step, double ema_decay, float* total_norm_out, void* stream);

/* ABI 9 - train-mode statistics of ALL batch groups of a BatchNorm3d layer (torch_blocks.py:20-25; the groups are the
 * reference's separate calls D(real), D(fake) of one iteration, wind_field_GAN_3D.py:247-304, batched into one pass) in four
 * launches: what wsr_bn_stats + wsr_bn_mean + wsr_bn_stats(shift = mean) + wsr_bn_finalize compute per group in twelve,
 * bit for bit.  x: `groups` consecutive blocks of nvox_g voxels x C channels (NDHWC).  work: [groups][2C] floats out - mean
 * | 1 / sqrt(biased var + eps) of each group.  running_mean / running_var (NULL: untouched) are updated once per group, in
 * group order, as the groups' separate calls would (momentum; unbiased variance).  partials: caller-owned scratch of
 * groups * WSR_CHAN_SUM_ROWS * 2C floats.  C a multiple of 4, <= 512; 1 <= groups <= 64.                          */
int wsr_bn_train_stats(const void* x, int32_t C, int64_t nvox_g, int32_t groups, float eps, float momentum, float* work,
                       float* running_mean, float* running_var, float* partials, int32_t dtype, void* stream);

/* ---- relativistic average GAN loss -------------------------------------------
 * ABI 9 - the adversarial term of a generator iteration (wind_field_GAN_3D.py:360-364) and the loss of a
 * discriminator iteration (:552-556), both of the form
 *     L = ( BCEWithLogits(u - mean(v), lu) + BCEWithLogits(v - mean(u), lv) ) / 2
 * (generator: u = D(fake), v = D(real); discriminator: u = D(real), v = D(fake); lu / lv the label vectors of
 * :627-678), forward AND every partial derivative in one launch - the reference's composed ops are ~25 launches of
 * B-element kernels per loss and pass.  u, v, lu, lv: B floats each.  mu / mv: device scalars holding mean(u) /
 * mean(v) when the caller computed them (data parallelism: batch-global means from a collective), NULL: taken here
 * over the B elements and the chain rule through them folded into du / dv.  out: 2 B + 3 floats
 *     [0] L, [1 .. B] dL/du, [B+1 .. 2B] dL/dv, [2B+1] dL/dmu, [2B+2] dL/dmv   (the last two 0 when mu / mv are NULL)
 * BCEWithLogits(x, t) = mean_i (1 - t_i) x_i - logsigmoid(x_i), torch's formula.  1 <= B <= 65536.             */
int wsr_ragan_loss(const float* u, const float* v, const float* lu, const float* lv, const float* mu, const float* mv,
                   int32_t B, float* out, void* stream);

/* ---- device-resident training data ---------------------------------------------
 * One training batch out of a resident store (device_data.py): slice, coarsen, rotate and mirror of
 * CustomizedDataset.__getitem__ (process_data.py), as pure data movement (copies and sign flips).
 * store: fp32 (n_samples, Cin + 1, X, Y, NZ) - channels [0, Cin) the normalised LR channels at full resolution (0..2 =
 * the HR wind), channel Cin the raw altitude Z.  desc: int32 [B][6] = sample, x0, y0, k, fx, fy per batch entry.
 * S = slice size (0: the whole X x Y domain; then X == Y unless every k is even), s = coarseness.  Writes planar
 * lr (B, Cin, ceil(S/s), ceil(S/s), NZ), hr (B, 3, S, S, NZ), z (B, 1, S, S, NZ): slice -> [::s, ::s] (lr) ->
 * rot90(k, dims (x, y)) with the u / v mixing of the rotation -> mirror x (u negated) if fx -> mirror y (v negated)
 * if fy.  A batch entry whose descriptor falls outside the store is not written.                                */
int wsr_gather_batch(const float* store, int64_t n_samples, const int32_t* desc, int32_t B, int32_t Cin, int32_t s,
                     int32_t S, int32_t X, int32_t Y, int32_t NZ, float* lr, float* hr, float* z, void* stream);

/* wsr_gather_batch with the anti-aliased LR degradation of [DEGRADATION] (degradation.py; csrc/data_gather.hip), still
 * one launch for lr, hr and z.  hr, z and the lr planes read from store channels >= n_filt are the copies of
 * wsr_gather_batch.  An lr plane read from a store channel < n_filt is, in the slice frame before rotation and mirrors
 * (W x H = S x S, or X x Y when S = 0), with f the store channel inside the slice,
 *     g[i][y]  = sum over d = 0 .. 2R ascending of fl(wx[i][d] * f[s i + d - R][y])       (x pass first)
 *     lr[i][j] = sum over d = 0 .. 2R ascending of fl(wy[j][d] * g[i][s j + d - R])
 * per z level: fp32, every product and every sum rounded (no fused multiply-add), sums started from +0.0f, taps outside
 * the slice skipped (not multiplied by zero), z never filtered; the sign flips of rotation and mirrors are applied to
 * the finished sum.  wx: fp32 (ceil(W/s), 2R+1), wy: fp32 (ceil(H/s), 2R+1) device tables (degradation.axis_weights),
 * 0 <= R <= WSR_DEGRADE_MAX_R, 0 <= n_filt <= Cin.  Reads stay inside the slice, hence inside the store.            */
#define WSR_DEGRADE_MAX_R 32
int wsr_gather_batch_filtered(const float* store, int64_t n_samples, const int32_t* desc, int32_t B, int32_t Cin,
                              int32_t s, int32_t S, int32_t X, int32_t Y, int32_t NZ, const float* wx, const float* wy,
                              int32_t R, int32_t n_filt, float* lr, float* hr, float* z, void* stream);

/* ---- device-side evaluation ([EVAL] device_metrics; csrc/eval_metrics.hip) ---------------------------
 * Everything fp32 planar (B, C, X, Y, NZ), z innermost; replaces the ATen / numpy work of test.py:101-115 and
 * wind_field_GAN_3D.py:594-597 (F.interpolate, about fifteen reductions per field, np.interp per column).
 *
 * wsr_trilinear_xy: tl (B, 3, Xl*s, Yl*s, NZ) = F.interpolate(lr[:, :3], scale_factor=(s, s, 1), mode="trilinear",
 * align_corners=True) of lr (B, Cin >= 3, Xl, Yl, NZ); only channels 0..2 of lr are read.
 *
 * wsr_field_metrics: sums (B, WSR_FIELD_METRICS_SUMS) doubles per sample over channels 0..2 of hr (B, hr_c, X, Y, NZ) and
 * sr (B, sr_c, X, Y, NZ): sum (hr-sr)^2, sum (hr-tl)^2, sum |hr-sr|, sum |hr-tl| over components, then sum ||hr-sr||,
 * sum ||hr-tl||, sum ||hr|| over voxels (vector lengths).  The baseline is EITHER the tensor tl (B, tl_c >= 3, X, Y, NZ)
 * with lr = NULL, OR made on the fly from lr (B, lr_c >= 3, X/s, Y/s, NZ) and s with tl = NULL (same bits as
 * wsr_trilinear_xy; never written to memory).  partials: workspace of B * WSR_FIELD_METRICS_MAX_ROWS *
 * WSR_FIELD_METRICS_SUMS floats.  No atomics: a fixed summation order, the same bits on every call.
 *
 * wsr_column_interp: out[b, c, col, :] = np.interp(z_dst[b, col, :], z_src[b, col, :], vals[b, c, col, :]) for the
 * ncols = X * Y columns of every sample; z_src / z_dst (B, 1, X, Y, NZ), vals / out (B, C, X, Y, NZ), NZ <= 128.
 * z_src increasing along z.  Queries outside the source range get the end values; slope and blend are evaluated in
 * double and rounded once to fp32.                                                                              */
#define WSR_FIELD_METRICS_SUMS 7
#define WSR_FIELD_METRICS_MAX_ROWS 2048
int wsr_trilinear_xy(const float* lr, int32_t B, int32_t Cin, int32_t Xl, int32_t Yl, int32_t NZ, int32_t s, float* tl,
                     void* stream);
int wsr_field_metrics(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                      const float* lr, int32_t lr_c, int32_t s, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                      float* partials, double* sums, void* stream);
int wsr_column_interp(const float* vals, const float* z_src, const float* z_dst, int32_t B, int32_t C, int64_t ncols,
                      int32_t NZ, float* out, void* stream);

/* ---- geometric self-ensemble ([ENSEMBLE]; csrc/ensemble.hip) ------------------------------------------
 * The eight symmetries of the square on fp32 planar tensors (B, C, X, Y, NZ).  A member is (k, fx), code k + 4 * fx:
 * k quarter turns as process_data._rotate_wind does them, then, if fx, a mirror along x with u negated (the order of
 * CustomizedDataset.__getitem__: rotate, then flip).  Its inverse: undo the mirror, then _rotate_wind by (4 - k) % 4.
 * codes: a HOST array of K codes, K = 1, 2, 4 or 8 (passed to the kernel by value).  A code with odd k needs X == Y
 * (WSR_EINVAL otherwise, nothing is written).  Only sign bits change: bit-identical to the CPU rules.
 *
 * wsr_dihedral_members: dst (K, B, C, X', Y', NZ) = the K transformed copies of src (B, C, X, Y, NZ) in ONE launch
 * ((X', Y') = (Y, X) for odd k).  is_vector: channels 0 and 1 are the horizontal wind and turn with the grid
 * (C >= 2); 0: every channel is a scalar and is only permuted.
 *
 * wsr_ensemble_reduce: members (K, B, 3, X', Y', NZ), member m transformed by codes[m] -> mean (B, 3, X, Y, NZ) of the
 * members mapped back through their inverses: the pairwise tree sum in member order ((m0 + m1) + (m2 + m3)) + ...
 * times 1 / K, so K identical members give the member back bit for bit.  var (B, 3, X, Y, NZ) or NULL: the population
 * variance per component, the same tree over (m_k - mean)^2.  One pass, no atomics: the same bits on every call.  */
#define WSR_ENSEMBLE_MAX_MEMBERS 8
int wsr_dihedral_members(const float* src, int32_t B, int32_t C, int32_t X, int32_t Y, int32_t NZ,
                         const int32_t* codes, int32_t K, int32_t is_vector, float* dst, void* stream);
int wsr_ensemble_reduce(const float* members, const int32_t* codes, int32_t K, int32_t B, int32_t X, int32_t Y,
                        int32_t NZ, float* mean, float* var, void* stream);

/* ---- tiled whole-domain inference ([TILE]; csrc/tiling.hip) --------------------------------------------
 * Overlapping (x, y) tiles of fp32 planar tensors (B, C, X, Y, NZ) and the blend of per-tile results back into one
 * field; z is never tiled.  Origin lists are HOST arrays.
 *
 * wsr_tile_gather: dst (n, B, C, tx, ty, NZ) = the n tiles src[:, :, x0[k]:x0[k]+tx, y0[k]:y0[k]+ty, :], a pure copy,
 * in one launch (per 256 tiles).  WSR_EINVAL, and nothing is written, if any tile leaves the domain.
 *
 * wsr_tile_stitch: tiles (nx * ny, B, C, Tx, Ty, NZ), tile ix * ny + iy at origin (xs[ix], ys[iy]) of out
 * (B, C, X, Y, NZ); every size in voxels of out.  On one axis, for a tile at origin a of side T on an axis of length N
 * with ramp R, the weight at p = i - a is w(p) = min(L(p), Rr(p)), L(p) = R + 1 if a == 0 else min(p + 1, R + 1),
 * Rr(p) = R + 1 if a + T == N else min(T - p, R + 1): integers >= 1 inside the tile, no ramp at a domain border.
 * The share of tile (ix, iy) at (i, j) is alpha = (wx / Wx(i)) * (wy / Wy(j)), Wx the sum of wx over the tiles of the
 * x axis that cover i; out = sum alpha x_T in tile order, seam (same shape, or NULL) = sum alpha (x_T - out)^2.
 * Where one tile covers a voxel alpha is 1.0f: its value comes back bit for bit and seam is exactly 0.  Every output
 * voxel gathers its tiles and is written once: no atomics, no zero fill, the same bits on every call and with or
 * without seam.  Each origin list must start at 0, increase strictly, leave no gap wider than the tile and end at
 * N - T; 0 <= R <= 32768 (WSR_EINVAL otherwise, nothing is written).  The origins travel by value: more than
 * WSR_TILE_MAX_PER_AXIS of an axis, X or Y > 32768 or X * Y * NZ >= 2^31 return WSR_EUNSUPPORTED.                 */
#define WSR_TILE_MAX_PER_AXIS 128
int wsr_tile_gather(const float* src, int32_t B, int32_t C, int32_t X, int32_t Y, int32_t NZ, const int32_t* x0,
                    const int32_t* y0, int32_t n, int32_t tx, int32_t ty, float* dst, void* stream);
int wsr_tile_stitch(const float* tiles, const int32_t* xs, int32_t nx, const int32_t* ys, int32_t ny, int32_t B,
                    int32_t C, int32_t X, int32_t Y, int32_t NZ, int32_t Tx, int32_t Ty, int32_t Rx, int32_t Ry,
                    float* out, float* seam, void* stream);

/* ---- per-level evaluation diagnostics ([DIAGNOSTICS]; csrc/diagnostics.hip) -----------------------------
 * wsr_level_diagnostics: sums (B, NZ, WSR_LEVEL_DIAG_SUMS) doubles, each a sum over the X * Y columns of one z level of
 * one sample, from one pass over channels 0..2 of hr (B, hr_c, X, Y, NZ), sr (B, sr_c, ...) and the baseline tl
 * (B, tl_c, ...), the raw altitude zc (B, 1, X, Y, NZ) and the coordinate vectors xs (X), ys (Y); all fp32 planar:
 *    0        ||hr||
 *    1, 2     ||hr - sr||, ||hr - tl||
 *    3, 4     ||sr|| - ||hr||, ||tl|| - ||hr||                      (signed speed bias)
 *    5, 6     | ||sr|| - ||hr|| |, | ||tl|| - ||hr|| |
 *    7        h = sqrt(hr_u^2 + hr_v^2)
 *    8, 9     h * theta(hr, sr), h * theta(hr, tl),  theta(a, b) = atan2f(|a_u b_v - a_v b_u|, a_u b_u + a_v b_v) in
 *             [0, pi], 0 when both arguments are 0
 *    10..12   div(hr)^2, div(sr)^2, div(tl)^2,  div = du/dx + dv/dy + dw/dz with the stencils of wsr_wind_gradient
 *             (three-point non-uniform inside, one-sided at the domain borders, zc of the own column for z, 0 along an
 *             axis of length 1)
 *    13, 14   zc, zc - zc at level 0 of the same column
 * workspace: wsr_level_diagnostics_workspace_floats(B, X, Y, NZ) floats (0 for sizes the entry refuses): one partial
 * row of NZ * WSR_LEVEL_DIAG_SUMS floats per workgroup, at most WSR_LEVEL_DIAG_MAX_ROWS rows per sample, added in a
 * fixed order in double by a second kernel.  No atomics, no zero fill, evaluated without contraction: the same bits on
 * every call.  A null pointer, a channel count < 3 or a non-positive size: WSR_EINVAL; NZ > 256, B > 65535, X or
 * Y > 32768 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is written in either case.                             */
#define WSR_LEVEL_DIAG_SUMS 15
#define WSR_LEVEL_DIAG_MAX_ROWS 1024
int64_t wsr_level_diagnostics_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ);
int wsr_level_diagnostics(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                          const float* zc, const float* xs, const float* ys, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                          float* workspace, double* sums, void* stream);

/* ---- horizontal energy spectra ([SPECTRUM]; csrc/spectra.hip) ---------------------------------------------
 * wsr_level_spectra: out (B, NZ, NK, WSR_SPECTRUM_SUMS) doubles, NK = wsr_level_spectra_bins(X, Y): per sample, z level
 * and wavenumber bin the kinetic energy of hr, sr and the baseline tl and the co-spectra of hr with sr and with tl
 * (e_hr, e_sr, e_tl, c_sr, c_tl), from ONE 2-D DFT over (X, Y) per sample, field, component (channels 0..2 of
 * hr (B, hr_c, X, Y, NZ), sr (B, sr_c, ...), tl (B, tl_c, ...), fp32 planar) and level:
 *    g = (f - m) * wx(i) * wy(j)       m the plain mean of f over the plane; window WSR_SPECTRUM_WINDOW_HANN:
 *                                      wx(i) = sin^2(pi (i + 1/2) / X), likewise wy, an axis of length 1 has weight 1;
 *                                      WSR_SPECTRUM_WINDOW_NONE: 1
 *    F(kx, ky) = sum g exp(-2 pi i (kx i / X + ky j / Y)),   ky = 0 .. Y / 2, Hermitian weight h(ky) = 1 for ky = 0
 *                                      and, Y even, for ky = Y / 2, else 2
 *    bin(kx, ky): with N = max(X, Y), kx' the signed frequency of kx and q = (kx' Y)^2 + (ky X)^2 the k >= 0 with
 *                                      (2k - 1)^2 (XY)^2 <= 4 N^2 q < (2k + 1)^2 (XY)^2 (k = 0: the right half alone), that
 *                                      is floor(N sqrt((kx'/X)^2 + (ky/Y)^2) + 1/2), decided in 64-bit integers;
 *                                      NK = floor(N / sqrt(2) + 1/2) + 1
 *    e_a = 1/2 sum_comp sum_modes-in-bin h |F_a|^2 / (X Y W2),     W2 = sum (wx wy)^2 in double
 *    c_b = 1/2 sum_comp sum_modes-in-bin h Re(F_hr conj F_b) / (X Y W2)
 * The transform is a direct separable DFT in fp32 (twiddles from a table of double-precision sincospi values, indexed by
 * (k i) mod n in integers); the modes of a bin are added in ascending (ky, kx), per ky in fp32, over ky in double: no
 * atomics, evaluated without contraction, the same bits on every call, and c_sr = e_hr bit for bit when sr = hr.
 * workspace: wsr_level_spectra_workspace_floats(B, X, Y, NZ) floats (0 for sizes the entry refuses), 16-byte aligned:
 * the bin table, the window, mean partials, the row transform (B * 9 * X * (Y/2 + 1) * NZ complex values) and one
 * partial table per ky.  A null pointer, a channel count < 3, a non-positive size or an unknown window: WSR_EINVAL;
 * X or Y > 1024, B > 65535, NZ > 65535 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is written in either case. */
#define WSR_SPECTRUM_SUMS 5
#define WSR_SPECTRUM_MAX_XY 1024
#define WSR_SPECTRUM_WINDOW_NONE 0
#define WSR_SPECTRUM_WINDOW_HANN 1
int32_t wsr_level_spectra_bins(int32_t X, int32_t Y);
int64_t wsr_level_spectra_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ);
int wsr_level_spectra(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                      int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t window, float* workspace, double* out,
                      void* stream);

/* ---- energy-spectrum loss of generator training ([SPECTRAL_LOSS]; csrc/spectral_loss.hip) -------------------
 * Everything of wsr_level_spectra above carries over unchanged: g = (f - m) w, F(kx, ky) for ky = 0 .. Y / 2, the Hermitian
 * weight h, the integer-decided bin, NK = wsr_level_spectra_bins(X, Y), scale = 1 / (2 X Y W2) and
 *    e_a(b, z, k) = scale * sum_comp sum_{modes in k} h |F_a|^2.
 * wsr_spectral_energy: out (B, NZ, NK, 2) doubles = [e_hr, e_sr] from channels 0..2 of hr (B, hr_c, X, Y, NZ) and
 * sr (B, sr_c, ...), fp32 planar (surplus channels are never read): the passes of wsr_level_spectra over six planes, the
 * same arithmetic, so sr = hr gives e_sr = e_hr bit for bit.  saved, when not null: the column pass also writes
 * F_sr (B, 3, X, Y / 2 + 1, NZ) complex fp32 (wsr_spectral_energy_saved_floats(B, X, Y, NZ) floats, 8-byte aligned), the
 * operand of the backward.
 * wsr_spectral_energy_bwd: the vector-Jacobian product of e_sr towards sr.  gbin (B, NZ, NK) doubles = dL/de_sr with the
 * upstream gradient applied, rounded to fp32 once, G below; dsr (B, 3, X, Y, NZ) fp32 planar, every element written:
 *    C(x, ky) = sum_kx G(bin(kx, ky)) F_sr(kx, ky) exp(+2 pi i kx x / X)
 *    u(x, y)  = sum_{ky = 0 .. Y / 2} h(ky) Re( C(x, ky) exp(+2 pi i ky y / Y) )
 *    v        = 2 scale w u,            dsr = v - mean_plane(v)        (the last term: the adjoint of the detrend)
 * fp32 transforms as in the forward, the plane sums of v as fp32 partial rows added in double.  No atomics, evaluated
 * without contraction: the same bits on every call.
 * workspace: wsr_spectral_energy_workspace_floats(B, X, Y, NZ) floats (0 for sizes the entries refuse), 16-byte aligned,
 * enough for either entry; nothing in it is carried from the forward to the backward.
 * A null pointer (saved of the forward apart), a channel count < 3, a non-positive size or an unknown window: WSR_EINVAL;
 * X or Y > 1024, B > 65535, NZ > 65535 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is written in either case. */
int64_t wsr_spectral_energy_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ);
int64_t wsr_spectral_energy_saved_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ);
int wsr_spectral_energy(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, int32_t B, int32_t X, int32_t Y,
                        int32_t NZ, int32_t window, float* workspace, float* saved, double* out, void* stream);
int wsr_spectral_energy_bwd(const float* saved, const double* gbin, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                            int32_t window, float* workspace, float* dsr, void* stream);

/* ---- structural similarity on horizontal planes ([SSIM]; csrc/ssim.hip) ---------------------------------------
 * wsr_level_ssim: out (B, NZ, 3, WSR_SSIM_SUMS) doubles: per sample, z level and component c (channels 0..2 of
 * hr (B, hr_c, X, Y, NZ), sr (B, sr_c, ...), tl (B, tl_c, ...), fp32 planar) the sums over the (X - win + 1) (Y - win + 1)
 * valid window positions of the plane of (ssim_sr, cs_sr, ssim_tl, cs_tl), with a = hr, s = sr (then tl) of that plane:
 *    mu_a, mu_s, S_aa, S_ss, S_as     the separable window g(i) g(j), g = taps[0 .. win) (device, fp32, sum 1), applied to
 *                                     a, s, a a, s s, a s: along x, then along y, taps ascending, no padding
 *    var_a = S_aa - mu_a^2, var_s = S_ss - mu_s^2, cov = S_as - mu_a mu_s
 *    l  = (2 mu_a mu_s + c1) / (mu_a^2 + mu_s^2 + c1),   cs = (2 cov + c2) / (var_a + var_s + c2),   ssim = l cs
 * z is never windowed.  The moments of hr are computed once for both pairs.  fp32 without contraction, the positions of a
 * workgroup added in a fixed order in fp32, the workgroups of a plane in double: no atomics, the same bits on every call,
 * and ssim_sr = cs_sr = the number of positions exactly when sr equals hr bit for bit (likewise tl).
 * workspace: wsr_level_ssim_workspace_floats(B, X, Y, NZ, win) floats (0 for arguments the entry refuses): one partial
 * row per workgroup.  A null pointer, a channel count < 3, win even or outside 3 .. WSR_SSIM_MAX_WIN, X or Y < win, a
 * non-positive size, c1 or c2 not > 0: WSR_EINVAL; NZ > 256, B > 65535, X or Y > 32768 or X * Y * NZ >= 2^31:
 * WSR_EUNSUPPORTED; nothing is written in either case. */
#define WSR_SSIM_SUMS 4
#define WSR_SSIM_MAX_WIN 15
int64_t wsr_level_ssim_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t win);
int wsr_level_ssim(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                   const float* taps, int32_t win, float c1, float c2, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                   float* workspace, double* out, void* stream);

/* ---- wind-speed distribution and wind rose ([DISTRIBUTION]; csrc/distribution.hip) ----------------------------
 * wsr_level_distribution: out (B, NZ, 3, ns, nd + 1) doubles, written completely: per sample, z level and source
 * (0 hr, 1 sr, 2 tl; fp32 planar (B, c, X, Y, NZ), channels 0 = u and 1 = v read) the number of voxels of the plane in
 * every class (speed bin j, sector): in fp32, every product and sum rounded, nothing contracted,
 *    hs2 = u u + v v;   j = the number of i in [0, ns - 1) with hs2 >= edge2[i]   (edge2 ascending; a NaN: 0)
 *    p = (-u, -v);   cross_k(q) = by[k] q.x - bx[k] q.y, k in [0, nd / 2);
 *    second = cross_0(p) < 0 || (cross_0(p) == 0 && cross_1(p) > 0);
 *    q = second ? -p : p;   cnt = the number of k with cross_k(q) >= 0;
 *    sector = max(cnt, 1) - 1 + (second ? nd / 2 : 0);   sector = nd (calm) unless hs2 > calm2
 * edge2 (ns - 1 floats), bx, by (nd / 2 floats each): device, fp32.  Every (b, z, source) slice sums to X * Y.  tl may
 * be NULL: its slices are written as zeros.  Integer counting in LDS and in the workspace, no floating-point atomics:
 * the same bits on every call.  A workgroup counts min(NZ, WSR_DISTRIBUTION_LDS_COUNTERS / (ns (nd + 1))) consecutive
 * levels.
 * workspace: wsr_level_distribution_workspace_floats(B, X, Y, NZ, ns, nd) 4-byte words (0 for arguments the entry
 * refuses): the integer tables.  A null pointer (but tl), a channel count < 3, ns outside 2 .. 64, nd odd or outside
 * 4 .. 36, a non-positive size: WSR_EINVAL; B > 65535, X * Y >= 2^31 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is
 * written in either case. */
#define WSR_DISTRIBUTION_MAX_SPEED_BINS 64
#define WSR_DISTRIBUTION_MAX_SECTORS 36
#define WSR_DISTRIBUTION_LDS_COUNTERS 15360
int64_t wsr_level_distribution_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns, int32_t nd);
int wsr_level_distribution(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                           const float* edge2, int32_t ns, const float* bx, const float* by, int32_t nd, float calm2,
                           int32_t B, int32_t X, int32_t Y, int32_t NZ, void* workspace, double* out, void* stream);

/* ---- SSIM loss of generator training ([SSIM_LOSS]; csrc/ssim_loss.hip) -----------------------------------------
 * wsr_ssim_pair_sums: out (B, NZ, 3, 2) doubles: per sample, z level and component c (channels 0..2 of hr
 * (B, hr_c, X, Y, NZ) and sr (B, sr_c, ...), fp32 planar) the sums over the valid window positions of the plane of
 * (l cs, cs), by the definitions, the arithmetic, the tile geometry and the summation order of wsr_level_ssim: both
 * columns carry the bits of its ssim_sr and cs_sr on the same inputs, and equal the number of positions exactly when sr
 * equals hr bit for bit.  workspace: wsr_ssim_pair_sums_workspace_floats(B, X, Y, NZ, win) floats (0 for arguments the
 * entry refuses).  Nothing is saved for the backward.
 * wsr_ssim_pair_sums_bwd: dsr (B, 3, X, Y, NZ) fp32, every element written: the vector-Jacobian product of both columns
 * towards sr.  With gout (B, NZ, 3, 2) doubles (device) = (G0, G1) of a plane and, per valid position,
 *    D1 = mu_a^2 + mu_s^2 + c1,  D2 = var_a + var_s + c2,  h = G0 l + G1
 *    alpha = G0 cs (2 mu_a - 2 mu_s l) / D1 + h (2 mu_s cs - 2 mu_a) / D2,   beta = -h cs / D2,   gamma = 2 h / D2
 *    dsr(p) = (g2^T alpha)(p) + 2 s(p) (g2^T beta)(p) + a(p) (g2^T gamma)(p)
 *    (g2^T m)(px, py) = sum_{i, j} g(i) g(j) m(px - i, py - j) over the valid positions (px - i, py - j)
 * One launch that recomputes the moments (the forward's operation sequence) around a tile of output pixels; fp32 without
 * contraction, no atomics, no zero fill, the grid a function of the shape: the same bits on every call.
 * wsr_ssim_pair_sums_bwd_tile: tile[0 .. 3) = (TX, TY, ZC), the output pixels and levels a workgroup of the backward
 * owns, a function of (X, Y, NZ, win) alone (host only).
 * The refusals of all three are those of wsr_level_ssim (without tl): WSR_EINVAL / WSR_EUNSUPPORTED, nothing launched,
 * nothing written. */
int64_t wsr_ssim_pair_sums_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t win);
int wsr_ssim_pair_sums(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* taps, int32_t win,
                       float c1, float c2, int32_t B, int32_t X, int32_t Y, int32_t NZ, float* workspace, double* out,
                       void* stream);
int wsr_ssim_pair_sums_bwd(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const double* gout,
                           const float* taps, int32_t win, float c1, float c2, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                           float* dsr, void* stream);
int wsr_ssim_pair_sums_bwd_tile(int32_t X, int32_t Y, int32_t NZ, int32_t win, int32_t* tile);

/* ---- wind-speed distribution loss of generator training ([DISTRIBUTION_LOSS]; csrc/distribution_loss.hip) -------
 * wsr_speed_soft_counts: out (2, B, NZ, ns + 1) doubles, written completely: per source (0 hr, 1 sr; fp32 planar
 * (B, c, X, Y, NZ), channels 0 = u and 1 = v read), sample and z level the soft (linearly binned) histogram of the
 * horizontal speed of the plane.  In fp32, every product and sum rounded, nothing contracted, the square root correctly
 * rounded, per voxel:
 *    hs2 = u u + v v;   t = sqrt(hs2) c - 0.5;   t = min(max(t, 0), ns - 1);   k0 = min(floor(t), ns - 2);   f = t - k0
 *    fi = rint(f 65536): bin k0 gets the integer 65536 - fi, bin k0 + 1 gets fi; a voxel whose hs2 is not finite enters
 *    no bin and adds 65536 to column ns
 * out = (double)count / 65536: every (source, b, z) row sums to X * Y exactly.  c = UVW_MAX / bin_width, finite and > 0.
 * 32-bit integer counting in LDS (a workgroup holds all NZ levels of at most 65535 columns), 64-bit integer adds in the
 * workspace, no floating-point atomics: the same bits on every call.  Nothing is saved for the backward.
 * workspace: wsr_speed_soft_counts_workspace_floats(B, X, Y, NZ, ns) 4-byte words (0 for arguments the entry refuses),
 * 8-byte aligned: the integer tables.
 * wsr_speed_soft_counts_bwd: dsr (B, sr_c, X, Y, NZ) fp32, every element written exactly once: the vector-Jacobian
 * product towards sr.  With gtab (B, NZ, ns) fp32 (device) = dL/dout[1][b, z, 0 .. ns) and t before the clamp, for a voxel
 * with a finite hs2, r = sqrt(hs2) > 0 and 0 < t < ns - 1:
 *    dsr[b, 0] = ((gtab[k0 + 1] - gtab[k0]) c) u / r,   dsr[b, 1] likewise with v;
 * zero otherwise and in every channel from 2 on.  One launch that recomputes t with the forward's operations; gtab is
 * staged in LDS; no atomics: the same bits on every call.
 * wsr_speed_soft_counts_geometry: geom[0 .. 4) = (the columns a workgroup of the counting launch owns, its column ranges
 * per (sample, source), the elements a workgroup of the backward owns, its element ranges per sample), a function of the
 * shape alone (host only).
 * A null pointer, a misaligned workspace, a channel count < 2, ns outside 2 .. 64, c not finite or not > 0, a
 * non-positive size: WSR_EINVAL; (ns + 1) * NZ > WSR_DISTRIBUTION_LOSS_LDS_COUNTERS, B > 65535, X * Y >= 2^31 or
 * X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is launched and nothing is written in either case. */
#define WSR_DISTRIBUTION_LOSS_LDS_COUNTERS 8320
int64_t wsr_speed_soft_counts_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns);
int wsr_speed_soft_counts(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, float c, int32_t ns, int32_t B,
                          int32_t X, int32_t Y, int32_t NZ, void* workspace, double* out, void* stream);
int wsr_speed_soft_counts_bwd(const float* sr, int32_t sr_c, const float* gtab, float c, int32_t ns, int32_t B, int32_t X,
                              int32_t Y, int32_t NZ, float* dsr, void* stream);
int wsr_speed_soft_counts_geometry(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns, int32_t* geom);

/* ---- coarse-grained consistency loss of generator training ([CONSISTENCY_LOSS]; csrc/consistency_loss.hip) ------
 * wsr_coarse_residual: r (B, 3, XL, YL, NZ) fp32, XL = ceil(X / s), YL = ceil(Y / s), every element written exactly
 * once: the anti-aliased coarse-graining of [DEGRADATION] applied to the difference of the wind components of sr and hr
 * (fp32 planar (B, c, X, Y, NZ), channels 0..2 read).  wx (XL, 2 R + 1) and wy (YL, 2 R + 1) fp32 (device) are the
 * tables of degradation.axis_weights.  In fp32, every product and sum rounded, nothing contracted, accumulators from
 * +0.0f, taps ascending, a tap outside [0, n) skipped and never read:
 *    e[x, y, z] = sr - hr
 *    g[i, y, z] = sum_d wx[i, d] e[s i + d - R, y, z]
 *    r[i, j, z] = sum_d wy[j, d] g[i, s j + d - R, z]
 * One launch, no workspace, no atomics; nothing is saved for the backward.
 * wsr_coarse_residual_bwd: dsr (B, sr_c, X, Y, NZ) fp32, every element written exactly once: the vector-Jacobian product
 * towards sr.  With G (B, 3, XL, YL, NZ) fp32 (device) = dL/dr, indices ascending:
 *    t[x; j, z]   = sum_i wx[i, x - s i + R] G[i, j, z]          over the i with 0 <= x - s i + R <= 2 R
 *    dsr[x, y, z] = sum_j wy[j, y - s j + R] t[x; j, z]          over the j with 0 <= y - s j + R <= 2 R
 * zero in every channel from 3 on.  One launch, no atomics.  Both entries give the same bits on every call.
 * wsr_coarse_residual_geometry: geom[0 .. 8) = (XL, YL, the coarse rows a forward workgroup owns, its runs of them per
 * (sample, channel, coarse column), the rows a backward workgroup owns, its runs of them per (sample, channel, column),
 * the floats of LDS of a forward and of a backward workgroup), a function of the arguments alone (host only).
 * A null pointer, a channel count < 3, s outside 2 .. 32, R outside 0 .. WSR_DEGRADE_MAX_R, a non-positive size:
 * WSR_EINVAL; an LDS strip above WSR_CONSISTENCY_LOSS_LDS_FLOATS floats (the forward holds the
 * min(Y, s (TJ - 1) + 2 R + 1) NZ x-pass values of its run, the backward the t of the coarse rows its run reaches; R = 32
 * with NZ = 128 fits), 3 B or sr_c B > 65535, X > 65535 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is launched and
 * nothing is written in either case. */
#define WSR_CONSISTENCY_LOSS_LDS_FLOATS 16384
int wsr_coarse_residual(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* wx, const float* wy,
                        int32_t s, int32_t R, int32_t B, int32_t X, int32_t Y, int32_t NZ, float* r, void* stream);
int wsr_coarse_residual_bwd(const float* G, const float* wx, const float* wy, int32_t s, int32_t R, int32_t sr_c,
                            int32_t B, int32_t X, int32_t Y, int32_t NZ, float* dsr, void* stream);
int wsr_coarse_residual_geometry(int32_t s, int32_t R, int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t* geom);

/* ---- fractions skill score ([FSS]; csrc/fss.hip) ---------------------------------------------------------------
 * wsr_level_fss: out (B, NZ, nt, nn, 5) doubles, written completely: per sample, z level, threshold t and
 * neighbourhood n = scales[k] five exact integers.  Sources 0 hr, 1 sr, 2 tl: fp32 planar (B, c, X, Y, NZ), channels
 * 0 = u and 1 = v read.  In fp32, every product and sum rounded, nothing contracted, no sqrt:
 *    hs2 = u u + v v;   event I_t = hs2 >= thr2[t]   (thr2 ascending; a NaN is no event, a tie and +Inf are events)
 *    c_f,t,n(x, y) = the number of events of source f in the n x n box centred on (x, y) of the level's plane, cells
 *                    outside the plane counting 0 (zero padding): an integer 0 .. n^2
 *    summed over ALL X * Y positions:  [0] hr2 = sum c_hr^2   [1] sr2 = sum c_sr^2   [2] srd = sum (c_sr - c_hr)^2
 *                                      [3] tl2 = sum c_tl^2   [4] tld = sum (c_tl - c_hr)^2
 * thr2 (nt floats): device, fp32.  scales (nn int32): HOST, read during the call: odd, strictly ascending, the first
 * one 1, the last one <= WSR_FSS_MAX_SCALE; a neighbourhood wider than the plane is allowed.  z is never windowed.  tl
 * may be NULL: entries 3 and 4 are written as zeros.  The counts come from a table of running sums in LDS over a
 * 32 x 32 tile with a halo of the largest radius; squares are added as 32-bit integers per workgroup and as 64-bit
 * integers in the workspace, no floating-point atomics: the same bits on every call.
 * workspace: wsr_level_fss_workspace_floats(B, X, Y, NZ, nt, nn, max_n) 4-byte words, max_n = scales[nn - 1] (0 for
 * arguments the entry refuses), 8-byte aligned: the integer table.  A null pointer (but tl), a misaligned workspace, a
 * channel count < 3, nt outside 1 .. 8, nn outside 1 .. 8, a scale that is even, not ascending, not 1 at the front or
 * > 33, a non-positive size: WSR_EINVAL; B > 65535, X * Y >= 2^31 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is
 * written in either case. */
#define WSR_FSS_MAX_THRESHOLDS 8
#define WSR_FSS_MAX_SCALES 8
#define WSR_FSS_MAX_SCALE 33
int64_t wsr_level_fss_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t nt, int32_t nn,
                                       int32_t max_n);
int wsr_level_fss(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                  const float* thr2, int32_t nt, const int32_t* scales, int32_t nn, int32_t B, int32_t X, int32_t Y,
                  int32_t NZ, double* out, void* workspace, void* stream);

/* ---- hub-height wind resource ([HUB_HEIGHT]; csrc/hub_height.hip) ----------------------------------------------
 * wsr_hub_height: out (B, nh, 18) doubles, written completely: per sample and height q = heights[k] (metres above
 * ground) the sums over the VALID columns of the plane.  Sources 0 hr, 1 sr, 2 tl: fp32 planar (B, c, X, Y, NZ),
 * channels 0 = u and 1 = v read; z: the raw altitude (B, 1, X, Y, NZ), taken as strictly increasing along z (not
 * checked); terrain: the ground altitude (X, Y).  Per column:
 *    h_k = z_k - terrain, ONE fp32 subtraction;  valid iff h_0 <= q <= h_{NZ-1} in fp32 (false for a NaN), no h_k is a
 *    NaN and, with log_mode, h_0 > 0: no extrapolation, an invalid column enters no sum
 *    j = the largest index with h_j <= q;  j = NZ - 1: the top level's value;  else the weight in double from the fp32
 *    heights, w = (q - h_j) / (h_{j+1} - h_j), with log_mode ln(q / h_j) / ln(h_{j+1} / h_j), and every component
 *    f_j + w (f_{j+1} - f_j) in double, rounded once to fp32 (w = 0: the knot's value bit for bit)
 *    V = sqrtf(u u + v v), nothing contracted;  P = np.interp(V, curve_v, curve_p) (the end values outside) in double,
 *    rounded once;  angle(a, b) = atan2f(|a_u b_v - a_v b_u|, a_u b_u + a_v b_v), 0 when both arguments are 0
 *    [0] n_valid   [1..3] sum V of hr, sr, tl   [4, 5] sum |V_s - V_hr|, s = sr, tl   [6, 7] sum (V_s - V_hr)^2
 *    [8..10] sum V^3   [11..13] sum P   [14, 15] sum |P_s - P_hr|   [16, 17] sum V_hr angle(hr, s)
 * tl may be NULL: its sums are written as zeros.  cols may be NULL; else (B, nh, 7, X, Y) fp32, every element written
 * exactly once: planes 0..2 V of hr, sr, tl, 3..5 P of hr, sr, tl (zeros for an invalid column and for an absent tl),
 * 6 validity as 1.0 / 0.0.  heights (nh floats), curve_v and curve_p (nk floats, speeds in the fields' normalised
 * units): HOST arrays, read during the call and passed to the kernel as arguments.  A workgroup stages runs of
 * consecutive columns in LDS with coalesced loads, a thread owns (column, height) pairs, bisects once per pair and
 * keeps fp32 partial sums; one partial row per workgroup, added in a fixed order in double: no atomics, the same bits
 * on every call, n_valid an exact integer.
 * workspace: wsr_hub_height_workspace_floats(B, X, Y, NZ, nh) floats (0 for arguments the entry refuses).  A null
 * pointer (but tl and cols), a channel count < 3, nh outside 1 .. 8, nk outside 2 .. 32, heights not > 0 and strictly
 * ascending, curve_v not >= 0 and strictly ascending, log_mode not 0 or 1, B, X or Y < 1, NZ < 2: WSR_EINVAL;
 * NZ > 128, B > 65535, X or Y > 32768, X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is written in either case. */
#define WSR_HUB_HEIGHT_SUMS 18
#define WSR_HUB_HEIGHT_PLANES 7
#define WSR_HUB_HEIGHT_MAX_HEIGHTS 8
#define WSR_HUB_HEIGHT_MAX_KNOTS 32
#define WSR_HUB_HEIGHT_MAX_NZ 128
#define WSR_HUB_HEIGHT_MAX_ROWS 2048
int64_t wsr_hub_height_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t nh);
int wsr_hub_height(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                   const float* z, const float* terrain, const float* heights, int32_t nh, const float* curve_v,
                   const float* curve_p, int32_t nk, int32_t log_mode, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                   float* workspace, double* out, float* cols, void* stream);

/* ---- structure functions ([INCREMENTS]; csrc/increments.hip) ---------------------------------------------------
 * wsr_level_increments: out (B, NZ, 3, nr, 2, 3, 3) doubles, written completely: per sample, z level, source (0 hr,
 * 1 sr, 2 tl), separation r = separations[k], direction a (0 x, 1 y), kind (0 L: the component along a - u for x, v for
 * y; 1 T: the horizontal component across a; 2 W: w) and order (2, 3, 4) the sum over every pair (p, p + r e_a) with
 * both ends inside the level's plane - no padding, max(X - r, 0) * Y pairs along x and X * max(Y - r, 0) along y - of
 *    delta = f(p + r e_a) - f(p), ONE fp32 subtraction;   q = delta delta;   [0] q   [1] q delta   [2] q q
 * every product rounded to fp32, nothing contracted.  Sources: fp32 planar (B, c, X, Y, NZ), channels 0 = u, 1 = v and
 * 2 = w read.  z is never paired.  An entry without pairs is 0; a NaN or Inf operand makes exactly the entries whose
 * pairs contain it non-finite.  tl may be NULL: its slices are written as zeros.  separations (nr int32): HOST, read
 * during the call: 1 .. 8 entries, strictly ascending, each 1 .. 32.  A workgroup stages a 32 x 32 tile of one component
 * with a forward halo of the largest separation in LDS, keeps fp32 partial sums in a fixed order (a chain of at most 96
 * additions) and writes one partial row; the rows are added in a fixed order in double: no atomics, the same bits on
 * every call, the three sources through the same code.
 * workspace: wsr_level_increments_workspace_floats(B, X, Y, NZ, separations, nr) floats (0 for arguments the entry
 * refuses).  A null pointer (but tl), a channel count < 3, a non-positive size, nr outside 1 .. 8, a separation outside
 * 1 .. 32 or not ascending: WSR_EINVAL; B > 65535, X * Y >= 2^31 or X * Y * NZ >= 2^31: WSR_EUNSUPPORTED; nothing is
 * written in either case. */
#define WSR_INCREMENTS_MAX_SEPARATIONS 8
#define WSR_INCREMENTS_MAX_SEPARATION 32
int64_t wsr_level_increments_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, const int32_t* separations,
                                              int32_t nr);
int wsr_level_increments(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                         const int32_t* separations, int32_t nr, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                         float* workspace, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDSR_HIP_H */
