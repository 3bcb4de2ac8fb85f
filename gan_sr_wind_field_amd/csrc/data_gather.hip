// One training batch out of the device-resident store (device_data.py): the slice / coarsen / rot90 / mirror
// augmentation of CustomizedDataset.__getitem__ as a gather.  Rotation and mirrors only permute (x, y), so every
// output column (b, c, i, j, 0..NZ) is a contiguous run of NZ floats from ONE store column, copied or with its sign
// flipped.  Each workgroup covers a chunk of one output plane (b, c): the plane's descriptor, source channel, sign and
// index map are workgroup-uniform; a thread moves V consecutive floats (V | NZ, so a piece never straddles two
// columns), consecutive threads move consecutive pieces: stores are fully coalesced, loads are contiguous runs of NZ
// floats.  No arithmetic on the values besides the sign bit, which keeps the batch bit-identical to the CPU path.
//
// wsr_gather_batch_filtered folds the anti-aliased LR degradation of [DEGRADATION] (degradation.py) into the same
// launch, which still writes LR, HR and Z of a batch.  It is the same kernel (data_gather_kernels.h) with the filtered
// branch compiled in: HR and Z planes and the LR channels that stay point-sampled take the plain gather's workgroup ->
// plane map, index map and sign XOR.  A filtered LR plane evaluates, per output column and V consecutive levels, the
// two-pass definition in the pre-rotation slice frame at the sample point (s a, s bb):
//     g(y)  = sum_dx fl(wx[a][dx] * f[s a + dx - R][y])        x pass, taps ascending, from +0.0f
//     LR    = sum_dy fl(wy[bb][dy] * g(s bb + dy - R))         y pass, taps ascending, from +0.0f
// The direct form: a thread recomputes the g values its output reads, which repeats the arithmetic of the two whole-array
// passes of degradation.degrade_lr operation for operation - every product and every sum rounded to fp32 (no
// contraction into fma), taps outside the SLICE skipped - so the batch equals the CPU loader's bit for bit.  The taps
// never leave the slice [x0, x0 + W) x [y0, y0 + H), which the descriptor guard keeps inside the store.  Lanes run along
// z, then y: the loads of one tap are runs of NZ floats s columns apart; the store columns a workgroup re-reads stay
// in L2.  The sign of the rotation / mirrors is applied to the finished sum, where __getitem__ negates.
#include "common.h"
#include "data_gather_kernels.h"

namespace {

template <int V, bool FILTERED>
int launch(const float* store, const int32_t* desc, const float* wx, const float* wy, GatherGeom g, float* lr, float* hr,
           float* z, hipStream_t st) {
  const long blocks = gb_plan<V>(g);
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL((gather_batch_kernel<V, FILTERED>), dim3((unsigned)blocks), dim3(GB_BLOCK), 0, st, store, desc, wx, wy,
                     g, lr, hr, z);
  WSR_LAUNCH_CHECK();
  return 0;
}

// V: the widest of 4, 2 and 1 floats that divides NZ
template <bool FILTERED>
int launch_widest(const float* store, const int32_t* desc, const float* wx, const float* wy, const GatherGeom& g,
                  float* lr, float* hr, float* z, void* stream) {
  const hipStream_t st = as_stream(stream);
  if (g.NZ % 4 == 0) return launch<4, FILTERED>(store, desc, wx, wy, g, lr, hr, z, st);
  if (g.NZ % 2 == 0) return launch<2, FILTERED>(store, desc, wx, wy, g, lr, hr, z, st);
  return launch<1, FILTERED>(store, desc, wx, wy, g, lr, hr, z, st);
}

}  // namespace

extern "C" int wsr_gather_batch(const float* store, int64_t n_samples, const int32_t* desc, int32_t B, int32_t Cin,
                                int32_t s, int32_t S, int32_t X, int32_t Y, int32_t NZ, float* lr, float* hr, float* z,
                                void* stream) {
  if (!store || !desc || !lr || !hr || !z) return WSR_EINVAL;
  GatherGeom g{};
  if (const int rc = gb_geom(g, n_samples, B, Cin, s, S, X, Y, NZ, 0, 0)) return rc;
  return launch_widest<false>(store, desc, nullptr, nullptr, g, lr, hr, z, stream);
}

extern "C" int wsr_gather_batch_filtered(const float* store, int64_t n_samples, const int32_t* desc, int32_t B,
                                         int32_t Cin, int32_t s, int32_t S, int32_t X, int32_t Y, int32_t NZ,
                                         const float* wx, const float* wy, int32_t R, int32_t n_filt, float* lr,
                                         float* hr, float* z, void* stream) {
  if (!store || !desc || !lr || !hr || !z || !wx || !wy) return WSR_EINVAL;
  GatherGeom g{};
  if (const int rc = gb_geom(g, n_samples, B, Cin, s, S, X, Y, NZ, R, n_filt)) return rc;
  return launch_widest<true>(store, desc, wx, wy, g, lr, hr, z, stream);
}
