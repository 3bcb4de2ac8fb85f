// wsr_gather_batch (data_gather.hip) with the anti-aliased LR degradation of [DEGRADATION] (degradation.py) folded in: one
// launch still writes LR, HR and Z of a batch.  HR and Z planes and the LR channels that stay point-sampled are the
// copies of data_gather.hip (same workgroup -> plane map, same index map, same sign XOR).  A filtered LR plane
// evaluates, per output column and V consecutive levels, the two-pass definition in the pre-rotation slice frame at
// the sample point (s a, s bb):
//     g(y)  = sum_dx fl(wx[a][dx] * f[s a + dx - R][y])        x pass, taps ascending, from +0.0f
//     LR    = sum_dy fl(wy[bb][dy] * g(s bb + dy - R))         y pass, taps ascending, from +0.0f
// The direct form: a thread recomputes the g values its output reads, which repeats the arithmetic of the two whole-array
// passes of degradation.degrade_lr operation for operation - every product and every sum rounded to fp32 (no
// contraction into fma), taps outside the SLICE skipped - so the batch equals the CPU loader's bit for bit.  The taps
// never leave the slice [x0, x0 + W) x [y0, y0 + H), which the descriptor guard keeps inside the store.  Lanes run along
// z, then y: the loads of one tap are runs of NZ floats s columns apart; the store columns a workgroup re-reads stay
// in L2.  The sign of the rotation / mirrors is applied to the finished sum, where __getitem__ negates.
#include "common.h"
#include "data_degrade_kernels.h"

namespace {

template <int V>
int launch(const float* store, const int32_t* desc, const float* wx, const float* wy, DegradeGeom g, float* lr,
           float* hr, float* z, hipStream_t st) {
  const long blocks = gd_plan<V>(g);
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(gather_batch_filtered_kernel<V>, dim3((unsigned)blocks), dim3(GD_BLOCK), 0, st, store, desc, wx,
                     wy, g, lr, hr, z);
  WSR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int wsr_gather_batch_filtered(const float* store, int64_t n_samples, const int32_t* desc, int32_t B,
                                         int32_t Cin, int32_t s, int32_t S, int32_t X, int32_t Y, int32_t NZ,
                                         const float* wx, const float* wy, int32_t R, int32_t n_filt, float* lr,
                                         float* hr, float* z, void* stream) {
  if (!store || !desc || !lr || !hr || !z || !wx || !wy) return WSR_EINVAL;
  DegradeGeom g{};
  if (const int rc = gd_geom(g, n_samples, B, Cin, s, S, X, Y, NZ, R, n_filt)) return rc;
  const hipStream_t st = as_stream(stream);
  if (NZ % 4 == 0) return launch<4>(store, desc, wx, wy, g, lr, hr, z, st);
  if (NZ % 2 == 0) return launch<2>(store, desc, wx, wy, g, lr, hr, z, st);
  return launch<1>(store, desc, wx, wy, g, lr, hr, z, st);
}
