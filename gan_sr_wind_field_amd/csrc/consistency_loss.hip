// The coarse-grained consistency loss of generator training ([CONSISTENCY_LOSS]; consistency_loss.py holds the
// definition): r = D(fl(SR - HR)), the anti-aliased coarse-graining D of [DEGRADATION] (degradation.py: box or gaussian
// taps centred on the sample point, renormalised at the borders, x pass then y pass in fp32) applied to the difference of
// the three wind components (wsr_coarse_residual), and its vector-Jacobian product towards SR, D^T
// (wsr_coarse_residual_bwd).  All tensors fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0..2 are read.  ONE
// launch each, no workspace, no atomics, every output element written exactly once, nothing saved by the forward: the
// backward needs only the upstream gradient and the two weight tables.  The kernels are in consistency_loss_kernels.h.
#include "common.h"
#include "consistency_loss_kernels.h"

namespace {

template <int V>
int launch_fwd(const float* hr, int hr_c, const float* sr, int sr_c, const float* wx, const float* wy, const ClGeom& g,
               float* r, hipStream_t st) {
  hipLaunchKernelGGL((cl_fwd_kernel<V>), dim3((unsigned)g.njr, (unsigned)g.XL, (unsigned)(3 * g.B)), dim3(CL_BLOCK),
                     (size_t)g.fwd_lds * sizeof(float), st, hr, hr_c, sr, sr_c, wx, wy, g, r);
  WSR_LAUNCH_CHECK();
  return 0;
}

template <int V>
int launch_bwd(const float* G, const float* wx, const float* wy, const ClGeom& g, int sr_c, float* dsr, hipStream_t st) {
  hipLaunchKernelGGL((cl_bwd_kernel<V>), dim3((unsigned)g.nyr, (unsigned)g.X, (unsigned)(sr_c * g.B)), dim3(CL_BLOCK),
                     (size_t)g.bwd_lds * sizeof(float), st, G, wx, wy, g, sr_c, dsr);
  WSR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int wsr_coarse_residual_geometry(int32_t s, int32_t R, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                            int32_t* geom) {
  ClGeom g{};
  if (!geom) return WSR_EINVAL;
  if (const int rc = cl_geom(g, s, R, B, X, Y, NZ)) return rc;
  geom[0] = g.XL, geom[1] = g.YL, geom[2] = g.TJ, geom[3] = g.njr, geom[4] = g.TY, geom[5] = g.nyr;
  geom[6] = g.fwd_lds, geom[7] = g.bwd_lds;
  return 0;
}

extern "C" int wsr_coarse_residual(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* wx,
                                   const float* wy, int32_t s, int32_t R, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                   float* r, void* stream) {
  if (!hr || !sr || !wx || !wy || !r || hr_c < 3 || sr_c < 3) return WSR_EINVAL;
  ClGeom g{};
  if (const int rc = cl_geom(g, s, R, B, X, Y, NZ)) return rc;
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {hr, sr})) {
    case 4: return launch_fwd<4>(hr, hr_c, sr, sr_c, wx, wy, g, r, st);
    case 2: return launch_fwd<2>(hr, hr_c, sr, sr_c, wx, wy, g, r, st);
    default: return launch_fwd<1>(hr, hr_c, sr, sr_c, wx, wy, g, r, st);
  }
}

extern "C" int wsr_coarse_residual_bwd(const float* G, const float* wx, const float* wy, int32_t s, int32_t R,
                                       int32_t sr_c, int32_t B, int32_t X, int32_t Y, int32_t NZ, float* dsr,
                                       void* stream) {
  if (!G || !wx || !wy || !dsr || sr_c < 3) return WSR_EINVAL;
  ClGeom g{};
  if (const int rc = cl_geom(g, s, R, B, X, Y, NZ)) return rc;
  if ((long)B * sr_c > 65535) return WSR_EUNSUPPORTED;
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {G, dsr})) {
    case 4: return launch_bwd<4>(G, wx, wy, g, sr_c, dsr, st);
    case 2: return launch_bwd<2>(G, wx, wy, g, sr_c, dsr, st);
    default: return launch_bwd<1>(G, wx, wy, g, sr_c, dsr, st);
  }
}
