// The SSIM loss of generator training ([SSIM_LOSS]; ssim_loss.py holds the definition): per sample, z level and wind
// component the sums over the valid window positions of l cs and of cs for the pair (HR, SR), P (B, NZ, 3, 2) in double
// (wsr_ssim_pair_sums), and the vector-Jacobian product of both columns towards SR (wsr_ssim_pair_sums_bwd).  All tensors
// fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0..2 are read.  The forward is the tile and final kernels of
// csrc/ssim.hip instantiated for two fields (ssim_kernels.h), on the same tile geometry, so both columns carry the bits
// of wsr_level_ssim's ssim_sr and cs_sr.  The backward is one launch that recomputes the moments around a tile of output
// pixels; nothing is saved by the forward.  Its kernel, and what each pass does, is in ssim_loss_kernels.h.
#include "common.h"
#include "ssim_loss_kernels.h"

extern "C" int64_t wsr_ssim_pair_sums_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t win) {
  SsGeom g{};
  if (ss_geom(g, B, X, Y, NZ, win) != 0) return 0;
  return ss_workspace_floats<2>(g);
}

extern "C" int wsr_ssim_pair_sums(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* taps,
                                  int32_t win, float c1, float c2, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                  float* workspace, double* out, void* stream) {
  if (!hr || !sr || !taps || !workspace || !out || hr_c < 3 || sr_c < 3) return WSR_EINVAL;
  if (!(c1 > 0.f) || !(c2 > 0.f)) return WSR_EINVAL;
  SsGeom g{};
  if (const int rc = ss_geom(g, B, X, Y, NZ, win)) return rc;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ssim_tile_kernel<2>, dim3((unsigned)(g.ntxy * g.nzc), 3u, (unsigned)B), dim3(SS_BLOCK), 0, st, hr,
                     hr_c, sr, sr_c, (const float*)nullptr, 0, taps, c1, c2, g, workspace);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_final_kernel<2>, dim3((unsigned)((g.ZC * ss_ns<2> + 63) / 64), (unsigned)(3 * g.nzc), (unsigned)B),
                     dim3(SS_FBLOCK), 0, st, workspace, g, out);
  WSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int wsr_ssim_pair_sums_bwd_tile(int32_t X, int32_t Y, int32_t NZ, int32_t win, int32_t* tile) {
  SslBwdGeom g{};
  if (!tile) return WSR_EINVAL;
  if (const int rc = ssl_bwd_geom(g, 1, X, Y, NZ, win)) return rc;
  tile[0] = g.TX, tile[1] = g.TY, tile[2] = g.ZC;
  return 0;
}

extern "C" int wsr_ssim_pair_sums_bwd(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const double* gout,
                                      const float* taps, int32_t win, float c1, float c2, int32_t B, int32_t X, int32_t Y,
                                      int32_t NZ, float* dsr, void* stream) {
  if (!hr || !sr || !gout || !taps || !dsr || hr_c < 3 || sr_c < 3) return WSR_EINVAL;
  if (!(c1 > 0.f) || !(c2 > 0.f)) return WSR_EINVAL;
  SslBwdGeom g{};
  if (const int rc = ssl_bwd_geom(g, B, X, Y, NZ, win)) return rc;
  hipLaunchKernelGGL(ssl_bwd_kernel, dim3((unsigned)(g.ntxy * g.nzc), 3u, (unsigned)B), dim3(SS_BLOCK), 0,
                     as_stream(stream), hr, hr_c, sr, sr_c, gout, taps, c1, c2, g, dsr);
  WSR_LAUNCH_CHECK();
  return 0;
}
