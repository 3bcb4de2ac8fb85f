// Structural similarity on horizontal planes ([SSIM]; ssim.py holds the definition): per sample, z level and wind
// component the sums over the valid window positions of SSIM and of its contrast-structure factor, for the pair
// (HR, SR) and the pair (HR, TL).  All tensors fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0..2 are read.
// One launch of ssim_tile_kernel<3> stages each tile with its halo in LDS, filters separably (the x pass into LDS, the y
// pass in registers) and leaves one partial row per workgroup; ssim_final_kernel<3> adds the rows in double.  No moment map
// and no SSIM map reaches global memory.  The kernels are in ssim_kernels.h.
#include "common.h"
#include "ssim_kernels.h"

extern "C" int64_t wsr_level_ssim_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t win) {
  SsGeom g{};
  if (ss_geom(g, B, X, Y, NZ, win) != 0) return 0;
  return ss_workspace_floats<3>(g);
}

extern "C" int wsr_level_ssim(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                              const float* taps, int32_t win, float c1, float c2, int32_t B, int32_t X, int32_t Y,
                              int32_t NZ, float* workspace, double* out, void* stream) {
  if (!hr || !sr || !tl || !taps || !workspace || !out || hr_c < 3 || sr_c < 3 || tl_c < 3) return WSR_EINVAL;
  if (!(c1 > 0.f) || !(c2 > 0.f)) return WSR_EINVAL;
  SsGeom g{};
  if (const int rc = ss_geom(g, B, X, Y, NZ, win)) return rc;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ssim_tile_kernel<3>, dim3((unsigned)(g.ntxy * g.nzc), 3u, (unsigned)B), dim3(SS_BLOCK), 0, st, hr, hr_c,
                     sr, sr_c, tl, tl_c, taps, c1, c2, g, workspace);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_final_kernel<3>, dim3((unsigned)((g.ZC * ss_ns<3> + 63) / 64), (unsigned)(3 * g.nzc), (unsigned)B),
                     dim3(SS_FBLOCK), 0, st, workspace, g, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
