// Hub-height wind resource ([HUB_HEIGHT]; hub_height.py holds the definition): per sample and requested height above
// ground 18 sums over the valid columns of the wind speed, its cube, the power-curve output and the direction error of
// HR, SR and the trilinear baseline TL, every column interpolated to the height from its terrain-following levels.  All
// fields fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0 and 1 are read; z is the raw altitude (B, 1, X, Y,
// NZ), terrain the ground altitude (X, Y).  ONE launch of hub_height_kernel reads every operand once and writes one
// partial row per workgroup (and, on request, the seven per-column planes); hub_height_final_kernel adds the rows in
// double.  No atomics: the same bits on every call.  The kernels are in hub_height_kernels.h.
#include "common.h"
#include "hub_height_kernels.h"

extern "C" int64_t wsr_hub_height_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t nh) {
  if (nh < 1 || nh > HH_MAX_NH) return 0;
  float heights[HH_MAX_NH];
  for (int k = 0; k < HH_MAX_NH; ++k) heights[k] = (float)(k + 1);
  const float curve_v[2] = {0.f, 1.f};  // (the size depends on the shape and the number of heights alone)
  HhGeom g{};
  if (hh_geom(g, B, X, Y, NZ, heights, nh, curve_v, 2, 0) != 0) return 0;
  return hh_workspace_floats(g, B);
}

extern "C" int wsr_hub_height(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                              const float* z, const float* terrain, const float* heights, int32_t nh,
                              const float* curve_v, const float* curve_p, int32_t nk, int32_t log_mode, int32_t B,
                              int32_t X, int32_t Y, int32_t NZ, float* workspace, double* out, float* cols,
                              void* stream) {
  if (!hr || !sr || !z || !terrain || !heights || !curve_v || !curve_p || !workspace || !out) return WSR_EINVAL;
  if (hr_c < 3 || sr_c < 3 || (tl && tl_c < 3)) return WSR_EINVAL;
  HhGeom g{};
  if (const int rc = hh_geom(g, B, X, Y, NZ, heights, nh, curve_v, nk, log_mode)) return rc;
  HhTables tab{};
  for (int k = 0; k < nh; ++k) tab.q[k] = heights[k];
  for (int k = 0; k < nk; ++k) tab.cv[k] = curve_v[k], tab.cp[k] = curve_p[k];
  const int items = nh * HH_NS;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(hub_height_kernel, dim3((unsigned)g.nb, (unsigned)B), dim3(HH_BLOCK), 0, st, hr, hr_c, sr, sr_c, tl,
                     tl_c, z, terrain, tab, g, workspace, cols);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(hub_height_final_kernel, dim3((unsigned)((items + 63) / 64), (unsigned)B), dim3(HH_FBLOCK), 0, st,
                     workspace, g.nb, items, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
