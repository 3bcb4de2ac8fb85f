// Structure functions ([INCREMENTS]; increments.py holds the definition): per sample, z level, source (HR, SR, TL),
// separation, direction (x, y), kind (longitudinal, transverse, vertical component) and order (2, 3, 4) the sum over the
// plane of the powers of the increments f(p + r e_a) - f(p), every pair with both ends inside the plane.  All tensors fp32
// planar (B, C, X, Y, NZ), z innermost; only channels 0, 1 and 2 are read.  ONE launch of increments_kernel stages every
// tile once per component with a forward halo in LDS, takes the increments of all separations from there and writes one
// partial row per workgroup; increments_final_kernel adds the rows in double.  No atomics: the same bits on every call.
// The kernels are in increments_kernels.h.
#include "common.h"
#include "increments_kernels.h"

extern "C" int64_t wsr_level_increments_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                                         const int32_t* separations, int32_t nr) {
  IncGeom g{};
  if (inc_geom(g, B, X, Y, NZ, separations, nr) != 0) return 0;
  return inc_workspace_floats(g);
}

extern "C" int wsr_level_increments(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl,
                                    int32_t tl_c, const int32_t* separations, int32_t nr, int32_t B, int32_t X, int32_t Y,
                                    int32_t NZ, float* workspace, double* out, void* stream) {
  if (!hr || !sr || !separations || !workspace || !out || hr_c < 3 || sr_c < 3 || (tl && tl_c < 3)) return WSR_EINVAL;
  IncGeom g{};
  if (const int rc = inc_geom(g, B, X, Y, NZ, separations, nr)) return rc;
  const int nsrc = tl ? 3 : 2;
  const long per_sample = (long)NZ * 3 * nr * 18;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(increments_kernel, dim3((unsigned)(g.ntx * g.nty * g.nzc), (unsigned)(3 * nsrc), (unsigned)B),
                     dim3(INC_BLOCK), 0, st, hr, hr_c, sr, sr_c, tl, tl_c, g, workspace);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(increments_final_kernel, dim3((unsigned)((per_sample + INC_BLOCK - 1) / INC_BLOCK), (unsigned)B),
                     dim3(INC_BLOCK), 0, st, workspace, g, nsrc, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
