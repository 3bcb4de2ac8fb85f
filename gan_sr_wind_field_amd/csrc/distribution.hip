// Wind-speed distribution and wind rose ([DISTRIBUTION]; distribution.py holds the definition): per sample, z level and
// source (HR, SR, TL) the joint count table speed bin x (direction sector, calm) of the horizontal wind.  All tensors
// fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0 and 1 are read.  dist_zero_kernel clears the integer tables
// in the workspace, ONE launch of dist_count_kernel reads every operand once and counts in LDS, dist_convert_kernel
// writes the counts as doubles.  Integer adds only: the same bits on every call.  The kernels are in
// distribution_kernels.h.
#include "common.h"
#include "distribution_kernels.h"

extern "C" int64_t wsr_level_distribution_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns,
                                                           int32_t nd) {
  DsGeom g{};
  if (ds_geom(g, B, X, Y, NZ, ns, nd) != 0) return 0;
  return ds_workspace_words(g);
}

extern "C" int wsr_level_distribution(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl,
                                      int32_t tl_c, const float* edge2, int32_t ns, const float* bx, const float* by,
                                      int32_t nd, float calm2, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                      void* workspace, double* out, void* stream) {
  if (!hr || !sr || !edge2 || !bx || !by || !workspace || !out || hr_c < 3 || sr_c < 3 || (tl && tl_c < 3))
    return WSR_EINVAL;
  DsGeom g{};
  if (const int rc = ds_geom(g, B, X, Y, NZ, ns, nd)) return rc;
  const long n = ds_workspace_words(g);
  const long nblocks = (n + DS_BLOCK - 1) / DS_BLOCK;
  if (nblocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  unsigned* table = static_cast<unsigned*>(workspace);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dist_zero_kernel, dim3((unsigned)nblocks), dim3(DS_BLOCK), 0, st, table, n);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(dist_count_kernel, dim3((unsigned)(g.ncb * g.nzc), tl ? 3u : 2u, (unsigned)B), dim3(DS_BLOCK), 0,
                     st, hr, hr_c, sr, sr_c, tl, tl_c, edge2, bx, by, calm2, g, table);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(dist_convert_kernel, dim3((unsigned)nblocks), dim3(DS_BLOCK), 0, st, table, n, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
