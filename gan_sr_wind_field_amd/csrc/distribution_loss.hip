// The wind-speed distribution loss of generator training ([DISTRIBUTION_LOSS]; distribution_loss.py holds the definition):
// per source (HR, SR), sample and z level the soft (linearly binned) histogram of the horizontal wind speed in fixed point,
// H (2, B, NZ, ns + 1) in double (wsr_speed_soft_counts), and its vector-Jacobian product towards SR
// (wsr_speed_soft_counts_bwd).  All tensors fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0 and 1 are read.
// dl_zero_kernel clears the 64-bit integer tables in the workspace, ONE launch of dl_count_kernel reads every operand once
// and counts in LDS, dl_convert_kernel writes the counts as doubles.  Integer adds only: the same bits on every call.  The
// backward is one launch that recomputes the positions; nothing is saved by the forward.  The kernels are in
// distribution_loss_kernels.h.
#include "common.h"
#include "distribution_loss_kernels.h"

extern "C" int64_t wsr_speed_soft_counts_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns) {
  DlGeom g{};
  if (dl_geom(g, B, X, Y, NZ, ns) != 0) return 0;
  return 2 * dl_table_words(g);
}

extern "C" int wsr_speed_soft_counts_geometry(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t ns, int32_t* geom) {
  DlGeom g{};
  if (!geom) return WSR_EINVAL;
  if (const int rc = dl_geom(g, B, X, Y, NZ, ns)) return rc;
  geom[0] = g.CB, geom[1] = g.ncb, geom[2] = DL_BWD_ELEMS, geom[3] = g.nbwd;
  return 0;
}

extern "C" int wsr_speed_soft_counts(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, float c, int32_t ns,
                                     int32_t B, int32_t X, int32_t Y, int32_t NZ, void* workspace, double* out,
                                     void* stream) {
  if (!hr || !sr || !workspace || !out || hr_c < 2 || sr_c < 2) return WSR_EINVAL;
  if (!aligned_to(workspace, 8)) return WSR_EINVAL;
  if (!(c > 0.f) || !__builtin_isfinite(c)) return WSR_EINVAL;
  DlGeom g{};
  if (const int rc = dl_geom(g, B, X, Y, NZ, ns)) return rc;
  const long n = dl_table_words(g);
  const long nblocks = (n + DL_BLOCK - 1) / DL_BLOCK;
  if (nblocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  dl_u64* table = static_cast<dl_u64*>(workspace);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dl_zero_kernel, dim3((unsigned)nblocks), dim3(DL_BLOCK), 0, st, table, n);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(dl_count_kernel, dim3((unsigned)g.ncb, (unsigned)DL_SOURCES, (unsigned)B), dim3(DL_BLOCK), 0, st, hr,
                     hr_c, sr, sr_c, c, g, table);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(dl_convert_kernel, dim3((unsigned)nblocks), dim3(DL_BLOCK), 0, st, table, n, out);
  WSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int wsr_speed_soft_counts_bwd(const float* sr, int32_t sr_c, const float* gtab, float c, int32_t ns, int32_t B,
                                         int32_t X, int32_t Y, int32_t NZ, float* dsr, void* stream) {
  if (!sr || !gtab || !dsr || sr_c < 2) return WSR_EINVAL;
  if (!(c > 0.f) || !__builtin_isfinite(c)) return WSR_EINVAL;
  DlGeom g{};
  if (const int rc = dl_geom(g, B, X, Y, NZ, ns)) return rc;
  hipLaunchKernelGGL(dl_bwd_kernel, dim3((unsigned)g.nbwd, (unsigned)B), dim3(DL_BLOCK), 0, as_stream(stream), sr, sr_c,
                     gtab, c, g, dsr);
  WSR_LAUNCH_CHECK();
  return 0;
}
