// Fractions skill score ([FSS]; fss.py holds the definition): per sample, z level, exceedance threshold of the horizontal
// wind speed and neighbourhood size the five sums over the plane of the squared box-window event counts of HR, SR and TL
// and of their squared differences.  All tensors fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0 and 1 are
// read.  fss_zero_kernel clears the 64-bit integer table in the workspace, ONE launch of fss_count_kernel reads every
// operand once per tile (with its halo), classifies in LDS and takes the counts of all neighbourhoods from one table of
// running sums per threshold, fss_convert_kernel writes the sums as doubles.  Integer adds only: the same bits on every
// call.  The kernels are in fss_kernels.h.
#include "common.h"
#include "fss_kernels.h"

extern "C" int64_t wsr_level_fss_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t nt, int32_t nn,
                                                  int32_t max_n) {
  if (nn < 1 || nn > FS_MAX_NN || max_n < 1 || max_n > WSR_FSS_MAX_SCALE || !(max_n & 1) || (nn == 1) != (max_n == 1))
    return 0;
  // (the size depends on the number of neighbourhoods alone: any valid list of nn scales that ends in max_n)
  int scales[FS_MAX_NN];
  for (int k = 0; k < nn; ++k) scales[k] = 2 * k + 1;
  if (scales[nn - 1] > max_n) return 0;
  scales[nn - 1] = max_n;
  FsGeom g{};
  if (fs_geom(g, B, X, Y, NZ, nt, scales, nn) != 0) return 0;
  return 2 * fs_table_entries(g);
}

extern "C" int wsr_level_fss(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl, int32_t tl_c,
                             const float* thr2, int32_t nt, const int32_t* scales, int32_t nn, int32_t B, int32_t X,
                             int32_t Y, int32_t NZ, double* out, void* workspace, void* stream) {
  if (!hr || !sr || !thr2 || !scales || !workspace || !out || hr_c < 3 || sr_c < 3 || (tl && tl_c < 3)) return WSR_EINVAL;
  if (!aligned_to(workspace, 8)) return WSR_EINVAL;
  FsGeom g{};
  if (const int rc = fs_geom(g, B, X, Y, NZ, nt, scales, nn)) return rc;
  const long n = fs_table_entries(g);
  const long nblocks = (n + FS_BLOCK - 1) / FS_BLOCK;
  if (nblocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  fs_u64* table = static_cast<fs_u64*>(workspace);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(fss_zero_kernel, dim3((unsigned)nblocks), dim3(FS_BLOCK), 0, st, table, n);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fss_count_kernel, dim3((unsigned)(g.ntx * g.nty * g.nzc), 1u, (unsigned)B), dim3(FS_BLOCK), 0, st, hr,
                     hr_c, sr, sr_c, tl, tl_c, thr2, g, table);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(fss_convert_kernel, dim3((unsigned)nblocks), dim3(FS_BLOCK), 0, st, table, n, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
