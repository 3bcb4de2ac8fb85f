// Horizontal energy spectra ([SPECTRUM]): per sample, z level and wavenumber bin the kinetic energy of HR, SR and the
// trilinear baseline TL and the co-spectra of HR with SR and with TL, from one 2-D DFT over (X, Y) of every (sample,
// field, component, level) plane.  All tensors fp32 planar (B, C, X, Y, NZ), z innermost; only channels 0..2 are read.
// The formulas are those of include/windsr_hip.h (wsr_level_spectra).
//
// The five launches - prep, mean, row, column, final - and what each does are in spectrum_kernels.h, instantiated here
// for three fields; csrc/spectral_loss.hip instantiates the same kernels for two, so e_hr and e_sr of both carry the same
// bits.
#include "common.h"
#pragma clang fp contract(off)
#include <math.h>

#include "spectrum_kernels.h"

namespace {

constexpr int NF = 3;  // HR, SR, TL

}  // namespace

extern "C" int32_t wsr_level_spectra_bins(int32_t X, int32_t Y) {
  if (X <= 0 || Y <= 0 || X > SP_MAX_XY || Y > SP_MAX_XY) return 0;
  return sp_bins(X, Y);
}

extern "C" int64_t wsr_level_spectra_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ) {
  SpGeom g{};
  if (sp_geom(g, NF, B, X, Y, NZ) != 0) return 0;
  return g.total_f;
}

extern "C" int wsr_level_spectra(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl,
                                 int32_t tl_c, int32_t B, int32_t X, int32_t Y, int32_t NZ, int32_t window,
                                 float* workspace, double* out, void* stream) {
  if (!hr || !sr || !tl || !workspace || !out || hr_c < 3 || sr_c < 3 || tl_c < 3) return WSR_EINVAL;
  if (window != WSR_SPECTRUM_WINDOW_NONE && window != WSR_SPECTRUM_WINDOW_HANN) return WSR_EINVAL;
  SpGeom g{};
  const int rc = sp_geom(g, NF, B, X, Y, NZ);
  if (rc != 0) return rc;
  if (!aligned_to(workspace, 16)) return WSR_EINVAL;
  const SpFields f{{hr, sr, tl}, {hr_c, sr_c, tl_c}};
  int* bins = reinterpret_cast<int*>(workspace + g.o_bins);
  float *wx = workspace + g.o_wx, *wy = workspace + g.o_wy, *mpart = workspace + g.o_mean;
  float2* A = reinterpret_cast<float2*>(workspace + g.o_a);
  float* part = workspace + g.o_part;
  const double scale = 0.5 / ((double)X * (double)Y * sp_w2(X, Y, window));
  const hipStream_t st = as_stream(stream);
  const unsigned ub = (unsigned)B;
  hipLaunchKernelGGL(sp_prep_kernel, dim3((unsigned)((X * g.KY + X + Y + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0,
                     st, g, (int)window, bins, wx, wy, (const double*)nullptr, (float*)nullptr);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_mean_kernel, dim3((unsigned)(g.nzc1 * g.rb), sp_planes<NF>, ub), dim3(SP_BLOCK), 0, st, f, g, mpart);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_row_kernel<NF>, dim3((unsigned)(g.nxb * g.nzc2), sp_planes<NF>, ub), dim3(SP_BLOCK), 0, st, f, g,
                     mpart, wx, wy, A);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_col_kernel<NF>, dim3((unsigned)g.nzc3, (unsigned)g.KY, ub), dim3(SP_BLOCK), 0, st, g, bins, A, part,
                     (float2*)nullptr);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_final_kernel<NF>, dim3((unsigned)((g.NK * sp_ns<NF> * NZ + SP_BLOCK - 1) / SP_BLOCK), ub),
                     dim3(SP_BLOCK), 0, st, g, part, scale, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
