// The energy-spectrum loss of generator training ([SPECTRAL_LOSS]): the binned horizontal kinetic-energy spectra of HR
// and SR, E (B, NZ, NK, 2) = [e_hr, e_sr] in double (wsr_spectral_energy), and the vector-Jacobian product of e_sr
// towards SR (wsr_spectral_energy_bwd).  The formulas are those of include/windsr_hip.h; the kernels, and what each pass
// does, are in spectrum_kernels.h (the forward, shared with csrc/spectra.hip and instantiated here for two fields, so e_hr
// and e_sr here carry the bits of wsr_level_spectra's) and spectral_loss_kernels.h (the backward).
//
// The backward reads F_sr as the forward's column pass saved it (B, 3, X, KY, NZ complex fp32) instead of transforming SR
// again: recomputing it is the forward's mean, row and column passes for three planes, half of the forward, against one
// write and one read of 8 X KY NZ 3 bytes per sample.
//
// Compiled without contraction, twiddles from per-workgroup LDS tables of double sincospi values indexed by a running
// integer (k i) mod n, fp32 transforms with explicit fmaf, no atomics, no zero fill, every sum in a fixed order: two calls
// give the same bits.  Grids and workspace offsets are functions of the shape alone.
#include "common.h"
#pragma clang fp contract(off)
#include <math.h>

#include "spectral_loss_kernels.h"

namespace {

constexpr int NF = 2;  // HR, SR

inline unsigned sl_blocks(int64_t n) { return (unsigned)((n + SP_BLOCK - 1) / SP_BLOCK); }

}  // namespace

extern "C" int64_t wsr_spectral_energy_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ) {
  SpGeom g{};
  if (sp_geom(g, NF, B, X, Y, NZ) != 0) return 0;
  return g.total_f > g.total_b ? g.total_f : g.total_b;
}

extern "C" int64_t wsr_spectral_energy_saved_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ) {
  SpGeom g{};
  if (sp_geom(g, NF, B, X, Y, NZ) != 0) return 0;
  return (int64_t)B * 3 * X * g.KY * NZ * 2;
}

extern "C" int wsr_spectral_energy(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, int32_t B, int32_t X,
                                   int32_t Y, int32_t NZ, int32_t window, float* workspace, float* saved, double* out,
                                   void* stream) {
  if (!hr || !sr || !workspace || !out || hr_c < 3 || sr_c < 3) return WSR_EINVAL;
  if (window != WSR_SPECTRUM_WINDOW_NONE && window != WSR_SPECTRUM_WINDOW_HANN) return WSR_EINVAL;
  SpGeom g{};
  const int rc = sp_geom(g, NF, B, X, Y, NZ);
  if (rc != 0) return rc;
  if (!aligned_to(workspace, 16) || (saved && !aligned_to(saved, 8))) return WSR_EINVAL;
  const SpFields f{{hr, sr, nullptr}, {hr_c, sr_c, 0}};
  int* bins = reinterpret_cast<int*>(workspace + g.o_bins);
  float *wx = workspace + g.o_wx, *wy = workspace + g.o_wy, *mpart = workspace + g.o_mean;
  float2* A = reinterpret_cast<float2*>(workspace + g.o_a);
  float* part = workspace + g.o_part;
  const double scale = 0.5 / ((double)X * (double)Y * sp_w2(X, Y, window));
  const hipStream_t st = as_stream(stream);
  const unsigned ub = (unsigned)B;
  hipLaunchKernelGGL(sp_prep_kernel, dim3(sl_blocks((int64_t)X * g.KY + X + Y)), dim3(SP_BLOCK), 0, st, g, (int)window, bins,
                     wx, wy, (const double*)nullptr, (float*)nullptr);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_mean_kernel, dim3((unsigned)(g.nzc1 * g.rb), sp_planes<NF>, ub), dim3(SP_BLOCK), 0, st, f, g, mpart);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_row_kernel<NF>, dim3((unsigned)(g.nxb * g.nzc2), sp_planes<NF>, ub), dim3(SP_BLOCK), 0, st, f, g, mpart, wx,
                     wy, A);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_col_kernel<NF>, dim3((unsigned)g.nzc3, (unsigned)g.KY, ub), dim3(SP_BLOCK), 0, st, g, bins, A, part,
                     reinterpret_cast<float2*>(saved));
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_final_kernel<NF>, dim3(sl_blocks((int64_t)g.NK * sp_ns<NF> * NZ), ub), dim3(SP_BLOCK), 0, st, g, part, scale,
                     out);
  WSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int wsr_spectral_energy_bwd(const float* saved, const double* gbin, int32_t B, int32_t X, int32_t Y, int32_t NZ,
                                       int32_t window, float* workspace, float* dsr, void* stream) {
  if (!saved || !gbin || !workspace || !dsr) return WSR_EINVAL;
  if (window != WSR_SPECTRUM_WINDOW_NONE && window != WSR_SPECTRUM_WINDOW_HANN) return WSR_EINVAL;
  SpGeom g{};
  const int rc = sp_geom(g, NF, B, X, Y, NZ);
  if (rc != 0) return rc;
  if (!aligned_to(workspace, 16) || !aligned_to(saved, 8) || !aligned_to(gbin, 8)) return WSR_EINVAL;
  int* bins = reinterpret_cast<int*>(workspace + g.o_bins);
  float *wx = workspace + g.o_wx, *wy = workspace + g.o_wy, *gf = workspace + g.o_gf;
  float2* Cw = reinterpret_cast<float2*>(workspace + g.o_c);
  float *mpart = workspace + g.o_mv, *mfin = workspace + g.o_mf;
  const double scale = 0.5 / ((double)X * (double)Y * sp_w2(X, Y, window));
  const SpFields f{{dsr, nullptr, nullptr}, {3, 0, 0}};
  const hipStream_t st = as_stream(stream);
  const unsigned ub = (unsigned)B;
  hipLaunchKernelGGL(sp_prep_kernel, dim3(sl_blocks((int64_t)X * g.KY + X + Y + (int64_t)B * g.NK * NZ)), dim3(SP_BLOCK), 0,
                     st, g, (int)window, bins, wx, wy, gbin, gf);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_icol_kernel, dim3((unsigned)(g.nzc4 * 3), (unsigned)g.KY, ub), dim3(SP_BLOCK), 0, st, g, bins, gf,
                     reinterpret_cast<const float2*>(saved), Cw);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_irow_kernel, dim3((unsigned)(g.nxb5 * g.nzc5), 3, ub), dim3(SP_BLOCK), 0, st, g, Cw, wx, wy,
                     (float)(2.0 * scale), dsr);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sp_mean_kernel, dim3((unsigned)(g.nzc1 * g.rb), 3, ub), dim3(SP_BLOCK), 0, st, f, g, mpart);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_mfin_kernel, dim3(sl_blocks((int64_t)B * 3 * NZ)), dim3(SP_BLOCK), 0, st, g, mpart, mfin);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_sub_kernel, dim3(sl_blocks((int64_t)X * Y * NZ), 3, ub), dim3(SP_BLOCK), 0, st, g, mfin, dsr);
  WSR_LAUNCH_CHECK();
  return 0;
}
