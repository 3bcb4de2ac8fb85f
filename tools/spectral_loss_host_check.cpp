// Runs every kernel of csrc/spectral_loss.hip, and the forward of csrc/spectra.hip, block by block on 256 host threads,
// for the address and undefined-behaviour sanitisers, on the shim of tools/host_shim.h with float2 / float4, sinpi and
// sincospi added.  Every buffer is a heap allocation of exactly the size the C ABI documents, so an access outside the
// workspace, the saved spectrum, the output or an LDS array is reported.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/spectral_loss_host_check.cpp -o spectral_loss_host_check
//   ./spectral_loss_host_check B X Y NZ window hr_c sr_c [dump.bin]
//
// window: 0 none, 1 hann.  The launches are those of wsr_spectral_energy and wsr_spectral_energy_bwd.  With a last
// argument the operands and results are written as raw arrays - hr, sr (float32), gbin, out (float64), saved, dsr
// (float32) - for a comparison with a float64 evaluation of the formulas.
//
// Then the launches of wsr_level_spectra (the same kernels with three fields) on the same HR and SR with TL = HR: every
// sum must be finite, and e_tl and c_tl must equal e_hr bit for bit.
#include <string.h>

#include "host_shim.h"

struct float2 {
  float x, y;
};
struct alignas(16) float4 {
  float x, y, z, w;
};
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline void sl_host_sincospi(double x, double* s, double* c) { *s = sin(M_PI * x), *c = cos(M_PI * x); }
static inline double sl_host_sinpi(double x) { return sin(M_PI * x); }
#define sincospi sl_host_sincospi
#define sinpi sl_host_sinpi

#include "../gan_sr_wind_field_amd/csrc/spectral_loss_kernels.h"

namespace {

unsigned blocks(int64_t n) { return (unsigned)((n + SP_BLOCK - 1) / SP_BLOCK); }

// the five launches of the forward with NF fields; saved may be null
template <int NF>
void forward(const SpGeom& g, const SpFields& f, int window, float* w, float2* saved, double* out) {
  int* bins = reinterpret_cast<int*>(w + g.o_bins);
  float *wx = w + g.o_wx, *wy = w + g.o_wy, *mpart = w + g.o_mean, *part = w + g.o_part;
  float2* A = reinterpret_cast<float2*>(w + g.o_a);
  const int X = g.X, Y = g.Y, NZ = g.NZ;
  const unsigned ub = (unsigned)g.B;
  const double scale = 0.5 / ((double)X * (double)Y * sp_w2(X, Y, window));
  launch(SP_BLOCK, blocks((int64_t)X * g.KY + X + Y), 1, 1, [&] { sp_prep_kernel(g, window, bins, wx, wy, nullptr, nullptr); });
  launch(SP_BLOCK, (unsigned)(g.nzc1 * g.rb), sp_planes<NF>, ub, [&] { sp_mean_kernel(f, g, mpart); });
  launch(SP_BLOCK, (unsigned)(g.nxb * g.nzc2), sp_planes<NF>, ub, [&] { sp_row_kernel<NF>(f, g, mpart, wx, wy, A); });
  launch(SP_BLOCK, (unsigned)g.nzc3, (unsigned)g.KY, ub, [&] { sp_col_kernel<NF>(g, bins, A, part, saved); });
  launch(SP_BLOCK, blocks((int64_t)g.NK * sp_ns<NF> * NZ), ub, 1, [&] { sp_final_kernel<NF>(g, part, scale, out); });
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s B X Y NZ window hr_c sr_c [dump.bin]\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]), window = atoi(argv[5]);
  const int hr_c = atoi(argv[6]), sr_c = atoi(argv[7]);
  SpGeom g{}, g3{};
  if (sp_geom(g, 2, B, X, Y, NZ) != 0 || sp_geom(g3, 3, B, X, Y, NZ) != 0 || hr_c < 3 || sr_c < 3 ||
      (window != 0 && window != 1)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const size_t vol = (size_t)X * Y * NZ;
  const size_t n_saved = (size_t)B * 3 * X * g.KY * NZ * 2, n_out = (size_t)B * NZ * g.NK * sp_ns<2>;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // exact-size heap buffers; the workspace of each entry its own, filled with NaN: nothing is carried across
  std::vector<float> hr((size_t)B * hr_c * vol, nan), sr((size_t)B * sr_c * vol, nan), saved(n_saved, nan);
  std::vector<float> ws_f((size_t)g.total_f, nan), ws_b((size_t)g.total_b, nan), dsr((size_t)B * 3 * vol, nan);
  std::vector<double> out(n_out, (double)nan), gbin((size_t)B * NZ * g.NK);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (size_t i = 0; i < vol; ++i) {
        hr[((size_t)b * hr_c + c) * vol + i] = (float)(uniform() + 0.5 * c);
        sr[((size_t)b * sr_c + c) * vol + i] = (float)(uniform() * 1.5 - 0.25 * c);
      }
  for (double& v : gbin) v = uniform();

  // ---- wsr_spectral_energy
  forward<2>(g, SpFields{{hr.data(), sr.data(), nullptr}, {hr_c, sr_c, 0}}, window, ws_f.data(),
             reinterpret_cast<float2*>(saved.data()), out.data());
  {  // ---- wsr_spectral_energy_bwd
    float* w = ws_b.data();
    int* bins = reinterpret_cast<int*>(w + g.o_bins);
    float *wx = w + g.o_wx, *wy = w + g.o_wy, *gf = w + g.o_gf, *mpart = w + g.o_mv, *mfin = w + g.o_mf;
    float2* Cw = reinterpret_cast<float2*>(w + g.o_c);
    const float2* sv = reinterpret_cast<const float2*>(saved.data());
    const double scale = 0.5 / ((double)X * (double)Y * sp_w2(X, Y, window));
    const SpFields fd{{dsr.data(), nullptr, nullptr}, {3, 0, 0}};
    launch(SP_BLOCK, blocks((int64_t)X * g.KY + X + Y + (int64_t)B * g.NK * NZ), 1, 1,
           [&] { sp_prep_kernel(g, window, bins, wx, wy, gbin.data(), gf); });
    launch(SP_BLOCK, (unsigned)(g.nzc4 * 3), (unsigned)g.KY, (unsigned)B, [&] { sl_icol_kernel(g, bins, gf, sv, Cw); });
    launch(SP_BLOCK, (unsigned)(g.nxb5 * g.nzc5), 3, (unsigned)B,
           [&] { sl_irow_kernel(g, Cw, wx, wy, (float)(2.0 * scale), dsr.data()); });
    launch(SP_BLOCK, (unsigned)(g.nzc1 * g.rb), 3, (unsigned)B, [&] { sp_mean_kernel(fd, g, mpart); });
    launch(SP_BLOCK, blocks((int64_t)B * 3 * NZ), 1, 1, [&] { sl_mfin_kernel(g, mpart, mfin); });
    launch(SP_BLOCK, blocks((int64_t)vol), 3, (unsigned)B, [&] { sl_sub_kernel(g, mfin, dsr.data()); });
  }
  size_t bad = 0;  // every element of the results written, and finite: the surplus channels' NaN never read
  for (double v : out) bad += !isfinite(v);
  for (float v : saved) bad += !isfinite(v);
  for (float v : dsr) bad += !isfinite(v);
  if (argc > 8) {
    FILE* fp = fopen(argv[8], "wb");
    if (!fp) return 3;
    dump(fp, hr.data(), hr.size());
    dump(fp, sr.data(), sr.size());
    dump(fp, gbin.data(), gbin.size());
    dump(fp, out.data(), out.size());
    dump(fp, saved.data(), saved.size());
    dump(fp, dsr.data(), dsr.size());
    fclose(fp);
  }
  printf("B %d X %d Y %d NZ %d window %d channels %d %d: NK %d, %zu non-finite results\n", B, X, Y, NZ, window, hr_c, sr_c,
         g.NK, bad);

  // ---- wsr_level_spectra with TL = HR
  std::vector<float> ws3((size_t)g3.total_f, nan);
  std::vector<double> out3((size_t)B * NZ * g3.NK * sp_ns<3>, (double)nan);
  forward<3>(g3, SpFields{{hr.data(), sr.data(), hr.data()}, {hr_c, sr_c, hr_c}}, window, ws3.data(), nullptr, out3.data());
  size_t bad3 = 0, off3 = 0;  // sums of a bin: e_hr, e_sr, e_tl, c_sr, c_tl
  for (size_t i = 0; i < out3.size(); i += sp_ns<3>) {
    const double* s = &out3[i];
    for (int k = 0; k < sp_ns<3>; ++k) bad3 += !isfinite(s[k]);
    off3 += memcmp(&s[2], &s[0], sizeof(double)) != 0;
    off3 += memcmp(&s[4], &s[0], sizeof(double)) != 0;
  }
  printf("three fields, TL = HR: %zu non-finite sums, %zu of e_tl and c_tl not the bits of e_hr\n", bad3, off3);
  return bad || bad3 || off3 ? 1 : 0;
}
