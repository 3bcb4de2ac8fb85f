// Runs the two kernels of csrc/ssim.hip (ssim_kernels.h with three fields) block by block on host threads, for the address
// and undefined-behaviour sanitisers, on the shim of tools/host_shim.h.  Every buffer is a heap allocation of exactly the
// size the C ABI documents - the three fields, the taps (win floats), the workspace and the sums - so an access outside
// one of them is reported; the LDS arrays are statics of the kernels' own sizes.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/ssim_host_check.cpp -o ssim_host_check
//   ./ssim_host_check B X Y NZ win sigma hr_c sr_c tl_c [dump.bin]
//
// The launches are those of wsr_level_ssim with data_range 2.  SR is HR plus noise, TL a copy of HR: the program checks
// that every result is finite and that the TL pair's sums equal the number of positions exactly.  With a last argument
// the operands and results are written as raw arrays - hr, sr, tl, taps (float32), out (float64) - for a comparison
// with ssim.level_ssim_reference.
#include "host_shim.h"

#include "../gan_sr_wind_field_amd/csrc/ssim_kernels.h"

int main(int argc, char** argv) {
  if (argc < 10) {
    fprintf(stderr, "usage: %s B X Y NZ win sigma hr_c sr_c tl_c [dump.bin]\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]), win = atoi(argv[5]);
  const double sigma = atof(argv[6]);
  const int hr_c = atoi(argv[7]), sr_c = atoi(argv[8]), tl_c = atoi(argv[9]);
  SsGeom g{};
  if (ss_geom(g, B, X, Y, NZ, win) != 0 || hr_c < 3 || sr_c < 3 || tl_c < 3 || !(sigma > 0)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const size_t vol = (size_t)X * Y * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // exact-size heap buffers, filled with NaN: the surplus channels and the unwritten workspace must never be read
  std::vector<float> hr((size_t)B * hr_c * vol, nan), sr((size_t)B * sr_c * vol, nan), tl((size_t)B * tl_c * vol, nan);
  std::vector<float> taps((size_t)win), ws((size_t)ss_workspace_floats<3>(g), nan);
  std::vector<double> out((size_t)B * NZ * 3 * ss_ns<3>, (double)nan);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (size_t i = 0; i < vol; ++i) {
        const float a = (float)uniform();
        hr[((size_t)b * hr_c + c) * vol + i] = a;
        sr[((size_t)b * sr_c + c) * vol + i] = (float)(a + 0.1 * uniform());
        tl[((size_t)b * tl_c + c) * vol + i] = a;
      }
  {
    std::vector<double> gd((size_t)win);
    double sum = 0.0;
    for (int k = 0; k < win; ++k) sum += gd[k] = exp(-(k - (win - 1) / 2.0) * (k - (win - 1) / 2.0) / (2.0 * sigma * sigma));
    for (int k = 0; k < win; ++k) taps[k] = (float)(gd[k] / sum);
  }
  const float c1 = (float)(0.02 * 0.02), c2 = (float)(0.06 * 0.06);
  launch(SS_BLOCK, (unsigned)(g.ntxy * g.nzc), 3, (unsigned)B, [&] {
    ssim_tile_kernel<3>(hr.data(), hr_c, sr.data(), sr_c, tl.data(), tl_c, taps.data(), c1, c2, g, ws.data());
  });
  launch(SS_FBLOCK, (unsigned)((g.ZC * ss_ns<3> + 63) / 64), (unsigned)(3 * g.nzc), (unsigned)B,
         [&] { ssim_final_kernel<3>(ws.data(), g, out.data()); });

  const double npos = (double)g.PX * g.PY;
  size_t bad = 0, off = 0;  // every sum written and finite; TL = HR: exactly npos
  for (size_t i = 0; i < out.size(); ++i) {
    bad += !isfinite(out[i]);
    if (i % ss_ns<3> >= 2) off += out[i] != npos;
  }
  if (argc > 10) {
    FILE* fp = fopen(argv[10], "wb");
    if (!fp) return 3;
    dump(fp, hr.data(), hr.size());
    dump(fp, sr.data(), sr.size());
    dump(fp, tl.data(), tl.size());
    dump(fp, taps.data(), taps.size());
    dump(fp, out.data(), out.size());
    fclose(fp);
  }
  printf("B %d X %d Y %d NZ %d win %d channels %d %d %d: tile %d x %d x %d, %d x %d x %d workgroups, %zu non-finite sums, "
         "%zu sums of the TL = HR pair off npos\n", B, X, Y, NZ, win, hr_c, sr_c, tl_c, g.TX, g.TY, g.ZC, g.ntx, g.nty, g.nzc,
         bad, off);
  return bad || off ? 1 : 0;
}
