// Runs the kernels of csrc/ssim_loss.hip (ssim_kernels.h with two fields, ssim_loss_kernels.h) block by block on host
// threads, for the address and undefined-behaviour sanitisers, on the shim of tools/host_shim.h.  Every buffer is a heap
// allocation of exactly the size the C ABI documents - the two fields, the taps (win floats), the workspace, the sums,
// gout and dsr - so an access outside one of them is reported; the LDS arrays are statics of the kernels' own sizes.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/ssim_loss_host_check.cpp -o ssim_loss_host_check
//   ./ssim_loss_host_check                       (the built-in shapes)
//   ./ssim_loss_host_check B X Y NZ win sigma hr_c sr_c
//
// The launches are those of wsr_ssim_pair_sums and wsr_ssim_pair_sums_bwd with data_range 2.  SR is HR plus noise, gout
// random in both columns, dsr filled with NaN before the launch.  The program checks both sums against, and every
// gradient element against, a plain double loop over the definition (the moments of each position from the win x win
// pixels, the three coefficients, then for each pixel the sum over the positions whose window holds it), and, with SR a
// copy of HR, that every sum equals the number of positions exactly.  The built-in shapes hold a plane that is one
// tile, planes of several tiles with clipped border tiles, and a partial last z chunk.
#include "host_shim.h"

#include "../gan_sr_wind_field_amd/csrc/ssim_loss_kernels.h"

namespace {

// 0: fine
int run(int B, int X, int Y, int NZ, int win, double sigma, int hr_c, int sr_c) {
  SsGeom g{};
  SslBwdGeom gb{};
  if (ss_geom(g, B, X, Y, NZ, win) != 0 || ssl_bwd_geom(gb, B, X, Y, NZ, win) != 0 || hr_c < 3 || sr_c < 3 || !(sigma > 0)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const size_t vol = (size_t)X * Y * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // exact-size heap buffers, filled with NaN: the surplus channels and the unwritten workspace must never be read
  std::vector<float> hr((size_t)B * hr_c * vol, nan), sr((size_t)B * sr_c * vol, nan), same((size_t)B * 3 * vol);
  std::vector<float> taps((size_t)win), ws((size_t)ss_workspace_floats<2>(g), nan), dsr((size_t)B * 3 * vol, nan);
  std::vector<double> out((size_t)B * NZ * 3 * ss_ns<2>, (double)nan), out_same(out.size(), (double)nan), gout(out.size());
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (size_t i = 0; i < vol; ++i) {
        const float a = (float)uniform();
        hr[((size_t)b * hr_c + c) * vol + i] = a;
        sr[((size_t)b * sr_c + c) * vol + i] = (float)(a + 0.1 * uniform());
        same[((size_t)b * 3 + c) * vol + i] = a;
      }
  for (double& v : gout) v = uniform();
  std::vector<double> gd((size_t)win);
  {
    double sum = 0.0;
    for (int k = 0; k < win; ++k) sum += gd[k] = exp(-(k - (win - 1) / 2.0) * (k - (win - 1) / 2.0) / (2.0 * sigma * sigma));
    for (int k = 0; k < win; ++k) gd[k] = (double)(taps[k] = (float)(gd[k] / sum));
  }
  const float c1 = (float)(0.02 * 0.02), c2 = (float)(0.06 * 0.06);
  const unsigned fgrid = (unsigned)((g.ZC * ss_ns<2> + 63) / 64);
  launch(SS_BLOCK, (unsigned)(g.ntxy * g.nzc), 3, (unsigned)B,
         [&] { ssim_tile_kernel<2>(hr.data(), hr_c, sr.data(), sr_c, nullptr, 0, taps.data(), c1, c2, g, ws.data()); });
  launch(SS_FBLOCK, fgrid, (unsigned)(3 * g.nzc), (unsigned)B, [&] { ssim_final_kernel<2>(ws.data(), g, out.data()); });
  launch(SS_BLOCK, (unsigned)(gb.ntxy * gb.nzc), 3, (unsigned)B, [&] {
    ssl_bwd_kernel(hr.data(), hr_c, sr.data(), sr_c, gout.data(), taps.data(), c1, c2, gb, dsr.data());
  });
  // SR a copy of HR (three channels): every sum is the number of positions
  launch(SS_BLOCK, (unsigned)(g.ntxy * g.nzc), 3, (unsigned)B,
         [&] { ssim_tile_kernel<2>(hr.data(), hr_c, same.data(), 3, nullptr, 0, taps.data(), c1, c2, g, ws.data()); });
  launch(SS_FBLOCK, fgrid, (unsigned)(3 * g.nzc), (unsigned)B, [&] { ssim_final_kernel<2>(ws.data(), g, out_same.data()); });

  // ---- the definition, in double
  const int PX = g.PX, PY = g.PY;
  const double npos = (double)PX * PY;
  size_t bad_sum = 0, bad_same = 0, bad_grad = 0;
  double worst_sum = 0.0, worst_grad = 0.0;
  std::vector<double> al((size_t)PX * PY), be(al.size()), ga(al.size());
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (int z = 0; z < NZ; ++z) {
        const float* pa = hr.data() + ((size_t)b * hr_c + c) * vol;
        const float* ps = sr.data() + ((size_t)b * sr_c + c) * vol;
        auto at = [&](const float* p, int x, int y) { return (double)p[((size_t)x * Y + y) * NZ + z]; };
        const size_t gi = (((size_t)b * NZ + z) * 3 + c) * ss_ns<2>;
        const double G0 = (double)(float)gout[gi], G1 = (double)(float)gout[gi + 1];
        double s0 = 0.0, s1 = 0.0;
        for (int qx = 0; qx < PX; ++qx)
          for (int qy = 0; qy < PY; ++qy) {
            double ma = 0, ms = 0, aa = 0, ss = 0, as = 0;
            for (int i = 0; i < win; ++i)
              for (int j = 0; j < win; ++j) {
                const double w = gd[i] * gd[j], a = at(pa, qx + i, qy + j), s = at(ps, qx + i, qy + j);
                ma += w * a, ms += w * s, aa += w * a * a, ss += w * s * s, as += w * a * s;
              }
            const double d1 = ma * ma + ms * ms + c1, d2 = (aa - ma * ma) + (ss - ms * ms) + c2;
            const double l = (2 * ma * ms + c1) / d1, cs = (2 * (as - ma * ms) + c2) / d2;
            s0 += l * cs, s1 += cs;
            const double h = G0 * l + G1;
            al[(size_t)qx * PY + qy] = G0 * cs * (2 * ma - 2 * ms * l) / d1 + h * (2 * ms * cs - 2 * ma) / d2;
            be[(size_t)qx * PY + qy] = -h * cs / d2;
            ga[(size_t)qx * PY + qy] = 2 * h / d2;
          }
        const double want[2] = {s0, s1};
        for (int j = 0; j < 2; ++j) {
          const double err = fabs(out[gi + j] - want[j]) / npos;
          if (!(err <= 1e-4)) ++bad_sum;
          if (err > worst_sum) worst_sum = err;
          bad_same += out_same[gi + j] != npos;
        }
        double gmax = 0.0;
        std::vector<double> ref((size_t)X * Y);
        for (int px = 0; px < X; ++px)
          for (int py = 0; py < Y; ++py) {
            double A = 0, Bq = 0, C = 0;
            for (int i = 0; i < win; ++i)
              for (int j = 0; j < win; ++j) {
                const int qx = px - i, qy = py - j;
                if (qx < 0 || qx >= PX || qy < 0 || qy >= PY) continue;
                const double w = gd[i] * gd[j];
                const size_t q = (size_t)qx * PY + qy;
                A += w * al[q], Bq += w * be[q], C += w * ga[q];
              }
            const double v = A + 2 * at(ps, px, py) * Bq + at(pa, px, py) * C;
            ref[(size_t)px * Y + py] = v;
            if (fabs(v) > gmax) gmax = fabs(v);
          }
        const float* pd = dsr.data() + ((size_t)b * 3 + c) * vol;
        for (int px = 0; px < X; ++px)
          for (int py = 0; py < Y; ++py) {
            const double err = fabs((double)pd[((size_t)px * Y + py) * NZ + z] - ref[(size_t)px * Y + py]) / gmax;
            if (!(err <= 1e-4)) ++bad_grad;  // (a NaN - an element the kernel did not write - fails)
            if (err > worst_grad) worst_grad = err;
          }
      }
  printf("B %d X %d Y %d NZ %d win %d channels %d %d: fwd tile %d x %d x %d, bwd tile %d x %d x %d in %d x %d x %d workgroups; "
         "sums off by %.2e of npos at most (%zu bad), %zu sums of SR = HR off npos, gradient off by %.2e of the plane's "
         "largest at most (%zu bad)\n", B, X, Y, NZ, win, hr_c, sr_c, g.TX, g.TY, g.ZC, gb.TX, gb.TY, gb.ZC, gb.ntx, gb.nty,
         gb.nzc, worst_sum, bad_sum, bad_same, worst_grad, bad_grad);
  return bad_sum || bad_same || bad_grad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 9)
    return run(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atof(argv[6]), atoi(argv[7]),
               atoi(argv[8]));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [B X Y NZ win sigma hr_c sr_c]\n", argv[0]);
    return 2;
  }
  int rc = 0;
  rc |= run(2, 7, 6, 5, 3, 1.0, 3, 5);      // one tile, surplus channels
  rc |= run(1, 3, 3, 4, 3, 0.8, 4, 3);      // one position
  rc |= run(1, 16, 16, 10, 11, 1.5, 3, 3);  // a window wider than the tile: every tile is a border tile
  rc |= run(1, 40, 12, 8, 7, 1.0, 3, 3);    // several tiles along x, the last one clipped
  rc |= run(1, 13, 12, 19, 5, 1.2, 3, 4);   // a partial last z chunk
  rc |= run(1, 17, 15, 4, 15, 2.0, 3, 3);   // the largest window
  return rc;
}
