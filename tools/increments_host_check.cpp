//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/increments_host_check.cpp -o increments_host_check
//   ./increments_host_check B X Y NZ hr_c sr_c tl_c r1 [r2 ...]      (tl_c 0: no baseline; 1 .. 8 separations)
//
// Runs the two kernels of csrc/increments.hip block by block on host threads, for the address and undefined-behaviour
// sanitisers: the shim of tools/host_shim.h (__global__, __shared__ as a static array, one block at a time, threadIdx /
// blockIdx, __syncthreads as a pthread barrier).  Every buffer is a heap allocation of exactly the size the C ABI
// documents - the three fields, the workspace and the sums - so an access outside one of them is reported; the LDS array
// is a static of the kernel's own size.
//
// The launches are those of wsr_level_increments.  The fields are random components of standard deviation about 0.3,
// the surplus channels NaN (never read); workspace and sums start as NaN, so an element that a kernel leaves unwritten
// shows.  The program computes the same sums with a plain loop over the definition of increments.py (one fp32
// subtraction, every product rounded to fp32, double sums) and exits non-zero when a sum is further away than
// 16 sqrt(pairs) 2^-24 times the sum of its terms' magnitudes, when an entry without pairs or a sum of the absent
// baseline is not exactly zero, or when SR (a copy of HR with another channel count) does not give HR's bits.
#include "host_shim.h"

#include <string.h>

#include "../gan_sr_wind_field_amd/csrc/increments_kernels.h"

int main(int argc, char** argv) {
  if (argc < 9 || argc > 8 + INC_MAX_NR) {
    fprintf(stderr, "usage: %s B X Y NZ hr_c sr_c tl_c r1 [r2 ...]\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]);
  const int chan[3] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
  const int nr = argc - 8;
  int sep[INC_MAX_NR] = {0};
  for (int k = 0; k < nr; ++k) sep[k] = atoi(argv[8 + k]);
  IncGeom g{};
  if (inc_geom(g, B, X, Y, NZ, sep, nr) != 0 || chan[0] < 3 || chan[1] < 3 || (chan[2] != 0 && chan[2] < 3)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const int nsrc = chan[2] ? 3 : 2;
  const size_t vol = (size_t)X * Y * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN();

  // exact-size heap buffers; SR = HR in its first three channels, the surplus channels hold NaN and are never read
  std::vector<std::vector<float>> f((size_t)nsrc);
  for (int s = 0; s < nsrc; ++s) f[s].assign((size_t)B * chan[s] * vol, nan);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (size_t i = 0; i < vol; ++i) {
        const float v = (float)(0.52 * uniform());
        f[0][((size_t)b * chan[0] + c) * vol + i] = v;
        f[1][((size_t)b * chan[1] + c) * vol + i] = v;
        if (nsrc == 3) f[2][((size_t)b * chan[2] + c) * vol + i] = (float)(0.8 * v + 0.1 * uniform());
      }

  const size_t n_ws = (size_t)inc_workspace_floats(g), per_sample = (size_t)NZ * 3 * nr * 18, n_out = (size_t)B * per_sample;
  std::vector<float> ws(n_ws, nan);
  std::vector<double> out(n_out, (double)nan);
  launch(INC_BLOCK, (unsigned)(g.ntx * g.nty * g.nzc), (unsigned)(3 * nsrc), (unsigned)B, [&] {
    increments_kernel(f[0].data(), chan[0], f[1].data(), chan[1], nsrc == 3 ? f[2].data() : nullptr, chan[2], g, ws.data());
  });
  launch(INC_BLOCK, (unsigned)((per_sample + INC_BLOCK - 1) / INC_BLOCK), (unsigned)B, 1,
         [&] { increments_final_kernel(ws.data(), g, nsrc, out.data()); });

  // the definition, pair by pair
  std::vector<double> want(n_out, 0.0), mag(n_out, 0.0), pairs(n_out, 0.0);
  for (int b = 0; b < B; ++b)
    for (int z = 0; z < NZ; ++z)
      for (int s = 0; s < nsrc; ++s)
        for (int k = 0; k < nr; ++k)
          for (int a = 0; a < 2; ++a)
            for (int kind = 0; kind < 3; ++kind) {
              const int comp = kind == 2 ? 2 : (a == 0 ? kind : 1 - kind), r = sep[k];
              const float* p = f[s].data() + ((size_t)b * chan[s] + comp) * vol;
              double sum[3] = {0, 0, 0}, m[3] = {0, 0, 0}, n = 0;
              for (int x = 0; x + (a == 0 ? r : 0) < X; ++x)
                for (int y = 0; y + (a == 1 ? r : 0) < Y; ++y) {
                  const float lo = p[((size_t)x * Y + y) * NZ + z];
                  const float hi = p[((size_t)(x + (a == 0 ? r : 0)) * Y + y + (a == 1 ? r : 0)) * NZ + z];
                  const float d = hi - lo;
                  const float q = d * d;
                  const float cu = q * d, fo = q * q;
                  sum[0] += q, sum[1] += cu, sum[2] += fo;
                  m[0] += fabs((double)q), m[1] += fabs((double)cu), m[2] += fabs((double)fo);
                  n += 1;
                }
              for (int o = 0; o < 3; ++o) {
                const size_t i = ((((((size_t)b * NZ + z) * 3 + s) * nr + k) * 2 + a) * 3 + kind) * 3 + o;
                want[i] = sum[o], mag[i] = m[o], pairs[i] = n;
              }
            }
  size_t bad = 0, empty = 0, filled = 0;
  double worst = 0.0;
  for (size_t i = 0; i < n_out; ++i) {
    const double bound = pairs[i] > 0 ? 16.0 * sqrt(pairs[i]) * ldexp(1.0, -24) * mag[i] + ldexp(1.0, -100) : 0.0;
    const double err = fabs(out[i] - want[i]);
    (pairs[i] > 0 ? filled : empty) += 1;
    if (!(err <= bound)) {
      if (bad++ < 8) fprintf(stderr, "sum %zu: got %.17g want %.17g bound %.3g\n", i, out[i], want[i], bound);
    } else if (bound > 0 && mag[i] > 0) {
      worst = err / bound > worst ? err / bound : worst;
    }
  }
  size_t unequal = 0;  // SR = HR: the same bits
  for (int b = 0; b < B; ++b)
    for (int z = 0; z < NZ; ++z) {
      const double* h = out.data() + (((size_t)b * NZ + z) * 3 + 0) * nr * 18;
      unequal += memcmp(h, h + (size_t)nr * 18, sizeof(double) * nr * 18) != 0;
    }
  printf("B %d X %d Y %d NZ %d channels %d %d %d separations %d (largest %d): %d x %d tiles, %d chunks of %d levels, %zu "
         "entries with pairs and %zu without, %zu of %zu sums outside the bound (worst error / bound %.3g), %zu levels "
         "where SR differs from HR\n", B, X, Y, NZ, chan[0], chan[1], chan[2], nr, g.R, g.ntx, g.nty, g.nzc, g.ZC, filled,
         empty, bad, n_out, worst, unequal);
  return bad || unequal || filled == 0 ? 1 : 0;
}
