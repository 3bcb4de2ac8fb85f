//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/distribution_loss_host_check.cpp -o distribution_loss_host_check
//   ./distribution_loss_host_check                          (the built-in shapes)
//   ./distribution_loss_host_check B X Y NZ speed_bins hr_c sr_c
//
// Runs the kernels of csrc/distribution_loss.hip block by block on host threads, for the address and undefined-behaviour
// sanitisers: the shim of tools/host_shim.h (__global__, __shared__ as a static array, one block at a time, threadIdx /
// blockIdx, __syncthreads as a pthread barrier) with its integer add for the 32-bit LDS counters and the 64-bit tables,
// and sqrtf (correctly rounded) for the square root.  Every buffer is a heap allocation of exactly the size the C ABI
// documents - the two fields, the workspace, the tables, the upstream table and dsr - so an access outside one of them is
// reported; the LDS arrays are statics of the kernels' own sizes.
//
// The launches are those of wsr_speed_soft_counts and wsr_speed_soft_counts_bwd with c = 32 / 1.5.  HR and SR hold random
// vectors whose speeds span both clamps and, at the first and the last voxels of every sample, the special voxels of the
// tests: below the first centre, beyond the last centre, exactly on a centre, zeros, NaN and +-Inf.  dsr is filled with
// NaN before the launch.  The program computes the same integers and the same gradient with a plain loop over the
// definition of distribution_loss.py and exits non-zero on any differing count, on a row that does not sum to
// X * Y * 65536, on a gradient element that differs (the loop is the kernel's arithmetic: bit for bit) or was not written.
#include "host_shim.h"

#include <string.h>

#define DL_LDS_ADD(p, v) HOST_SHIM_ADD((p), (v))
#define DL_GLOBAL_ADD(p, v) HOST_SHIM_ADD((p), (v))
#define DL_SQRT(x) sqrtf(x)

#include "../gan_sr_wind_field_amd/csrc/distribution_loss_kernels.h"

namespace {

// the definition for one voxel: false when hs2 is not finite; else t before the clamp, k0 and fi
bool position(float u, float v, float c, int ns, float& t, float& r, int& k0, unsigned& fi) {
  const float uu = u * u, vv = v * v;
  const float hs2 = uu + vv;
  if (!std::isfinite(hs2)) return false;
  r = sqrtf(hs2);
  const float rc = r * c;
  t = rc - 0.5f;
  float p = t < 0.f ? 0.f : t;
  p = p > (float)(ns - 1) ? (float)(ns - 1) : p;
  k0 = (int)floorf(p);
  if (k0 > ns - 2) k0 = ns - 2;
  fi = (unsigned)rintf((p - (float)k0) * 65536.f);
  return true;
}

// 0: fine
int run(int B, int X, int Y, int NZ, int ns, int hr_c, int sr_c) {
  DlGeom g{};
  if (dl_geom(g, B, X, Y, NZ, ns) != 0 || hr_c < 2 || sr_c < 2) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const int chan[2] = {hr_c, sr_c};
  const size_t vol = (size_t)g.vol;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float c = (float)(32.0 / 1.5);
  const float centre3 = 3.5f / c;  // (close to the centre of bin 3)
  const float special[][2] = {
      {0.f, 0.f}, {-0.f, 0.f}, {0.25f / c, 0.f}, {0.f, -0.5f / c}, {centre3, 0.f}, {0.f, 1.5f / c},
      {((float)ns + 3.f) / c, 0.f}, {0.f, -((float)ns - 0.5f) / c}, {nan, 0.1f}, {0.1f, nan}, {inf, 0.f}, {-inf, inf},
      {3e38f, 3e38f}, {1e-30f, -1e-30f}, {0.75f / c, 0.75f / c}};
  const size_t K = sizeof(special) / sizeof(special[0]);
  const double span = 1.2 * ns / c / 1.5;  // (a sum of three uniforms: speeds up to beyond the last centre)
  std::vector<std::vector<float>> f(2);
  for (int s = 0; s < 2; ++s) {
    f[s].assign((size_t)B * chan[s] * vol, nan);  // (the surplus channels are never read)
    for (int b = 0; b < B; ++b) {
      float* pu = f[s].data() + ((size_t)b * chan[s] + 0) * vol;
      float* pv = f[s].data() + ((size_t)b * chan[s] + 1) * vol;
      for (size_t i = 0; i < vol; ++i) {
        pu[i] = (float)(span * (uniform() + uniform() + uniform()) / 3.0);
        pv[i] = (float)(span * (uniform() + uniform() + uniform()) / 3.0);
      }
      for (size_t k = 0; k < K; ++k) {
        const size_t rot = (k + (size_t)s) % K;  // (the sources differ)
        const size_t first = k % vol, last = vol - 1 - k % vol;
        pu[first] = special[rot][0], pv[first] = special[rot][1];
        pu[last] = special[(rot + 5) % K][0], pv[last] = special[(rot + 5) % K][1];
      }
    }
  }
  const size_t words = (size_t)dl_table_words(g);
  std::vector<dl_u64> ws(words, 0xdeadbeefdeadbeefull);
  std::vector<double> out(words, (double)nan);
  const unsigned nblocks = (unsigned)((words + DL_BLOCK - 1) / DL_BLOCK);
  launch(DL_BLOCK, nblocks, 1, 1, [&] { dl_zero_kernel(ws.data(), (long)words); });
  launch(DL_BLOCK, (unsigned)g.ncb, (unsigned)DL_SOURCES, (unsigned)B,
         [&] { dl_count_kernel(f[0].data(), chan[0], f[1].data(), chan[1], c, g, ws.data()); });
  launch(DL_BLOCK, nblocks, 1, 1, [&] { dl_convert_kernel(ws.data(), (long)words, out.data()); });

  std::vector<dl_u64> want(words, 0ull);
  for (int s = 0; s < 2; ++s)
    for (int b = 0; b < B; ++b) {
      const float* pu = f[s].data() + ((size_t)b * chan[s] + 0) * vol;
      const float* pv = f[s].data() + ((size_t)b * chan[s] + 1) * vol;
      for (size_t i = 0; i < vol; ++i) {
        dl_u64* row = want.data() + (((size_t)s * B + b) * NZ + i % (size_t)NZ) * g.T;
        float t, r;
        int k0;
        unsigned fi;
        if (!position(pu[i], pv[i], c, ns, t, r, k0, fi)) {
          row[ns] += 65536ull;
          continue;
        }
        row[k0] += 65536ull - fi, row[k0 + 1] += fi;
      }
    }
  size_t differ = 0, badsum = 0, badout = 0;
  for (size_t i = 0; i < words; ++i) {
    differ += ws[i] != want[i];
    badout += !(out[i] == (double)want[i] / 65536.0);
  }
  for (size_t row = 0; row < (size_t)2 * B * NZ; ++row) {
    dl_u64 sum = 0;
    for (int k = 0; k < g.T; ++k) sum += ws[row * g.T + k];
    badsum += sum != (dl_u64)X * Y * 65536ull;
  }

  // the backward: a random upstream table, dsr filled with NaN
  std::vector<float> gtab((size_t)B * NZ * ns), dsr((size_t)B * sr_c * vol, nan);
  for (auto& v : gtab) v = (float)uniform();
  launch(DL_BLOCK, (unsigned)g.nbwd, (unsigned)B, 1, [&] { dl_bwd_kernel(f[1].data(), sr_c, gtab.data(), c, g, dsr.data()); });
  size_t gdiffer = 0, unwritten = 0, live = 0;
  for (int b = 0; b < B; ++b) {
    const float* pu = f[1].data() + ((size_t)b * sr_c + 0) * vol;
    const float* pv = pu + vol;
    for (size_t i = 0; i < vol; ++i) {
      float gu = 0.f, gv = 0.f, t, r;
      int k0;
      unsigned fi;
      if (position(pu[i], pv[i], c, ns, t, r, k0, fi) && t > 0.f && t < (float)(ns - 1) && r > 0.f) {
        const float* row = gtab.data() + ((size_t)b * NZ + i % (size_t)NZ) * ns;
        const float d = row[k0 + 1] - row[k0];
        const float dc = d * c;
        const float du = dc * pu[i], dv = dc * pv[i];
        gu = du / r, gv = dv / r;
        ++live;
      }
      for (int ch = 0; ch < sr_c; ++ch) {
        const float got = dsr[((size_t)b * sr_c + ch) * vol + i];
        const float ref = ch == 0 ? gu : (ch == 1 ? gv : 0.f);
        unwritten += std::isnan(got);
        gdiffer += memcmp(&got, &ref, sizeof(float)) != 0 && !(got == 0.f && ref == 0.f);
      }
    }
  }
  printf("B %d X %d Y %d NZ %d bins %d channels %d %d: %d columns x %d ranges, %d backward ranges; %zu counts differ, %zu "
         "outputs differ, %zu rows with a wrong sum; %zu of %zu voxels carry gradient, %zu gradient elements differ, %zu "
         "unwritten\n", B, X, Y, NZ, ns, hr_c, sr_c, g.CB, g.ncb, g.nbwd, differ, badout, badsum, live, (size_t)B * vol, gdiffer,
         unwritten);
  return differ || badout || badsum || gdiffer || unwritten || live == 0 ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 8)
    return run(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [B X Y NZ speed_bins hr_c sr_c]\n", argv[0]);
    return 2;
  }
  // odd sizes; the reference's patch with a surplus channel; the largest LDS table; two bins; several column ranges and
  // several backward ranges per sample
  const int shapes[][7] = {{2, 5, 7, 3, 32, 3, 3}, {1, 16, 16, 10, 32, 3, 4}, {1, 8, 8, 128, 64, 3, 3},
                           {2, 6, 5, 4, 2, 2, 5}, {1, 64, 64, 10, 32, 3, 3}};
  int rc = 0;
  for (const auto& s : shapes) rc |= run(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
  return rc;
}
