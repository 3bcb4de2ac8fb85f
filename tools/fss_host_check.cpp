//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/fss_host_check.cpp -o fss_host_check
//   ./fss_host_check B X Y NZ hr_c sr_c tl_c nt scale [scale ...]      (tl_c 0: no baseline; nt thresholds 1 .. 8)
//
// Runs the three kernels of csrc/fss.hip block by block on host threads, for the address and undefined-behaviour
// sanitisers: the shim of tools/host_shim.h (__global__, __shared__ as a static array, one block at a time, threadIdx /
// blockIdx, __syncthreads as a pthread barrier) with the LDS and global integer adds (__atomic_fetch_add) and the wave sum
// (every host thread is a wave of its own: the sum is its value, and every thread is a leader).  Every buffer is a heap allocation
// of exactly the size the C ABI documents - the three fields, the nt thresholds, the workspace and the sums - so an
// access outside one of them is reported; the LDS arrays are statics of the kernels' own sizes.
//
// The launches are those of wsr_level_fss with UVW_MAX 32 and the thresholds 4, 8, 10, 12, ... m/s.  HR, SR and TL hold
// random vectors (a sum of uniforms of standard deviation about 0.25) and, at the first and the last voxels of every
// sample, on both sides of the first tile boundary and of the first level-chunk boundary, the special voxels of the
// tests: a tie with the threshold 8 (u = 0.25, v = 0), values next to it, zeros, NaN and +-Inf.  The program computes
// the same sums with a plain loop over the definition of fss.py (every box clipped to the plane, position by position)
// and exits non-zero on any differing sum and on an entry of the absent baseline that is not zero.
#include "host_shim.h"

#define FS_LDS_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define FS_GLOBAL_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define FS_WAVE_SUM(v) (v)
#define FS_WAVE_LEADER(t) true

#include "../gan_sr_wind_field_amd/csrc/fss_kernels.h"

int main(int argc, char** argv) {
  if (argc < 10) {
    fprintf(stderr, "usage: %s B X Y NZ hr_c sr_c tl_c nt scale [scale ...]\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]);
  const int chan[3] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
  const int nt = atoi(argv[8]), nn = argc - 9;
  std::vector<int> scales((size_t)nn);
  for (int k = 0; k < nn; ++k) scales[k] = atoi(argv[9 + k]);
  FsGeom g{};
  if (nn > FS_MAX_NN || fs_geom(g, B, X, Y, NZ, nt, scales.data(), nn) != 0 || chan[0] < 3 || chan[1] < 3 ||
      (chan[2] != 0 && chan[2] < 3)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const int nsrc = chan[2] ? 3 : 2;
  const size_t vol = (size_t)X * Y * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const double uvw = 32.0;
  const double thr_ms[8] = {4, 8, 10, 12, 14, 16, 18, 20};
  std::vector<float> thr2((size_t)nt);
  for (int q = 0; q < nt; ++q) thr2[q] = (float)((thr_ms[q] / uvw) * (thr_ms[q] / uvw));
  const float below = nextafterf(0.25f, 0.f), above = nextafterf(0.25f, 1.f);
  const float special[][2] = {{0.25f, 0.f}, {0.f, -0.25f}, {below, 0.f}, {above, 0.f}, {0.f, 0.f}, {-0.f, 0.f},
                              {nan, 0.9f}, {0.9f, nan}, {nan, nan}, {inf, 0.f}, {0.f, -inf}, {-inf, inf}, {inf, nan},
                              {1e-30f, -1e-30f}, {3e38f, 3e38f}, {0.125f, 0.f}};
  const size_t K = sizeof(special) / sizeof(special[0]);
  // exact-size heap buffers, filled with NaN: the surplus channels are never read
  std::vector<std::vector<float>> f((size_t)nsrc);
  for (int s = 0; s < nsrc; ++s) {
    f[s].assign((size_t)B * chan[s] * vol, nan);
    for (int b = 0; b < B; ++b) {
      float* pu = f[s].data() + ((size_t)b * chan[s] + 0) * vol;
      float* pv = f[s].data() + ((size_t)b * chan[s] + 1) * vol;
      for (size_t i = 0; i < vol; ++i) {
        pu[i] = (float)(0.25 * (uniform() + uniform() + uniform()));
        pv[i] = (float)(0.25 * (uniform() + uniform() + uniform()));
      }
      for (size_t k = 0; k < K; ++k) {
        const size_t rot = (k + (size_t)s) % K;  // (the sources differ)
        const size_t first = k % vol, last = vol - 1 - k % vol;
        pu[first] = special[rot][0], pv[first] = special[rot][1];
        pu[last] = special[(rot + 5) % K][0], pv[last] = special[(rot + 5) % K][1];
        for (int d = -1; d <= 0; ++d) {
          if (X > FS_TILE) {  // both sides of the first tile boundary along x, row k
            const size_t at = (((size_t)(FS_TILE + d)) * Y + k % (size_t)Y) * NZ + k % (size_t)NZ;
            pu[at] = special[(rot + 7 + d) % K][0], pv[at] = special[(rot + 7 + d) % K][1];
          }
          if (Y > FS_TILE) {  // ... along y
            const size_t at = ((k % (size_t)X) * Y + (size_t)(FS_TILE + d)) * NZ + k % (size_t)NZ;
            pu[at] = special[(rot + 9 + d) % K][0], pv[at] = special[(rot + 9 + d) % K][1];
          }
          if (g.ZC < NZ) {  // both sides of the first chunk boundary, column k
            const size_t at = (k % ((size_t)X * Y)) * NZ + (size_t)(g.ZC + d);
            pu[at] = special[(rot + 11 + d) % K][0], pv[at] = special[(rot + 11 + d) % K][1];
          }
        }
      }
    }
  }
  const size_t entries = (size_t)fs_table_entries(g);
  std::vector<fs_u64> ws(entries, 0xdeadbeefdeadbeefull);
  std::vector<double> out(entries, (double)nan);
  const unsigned nblocks = (unsigned)((entries + FS_BLOCK - 1) / FS_BLOCK);
  launch(FS_BLOCK, nblocks, 1, 1, [&] { fss_zero_kernel(ws.data(), (long)entries); });
  launch(FS_BLOCK, (unsigned)(g.ntx * g.nty * g.nzc), 1, (unsigned)B, [&] {
    fss_count_kernel(f[0].data(), chan[0], f[1].data(), chan[1], nsrc == 3 ? f[2].data() : nullptr, chan[2], thr2.data(), g,
                     ws.data());
  });
  launch(FS_BLOCK, nblocks, 1, 1, [&] { fss_convert_kernel(ws.data(), (long)entries, out.data()); });

  // the definition: events, then every box clipped to the plane
  std::vector<double> want(entries, 0.0);
  std::vector<int> ev((size_t)3 * X * Y);
  for (int b = 0; b < B; ++b)
    for (int z = 0; z < NZ; ++z)
      for (int q = 0; q < nt; ++q) {
        for (int s = 0; s < 3; ++s)
          for (int p = 0; p < X * Y; ++p) {
            int e = 0;
            if (s < nsrc) {
              const float u = f[s][((size_t)b * chan[s] + 0) * vol + (size_t)p * NZ + z];
              const float v = f[s][((size_t)b * chan[s] + 1) * vol + (size_t)p * NZ + z];
              const float uu = u * u, vv = v * v;
              const float hs2 = uu + vv;
              e = hs2 >= thr2[q] ? 1 : 0;
            }
            ev[(size_t)s * X * Y + p] = e;
          }
        for (int k = 0; k < nn; ++k) {
          const int r = (scales[k] - 1) / 2;
          double sum[5] = {0, 0, 0, 0, 0};
          for (int x = 0; x < X; ++x)
            for (int y = 0; y < Y; ++y) {
              long c[3] = {0, 0, 0};
              for (int s = 0; s < 3; ++s)
                for (int xx = x - r < 0 ? 0 : x - r; xx <= x + r && xx < X; ++xx)
                  for (int yy = y - r < 0 ? 0 : y - r; yy <= y + r && yy < Y; ++yy) c[s] += ev[((size_t)s * X + xx) * Y + yy];
              sum[0] += (double)(c[0] * c[0]), sum[1] += (double)(c[1] * c[1]);
              sum[2] += (double)((c[1] - c[0]) * (c[1] - c[0]));
              if (nsrc == 3) sum[3] += (double)(c[2] * c[2]), sum[4] += (double)((c[2] - c[0]) * (c[2] - c[0]));
            }
          for (int i = 0; i < 5; ++i) want[((((size_t)b * NZ + z) * nt + q) * nn + k) * 5 + i] = sum[i];
        }
      }
  size_t differ = 0, events = 0;
  for (size_t i = 0; i < entries; ++i) differ += !(out[i] == want[i]);
  for (size_t i = 0; i < entries; i += 5) events += want[i] > 0;
  printf("B %d X %d Y %d NZ %d channels %d %d %d thresholds %d scales", B, X, Y, NZ, chan[0], chan[1], chan[2], nt);
  for (int k = 0; k < nn; ++k) printf(" %d", scales[k]);
  printf(": staged %d x %d, chunk %d levels, %d x %d x %d x %d workgroups, %zu of %zu sums differ (%zu (level, threshold, "
         "scale) with events)\n", g.S, g.S, g.ZC, g.ntx, g.nty, g.nzc, B, differ, entries, events);
  return differ ? 1 : 0;
}
