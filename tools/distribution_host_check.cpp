//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/distribution_host_check.cpp -o distribution_host_check
//   ./distribution_host_check B X Y NZ speed_bins sectors calm hr_c sr_c tl_c      (tl_c 0: no baseline)
//
// Runs the three kernels of csrc/distribution.hip block by block on host threads, for the address and
// undefined-behaviour sanitisers: the shim of tools/host_shim.h (__global__, __shared__ as a static array, one block at a
// time, threadIdx / blockIdx, __syncthreads as a pthread barrier) with the LDS and global integer adds
// (__atomic_fetch_add).  Every buffer is a
// heap allocation of exactly the size the C ABI documents - the three fields, the tables (speed_bins - 1 and twice
// sectors / 2 floats), the workspace and the counts - so an access outside one of them is reported; the LDS arrays are
// statics of the kernels' own sizes.
//
// The launches are those of wsr_level_distribution with UVW_MAX 32 and bin_width 1.  HR, SR and TL hold random vectors
// (a sum of uniforms of standard deviation about 0.25) and, at the first and the last voxels of every sample and on both
// sides of the first level-chunk boundary, the special voxels of the tests: the axis directions, the |u| = |v| ties,
// vectors on a bin edge, zeros, NaN and +-Inf.  The program computes the same table with a plain loop over the
// definition of distribution.py and exits non-zero on any differing count, on a slice that does not sum to X * Y and on
// a count of the absent baseline that is not zero.
#include "host_shim.h"

#define DS_LDS_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define DS_GLOBAL_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)

#include "../gan_sr_wind_field_amd/csrc/distribution_kernels.h"

namespace {

// the definition of distribution.py for one voxel -> the index j * (nd + 1) + sector
int classify(float u, float v, const std::vector<float>& edge2, const std::vector<float>& bx, const std::vector<float>& by,
             float calm2, int nd) {
  const float uu = u * u, vv = v * v;
  const float hs2 = uu + vv;
  int j = 0;
  for (size_t i = 0; i < edge2.size(); ++i) j += hs2 >= edge2[i] ? 1 : 0;
  int sector = nd;
  if (hs2 > calm2) {
    const float px = -u, py = -v;
    const float a0 = by[0] * px, b0 = bx[0] * py, a1 = by[1] * px, b1 = bx[1] * py;
    const float c0 = a0 - b0, c1 = a1 - b1;
    const bool second = c0 < 0.f || (c0 == 0.f && c1 > 0.f);
    const float qx = second ? -px : px, qy = second ? -py : py;
    int cnt = 0;
    for (int k = 0; k < nd / 2; ++k) {
      const float a = by[k] * qx, b = bx[k] * qy;
      cnt += (a - b) >= 0.f ? 1 : 0;
    }
    sector = (cnt > 1 ? cnt : 1) - 1 + (second ? nd / 2 : 0);
  }
  return j * (nd + 1) + sector;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: %s B X Y NZ speed_bins sectors calm hr_c sr_c tl_c\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]), ns = atoi(argv[5]);
  const int nd = atoi(argv[6]);
  const double calm = atof(argv[7]);
  const int chan[3] = {atoi(argv[8]), atoi(argv[9]), atoi(argv[10])};
  DsGeom g{};
  if (ds_geom(g, B, X, Y, NZ, ns, nd) != 0 || chan[0] < 3 || chan[1] < 3 || (chan[2] != 0 && chan[2] < 3) || !(calm >= 0)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const int nsrc = chan[2] ? 3 : 2;
  const size_t vol = (size_t)X * Y * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const double uvw = 32.0;
  std::vector<float> edge2((size_t)ns - 1), bx((size_t)nd / 2), by((size_t)nd / 2);
  for (int j = 1; j < ns; ++j) edge2[j - 1] = (float)((j / uvw) * (j / uvw));
  for (int k = 0; k < nd / 2; ++k) {
    const double beta = -M_PI / nd + 2.0 * M_PI * k / nd;
    bx[k] = (float)sin(beta), by[k] = (float)cos(beta);
  }
  const float calm2 = (float)((calm / uvw) * (calm / uvw));
  const float e = 1.f / 32.f;
  const float special[][2] = {
      {0.f, -0.25f}, {-0.25f, 0.f}, {0.f, 0.25f}, {0.25f, 0.f},                  // from north, east, south, west
      {0.25f, 0.25f}, {-0.25f, 0.25f}, {0.25f, -0.25f}, {-0.25f, -0.25f},        // |u| = |v|
      {e, 0.f}, {2 * e, 0.f}, {0.f, 3 * e}, {-(float)(ns - 1) * e, 0.f},         // on a bin edge
      {0.f, 0.f}, {-0.f, 0.f}, {nan, 0.1f}, {0.1f, nan}, {nan, nan},             // zeros, NaN
      {inf, 0.f}, {0.f, -inf}, {inf, inf}, {-inf, inf}, {inf, nan}, {1e-30f, -1e-30f}, {3e38f, 3e38f}};
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
        if (g.ZC < NZ) {  // both sides of the first chunk boundary, column k
          const size_t col = k % (size_t)g.ncols;
          for (int dz = -1; dz <= 0; ++dz) {
            const size_t at = col * NZ + (size_t)(g.ZC + dz);
            pu[at] = special[(rot + 11 + dz) % K][0], pv[at] = special[(rot + 11 + dz) % K][1];
          }
        }
      }
    }
  }
  const size_t words = (size_t)ds_workspace_words(g);
  std::vector<unsigned> ws(words, 0xdeadbeefu);
  std::vector<double> out(words, (double)nan);
  const unsigned nblocks = (unsigned)((words + DS_BLOCK - 1) / DS_BLOCK);
  launch(DS_BLOCK, nblocks, 1, 1, [&] { dist_zero_kernel(ws.data(), (long)words); });
  launch(DS_BLOCK, (unsigned)(g.ncb * g.nzc), (unsigned)nsrc, (unsigned)B, [&] {
    dist_count_kernel(f[0].data(), chan[0], f[1].data(), chan[1], nsrc == 3 ? f[2].data() : nullptr, chan[2], edge2.data(),
                      bx.data(), by.data(), calm2, g, ws.data());
  });
  launch(DS_BLOCK, nblocks, 1, 1, [&] { dist_convert_kernel(ws.data(), (long)words, out.data()); });

  std::vector<double> want(words, 0.0);
  for (int s = 0; s < nsrc; ++s)
    for (int b = 0; b < B; ++b) {
      const float* pu = f[s].data() + ((size_t)b * chan[s] + 0) * vol;
      const float* pv = f[s].data() + ((size_t)b * chan[s] + 1) * vol;
      for (size_t i = 0; i < vol; ++i) {
        const size_t z = i % (size_t)NZ;
        want[(((size_t)b * NZ + z) * 3 + (size_t)s) * g.T + (size_t)classify(pu[i], pv[i], edge2, bx, by, calm2, nd)] += 1.0;
      }
    }
  size_t differ = 0, badsum = 0;
  for (size_t i = 0; i < words; ++i) differ += !(out[i] == want[i]);
  for (size_t sl = 0; sl < (size_t)B * NZ * 3; ++sl) {
    double sum = 0.0;
    for (int k = 0; k < g.T; ++k) sum += out[sl * g.T + k];
    badsum += sum != ((int)(sl % 3) < nsrc ? (double)X * Y : 0.0);
  }
  printf("B %d X %d Y %d NZ %d bins %d sectors %d calm %g channels %d %d %d: chunk %d levels x %d columns, %d x %d x %d x %d "
         "workgroups, %zu counts differ, %zu slices with a wrong sum\n", B, X, Y, NZ, ns, nd, calm, chan[0], chan[1], chan[2],
         g.ZC, g.CB, g.ncb, g.nzc, nsrc, B, differ, badsum);
  return differ || badsum ? 1 : 0;
}
