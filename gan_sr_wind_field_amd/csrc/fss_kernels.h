// The kernels of csrc/fss.hip ([FSS]), kept in a header of their own so that a host program can run them block by block
// on threads under the address and undefined-behaviour sanitisers (tools/fss_host_check.cpp: a shim for __global__,
// __shared__, threadIdx / blockIdx, __syncthreads and the macros FS_LDS_ADD / FS_GLOBAL_ADD / FS_WAVE_SUM /
// FS_WAVE_LEADER).  Nothing here needs more of HIP than those.  No thread leaves a kernel that has a barrier before the
// last barrier.
//
// table[(((b * NZ + z) * nt + t) * nn + k) * 5 + i] in the workspace holds the five sums of fss.py as 64-bit integers, out
// the same as doubles.
//
// fss_zero_kernel     zeroes the integer table
// fss_count_kernel    one workgroup of 256 threads per (32 x 32 tile of the plane x chunk of ZC consecutive levels,
//                     sample).  1. It stages the tile with a halo of R = the largest radius: the element loop runs over
//                     (staged column, z) with z fastest, so a wave reads runs of the chunk's levels - when the chunk is all
//                     of NZ contiguous memory.  Every staged voxel of the three sources is classified once into the
//                     number of thresholds its hs2 reaches (the events are nested in the threshold), 4 bits per source
//                     in one 16-bit word of LDS; cells outside the plane hold 0.  Floats are not kept.
//                     2. Per level and threshold: the 2-D table of running sums P[src][i][j] = the events in staged rows
//                     < i and columns < j, built in LDS by a scan along y (one thread per source and row) and one along x
//                     (one thread per source and column).  The count of ANY box is four look-ups, so every position
//                     takes the counts of all neighbourhoods from the one table: no re-staging per neighbourhood, and no
//                     count map outside LDS.  A thread owns four positions of the tile; their squares are added in
//                     32-bit integers, summed over the wave, added once per wave into five LDS words and from there once
//                     per workgroup into the 64-bit table.
// fss_convert_kernel  out[i] = (double)table[i]: every element of out is written, entries 3 and 4 of an absent tl as zeros
//
// Why no accumulator overflows: a count is at most 33^2 = 1089, a squared count or squared difference at most
// 1089^2 = 1,185,921 < 2^21.  A thread adds 4 of them (< 2^23), a workgroup 1024 (< 1.22e9 < 2^32): 32 bits.  The table
// adds X * Y < 2^31 of them per entry (< 2^52): 64-bit integers, and exact as doubles.  The running sums P are at most
// 64 * 64 = 4096: 16 bits.
// Integer adds commute: the result is the same on every call whatever the order; there are no floating-point atomics.
#pragma once

#pragma clang fp contract(off)

#ifndef FS_LDS_ADD
#define FS_LDS_ADD(p, v) atomicAdd((p), (v))
#define FS_GLOBAL_ADD(p, v) atomicAdd((p), (v))
// the sum of v over the 64 lanes of the wave, in every lane (all 256 threads reach it: whole waves, no lane masked)
#define FS_WAVE_SUM(v) fs_wave_sum(v)
#define FS_WAVE_LEADER(t) (((t) & 63) == 0)
#define FS_DEVICE_WAVE_SUM 1
#endif

namespace {

constexpr int FS_BLOCK = 256;
constexpr int FS_TILE = 32;                          // positions of a workgroup: FS_TILE x FS_TILE
constexpr int FS_PER_THREAD = FS_TILE * FS_TILE / FS_BLOCK;
constexpr int FS_MAX_NT = WSR_FSS_MAX_THRESHOLDS;
constexpr int FS_MAX_NN = WSR_FSS_MAX_SCALES;
constexpr int FS_MAX_R = (WSR_FSS_MAX_SCALE - 1) / 2;
constexpr int FS_MAX_S = FS_TILE + 2 * FS_MAX_R;     // 64 staged rows / columns
constexpr int FS_P_PITCH = FS_MAX_S + 2;             // 66 halfwords = 33 words: rows of P start in different banks
constexpr int FS_P_WORDS = (FS_MAX_S + 1) * FS_P_PITCH;
constexpr int FS_CLS_WORDS = 26624;                  // 52 KiB of classes + 25.1 KiB of P: two workgroups per CU
constexpr int FS_MAX_ZC = 16;
constexpr int FS_SUMS = 5;

typedef unsigned long long fs_u64;

struct FsGeom {
  int B, X, Y, NZ, nt, nn;
  int rad[FS_MAX_NN];  // (n - 1) / 2, ascending
  int R, S;            // the largest radius; staged rows = columns = FS_TILE + 2 R
  int CP, LP;          // halfwords per staged row (CP / 2 odd) and per staged level (LP / 2 odd)
  int ntx, nty;        // tiles along x and y
  int ZC, nzc;         // levels per chunk; chunks
};

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_fss documents them.  scales: host.  A function of the arguments
// alone (and the sums do not depend on it): the chunk is what fits FS_CLS_WORDS, at most FS_MAX_ZC levels, the levels
// spread evenly over the chunks; it is halved while the launch has fewer than 512 workgroups.
inline int fs_geom(FsGeom& g, int B, int X, int Y, int NZ, int nt, const int* scales, int nn) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0 || !scales) return WSR_EINVAL;
  if (nt < 1 || nt > FS_MAX_NT || nn < 1 || nn > FS_MAX_NN) return WSR_EINVAL;
  for (int k = 0; k < nn; ++k) {
    const int n = scales[k];
    if (n < 1 || n > WSR_FSS_MAX_SCALE || !(n & 1) || (k == 0 ? n != 1 : n <= scales[k - 1])) return WSR_EINVAL;
  }
  if (B > 65535 || (long)X * Y > 0x7fffffffL || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.nt = nt, g.nn = nn;
  for (int k = 0; k < FS_MAX_NN; ++k) g.rad[k] = k < nn ? (scales[k] - 1) / 2 : 0;
  g.R = g.rad[nn - 1];
  g.S = FS_TILE + 2 * g.R;                              // even
  g.CP = ((g.S / 2) & 1) ? g.S : g.S + 2;
  g.LP = g.S * g.CP + 2;                                // S * CP / 2 is even: + 1 word
  g.ntx = (X + FS_TILE - 1) / FS_TILE, g.nty = (Y + FS_TILE - 1) / FS_TILE;
  int zc = FS_CLS_WORDS / g.LP;                         // >= 6
  if (zc > FS_MAX_ZC) zc = FS_MAX_ZC;
  if (zc > NZ) zc = NZ;
  for (;;) {
    g.nzc = (NZ + zc - 1) / zc;
    g.ZC = (NZ + g.nzc - 1) / g.nzc;
    if (g.ZC <= 2 || (long)g.ntx * g.nty * g.nzc * B >= 512) break;
    zc = (g.ZC + 1) / 2;
  }
  g.nzc = (NZ + g.ZC - 1) / g.ZC;
  if ((long)g.ntx * g.nty * g.nzc > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

// 64-bit entries of the integer table
inline long fs_table_entries(const FsGeom& g) { return (long)g.B * g.NZ * g.nt * g.nn * FS_SUMS; }

#ifdef FS_DEVICE_WAVE_SUM
__device__ __forceinline__ unsigned fs_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
#endif

__global__ __launch_bounds__(FS_BLOCK) void fss_zero_kernel(fs_u64* __restrict__ table, long n) {
  const long i = (long)blockIdx.x * FS_BLOCK + threadIdx.x;
  if (i < n) table[i] = 0ull;
}

// f0 / f1 / f2: HR, SR and TL, f2 possibly absent (then entries 3 and 4 stay zero)
__global__ __launch_bounds__(FS_BLOCK) void fss_count_kernel(const float* __restrict__ f0, int c0,
                                                             const float* __restrict__ f1, int c1,
                                                             const float* __restrict__ f2, int c2,
                                                             const float* __restrict__ thr2, FsGeom g,
                                                             fs_u64* __restrict__ table) {
  __shared__ unsigned short cls[FS_CLS_WORDS];       // [z][i][j]: 4 bits per source, the thresholds reached
  __shared__ unsigned short P[3][FS_P_WORDS];        // [src][i][j], i, j in 0 .. S: events in rows < i, columns < j
  __shared__ unsigned red[FS_MAX_NN * FS_SUMS];
  __shared__ float s_thr[FS_MAX_NT];
  const int t = threadIdx.x, b = blockIdx.z;
  const int zchunk = (int)(blockIdx.x % (unsigned)g.nzc), tile = (int)(blockIdx.x / (unsigned)g.nzc);
  const int ty = tile % g.nty, tx = tile / g.nty;
  const int x0 = tx * FS_TILE, y0 = ty * FS_TILE;    // the tile's first position
  const int z0 = zchunk * g.ZC;
  const int nz = g.NZ - z0 < g.ZC ? g.NZ - z0 : g.ZC;
  const int S = g.S, R = g.R, CP = g.CP, LP = g.LP, nt = g.nt, nn = g.nn;
  const int nsrc = f2 ? 3 : 2;

  if (t < nt) s_thr[t] = thr2[t];
  if (t < FS_MAX_NN * FS_SUMS) red[t] = 0u;
  // row 0 and column 0 of P are zeros and stay zeros
  for (int i = t; i < 3 * (S + 1); i += FS_BLOCK) {
    const int s = i / (S + 1), k = i - s * (S + 1);
    P[s][k] = 0, P[s][k * FS_P_PITCH] = 0;
  }
  __syncthreads();

  // 1. the classes of the staged voxels
  const long vol = (long)g.X * g.Y * g.NZ;           // (< 2^31: checked on the host)
  const float* pu[3] = {f0 + (long)b * c0 * vol, f1 + (long)b * c1 * vol, f2 ? f2 + (long)b * c2 * vol : nullptr};
  const int n_stage = S * S * nz;                    // <= 64 * 64 * 16
  for (int e = t; e < n_stage; e += FS_BLOCK) {
    const int col = e / nz, z = e - col * nz;
    const int i = col / S, j = col - i * S;
    const int x = x0 - R + i, y = y0 - R + j;
    unsigned c = 0u;
    if (x >= 0 && x < g.X && y >= 0 && y < g.Y) {
      const long at = ((long)x * g.Y + y) * g.NZ + z0 + z;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (s < nsrc) {
          const float u = pu[s][at], v = pu[s][vol + at];
          const float uu = u * u, vv = v * v;
          const float hs2 = uu + vv;
          unsigned k = 0u;                           // the thresholds ascend; a NaN compares false with every one
          for (int q = 0; q < nt; ++q) k += hs2 >= s_thr[q] ? 1u : 0u;
          c |= k << (4 * s);
        }
      }
    }
    cls[z * LP + i * CP + j] = (unsigned short)c;
  }
  __syncthreads();

  // 2. per level and threshold
  for (int z = 0; z < nz; ++z) {
    const unsigned short* cz = cls + z * LP;
    for (int q = 0; q < nt; ++q) {
      // along y: P[s][i + 1][j + 1] = the events of row i in columns <= j
      if (t < nsrc * S) {
        const int s = t / S, i = t - s * S;
        const unsigned short* row = cz + i * CP;
        unsigned short* prow = &P[s][(i + 1) * FS_P_PITCH + 1];
        const unsigned shift = 4u * s;
        unsigned run = 0u;
        for (int j = 0; j < S; ++j) {
          run += ((row[j] >> shift) & 15u) > (unsigned)q ? 1u : 0u;
          prow[j] = (unsigned short)run;
        }
      }
      __syncthreads();
      // along x: the running sum down every column
      if (t < nsrc * S) {
        const int s = t / S, j = t - s * S;
        unsigned short* pcol = &P[s][FS_P_PITCH + j + 1];
        unsigned run = 0u;
        for (int i = 0; i < S; ++i) {
          run += pcol[i * FS_P_PITCH];
          pcol[i * FS_P_PITCH] = (unsigned short)run;
        }
      }
      __syncthreads();
      // the counts of every neighbourhood at the thread's positions (lanes along y)
      for (int k = 0; k < nn; ++k) {
        const int r = g.rad[k];
        unsigned a[FS_SUMS] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < FS_PER_THREAD; ++p) {
          const int pos = t + p * FS_BLOCK;
          const int lx = pos / FS_TILE, ly = pos - lx * FS_TILE;
          if (x0 + lx < g.X && y0 + ly < g.Y) {
            // staged rows lx + R - r .. lx + R + r (all inside 0 .. S - 1, for r <= R)
            const int lo_i = (lx + R - r) * FS_P_PITCH, hi_i = (lx + R + r + 1) * FS_P_PITCH;
            const int lo_j = ly + R - r, hi_j = ly + R + r + 1;
            int c[3] = {0, 0, 0};
#pragma unroll
            for (int s = 0; s < 3; ++s)
              if (s < nsrc)
                c[s] = (int)P[s][hi_i + hi_j] - (int)P[s][lo_i + hi_j] - (int)P[s][hi_i + lo_j] + (int)P[s][lo_i + lo_j];
            const int ds = c[1] - c[0], dt = c[2] - c[0];
            a[0] += (unsigned)(c[0] * c[0]);
            a[1] += (unsigned)(c[1] * c[1]);
            a[2] += (unsigned)(ds * ds);
            a[3] += (unsigned)(c[2] * c[2]);
            a[4] += (unsigned)(dt * dt);
          }
        }
#pragma unroll
        for (int i = 0; i < FS_SUMS; ++i) {
          const unsigned w = FS_WAVE_SUM(a[i]);
          if (FS_WAVE_LEADER(t) && w != 0u) FS_LDS_ADD(&red[k * FS_SUMS + i], w);
        }
      }
      __syncthreads();
      // the workgroup's partial sums of (level, threshold): into the table, and cleared for the next round (which adds
      // to red only after two more barriers)
      if (t < nn * FS_SUMS) {
        const unsigned w = red[t];
        const int i = t % FS_SUMS;
        if (w != 0u && (i < 3 || nsrc == 3))
          FS_GLOBAL_ADD(&table[(((long)b * g.NZ + z0 + z) * nt + q) * (nn * FS_SUMS) + t], (fs_u64)w);
        red[t] = 0u;
      }
    }
  }
}

__global__ __launch_bounds__(FS_BLOCK) void fss_convert_kernel(const fs_u64* __restrict__ table, long n,
                                                               double* __restrict__ out) {
  const long i = (long)blockIdx.x * FS_BLOCK + threadIdx.x;
  if (i < n) out[i] = (double)table[i];
}

}  // namespace
