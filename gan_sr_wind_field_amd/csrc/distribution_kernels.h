// The kernels of csrc/distribution.hip ([DISTRIBUTION]), kept in a header of their own so that a host program can run
// them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/distribution_host_check.cpp: a shim for __global__, __shared__, threadIdx / blockIdx, __syncthreads and the two
// integer adds DS_LDS_ADD / DS_GLOBAL_ADD).  Nothing here needs more of HIP than those.  No thread leaves a kernel that
// has a barrier before the last barrier.
//
// A table is T = ns * (nd + 1) 32-bit counters: speed bin x (sector, calm).  table[((b * NZ + z) * 3 + source)][T] in
// the workspace holds the counts as integers, out the same as doubles.
//
// dist_zero_kernel   zeroes the integer tables
// dist_count_kernel  one workgroup of 256 threads per (column range x level chunk, source, sample): ZC consecutive
//                    levels and a range of columns of ONE source.  The element loop runs over (column, z) with z
//                    fastest, so a wave reads runs of the chunk's levels - when the chunk is all of NZ one contiguous
//                    run of memory - and the lanes of one load mostly add into different level tables.  The class of a
//                    voxel is that of distribution.py, operation for operation, nothing contracted; edge2, bx, by sit
//                    in LDS (reads of one address by a wave: broadcasts), the speed bin is a six-step search for the
//                    number of edges <= hs2.  Counting is an integer LDS add into cnt[z][T]; at the end the nonzero
//                    counters are added to the global integer table.
// dist_convert_kernel  out[i] = (double)table[i]: every element of out is written, the slices of an absent tl as zeros
//
// Integer adds commute: the result is the same on every call whatever the order, there are no floating-point atomics,
// and no counter can overflow (a slice holds X * Y < 2^31 voxels).
#pragma once

#pragma clang fp contract(off)

#ifndef DS_LDS_ADD
#define DS_LDS_ADD(p, v) atomicAdd((p), (v))
#define DS_GLOBAL_ADD(p, v) atomicAdd((p), (v))
#endif

namespace {

constexpr int DS_BLOCK = 256;
constexpr int DS_COUNTERS = WSR_DISTRIBUTION_LDS_COUNTERS;  // 60 KiB: two workgroups per CU at any table
constexpr int DS_MAX_NS = WSR_DISTRIBUTION_MAX_SPEED_BINS;
constexpr int DS_MAX_ND = WSR_DISTRIBUTION_MAX_SECTORS;
constexpr int DS_SOURCES = 3;

struct DsGeom {
  int B, X, Y, NZ, ns, nd;
  int T;           // ns * (nd + 1)
  int ncols;       // X * Y
  int ZC, nzc;     // levels per chunk: min(NZ, DS_COUNTERS / T); chunks
  int CB, ncb;     // columns per workgroup; column ranges
};

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_distribution documents them.  The column range: about 32768
// voxels per workgroup, halved down to 4096 while the launch has fewer than 1024 workgroups.  A function of the
// arguments alone (and the counts do not depend on it).
inline int ds_geom(DsGeom& g, int B, int X, int Y, int NZ, int ns, int nd) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (ns < 2 || ns > DS_MAX_NS || nd < 4 || nd > DS_MAX_ND || (nd & 1)) return WSR_EINVAL;
  if (B > 65535 || (long)X * Y > 0x7fffffffL || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.ns = ns, g.nd = nd;
  g.T = ns * (nd + 1);
  g.ncols = X * Y;
  const int zmax = DS_COUNTERS / g.T;  // >= 6
  g.ZC = NZ < zmax ? NZ : zmax;
  g.nzc = (NZ + g.ZC - 1) / g.ZC;
  long target = 32768;
  for (;;) {
    long cb = target / g.ZC;
    if (cb < 1) cb = 1;
    if (cb > g.ncols) cb = g.ncols;
    g.CB = (int)cb;
    g.ncb = (g.ncols + g.CB - 1) / g.CB;
    if (target <= 4096 || (long)g.ncb * g.nzc * DS_SOURCES * B >= 1024) break;
    target /= 2;
  }
  if ((long)g.ncb * g.nzc > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

// 32-bit words of the integer tables
inline long ds_workspace_words(const DsGeom& g) { return (long)g.B * g.NZ * DS_SOURCES * g.T; }

__global__ __launch_bounds__(DS_BLOCK) void dist_zero_kernel(unsigned* __restrict__ table, long n) {
  const long i = (long)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (i < n) table[i] = 0u;
}

// f0 / f1 / f2: the three sources, f2 possibly absent (then the grid has two sources)
__global__ __launch_bounds__(DS_BLOCK) void dist_count_kernel(const float* __restrict__ f0, int c0,
                                                              const float* __restrict__ f1, int c1,
                                                              const float* __restrict__ f2, int c2,
                                                              const float* __restrict__ edge2,
                                                              const float* __restrict__ bx,
                                                              const float* __restrict__ by, float calm2, DsGeom g,
                                                              unsigned* __restrict__ table) {
  __shared__ unsigned cnt[DS_COUNTERS];
  __shared__ float s_edge[DS_MAX_NS];
  __shared__ float s_bx[DS_MAX_ND / 2], s_by[DS_MAX_ND / 2];
  const int t = threadIdx.x, src = blockIdx.y, b = blockIdx.z;
  const int cblock = (int)(blockIdx.x / (unsigned)g.nzc), zchunk = (int)(blockIdx.x - (unsigned)cblock * g.nzc);
  const int z0 = zchunk * g.ZC;
  const int nz = g.NZ - z0 < g.ZC ? g.NZ - z0 : g.ZC;
  const int col0 = cblock * g.CB;
  const int nc = g.ncols - col0 < g.CB ? g.ncols - col0 : g.CB;
  const int T = g.T, nedge = g.ns - 1, half = g.nd >> 1, nd1 = g.nd + 1;
  const int used = nz * T;  // <= DS_COUNTERS

  for (int i = t; i < used; i += DS_BLOCK) cnt[i] = 0u;
  if (t < nedge) s_edge[t] = edge2[t];
  if (t < half) s_bx[t] = bx[t], s_by[t] = by[t];
  __syncthreads();

  const float* f = src == 0 ? f0 : (src == 1 ? f1 : f2);
  const int fc = src == 0 ? c0 : (src == 1 ? c1 : c2);
  const long vol = (long)g.ncols * g.NZ;  // (< 2^31: checked on the host)
  const float* pu = f + ((long)b * fc + 0) * vol;
  const float* pv = f + ((long)b * fc + 1) * vol;
  const int n = nc * nz;  // <= X * Y * NZ < 2^31
  for (int e = t; e < n; e += DS_BLOCK) {
    const int c = e / nz, z = e - c * nz;
    const long at = (long)(col0 + c) * g.NZ + z0 + z;
    const float u = pu[at], v = pv[at];
    const float uu = u * u, vv = v * v;
    const float hs2 = uu + vv;
    // the number of edges <= hs2 (the edges ascend; a NaN compares false: 0)
    int j = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
      if (j + step <= nedge && hs2 >= s_edge[j + step - 1]) j += step;
    int sector = g.nd;  // calm
    if (hs2 > calm2) {
      const float px = -u, py = -v;
      const float a0 = s_by[0] * px, b0 = s_bx[0] * py, a1 = s_by[1] * px, b1 = s_bx[1] * py;
      const float cr0 = a0 - b0, cr1 = a1 - b1;
      const bool second = cr0 < 0.f || (cr0 == 0.f && cr1 > 0.f);
      const float qx = second ? u : px, qy = second ? v : py;
      int k_cnt = 0;
      for (int k = 0; k < half; ++k) {
        const float a = s_by[k] * qx, bb = s_bx[k] * qy;
        k_cnt += (a - bb) >= 0.f ? 1 : 0;
      }
      sector = (k_cnt > 1 ? k_cnt : 1) - 1 + (second ? half : 0);
    }
    DS_LDS_ADD(&cnt[z * T + j * nd1 + sector], 1u);
  }
  __syncthreads();

  // the chunk's tables: table[((b * NZ + z0 + z) * 3 + src)][T]
  for (int i = t; i < used; i += DS_BLOCK) {
    const unsigned c = cnt[i];
    if (c != 0u) {
      const int z = i / T, k = i - z * T;
      DS_GLOBAL_ADD(&table[(((long)b * g.NZ + z0 + z) * DS_SOURCES + src) * T + k], c);
    }
  }
}

__global__ __launch_bounds__(DS_BLOCK) void dist_convert_kernel(const unsigned* __restrict__ table, long n,
                                                                double* __restrict__ out) {
  const long i = (long)blockIdx.x * DS_BLOCK + threadIdx.x;
  if (i < n) out[i] = (double)table[i];
}

}  // namespace
