// The kernels of csrc/distribution_loss.hip ([DISTRIBUTION_LOSS]), kept in a header of their own so that a host program
// can run them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/distribution_loss_host_check.cpp: the shim of tools/host_shim.h for __global__, __shared__, threadIdx / blockIdx
// and __syncthreads, with the integer adds DL_LDS_ADD / DL_GLOBAL_ADD and the square root DL_SQRT).  Nothing here needs
// more of HIP than those.  No thread leaves a kernel that has a barrier before the last barrier.
//
// A table is T = ns + 1 counters in units of 1 / 65536 of a voxel: the ns soft speed bins and, last, the voxels whose
// hs2 is not finite.  table[((source * B + b) * NZ + z)][T] in the workspace holds them as 64-bit integers, out the same
// as doubles divided by 65536 (source 0 hr, 1 sr).
//
// dl_zero_kernel     zeroes the integer tables
// dl_count_kernel    one workgroup of 256 threads per (column range, source, sample): all NZ levels of a range of columns
//                    of ONE source, which is one contiguous run of memory.  The element loop runs over (column, z) with z
//                    fastest, so the lanes of a load read consecutive floats and add into different level tables.  The
//                    position of a voxel is that of distribution_loss.py, operation for operation, nothing contracted,
//                    the square root correctly rounded: hs2 = u u + v v, t = sqrt(hs2) c - 0.5 clamped to [0, ns - 1],
//                    k0 = min(floor(t), ns - 2), fi = rint((t - k0) 65536); the voxel adds 65536 - fi to cnt[z][k0] and
//                    fi to cnt[z][k0 + 1] in LDS (an add of zero is skipped), 65536 to cnt[z][ns] when hs2 is not finite.
//                    A range holds at most 65535 columns, so no 32-bit counter can overflow.  At the end the nonzero
//                    counters are added to the global 64-bit table.
// dl_convert_kernel  out[i] = (double)table[i] / 65536: every element of out is written
// dl_bwd_kernel      one workgroup per (element range, sample): stages the upstream table g (NZ, ns) fp32 of the sample in
//                    LDS, recomputes t with the forward's operations and writes, for every element of the range,
//                    ((g[z][k0 + 1] - g[z][k0]) c) u / r to channel 0 and the same with v to channel 1 - zero unless hs2
//                    is finite, r > 0 and 0 < t < ns - 1 before the clamp - and zero to every channel from 2 on.  Every
//                    element of dsr is written exactly once; no atomics; nothing was saved by the forward.
//
// Integer adds commute: the counts are the same on every call whatever the order, and there are no floating-point
// atomics.
#pragma once

#pragma clang fp contract(off)

#ifndef DL_LDS_ADD
#define DL_LDS_ADD(p, v) atomicAdd((p), (v))
#define DL_GLOBAL_ADD(p, v) atomicAdd((p), (v))
#define DL_SQRT(x) __fsqrt_rn(x)
#endif

namespace {

typedef unsigned long long dl_u64;

constexpr int DL_BLOCK = 256;
constexpr int DL_COUNTERS = WSR_DISTRIBUTION_LOSS_LDS_COUNTERS;  // 65 * 128 words, 32.5 KiB: four workgroups per CU
constexpr int DL_MAX_NS = WSR_DISTRIBUTION_MAX_SPEED_BINS;
constexpr int DL_SOURCES = 2;
constexpr unsigned DL_ONE = 65536u;
constexpr int DL_MAX_COLUMNS = 65535;  // columns * 65536 < 2^32
constexpr int DL_BWD_ELEMS = 2048;     // elements of one (sample, channel) volume per workgroup of the backward

struct DlGeom {
  int B, X, Y, NZ, ns;
  int T;        // ns + 1
  int ncols;    // X * Y
  int CB, ncb;  // columns per workgroup; column ranges
  long vol;     // X * Y * NZ
  int nbwd;     // element ranges of the backward
};

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_speed_soft_counts documents them.  The column range: about 32768 voxels
// per workgroup, halved down to 4096 while the launch has fewer than 1024 workgroups (the rule of ds_geom).  A function
// of the arguments alone, and the counts do not depend on it.
inline int dl_geom(DlGeom& g, int B, int X, int Y, int NZ, int ns) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (ns < 2 || ns > DL_MAX_NS) return WSR_EINVAL;
  if (B > 65535 || (long)X * Y > 0x7fffffffL || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  if ((long)(ns + 1) * NZ > DL_COUNTERS) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.ns = ns;
  g.T = ns + 1;
  g.ncols = X * Y;
  g.vol = (long)g.ncols * NZ;
  long target = 32768;
  for (;;) {
    long cb = target / NZ;
    if (cb < 1) cb = 1;
    if (cb > g.ncols) cb = g.ncols;
    if (cb > DL_MAX_COLUMNS) cb = DL_MAX_COLUMNS;
    g.CB = (int)cb;
    g.ncb = (g.ncols + g.CB - 1) / g.CB;
    if (target <= 4096 || (long)g.ncb * DL_SOURCES * B >= 1024) break;
    target /= 2;
  }
  g.nbwd = (int)((g.vol + DL_BWD_ELEMS - 1) / DL_BWD_ELEMS);
  return 0;
}

// 64-bit words of the integer tables
inline long dl_table_words(const DlGeom& g) { return (long)DL_SOURCES * g.B * g.NZ * g.T; }

__global__ __launch_bounds__(DL_BLOCK) void dl_zero_kernel(dl_u64* __restrict__ table, long n) {
  const long i = (long)blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i < n) table[i] = 0ull;
}

// t before the clamp of a voxel with a finite hs2, the operations of distribution_loss.py
__device__ __forceinline__ float dl_position(float hs2, float c, float& r) {
  r = DL_SQRT(hs2);
  const float rc = r * c;
  return rc - 0.5f;
}

__global__ __launch_bounds__(DL_BLOCK) void dl_count_kernel(const float* __restrict__ f0, int c0,
                                                            const float* __restrict__ f1, int c1, float c, DlGeom g,
                                                            dl_u64* __restrict__ table) {
  __shared__ unsigned cnt[DL_COUNTERS];
  const int t = threadIdx.x, src = blockIdx.y, b = blockIdx.z;
  const int col0 = (int)blockIdx.x * g.CB;
  const int nc = g.ncols - col0 < g.CB ? g.ncols - col0 : g.CB;
  const int T = g.T, ns = g.ns, NZ = g.NZ;
  const int used = NZ * T;  // <= DL_COUNTERS

  for (int i = t; i < used; i += DL_BLOCK) cnt[i] = 0u;
  __syncthreads();

  const float* f = src == 0 ? f0 : f1;
  const int fc = src == 0 ? c0 : c1;
  const float* pu = f + ((long)b * fc + 0) * g.vol + (long)col0 * NZ;
  const float* pv = f + ((long)b * fc + 1) * g.vol + (long)col0 * NZ;
  const float top = (float)(ns - 1);
  const int n = nc * NZ;  // <= X * Y * NZ < 2^31
  for (int e = t; e < n; e += DL_BLOCK) {
    const int z = e % NZ;
    const float u = pu[e], v = pv[e];
    const float uu = u * u, vv = v * v;
    const float hs2 = uu + vv;
    unsigned* row = cnt + z * T;
    if (!__builtin_isfinite(hs2)) {
      DL_LDS_ADD(&row[ns], DL_ONE);
      continue;
    }
    float r;
    float p = dl_position(hs2, c, r);
    p = p < 0.f ? 0.f : p;
    p = p > top ? top : p;
    int k0 = (int)p;  // (p >= 0: truncation is the floor)
    k0 = k0 > ns - 2 ? ns - 2 : k0;
    const float fr = p - (float)k0;  // in [0, 1], exact
    const unsigned fi = (unsigned)__builtin_rintf(fr * 65536.f);
    if (fi != DL_ONE) DL_LDS_ADD(&row[k0], DL_ONE - fi);
    if (fi != 0u) DL_LDS_ADD(&row[k0 + 1], fi);
  }
  __syncthreads();

  // this workgroup's share of table[((src * B + b) * NZ + z)][T], z = 0 .. NZ - 1: `used` consecutive words
  dl_u64* dst = table + ((long)src * g.B + b) * used;
  for (int i = t; i < used; i += DL_BLOCK) {
    const unsigned w = cnt[i];
    if (w != 0u) DL_GLOBAL_ADD(&dst[i], (dl_u64)w);
  }
}

__global__ __launch_bounds__(DL_BLOCK) void dl_convert_kernel(const dl_u64* __restrict__ table, long n,
                                                              double* __restrict__ out) {
  const long i = (long)blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i < n) out[i] = (double)table[i] / 65536.0;
}

// sr (B, sr_c, X, Y, NZ), gtab (B, NZ, ns) fp32, dsr (B, sr_c, X, Y, NZ)
__global__ __launch_bounds__(DL_BLOCK) void dl_bwd_kernel(const float* __restrict__ sr, int sr_c,
                                                          const float* __restrict__ gtab, float c, DlGeom g,
                                                          float* __restrict__ dsr) {
  __shared__ float s_g[DL_MAX_NS * (DL_COUNTERS / (DL_MAX_NS + 1))];  // NZ * ns <= 64 * 128 floats
  const int t = threadIdx.x, b = blockIdx.y;
  const int ns = g.ns, NZ = g.NZ;
  const int ng = NZ * ns;
  const float* gb = gtab + (long)b * ng;
  for (int i = t; i < ng; i += DL_BLOCK) s_g[i] = gb[i];
  __syncthreads();

  const long e0 = (long)blockIdx.x * DL_BWD_ELEMS;
  const int n = g.vol - e0 < DL_BWD_ELEMS ? (int)(g.vol - e0) : DL_BWD_ELEMS;
  const long base = (long)b * sr_c * g.vol + e0;
  const float* pu = sr + base;
  const float* pv = pu + g.vol;
  float* du = dsr + base;
  float* dv = du + g.vol;
  const float top = (float)(ns - 1);
  const int zfirst = (int)(e0 % NZ);  // (the level of the range's first element: one 64-bit division per workgroup)
  for (int e = t; e < n; e += DL_BLOCK) {
    const int z = (zfirst + e) % NZ;
    const float u = pu[e], v = pv[e];
    const float uu = u * u, vv = v * v;
    const float hs2 = uu + vv;
    float gu = 0.f, gv = 0.f;
    if (__builtin_isfinite(hs2)) {
      float r;
      const float p = dl_position(hs2, c, r);
      if (p > 0.f && p < top && r > 0.f) {
        int k0 = (int)p;
        k0 = k0 > ns - 2 ? ns - 2 : k0;
        const float d = s_g[z * ns + k0 + 1] - s_g[z * ns + k0];
        const float dc = d * c;
        const float du_ = dc * u, dv_ = dc * v;
        gu = du_ / r, gv = dv_ / r;
      }
    }
    du[e] = gu, dv[e] = gv;
    for (int ch = 2; ch < sr_c; ++ch) du[(long)ch * g.vol + e] = 0.f;
  }
}

}  // namespace
