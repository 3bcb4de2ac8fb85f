// The kernels of csrc/consistency_loss.hip ([CONSISTENCY_LOSS]), kept in a header of their own so that a host program can
// run them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/consistency_loss_host_check.cpp: the shim of tools/host_shim.h for __global__, threadIdx / blockIdx and
// __syncthreads, with CL_LDS naming a heap buffer of exactly the launch's LDS size).  Nothing here needs more of HIP than
// those.  No thread leaves a kernel between its barrier and its end other than with its whole workgroup.
//
// All tensors fp32 planar, z innermost; (y, z) is the contiguous index m = y NZ + z.  K = 2 R + 1 taps; wx (XL, K) and
// wy (YL, K) are the tables of degradation.axis_weights.  Every product and every sum is rounded (no contraction),
// accumulators start from +0.0f, indices ascend, a tap outside [0, n) is skipped and never read.
//
// cl_fwd_kernel<V>  one workgroup of 256 threads per (run of TJ coarse rows j, coarse column i, (sample, channel)).  The x
//                   pass runs straight from global memory over the rows y the run's taps reach, clipped to [0, Y): a
//                   thread owns V consecutive m (V | NZ, one load of 4 V bytes per field and tap), consecutive threads
//                   consecutive pieces, so every load is a coalesced run for any NZ; e = fl(sr - hr) is formed in
//                   registers, g = sum_d fl(wx[i, d] e[s i + d - R]) goes to the LDS strip at m - m_lo, which consecutive
//                   lanes write to consecutive banks.  After ONE barrier the y pass reads the strip - lanes run over
//                   consecutive (j, z), the rows of one tap are s NZ floats apart - and writes the contiguous (j, z) run
//                   of r.  Every element of r is written exactly once.
// cl_bwd_kernel<V>  the mirror image: one workgroup per (run of TY rows y, column x, (sample, channel of dsr)).  A channel
//                   from 3 on is zero-filled.  Otherwise the workgroup forms t[x; j, z] = sum_i fl(wx[i, x - s i + R]
//                   G[i, j, z]) for the coarse rows j its y reach from the small, L2-resident G into the LDS strip, and
//                   after ONE barrier dsr[x, y, z] = sum_j fl(wy[j, y - s j + R] t[x; j, z]) per piece of V consecutive m.
//                   Every element of dsr is written exactly once; nothing was saved by the forward.
//
// No atomics anywhere, and every sum has a fixed order: the same bits on every call.
#pragma once

#pragma clang fp contract(off)

#ifndef CL_LDS
#define CL_LDS(name) extern __shared__ float name[]
#endif

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_MAX_LDS_FLOATS = WSR_CONSISTENCY_LOSS_LDS_FLOATS;  // 64 KiB: two workgroups per CU
constexpr int CL_TARGET_FLOATS = 4096;  // what a workgroup aims to hold / write: 16 pieces of 4 floats per thread
constexpr int CL_MAX_R = WSR_DEGRADE_MAX_R;
constexpr int CL_MIN_S = 2, CL_MAX_S = 32;

struct ClGeom {
  int B, X, Y, NZ, s, R;
  int XL, YL;    // ceil(X / s), ceil(Y / s)
  int TJ, njr;   // coarse rows per forward workgroup; runs of them
  int TY, nyr;   // rows per backward workgroup; runs of them
  int fwd_lds;   // floats of the forward's strip: the rows a run's taps reach, clipped to Y, times NZ
  int bwd_lds;   // floats of the backward's strip: the coarse rows a run reaches, clipped to YL, times NZ
};

template <int V> struct alignas(4 * V) ClPiece {
  float v[V];
};

// ceil(a / s) for s > 0 and any a
__device__ __forceinline__ int cl_ceil_div(int a, int s) { return a >= 0 ? (a + s - 1) / s : -((-a) / s); }

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_coarse_residual documents them.  A function of the arguments alone, and
// neither result depends on it.
inline int cl_geom(ClGeom& g, int s, int R, int B, int X, int Y, int NZ) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (s < CL_MIN_S || s > CL_MAX_S || R < 0 || R > CL_MAX_R) return WSR_EINVAL;
  if ((long)B * 3 > 65535 || X > 65535 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.s = s, g.R = R;
  g.XL = (X + s - 1) / s, g.YL = (Y + s - 1) / s;
  const long per = CL_TARGET_FLOATS / NZ;  // rows of NZ floats in the target
  long tj = (per - 2L * R - 1) / s + 1;    // s (TJ - 1) + 2 R + 1 <= per
  if (per < 2L * R + 1 || tj < 1) tj = 1;
  if (tj > g.YL) tj = g.YL;
  g.TJ = (int)tj;
  g.njr = (g.YL + g.TJ - 1) / g.TJ;
  long rows = (long)s * (g.TJ - 1) + 2L * R + 1;
  if (rows > Y) rows = Y;
  long ty = per < 1 ? 1 : per;
  if (ty > Y) ty = Y;
  g.TY = (int)ty;
  g.nyr = (Y + g.TY - 1) / g.TY;
  long nj = (g.TY - 1 + 2L * R) / s + 1;
  if (nj > g.YL) nj = g.YL;
  if (rows * NZ > CL_MAX_LDS_FLOATS || nj * NZ > CL_MAX_LDS_FLOATS) return WSR_EUNSUPPORTED;
  g.fwd_lds = (int)(rows * NZ), g.bwd_lds = (int)(nj * NZ);
  return 0;
}

// hr (B, hr_c, X, Y, NZ), sr (B, sr_c, X, Y, NZ), r (B, 3, XL, YL, NZ); grid (njr, XL, 3 B)
template <int V>
__global__ __launch_bounds__(CL_BLOCK) void cl_fwd_kernel(const float* __restrict__ hr, int hr_c,
                                                          const float* __restrict__ sr, int sr_c,
                                                          const float* __restrict__ wx, const float* __restrict__ wy,
                                                          ClGeom g, float* __restrict__ r) {
  CL_LDS(strip);
  const int t = threadIdx.x;
  const int j0 = (int)blockIdx.x * g.TJ, i = blockIdx.y;
  const int b = (int)blockIdx.z / 3, c = (int)blockIdx.z % 3;
  const int s = g.s, R = g.R, NZ = g.NZ, K = 2 * R + 1;
  const int nj = g.YL - j0 < g.TJ ? g.YL - j0 : g.TJ;
  int ylo = s * j0 - R, yhi = s * (j0 + nj - 1) + R + 1;  // the rows the run's taps reach: [ylo, yhi)
  ylo = ylo < 0 ? 0 : ylo;
  yhi = yhi > g.Y ? g.Y : yhi;
  const int n = (yhi - ylo) * NZ;  // <= g.fwd_lds

  // x pass: taps d with 0 <= s i + d - R < X
  int dlo = R - s * i, dhi = g.X - 1 - s * i + R;
  dlo = dlo < 0 ? 0 : dlo;
  dhi = dhi > 2 * R ? 2 * R : dhi;
  const long plane = (long)g.Y * NZ;
  const float* ph = hr + ((long)b * hr_c + c) * g.X * plane + (long)ylo * NZ;
  const float* ps = sr + ((long)b * sr_c + c) * g.X * plane + (long)ylo * NZ;
  const float* wrow = wx + (long)i * K;
  for (int e = t * V; e < n; e += CL_BLOCK * V) {
    ClPiece<V> acc;
    for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
    for (int d = dlo; d <= dhi; ++d) {
      const long off = (long)(s * i + d - R) * plane + e;
      const ClPiece<V> a = *reinterpret_cast<const ClPiece<V>*>(ps + off);
      const ClPiece<V> h = *reinterpret_cast<const ClPiece<V>*>(ph + off);
      const float w = wrow[d];
      for (int k = 0; k < V; ++k) {
        const float diff = a.v[k] - h.v[k];
        const float p = w * diff;
        acc.v[k] = acc.v[k] + p;
      }
    }
    *reinterpret_cast<ClPiece<V>*>(strip + e) = acc;
  }
  __syncthreads();

  // y pass: taps d with 0 <= s j + d - R < Y
  const int no = nj * NZ;
  float* pr = r + ((((long)b * 3 + c) * g.XL + i) * g.YL + j0) * NZ;
  for (int o = t; o < no; o += CL_BLOCK) {
    const int jj = o / NZ, z = o - jj * NZ, j = j0 + jj;
    int elo = R - s * j, ehi = g.Y - 1 - s * j + R;
    elo = elo < 0 ? 0 : elo;
    ehi = ehi > 2 * R ? 2 * R : ehi;
    const float* wrow_y = wy + (long)j * K;
    float acc = 0.f;
    for (int d = elo; d <= ehi; ++d) {
      const float p = wrow_y[d] * strip[(s * j + d - R - ylo) * NZ + z];
      acc = acc + p;
    }
    pr[o] = acc;
  }
}

// G (B, 3, XL, YL, NZ), dsr (B, sr_c, X, Y, NZ); grid (nyr, X, sr_c B)
template <int V>
__global__ __launch_bounds__(CL_BLOCK) void cl_bwd_kernel(const float* __restrict__ G, const float* __restrict__ wx,
                                                          const float* __restrict__ wy, ClGeom g, int sr_c,
                                                          float* __restrict__ dsr) {
  CL_LDS(strip);
  const int t = threadIdx.x;
  const int y0 = (int)blockIdx.x * g.TY, x = blockIdx.y;
  const int b = (int)blockIdx.z / sr_c, c = (int)blockIdx.z % sr_c;
  const int s = g.s, R = g.R, NZ = g.NZ, K = 2 * R + 1;
  const int ny = g.Y - y0 < g.TY ? g.Y - y0 : g.TY;
  const int n = ny * NZ;
  float* out = dsr + ((((long)b * sr_c + c) * g.X + x) * g.Y + y0) * NZ;
  if (c >= 3) {  // (the whole workgroup: no barrier is skipped by a part of it)
    ClPiece<V> zero;
    for (int k = 0; k < V; ++k) zero.v[k] = 0.f;
    for (int e = t * V; e < n; e += CL_BLOCK * V) *reinterpret_cast<ClPiece<V>*>(out + e) = zero;
    return;
  }

  // the coarse rows the run reaches: |y - s j| <= R for some y of it
  int jlo = cl_ceil_div(y0 - R, s), jhi = (y0 + ny - 1 + R) / s;
  jlo = jlo < 0 ? 0 : jlo;
  jhi = jhi > g.YL - 1 ? g.YL - 1 : jhi;
  const int nt = (jhi - jlo + 1) * NZ;  // <= g.bwd_lds; <= 0: no coarse cell reads this run
  // the coarse columns that read x: 0 <= x - s i + R <= 2 R
  int ilo = cl_ceil_div(x - R, s), ihi = (x + R) / s;
  ilo = ilo < 0 ? 0 : ilo;
  ihi = ihi > g.XL - 1 ? g.XL - 1 : ihi;
  const long cplane = (long)g.YL * NZ;
  const float* pg = G + ((long)b * 3 + c) * g.XL * cplane + (long)jlo * NZ;
  for (int e = t * V; e < nt; e += CL_BLOCK * V) {
    ClPiece<V> acc;
    for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
    for (int i = ilo; i <= ihi; ++i) {
      const ClPiece<V> u = *reinterpret_cast<const ClPiece<V>*>(pg + (long)i * cplane + e);
      const float w = wx[(long)i * K + (x - s * i + R)];
      for (int k = 0; k < V; ++k) {
        const float p = w * u.v[k];
        acc.v[k] = acc.v[k] + p;
      }
    }
    *reinterpret_cast<ClPiece<V>*>(strip + e) = acc;
  }
  __syncthreads();

  for (int e = t * V; e < n; e += CL_BLOCK * V) {
    const int yy = e / NZ, z = e - yy * NZ, y = y0 + yy;
    int ja = cl_ceil_div(y - R, s), jb = (y + R) / s;
    ja = ja < 0 ? 0 : ja;
    jb = jb > g.YL - 1 ? g.YL - 1 : jb;
    ClPiece<V> acc;
    for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
    for (int j = ja; j <= jb; ++j) {
      const float w = wy[(long)j * K + (y - s * j + R)];
      const ClPiece<V> u = *reinterpret_cast<const ClPiece<V>*>(strip + (j - jlo) * NZ + z);
      for (int k = 0; k < V; ++k) {
        const float p = w * u.v[k];
        acc.v[k] = acc.v[k] + p;
      }
    }
    *reinterpret_cast<ClPiece<V>*>(out + e) = acc;
  }
}

}  // namespace
