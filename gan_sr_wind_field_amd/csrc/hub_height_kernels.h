// The kernels of csrc/hub_height.hip ([HUB_HEIGHT]; hub_height.py holds the definition), kept in a header of their own so
// that a host program can run them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/hub_height_host_check.cpp: the shim of tools/host_shim.h and the macro HH_FLAG_SET).  Nothing here needs more of
// HIP than __global__, __shared__, threadIdx / blockIdx and __syncthreads.  No thread leaves a kernel that has a barrier
// before the last barrier.
//
// hub_height_kernel        grid (nb, B), 256 threads.  A workgroup strides over chunks of cps consecutive columns,
//                          cps = min(256 / NZ, 256 / nh).  1. Staging, thread t = (column slot t / NZ, level t % NZ): the
//                          height above ground h = z - terrain (ONE fp32 subtraction) and u, v of HR, SR and TL go to LDS
//                          with coalesced loads, every operand element read once; a NaN height flags its column.
//                          2. Thread t = (height t / cps, column slot t % cps) owns one (column, height) pair - the same
//                          height in every chunk, so its 18 sums are plain registers: validity from fp32 comparisons, one
//                          bisection of the staged column, the weight in double (linear in h, or in ln h), reused for the
//                          six component planes (blended in double, rounded once to fp32), V = sqrtf(u u + v v), the
//                          power curve from LDS.  With cols the seven planes of the pair are written here, lanes along
//                          the columns.  After the last chunk the slots of a height are added through LDS in slot order:
//                          ONE partial row of nh x 18 floats per workgroup.
// hub_height_final_kernel  adds the nb partial rows of a sample in a fixed order in double (the scheme of
//                          level_diag_final_kernel).
//
// No atomics, no zero fill: two calls give the same bits.  n_valid is a sum of 1.0f: a row counts at most the columns of
// its workgroup, cps <= 128 without the row cap and about X * Y / 2048 <= 2^19 with it (X, Y <= 32768) - far below 2^24,
// so every partial count is an exact integer and the double sum of the rows is exact.
#pragma once

#pragma clang fp contract(off)

#ifndef HH_FLAG_SET
// several threads of a workgroup may store the same 1 into one LDS word
#define HH_FLAG_SET(p) (*(p) = 1)
#endif

namespace {

constexpr int HH_BLOCK = 256;
constexpr int HH_NS = WSR_HUB_HEIGHT_SUMS;
constexpr int HH_MAX_NH = WSR_HUB_HEIGHT_MAX_HEIGHTS;
constexpr int HH_MAX_NK = WSR_HUB_HEIGHT_MAX_KNOTS;
constexpr int HH_MAX_NZ = WSR_HUB_HEIGHT_MAX_NZ;
constexpr int HH_MAX_ROWS = WSR_HUB_HEIGHT_MAX_ROWS;
constexpr int HH_PLANES = WSR_HUB_HEIGHT_PLANES;

// the heights (metres above ground) and the power curve (speeds in normalised units), passed by value: kernel arguments
struct HhTables {
  float q[HH_MAX_NH];
  float cv[HH_MAX_NK], cp[HH_MAX_NK];
};

struct HhGeom {
  int X, Y, NZ, nh, nk, log_mode;
  int cps;      // columns per chunk
  int ncols;    // X * Y
  int nchunks;  // ceil(ncols / cps)
  int nb;       // workgroups (partial rows) per sample
};

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_hub_height documents them.  heights, curve_v: host.
inline int hh_geom(HhGeom& g, int B, int X, int Y, int NZ, const float* heights, int nh, const float* curve_v, int nk,
                   int log_mode) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ < 2 || !heights || !curve_v) return WSR_EINVAL;
  if (nh < 1 || nh > HH_MAX_NH || nk < 2 || nk > HH_MAX_NK || (log_mode != 0 && log_mode != 1)) return WSR_EINVAL;
  for (int k = 0; k < nh; ++k)
    if (!(heights[k] > (k ? heights[k - 1] : 0.f)) || !(heights[k] <= 3.0e38f)) return WSR_EINVAL;
  for (int k = 0; k < nk; ++k)
    if (!(k ? curve_v[k] > curve_v[k - 1] : curve_v[k] >= 0.f) || !(curve_v[k] <= 3.0e38f)) return WSR_EINVAL;
  if (NZ > HH_MAX_NZ || B > 65535 || X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.X = X, g.Y = Y, g.NZ = NZ, g.nh = nh, g.nk = nk, g.log_mode = log_mode;
  const int by_z = HH_BLOCK / NZ, by_h = HH_BLOCK / nh;
  g.cps = by_z < by_h ? by_z : by_h;                    // >= 2
  g.ncols = X * Y;                                      // (< 2^30)
  g.nchunks = (g.ncols + g.cps - 1) / g.cps;
  g.nb = g.nchunks < HH_MAX_ROWS ? g.nchunks : HH_MAX_ROWS;
  return 0;
}

inline long hh_workspace_floats(const HhGeom& g, int B) { return (long)B * g.nb * g.nh * HH_NS; }

// np.interp(V, cv, cp) of an ascending table: the end values outside, slope * (V - cv[i]) + cp[i] inside, in double,
// rounded once; a NaN stays a NaN
__device__ __forceinline__ float hh_curve(float V, const float* cv, const float* cp, int nk) {
  if (V != V) return V;
  if (!(V > cv[0])) return cp[0];
  if (V >= cv[nk - 1]) return cp[nk - 1];
  int i = 0;  // the largest i with cv[i] <= V
  for (int k = 1; k < nk - 1; ++k) i += cv[k] <= V ? 1 : 0;
  const double x0 = (double)cv[i], x1 = (double)cv[i + 1], y0 = (double)cp[i], y1 = (double)cp[i + 1];
  const double slope = (y1 - y0) / (x1 - x0);
  return (float)(slope * ((double)V - x0) + y0);
}

// diagnostics.hip's angle between two horizontal vectors
__device__ __forceinline__ float hh_angle(float au, float av, float bu, float bv) {
  const float cr = fabsf(au * bv - av * bu), dt = au * bu + av * bv;
  return (cr == 0.f && dt == 0.f) ? 0.f : atan2f(cr, dt);
}

// partial rows: partials[((b * nb + blockIdx.x) * nh + height) * 18 + k]; cols (B, nh, 7, X, Y) or null; f2 may be null
__global__ __launch_bounds__(HH_BLOCK) void hub_height_kernel(const float* __restrict__ f0, int c0,
                                                              const float* __restrict__ f1, int c1,
                                                              const float* __restrict__ f2, int c2,
                                                              const float* __restrict__ zc,
                                                              const float* __restrict__ terrain, HhTables tab, HhGeom g,
                                                              float* __restrict__ partials, float* __restrict__ cols) {
  __shared__ float s_h[HH_BLOCK];                 // [slot][level]: metres above ground
  __shared__ float s_f[6][HH_BLOCK];              // u, v of HR, SR, TL
  __shared__ float s_acc[HH_NS][HH_BLOCK];
  __shared__ int s_nan[2][HH_BLOCK / 2];          // [chunk parity][slot]: the column holds a NaN height
  __shared__ float s_q[HH_MAX_NH], s_cv[HH_MAX_NK], s_cp[HH_MAX_NK];
  const int b = blockIdx.y, nb = gridDim.x, t = threadIdx.x;
  const int NZ = g.NZ, cps = g.cps, nh = g.nh, nk = g.nk, ncols = g.ncols;
  const int nsrc = f2 ? 3 : 2;
  const int slc = t / NZ, sk = t - slc * NZ;      // staging: (slot, level)
  const bool stager = slc < cps;
  const int qi = t / cps, lc = t - qi * cps;      // evaluation: (height, slot)
  const bool owner = qi < nh;
  const long vol = (long)ncols * NZ;              // (< 2^31: checked on the host)
  const float* p0 = f0 + (long)b * c0 * vol;
  const float* p1 = f1 + (long)b * c1 * vol;
  const float* p2 = f2 ? f2 + (long)b * c2 * vol : nullptr;
  const float* zp = zc + (long)b * vol;

  if (t < nh) s_q[t] = tab.q[t];
  if (t < nk) s_cv[t] = tab.cv[t], s_cp[t] = tab.cp[t];
  if (t < HH_BLOCK / 2) s_nan[0][t] = 0, s_nan[1][t] = 0;
  float acc[HH_NS];
#pragma unroll
  for (int k = 0; k < HH_NS; ++k) acc[k] = 0.f;

  int cur = 0;
  for (int chunk = blockIdx.x; chunk < g.nchunks; chunk += nb, cur ^= 1) {
    __syncthreads();  // the previous chunk's pairs are evaluated (and, before the first chunk, the tables are in LDS)
    const int col0 = chunk * cps;
    if (t < cps) s_nan[cur ^ 1][t] = 0;           // (read last in the previous chunk, written next in the following one)
    if (stager && col0 + slc < ncols) {
      const int col = col0 + slc;
      const long e = (long)col * NZ + sk;
      const float h = zp[e] - terrain[col];
      s_h[t] = h;                                 // (t = slc * NZ + sk for a stager)
      if (h != h) HH_FLAG_SET(&s_nan[cur][slc]);
      s_f[0][t] = p0[e], s_f[1][t] = p0[vol + e];
      s_f[2][t] = p1[e], s_f[3][t] = p1[vol + e];
      s_f[4][t] = p2 ? p2[e] : 0.f, s_f[5][t] = p2 ? p2[vol + e] : 0.f;
    }
    __syncthreads();
    const int col = col0 + lc;
    if (!owner || col >= ncols) continue;
    const float* hp = s_h + lc * NZ;
    const float q = s_q[qi];
    const float h0 = hp[0];
    bool valid = h0 <= q && q <= hp[NZ - 1] && s_nan[cur][lc] == 0;
    if (g.log_mode) valid = valid && h0 > 0.f;
    float V[3] = {0.f, 0.f, 0.f}, P[3] = {0.f, 0.f, 0.f};
    if (valid) {
      int lo = 0, hi = NZ - 1;                    // the largest j with hp[j] <= q
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hp[mid] <= q) lo = mid; else hi = mid - 1;
      }
      const int j = lo, j1 = lo < NZ - 1 ? lo + 1 : lo;
      double w = 0.0;                             // (on the top level: its value)
      if (j < NZ - 1) {
        const double hj = (double)hp[j], hj1 = (double)hp[j1], qd = (double)q;
        w = g.log_mode ? log(qd / hj) / log(hj1 / hj) : (qd - hj) / (hj1 - hj);
      }
      float c[6];
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const double a = (double)s_f[s][lc * NZ + j], d = (double)s_f[s][lc * NZ + j1];
        c[s] = (float)(a + w * (d - a));
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (s < nsrc) {
          const float uu = c[2 * s] * c[2 * s], vv = c[2 * s + 1] * c[2 * s + 1];
          V[s] = sqrtf(uu + vv);
          P[s] = hh_curve(V[s], s_cv, s_cp, nk);
        }
      }
      const float ds = V[1] - V[0], ps = P[1] - P[0];
      acc[0] += 1.f;
      acc[1] += V[0], acc[2] += V[1];
      acc[4] += fabsf(ds);
      acc[6] += ds * ds;
      acc[8] += (V[0] * V[0]) * V[0], acc[9] += (V[1] * V[1]) * V[1];
      acc[11] += P[0], acc[12] += P[1];
      acc[14] += fabsf(ps);
      acc[16] += V[0] * hh_angle(c[0], c[1], c[2], c[3]);
      if (nsrc == 3) {
        const float dt = V[2] - V[0], pt = P[2] - P[0];
        acc[3] += V[2];
        acc[5] += fabsf(dt);
        acc[7] += dt * dt;
        acc[10] += (V[2] * V[2]) * V[2];
        acc[13] += P[2];
        acc[15] += fabsf(pt);
        acc[17] += V[0] * hh_angle(c[0], c[1], c[4], c[5]);
      }
    }
    if (cols) {
      float* o = cols + (((long)b * nh + qi) * HH_PLANES) * ncols + col;
      o[0] = V[0], o[(long)ncols] = V[1], o[2L * ncols] = V[2];
      o[3L * ncols] = P[0], o[4L * ncols] = P[1], o[5L * ncols] = P[2];
      o[6L * ncols] = valid ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < HH_NS; ++k) s_acc[k][t] = acc[k];
  __syncthreads();
  float* row = partials + ((long)b * nb + blockIdx.x) * (nh * HH_NS);
  for (int item = t; item < nh * HH_NS; item += HH_BLOCK) {
    const int qq = item / HH_NS, k = item - qq * HH_NS;
    float s = s_acc[k][qq * cps];
    for (int slot = 1; slot < cps; ++slot) s += s_acc[k][qq * cps + slot];
    row[item] = s;
  }
}

// sums[b][item] = the nb partial rows of sample b in double: 64 items per workgroup of 16 waves, wave w adds rows w,
// w + 16, ... in order, the sixteen wave sums are then added in order
constexpr int HH_FBLOCK = 1024, HH_FWAVES = HH_FBLOCK / 64;
__global__ __launch_bounds__(HH_FBLOCK) void hub_height_final_kernel(const float* __restrict__ partials, int nb, int items,
                                                                     double* __restrict__ sums) {
  __shared__ double sh[HH_FWAVES][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x * 64 + lane;
  const float* rows = partials + (long)b * nb * items;
  double s = 0.0;
  if (item < items)
    for (int r = wave; r < nb; r += HH_FWAVES) s += (double)rows[(long)r * items + item];
  sh[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && item < items) {
    double a = sh[0][lane];
    for (int w = 1; w < HH_FWAVES; ++w) a += sh[w][lane];
    sums[(long)b * items + item] = a;
  }
}

}  // namespace
