// The kernels of csrc/spectral_loss.hip ([SPECTRAL_LOSS]), kept in a header of their own so that a host program can run
// them block by block on threads under the address and undefined-behaviour sanitisers (tools/spectral_loss_host_check.cpp:
// a shim for __global__, __shared__, threadIdx / blockIdx and __syncthreads).  Nothing here needs more of HIP than those,
// float2 / float4, fmaf, sinpi and sincospi.  No thread leaves a kernel that has a barrier before the last barrier.
//
// The forward follows csrc/spectra.hip pass for pass (prep / mean / row / column / final; see there for the layout of a
// workgroup in each) over SIX planes - HR and SR, three components each - and two sums per bin, e_hr and e_sr; the
// column pass also writes F_sr(b, comp, kx, ky, z), complex fp32, when asked to.  The backward is the adjoint:
//
//   bprep   bins and window as prep, and gbin (B, NZ, NK) double rounded ONCE to fp32 and laid out (B, NK, NZ)
//   icol    C(x, ky) = sum_kx G(bin(kx, ky)) F_sr(kx, ky) exp(+2 pi i kx x / X) per (b, comp, ky, chunk of <= 16 levels):
//           thread (x, z) holds SL_IKB values of x, G F comes through LDS in slabs of SL_IXT rows kx
//   irow    u(x, y) = sum_ky h Re(C exp(+2 pi i ky y / Y)), v = 2 scale wx wy u.  A workgroup owns M lines (rows x levels)
//           whose KY values h C it stages in LDS, re and im rows apart; a thread owns four consecutive lines of one y (two
//           float4 and one twiddle per eight fmaf) and writes v into dsr
//   mean    the plane sums of v (the forward's mean kernel on dsr), mfin adds the partial rows in double
//   sub     dsr -= mean_plane(v): the adjoint of the detrend
#pragma once

namespace {

constexpr int SL_BLOCK = 256;
constexpr int SL_NS = 2;           // e_hr, e_sr
constexpr int SL_MAX_XY = WSR_SPECTRUM_MAX_XY;
constexpr int SL_PLANES = 6;       // 2 fields x 3 components
constexpr int SL_MEAN_ROWS = 32;   // partial rows of the plane means, at most
constexpr int SL_GMAX = 8192;      // floats of the row passes' staged lines (32 KB)
constexpr int SL_BMAX = 7680;      // floats of the column pass' bin table (30 KB)
constexpr int SL_XT = 8;           // rows of A per LDS slab of the column pass
constexpr int SL_ZC3 = 16;         // levels per workgroup of the column passes, at most
constexpr int SL_KB = 2;           // modes kx per thread of the column pass
constexpr int SL_PRE = (SL_PLANES * SL_XT * SL_ZC3 + SL_BLOCK - 1) / SL_BLOCK;  // slab elements per thread
constexpr int SL_IXT = 64;         // rows kx of G F per LDS slab of the inverse column pass
constexpr int SL_IKB = 4;          // values of x per thread of the inverse column pass
constexpr int SL_IPRE = SL_IXT * SL_ZC3 / SL_BLOCK;

struct SlGeom {
  int B, X, Y, NZ, KY, NK;
  int zc1, nzc1, cpb1, rb;           // mean: levels per workgroup, z chunks, columns per pass, partial rows
  int zc2, nzc2, xb, nxb, M, MQ;     // row: levels and rows per workgroup, lines, quads of lines
  int zc3, nzc3, kxc;                // column: levels per workgroup, z chunks, kx per chunk
  int zc4, nzc4, xc4;                // inverse column: levels per workgroup, z chunks, x per chunk (times SL_IKB)
  int zc5, nzc5, xb5, nxb5, M5, MQ5; // inverse row: as row, with 2 KY floats per line
  int64_t o_bins, o_wx, o_wy, o_mean, o_a, o_part, total_f;  // workspace offsets of the forward, in floats
  int64_t o_gf, o_c, o_mv, o_mf, total_b;                    // ... of the backward (bins, wx, wy as in the forward)
};

struct SlFields {
  const float* p[2];
  int c[2];
};

// ---- prep: bins (X, KY) int32, wx (X), wy (Y); backward: also gf (B, NK, NZ) = (float)gbin (B, NZ, NK) -----------------
__global__ __launch_bounds__(SL_BLOCK) void sl_prep_kernel(SlGeom g, int window, int* __restrict__ bins,
                                                           float* __restrict__ wx, float* __restrict__ wy,
                                                           const double* __restrict__ gbin, float* __restrict__ gf) {
  const int X = g.X, Y = g.Y, KY = g.KY;
  const long e = (long)blockIdx.x * SL_BLOCK + threadIdx.x;
  const long n0 = (long)X * KY, n1 = n0 + X + Y;
  if (e < n0) {
    const int kx = (int)(e / KY), ky = (int)(e - (long)kx * KY);
    const long ks = kx <= X / 2 ? kx : kx - X;  // the signed frequency
    const long N = X > Y ? X : Y, xy = (long)X * Y;
    const long q = (ks * Y) * (ks * Y) + ((long)ky * X) * ((long)ky * X);
    const long lhs = 4 * N * N * q, xy2 = xy * xy;  // (< 2^62 for X, Y <= 1024)
    long k = (long)floor((double)N * sqrt((double)q) / (double)xy + 0.5);
    while (k > 0 && lhs < (2 * k - 1) * (2 * k - 1) * xy2) --k;
    while (lhs >= (2 * k + 1) * (2 * k + 1) * xy2) ++k;
    bins[e] = (int)(k < g.NK ? k : g.NK - 1);  // (every mode has a bin below NK: kappa <= N / sqrt(2))
  } else if (e < n1) {
    const int i = (int)(e - n0);
    const bool is_x = i < X;
    const int n = is_x ? X : Y, idx = is_x ? i : i - X;
    float w = 1.f;
    if (window == WSR_SPECTRUM_WINDOW_HANN && n > 1) {
      const double s = sinpi(((double)idx + 0.5) / (double)n);
      w = (float)(s * s);
    }
    (is_x ? wx : wy)[idx] = w;
  } else if (gbin && e - n1 < (long)g.B * g.NK * g.NZ) {
    const long i = e - n1;  // the element of gf: (b, bin, z)
    const int z = (int)(i % g.NZ);
    const long r = i / g.NZ;
    const int k = (int)(r % g.NK), b = (int)(r / g.NK);
    gf[i] = (float)gbin[((long)b * g.NZ + z) * g.NK + k];
  }
}

__device__ __forceinline__ const float* sl_plane(const SlFields& f, int p, int b, int vol) {
  const int fi = p / 3, comp = p - fi * 3;
  return f.p[fi] + ((long)b * f.c[fi] + comp) * vol;
}

// ---- mean: mpart[((b * np + p) * rb + row) * NZ + z] = the fp32 sum of plane p at level z over the columns of `row`,
// np = gridDim.y planes (6 in the forward, the 3 of dsr in the backward) -----------------------------------------------
__global__ __launch_bounds__(SL_BLOCK) void sl_mean_kernel(SlFields f, SlGeom g, float* __restrict__ mpart) {
  __shared__ float sh[SL_BLOCK];
  const int t = threadIdx.x, p = blockIdx.y, b = blockIdx.z, np = gridDim.y;
  const int zci = blockIdx.x / g.rb, row = blockIdx.x - zci * g.rb;
  const int NZ = g.NZ, ncols = g.X * g.Y, vol = ncols * NZ;
  const int slot = t / g.zc1, zl = t - slot * g.zc1, z = zci * g.zc1 + zl;
  const float* src = sl_plane(f, p, b, vol);
  float acc = 0.f;
  if (slot < g.cpb1 && z < NZ)
    for (int col = row * g.cpb1 + slot; col < ncols; col += g.rb * g.cpb1) acc += src[col * NZ + z];
  sh[t] = acc;
  __syncthreads();
  if (t < g.zc1 && zci * g.zc1 + t < NZ) {
    float s = sh[t];
    for (int q = 1; q < g.cpb1; ++q) s += sh[q * g.zc1 + t];
    mpart[((long)(b * np + p) * g.rb + row) * NZ + zci * g.zc1 + t] = s;
  }
}

// ---- row pass: A[(((b * 6 + p) * X + x) * KY + ky) * NZ + z] = sum_j g(x, j, z) exp(-2 pi i ky j / Y) ---------------
__global__ __launch_bounds__(SL_BLOCK) void sl_row_kernel(SlFields f, SlGeom g, const float* __restrict__ mpart,
                                                          const float* __restrict__ wx, const float* __restrict__ wy,
                                                          float2* __restrict__ A) {
  __shared__ __attribute__((aligned(16))) float sg[SL_GMAX];
  __shared__ float2 tw[SL_MAX_XY];
  __shared__ float smean[64];
  const int t = threadIdx.x, p = blockIdx.y, b = blockIdx.z;
  const int xbi = blockIdx.x / g.nzc2, zci = blockIdx.x - xbi * g.nzc2;
  const int X = g.X, Y = g.Y, NZ = g.NZ, KY = g.KY, M = g.M, MQ = g.MQ, MP = 4 * MQ, zc = g.zc2;
  const int x0 = xbi * g.xb, z0 = zci * zc, vol = X * Y * NZ;
  const float* src = sl_plane(f, p, b, vol);
  for (int j = t; j < Y; j += SL_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)j / (double)Y, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
  }
  if (t < zc && z0 + t < NZ) {
    const float* rows = mpart + (long)(b * SL_PLANES + p) * g.rb * NZ + z0 + t;
    double s = 0.0;
    for (int r = 0; r < g.rb; ++r) s += (double)rows[(long)r * NZ];
    smean[t] = (float)(s / ((double)X * (double)Y));
  }
  __syncthreads();
  for (int e = t; e < Y * MP; e += SL_BLOCK) {
    const int j = e / MP, m = e - j * MP;
    const int xl = m / zc, zl = m - xl * zc;
    const int x = x0 + xl, z = z0 + zl;
    float v = 0.f;
    if (m < M && x < X && z < NZ) v = (src[(x * Y + j) * NZ + z] - smean[zl]) * (wx[x] * wy[j]);
    sg[e] = v;
  }
  __syncthreads();
  const float4* sg4 = reinterpret_cast<const float4*>(sg);
  float2* dst = A + (size_t)(b * SL_PLANES + p) * X * KY * NZ;
  for (int it = t; it < KY * MQ; it += SL_BLOCK) {
    const int ky = it / MQ, mq = it - ky * MQ;
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;
    for (int j = 0; j < Y; ++j) {
      const float4 v = sg4[j * MQ + mq];
      const float2 w = tw[idx];
      re[0] = fmaf(v.x, w.x, re[0]);
      re[1] = fmaf(v.y, w.x, re[1]);
      re[2] = fmaf(v.z, w.x, re[2]);
      re[3] = fmaf(v.w, w.x, re[3]);
      im[0] = fmaf(-v.x, w.y, im[0]);
      im[1] = fmaf(-v.y, w.y, im[1]);
      im[2] = fmaf(-v.z, w.y, im[2]);
      im[3] = fmaf(-v.w, w.y, im[3]);
      idx += ky;
      if (idx >= Y) idx -= Y;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * mq + r;
      const int xl = m / zc, zl = m - xl * zc;
      const int x = x0 + xl, z = z0 + zl;
      if (m < M && x < X && z < NZ) dst[((size_t)x * KY + ky) * NZ + z] = make_float2(re[r], im[r]);
    }
  }
}

// ---- column pass: part[((b * KY + ky) * NK * 2 + bin * 2 + k) * NZ + z] = the modes (kx, ky) of the bin, ascending kx;
// saved (when not null) [(((b * 3 + comp) * X + kx) * KY + ky) * NZ + z] = F_sr -----------------------------------------
__global__ __launch_bounds__(SL_BLOCK) void sl_col_kernel(SlGeom g, const int* __restrict__ bins,
                                                          const float2* __restrict__ A, float* __restrict__ part,
                                                          float2* __restrict__ saved) {
  __shared__ float2 tw[SL_MAX_XY];
  __shared__ int sbin[SL_MAX_XY];
  __shared__ float2 sA[SL_PLANES * SL_XT * SL_ZC3];
  __shared__ float prod[SL_KB * SL_BLOCK * SL_NS];
  __shared__ float binsum[SL_BMAX];
  const int t = threadIdx.x, ky = blockIdx.y, b = blockIdx.z;
  const int X = g.X, NZ = g.NZ, KY = g.KY, NK = g.NK, zc = g.zc3, kxc = g.kxc;
  const int z0 = blockIdx.x * zc;
  const int kxl = t / zc, zl = t - kxl * zc;
  const bool live = kxl < kxc;
  for (int i = t; i < X; i += SL_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)i / (double)X, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
    sbin[i] = bins[i * KY + ky];
  }
  for (int e = t; e < NK * SL_NS * zc; e += SL_BLOCK) binsum[e] = 0.f;
  const int slab = SL_XT * zc;
  // the thread's SL_PRE elements of a slab: element e = t + i * 256 -> (plane, row of the slab, level)
  const float2* src[SL_PRE];
  int sxl[SL_PRE];  // the row of the slab, or X: never loaded (past the slab, or a level past NZ)
#pragma unroll
  for (int i = 0; i < SL_PRE; ++i) {
    const int e = t + i * SL_BLOCK;
    const int p = e / slab, r = e - p * slab;
    const int xl = r / zc, zz = r - xl * zc;
    const bool ok = e < SL_PLANES * slab && z0 + zz < NZ;
    sxl[i] = ok ? xl : X;
    src[i] = A + ((size_t)(b * SL_PLANES + (ok ? p : 0)) * X * KY + ky) * NZ + (ok ? z0 + zz : 0);
  }
  const size_t xstride = (size_t)KY * NZ;
  for (int kx0 = 0; kx0 < X; kx0 += SL_KB * kxc) {
    int kx[SL_KB], idx[SL_KB];
    float fr[SL_KB][SL_PLANES], fi[SL_KB][SL_PLANES];
#pragma unroll
    for (int r = 0; r < SL_KB; ++r) {  // (a thread past the end repeats the last mode, not deposited)
      kx[r] = kx0 + r * kxc + kxl < X ? kx0 + r * kxc + kxl : X - 1;
      idx[r] = 0;
#pragma unroll
      for (int p = 0; p < SL_PLANES; ++p) fr[r][p] = 0.f, fi[r][p] = 0.f;
    }
    float2 pre[SL_PRE];
#pragma unroll
    for (int i = 0; i < SL_PRE; ++i) pre[i] = sxl[i] < X ? src[i][(size_t)sxl[i] * xstride] : make_float2(0.f, 0.f);
    for (int xt0 = 0; xt0 < X; xt0 += SL_XT) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < SL_PRE; ++i)
        if (t + i * SL_BLOCK < SL_PLANES * slab) sA[t + i * SL_BLOCK] = pre[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < SL_PRE; ++i) {  // the next slab: in flight during the loop below
        const int x = xt0 + SL_XT + sxl[i];
        pre[i] = x < X ? src[i][(size_t)x * xstride] : make_float2(0.f, 0.f);
      }
      const int nx = X - xt0 < SL_XT ? X - xt0 : SL_XT;
      if (live)
        for (int xl = 0; xl < nx; ++xl) {
          float2 w[SL_KB];
#pragma unroll
          for (int r = 0; r < SL_KB; ++r) w[r] = tw[idx[r]];
#pragma unroll
          for (int p = 0; p < SL_PLANES; ++p) {  // a * (c - i s)
            const float2 a = sA[p * slab + xl * zc + zl];
#pragma unroll
            for (int r = 0; r < SL_KB; ++r) {
              fr[r][p] = fmaf(a.x, w[r].x, fr[r][p]);
              fr[r][p] = fmaf(a.y, w[r].y, fr[r][p]);
              fi[r][p] = fmaf(a.y, w[r].x, fi[r][p]);
              fi[r][p] = fmaf(-a.x, w[r].y, fi[r][p]);
            }
          }
#pragma unroll
          for (int r = 0; r < SL_KB; ++r) {
            idx[r] += kx[r];
            if (idx[r] >= X) idx[r] -= X;
          }
        }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < SL_KB; ++r) {
        const float* cr = fr[r];
        const float* ci = fi[r];
#pragma unroll
        for (int a = 0; a < SL_NS; ++a) {  // e_hr, e_sr: the same expression
          const int o = 3 * a;
          prod[((r * kxc + kxl) * SL_NS + a) * zc + zl] =
              ((cr[o] * cr[o] + ci[o] * ci[o]) + (cr[o + 1] * cr[o + 1] + ci[o + 1] * ci[o + 1])) +
              (cr[o + 2] * cr[o + 2] + ci[o + 2] * ci[o + 2]);
        }
        const int kxr = kx0 + r * kxc + kxl;
        if (saved && kxr < X && z0 + zl < NZ) {
#pragma unroll
          for (int comp = 0; comp < 3; ++comp)
            saved[(((size_t)(b * 3 + comp) * X + kxr) * KY + ky) * NZ + z0 + zl] = make_float2(cr[3 + comp], ci[3 + comp]);
        }
      }
    }
    __syncthreads();
    if (t < SL_NS * zc) {  // thread (sum q, level): the modes of this chunk in ascending kx, a run of one bin in a register
      const int q = t / zc, zz = t - q * zc;
      const int n = X - kx0 < SL_KB * kxc ? X - kx0 : SL_KB * kxc;
      int cur = sbin[kx0];
      float acc = binsum[(cur * SL_NS + q) * zc + zz];
      for (int l = 0; l < n; ++l) {
        const int bin = sbin[kx0 + l];
        const float v = prod[(l * SL_NS + q) * zc + zz];
        if (bin != cur) {
          binsum[(cur * SL_NS + q) * zc + zz] = acc;
          cur = bin;
          acc = binsum[(cur * SL_NS + q) * zc + zz];
        }
        acc += v;
      }
      binsum[(cur * SL_NS + q) * zc + zz] = acc;
    }
  }
  __syncthreads();
  float* dst = part + (size_t)(b * KY + ky) * NK * SL_NS * NZ;
  for (int e = t; e < NK * SL_NS * zc; e += SL_BLOCK) {
    const int r = e / zc, zz = e - r * zc;
    if (z0 + zz < NZ) dst[(size_t)r * NZ + z0 + zz] = binsum[e];
  }
}

// ---- final: out[((b * NZ + z) * NK + bin) * 2 + k] = scale * sum_ky h(ky) part[b][ky][bin][k][z], ascending, double ----
__global__ __launch_bounds__(SL_BLOCK) void sl_final_kernel(SlGeom g, const float* __restrict__ part, double scale,
                                                            double* __restrict__ out) {
  const int b = blockIdx.y, items = g.NK * SL_NS * g.NZ;
  const int e = blockIdx.x * SL_BLOCK + threadIdx.x;
  if (e >= items) return;
  const int r = e / g.NZ, z = e - r * g.NZ;
  const float* src = part + (size_t)b * g.KY * items + e;
  double s = 0.0;
  for (int ky = 0; ky < g.KY; ++ky) {
    const double h = (ky == 0 || 2 * ky == g.Y) ? 1.0 : 2.0;
    s += h * (double)src[(size_t)ky * items];
  }
  out[((size_t)b * g.NZ + z) * g.NK * SL_NS + r] = s * scale;
}

// ---- inverse column pass: Cw[(((b * 3 + comp) * X + x) * KY + ky) * NZ + z] = sum_kx gf(b, bin(kx, ky), z) F(kx, ky, z)
// exp(+2 pi i kx x / X), ascending kx.  The slab after the one in use is on its way into registers meanwhile. ----------
__global__ __launch_bounds__(SL_BLOCK) void sl_icol_kernel(SlGeom g, const int* __restrict__ bins,
                                                           const float* __restrict__ gf, const float2* __restrict__ F,
                                                           float2* __restrict__ Cw) {
  __shared__ float2 tw[SL_MAX_XY];
  __shared__ int sbin[SL_MAX_XY];
  __shared__ float2 sF[SL_IXT * SL_ZC3];
  const int t = threadIdx.x, ky = blockIdx.y, b = blockIdx.z;
  const int zci = blockIdx.x / 3, bp = b * 3 + (blockIdx.x - zci * 3);  // (the component: the fastest grid index)
  const int X = g.X, NZ = g.NZ, KY = g.KY, NK = g.NK, zc = g.zc4, xc = g.xc4;
  const int z0 = zci * zc;
  const int xl = t / zc, zl = t - xl * zc;
  const bool live = xl < xc;
  for (int i = t; i < X; i += SL_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)i / (double)X, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
    sbin[i] = bins[i * KY + ky];
  }
  const size_t xstride = (size_t)KY * NZ;
  const float2* src = F + ((size_t)bp * X * KY + ky) * NZ;
  float2* dst = Cw + ((size_t)bp * X * KY + ky) * NZ;
  const float* gsrc = gf + (size_t)b * NK * NZ;
  const int slab = SL_IXT * zc;
  // the thread's SL_IPRE elements of a slab: element e = t + i * 256 -> (row kx of the slab, level), or -1: never loaded
  int skl[SL_IPRE], szz[SL_IPRE];
#pragma unroll
  for (int i = 0; i < SL_IPRE; ++i) {
    const int e = t + i * SL_BLOCK;
    const int kl = e / zc, zz = e - kl * zc;
    const bool ok = e < slab && z0 + zz < NZ;
    skl[i] = ok ? kl : -1;
    szz[i] = ok ? z0 + zz : 0;
  }
  __syncthreads();  // (sbin, read by the loads below)
  for (int x0 = 0; x0 < X; x0 += SL_IKB * xc) {
    int xs[SL_IKB], idx[SL_IKB];
    float re[SL_IKB], im[SL_IKB];
#pragma unroll
    for (int r = 0; r < SL_IKB; ++r) {  // (a thread past the end repeats the last x, not written)
      xs[r] = x0 + r * xc + xl < X ? x0 + r * xc + xl : X - 1;
      idx[r] = 0, re[r] = 0.f, im[r] = 0.f;
    }
    float2 pre[SL_IPRE];
#pragma unroll
    for (int i = 0; i < SL_IPRE; ++i) {
      pre[i] = make_float2(0.f, 0.f);
      const int kx = skl[i];
      if (kx >= 0 && kx < X) {
        const float gv = gsrc[(size_t)sbin[kx] * NZ + szz[i]];
        const float2 a = src[(size_t)kx * xstride + szz[i]];
        pre[i] = make_float2(gv * a.x, gv * a.y);
      }
    }
    for (int k0 = 0; k0 < X; k0 += SL_IXT) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < SL_IPRE; ++i)
        if (t + i * SL_BLOCK < slab) sF[t + i * SL_BLOCK] = pre[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < SL_IPRE; ++i) {  // the next slab: in flight during the loop below
        pre[i] = make_float2(0.f, 0.f);
        const int kx = skl[i] >= 0 ? k0 + SL_IXT + skl[i] : X;
        if (kx < X) {
          const float gv = gsrc[(size_t)sbin[kx] * NZ + szz[i]];
          const float2 a = src[(size_t)kx * xstride + szz[i]];
          pre[i] = make_float2(gv * a.x, gv * a.y);
        }
      }
      const int nk = X - k0 < SL_IXT ? X - k0 : SL_IXT;
      if (live)
        for (int kl = 0; kl < nk; ++kl) {
          const float2 a = sF[kl * zc + zl];
#pragma unroll
          for (int r = 0; r < SL_IKB; ++r) {  // a * (c + i s)
            const float2 w = tw[idx[r]];
            re[r] = fmaf(a.x, w.x, re[r]);
            re[r] = fmaf(-a.y, w.y, re[r]);
            im[r] = fmaf(a.y, w.x, im[r]);
            im[r] = fmaf(a.x, w.y, im[r]);
            idx[r] += xs[r];
            if (idx[r] >= X) idx[r] -= X;
          }
        }
    }
    if (live && z0 + zl < NZ) {
#pragma unroll
      for (int r = 0; r < SL_IKB; ++r) {
        const int x = x0 + r * xc + xl;
        if (x < X) dst[(size_t)x * xstride + z0 + zl] = make_float2(re[r], im[r]);
      }
    }
  }
}

// ---- inverse row pass: dsr[((b * 3 + comp) * X + x) * Y + y) * NZ + z] = s2 wx wy sum_ky h Re(C exp(+2 pi i ky y / Y)) --
__global__ __launch_bounds__(SL_BLOCK) void sl_irow_kernel(SlGeom g, const float2* __restrict__ Cw,
                                                           const float* __restrict__ wx, const float* __restrict__ wy,
                                                           float s2, float* __restrict__ dsr) {
  __shared__ __attribute__((aligned(16))) float sc[SL_GMAX];
  __shared__ float2 tw[SL_MAX_XY];
  const int t = threadIdx.x;
  const int comp = blockIdx.y, b = blockIdx.z, plane = b * 3 + comp;
  const int xbi = blockIdx.x / g.nzc5, zci = blockIdx.x - xbi * g.nzc5;
  const int X = g.X, Y = g.Y, NZ = g.NZ, KY = g.KY, M = g.M5, MQ = g.MQ5, MP = 4 * MQ, zc = g.zc5;
  const int x0 = xbi * g.xb5, z0 = zci * zc;
  for (int j = t; j < Y; j += SL_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)j / (double)Y, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
  }
  const float2* src = Cw + (size_t)plane * X * KY * NZ;
  for (int e = t; e < KY * MP; e += SL_BLOCK) {
    const int ky = e / MP, m = e - ky * MP;
    const int xl = m / zc, zl = m - xl * zc;
    const int x = x0 + xl, z = z0 + zl;
    float2 v = make_float2(0.f, 0.f);
    if (m < M && x < X && z < NZ) {
      const float2 a = src[((size_t)x * KY + ky) * NZ + z];
      const float h = (ky == 0 || 2 * ky == Y) ? 1.f : 2.f;
      v = make_float2(h * a.x, h * a.y);
    }
    sc[(2 * ky) * MP + m] = v.x;
    sc[(2 * ky + 1) * MP + m] = v.y;
  }
  __syncthreads();
  const float4* sc4 = reinterpret_cast<const float4*>(sc);
  float* dst = dsr + (size_t)plane * X * Y * NZ;
  for (int it = t; it < Y * MQ; it += SL_BLOCK) {
    const int y = it / MQ, mq = it - y * MQ;
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;
    for (int ky = 0; ky < KY; ++ky) {
      const float4 cr = sc4[(2 * ky) * MQ + mq];
      const float4 ci = sc4[(2 * ky + 1) * MQ + mq];
      const float2 w = tw[idx];
      u[0] = fmaf(cr.x, w.x, u[0]);
      u[1] = fmaf(cr.y, w.x, u[1]);
      u[2] = fmaf(cr.z, w.x, u[2]);
      u[3] = fmaf(cr.w, w.x, u[3]);
      u[0] = fmaf(-ci.x, w.y, u[0]);
      u[1] = fmaf(-ci.y, w.y, u[1]);
      u[2] = fmaf(-ci.z, w.y, u[2]);
      u[3] = fmaf(-ci.w, w.y, u[3]);
      idx += y;
      if (idx >= Y) idx -= Y;
    }
    const float wyv = wy[y];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * mq + r;
      const int xl = m / zc, zl = m - xl * zc;
      const int x = x0 + xl, z = z0 + zl;
      if (m < M && x < X && z < NZ) dst[((size_t)x * Y + y) * NZ + z] = u[r] * (s2 * (wx[x] * wyv));
    }
  }
}

// ---- mfin: mfin[plane * NZ + z] = (float)(the partial rows of the plane sums of v added in double / (X Y)) ------------
__global__ __launch_bounds__(SL_BLOCK) void sl_mfin_kernel(SlGeom g, const float* __restrict__ mpart,
                                                           float* __restrict__ mfin) {
  const long e = (long)blockIdx.x * SL_BLOCK + threadIdx.x;
  if (e >= (long)g.B * 3 * g.NZ) return;
  const long plane = e / g.NZ;
  const int z = (int)(e - plane * g.NZ);
  const float* rows = mpart + plane * g.rb * g.NZ + z;
  double s = 0.0;
  for (int r = 0; r < g.rb; ++r) s += (double)rows[(long)r * g.NZ];
  mfin[e] = (float)(s / ((double)g.X * (double)g.Y));
}

// ---- sub: dsr(plane, col, z) -= mfin(plane, z); blockIdx.y the component, blockIdx.z the sample -----------------------
__global__ __launch_bounds__(SL_BLOCK) void sl_sub_kernel(SlGeom g, const float* __restrict__ mfin,
                                                          float* __restrict__ dsr) {
  const long vol = (long)g.X * g.Y * g.NZ;
  const long e = (long)blockIdx.x * SL_BLOCK + threadIdx.x;
  if (e >= vol) return;
  const long plane = (long)blockIdx.z * 3 + blockIdx.y;
  const int z = (int)(e % g.NZ);
  dsr[plane * vol + e] -= mfin[plane * g.NZ + z];
}

// ---- host side: the geometry of every pass and the workspace offsets, functions of the shape alone ---------------------
// floor(N / sqrt(2) + 1/2) + 1 in integers (wsr_level_spectra_bins): the largest k with (2k - 1)^2 <= 2 N^2, plus one
inline int sl_bins(int X, int Y) {
  const long N = X > Y ? X : Y;
  long k = (long)floor((double)N / sqrt(2.0) + 0.5);
  while (k > 0 && (2 * k - 1) * (2 * k - 1) > 2 * N * N) --k;
  while ((2 * k + 1) * (2 * k + 1) <= 2 * N * N) ++k;
  return (int)k + 1;
}

inline int64_t sl_up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_spectral_energy documents them
inline int sl_geom(SlGeom& g, int B, int X, int Y, int NZ) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (X > SL_MAX_XY || Y > SL_MAX_XY || B > 65535 || NZ > 65535 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ;
  g.KY = Y / 2 + 1;
  g.NK = sl_bins(X, Y);
  g.zc1 = NZ < 64 ? NZ : 64;
  g.nzc1 = (NZ + g.zc1 - 1) / g.zc1;
  g.cpb1 = SL_BLOCK / g.zc1;
  const long chunks = ((long)X * Y + g.cpb1 - 1) / g.cpb1;
  g.rb = (int)(chunks < SL_MEAN_ROWS ? chunks : SL_MEAN_ROWS);
  int mmax = (SL_GMAX / Y) & ~3;  // (>= 8)
  if (mmax > 64) mmax = 64;
  g.zc2 = NZ < mmax ? NZ : mmax;
  g.nzc2 = (NZ + g.zc2 - 1) / g.zc2;
  g.xb = mmax / g.zc2 < 1 ? 1 : mmax / g.zc2;
  if (g.xb > X) g.xb = X;
  g.nxb = (X + g.xb - 1) / g.xb;
  g.M = g.xb * g.zc2;
  g.MQ = (g.M + 3) / 4;
  g.zc3 = SL_BMAX / (SL_NS * g.NK);  // (>= 5: NK <= 726)
  if (g.zc3 > SL_ZC3) g.zc3 = SL_ZC3;
  if (g.zc3 > NZ) g.zc3 = NZ;
  g.nzc3 = (NZ + g.zc3 - 1) / g.zc3;
  g.kxc = SL_BLOCK / g.zc3;
  g.zc4 = NZ < SL_ZC3 ? NZ : SL_ZC3;
  g.nzc4 = (NZ + g.zc4 - 1) / g.zc4;
  g.xc4 = SL_BLOCK / g.zc4;
  int mmax5 = (SL_GMAX / (2 * g.KY)) & ~3;  // (>= 4: KY <= 513)
  if (mmax5 > 64) mmax5 = 64;
  g.zc5 = NZ < mmax5 ? NZ : mmax5;
  g.nzc5 = (NZ + g.zc5 - 1) / g.zc5;
  g.xb5 = mmax5 / g.zc5 < 1 ? 1 : mmax5 / g.zc5;
  if (g.xb5 > X) g.xb5 = X;
  g.nxb5 = (X + g.xb5 - 1) / g.xb5;
  g.M5 = g.xb5 * g.zc5;
  g.MQ5 = (g.M5 + 3) / 4;
  g.o_bins = 0;
  g.o_wx = sl_up4((int64_t)X * g.KY);
  g.o_wy = g.o_wx + sl_up4(X);
  const int64_t shared_end = g.o_wy + sl_up4(Y);
  g.o_mean = shared_end;
  g.o_a = g.o_mean + sl_up4((int64_t)B * SL_PLANES * g.rb * NZ);
  g.o_part = g.o_a + sl_up4((int64_t)B * SL_PLANES * X * g.KY * NZ * 2);
  g.total_f = g.o_part + sl_up4((int64_t)B * g.KY * g.NK * SL_NS * NZ);
  g.o_gf = shared_end;
  g.o_c = g.o_gf + sl_up4((int64_t)B * g.NK * NZ);
  g.o_mv = g.o_c + sl_up4((int64_t)B * 3 * X * g.KY * NZ * 2);
  g.o_mf = g.o_mv + sl_up4((int64_t)B * 3 * g.rb * NZ);
  g.total_b = g.o_mf + sl_up4((int64_t)B * 3 * NZ);
  return 0;
}

// sum of the squared window over the plane, in double: (sum wx^2) * (sum wy^2)
inline double sl_w2(int X, int Y, int window) {
  if (window == WSR_SPECTRUM_WINDOW_NONE) return (double)X * (double)Y;
  double s[2];
  const int n[2] = {X, Y};
  for (int a = 0; a < 2; ++a) {
    s[a] = 0.0;
    for (int i = 0; i < n[a]; ++i) {
      const double v = n[a] > 1 ? sin(M_PI * (i + 0.5) / n[a]) : 1.0;
      s[a] += (v * v) * (v * v);
    }
  }
  return s[0] * s[1];
}

}  // namespace
