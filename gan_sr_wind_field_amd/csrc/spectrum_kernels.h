// The forward spectrum pipeline of csrc/spectra.hip ([SPECTRUM]) and csrc/spectral_loss.hip ([SPECTRAL_LOSS]), kept in a
// header so that both are built from one definition and a host program can run the kernels block by block on threads
// under the address and undefined-behaviour sanitisers (tools/spectral_loss_host_check.cpp, on the shim of
// tools/host_shim.h).  Nothing here needs more of HIP than __global__, __shared__, threadIdx / blockIdx / gridDim,
// __syncthreads, float2 / float4, fmaf, sinpi and sincospi.  No thread leaves a kernel that has a barrier before the last
// barrier.  The including file turns contraction off (#pragma clang fp contract(off)) before this header.
//
// The row, column and final kernels are templates on the field count NF: 3 x NF planes (fields x components) and, per
// wavenumber bin, the NF energies and the NF - 1 co-spectra of HR with each other field when NF = 3.
//   NF = 3  wsr_level_spectra: HR, SR, TL; nine planes; e_hr, e_sr, e_tl, c_sr, c_tl
//   NF = 2  wsr_spectral_energy: HR, SR; six planes; e_hr, e_sr; the column pass also writes F_sr(b, comp, kx, ky, z),
//           complex fp32, when asked to
// A direct separable DFT: any X and Y (the raw-level domain and the tiles are no powers of two), no plan, and the 2-D
// spectrum never reaches memory.  Five launches, every grid and every workspace offset a function of the shape alone:
//
//   prep    the bin of every (kx, ky) - a double-precision guess corrected by the exact 64-bit integer test - and the
//           window factors wx, wy (double sinpi, rounded once); for the loss's backward also its gradient table
//   mean    fp32 partial sums of every plane per level in a fixed order (threads as in level_diag_kernel: column slot x
//           level, so loads along z are coalesced), SP_MEAN_ROWS rows at most; the row pass adds the rows in double
//   row     the real DFT along y of g = (f - m) * wx * wy.  A workgroup owns M = xb * zc "lines" (xb rows x, zc levels)
//           whose Y values it stages in LDS, g[j][line]; a thread owns four consecutive lines of one ky (one float4 and
//           one twiddle read per eight fmaf) and writes A(b, plane, x, ky, z), complex fp32 - the only intermediate
//   column  the complex DFT along x for all planes of a (b, ky, z chunk): thread (kx, z) holds the planes of SP_KB modes
//           in registers, A comes through LDS in slabs of SP_XT rows (the next slab on its way into registers
//           meanwhile), the products of a mode are formed in registers.  The modes of a chunk of kx are then added into
//           the workgroup's bin table in LDS in ascending kx by one thread per (sum, z): one fp32 table (NK, NS, z) per ky
//   final   adds the tables over ky in ascending order in double, with the Hermitian weight, and scales
//
// Twiddles come from a per-workgroup LDS table of cos, sin(2 pi j / n) built from double-precision sincospi and are
// indexed by (k * i) mod n, kept as a running integer: no fp32 angle is ever reduced.  The transforms accumulate with
// explicit fmaf; the products are evaluated without contraction, energy fr * fr + fi * fi and cross term
// fr_a * fr_b + fi_a * fi_b in the same order, so SR = HR gives c_sr = e_sr = e_hr bit for bit and SR = -HR their
// negatives.  No atomics, no zero fill: two calls give the same bits.
#pragma once

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_MAX_XY = WSR_SPECTRUM_MAX_XY;
constexpr int SP_MEAN_ROWS = 32;   // partial rows of the plane means, at most
constexpr int SP_GMAX = 8192;      // floats of the row passes' staged lines (32 KB)
constexpr int SP_BMAX = 7680;      // floats of the column pass' bin table (30 KB)
constexpr int SP_XT = 8;           // rows of A per LDS slab of the column pass
constexpr int SP_ZC3 = 16;         // levels per workgroup of the column passes, at most
constexpr int SP_KB = 2;           // modes kx per thread of the column pass
template <int NF> constexpr int sp_planes = 3 * NF;           // fields x components
template <int NF> constexpr int sp_ns = NF == 3 ? 5 : 2;      // sums per bin
template <int NF> constexpr int sp_pre = (sp_planes<NF> * SP_XT * SP_ZC3 + SP_BLOCK - 1) / SP_BLOCK;  // slab elements per thread
static_assert(sp_ns<3> == WSR_SPECTRUM_SUMS, "the five sums of wsr_level_spectra");

struct SpGeom {
  int B, X, Y, NZ, KY, NK;
  int zc1, nzc1, cpb1, rb;           // mean: levels per workgroup, z chunks, columns per pass, partial rows
  int zc2, nzc2, xb, nxb, M, MQ;     // row: levels and rows per workgroup, lines, quads of lines
  int zc3, nzc3, kxc;                // column: levels per workgroup, z chunks, kx per chunk
  int zc4, nzc4, xc4;                // inverse column: levels per workgroup, z chunks, x per chunk (times SL_IKB)
  int zc5, nzc5, xb5, nxb5, M5, MQ5; // inverse row: as row, with 2 KY floats per line
  int64_t o_bins, o_wx, o_wy, o_mean, o_a, o_part, total_f;  // workspace offsets of the forward, in floats
  int64_t o_gf, o_c, o_mv, o_mf, total_b;                    // ... of the backward (bins, wx, wy as in the forward)
};

struct SpFields {  // HR, SR and, with three fields, TL
  const float* p[3];
  int c[3];
};

// ---- prep: bins (X, KY) int32, wx (X), wy (Y); backward: also gf (B, NK, NZ) = (float)gbin (B, NZ, NK) -----------------
__global__ __launch_bounds__(SP_BLOCK) void sp_prep_kernel(SpGeom g, int window, int* __restrict__ bins,
                                                           float* __restrict__ wx, float* __restrict__ wy,
                                                           const double* __restrict__ gbin, float* __restrict__ gf) {
  const int X = g.X, Y = g.Y, KY = g.KY;
  const long e = (long)blockIdx.x * SP_BLOCK + threadIdx.x;
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

__device__ __forceinline__ const float* sp_plane(const SpFields& f, int p, int b, int vol) {
  const int fi = p / 3, comp = p - fi * 3;
  return f.p[fi] + ((long)b * f.c[fi] + comp) * vol;
}

// ---- mean: mpart[((b * np + p) * rb + row) * NZ + z] = the fp32 sum of plane p at level z over the columns of `row`,
// np = gridDim.y planes (9 or 6 in the forward, the 3 of dsr in the loss's backward) ------------------------------------
__global__ __launch_bounds__(SP_BLOCK) void sp_mean_kernel(SpFields f, SpGeom g, float* __restrict__ mpart) {
  __shared__ float sh[SP_BLOCK];
  const int t = threadIdx.x, p = blockIdx.y, b = blockIdx.z, np = gridDim.y;
  const int zci = blockIdx.x / g.rb, row = blockIdx.x - zci * g.rb;
  const int NZ = g.NZ, ncols = g.X * g.Y, vol = ncols * NZ;
  const int slot = t / g.zc1, zl = t - slot * g.zc1, z = zci * g.zc1 + zl;
  const float* src = sp_plane(f, p, b, vol);
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

// ---- row pass: A[(((b * PLANES + p) * X + x) * KY + ky) * NZ + z] = sum_j g(x, j, z) exp(-2 pi i ky j / Y) ----------
template <int NF>
__global__ __launch_bounds__(SP_BLOCK) void sp_row_kernel(SpFields f, SpGeom g, const float* __restrict__ mpart,
                                                          const float* __restrict__ wx, const float* __restrict__ wy,
                                                          float2* __restrict__ A) {
  constexpr int PLANES = sp_planes<NF>;
  __shared__ __attribute__((aligned(16))) float sg[SP_GMAX];
  __shared__ float2 tw[SP_MAX_XY];
  __shared__ float smean[64];
  const int t = threadIdx.x, p = blockIdx.y, b = blockIdx.z;
  const int xbi = blockIdx.x / g.nzc2, zci = blockIdx.x - xbi * g.nzc2;
  const int X = g.X, Y = g.Y, NZ = g.NZ, KY = g.KY, M = g.M, MQ = g.MQ, MP = 4 * MQ, zc = g.zc2;
  const int x0 = xbi * g.xb, z0 = zci * zc, vol = X * Y * NZ;
  const float* src = sp_plane(f, p, b, vol);
  for (int j = t; j < Y; j += SP_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)j / (double)Y, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
  }
  if (t < zc && z0 + t < NZ) {
    const float* rows = mpart + (long)(b * PLANES + p) * g.rb * NZ + z0 + t;
    double s = 0.0;
    for (int r = 0; r < g.rb; ++r) s += (double)rows[(long)r * NZ];
    smean[t] = (float)(s / ((double)X * (double)Y));
  }
  __syncthreads();
  for (int e = t; e < Y * MP; e += SP_BLOCK) {
    const int j = e / MP, m = e - j * MP;
    const int xl = m / zc, zl = m - xl * zc;
    const int x = x0 + xl, z = z0 + zl;
    float v = 0.f;
    if (m < M && x < X && z < NZ) v = (src[(x * Y + j) * NZ + z] - smean[zl]) * (wx[x] * wy[j]);
    sg[e] = v;
  }
  __syncthreads();
  const float4* sg4 = reinterpret_cast<const float4*>(sg);
  float2* dst = A + (size_t)(b * PLANES + p) * X * KY * NZ;
  for (int it = t; it < KY * MQ; it += SP_BLOCK) {
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

// ---- column pass: part[((b * KY + ky) * NK * NS + bin * NS + k) * NZ + z] = the modes (kx, ky) of the bin, ascending
// kx; saved (when not null) [(((b * 3 + comp) * X + kx) * KY + ky) * NZ + z] = F_sr -------------------------------------
// Thread (kxl, z) holds SP_KB modes, kx0 + kxl and kx0 + kxc + kxl: every value of A read from LDS feeds both.  The slab
// of A after the one being used is already on its way into registers (PRE values per thread) while the workgroup
// computes, so the latency of global memory is paid once per chunk of kx, not once per slab.
template <int NF>
__global__ __launch_bounds__(SP_BLOCK) void sp_col_kernel(SpGeom g, const int* __restrict__ bins,
                                                          const float2* __restrict__ A, float* __restrict__ part,
                                                          float2* __restrict__ saved) {
  constexpr int PLANES = sp_planes<NF>, NS = sp_ns<NF>, PRE = sp_pre<NF>;
  __shared__ float2 tw[SP_MAX_XY];
  __shared__ int sbin[SP_MAX_XY];
  __shared__ float2 sA[PLANES * SP_XT * SP_ZC3];
  __shared__ float prod[SP_KB * SP_BLOCK * NS];
  __shared__ float binsum[SP_BMAX];
  const int t = threadIdx.x, ky = blockIdx.y, b = blockIdx.z;
  const int X = g.X, NZ = g.NZ, KY = g.KY, NK = g.NK, zc = g.zc3, kxc = g.kxc;
  const int z0 = blockIdx.x * zc;
  const int kxl = t / zc, zl = t - kxl * zc;
  const bool live = kxl < kxc;
  for (int i = t; i < X; i += SP_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)i / (double)X, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
    sbin[i] = bins[i * KY + ky];
  }
  for (int e = t; e < NK * NS * zc; e += SP_BLOCK) binsum[e] = 0.f;
  const int slab = SP_XT * zc;
  // the thread's PRE elements of a slab: element e = t + i * 256 -> (plane, row of the slab, level)
  const float2* src[PRE];
  int sxl[PRE];  // the row of the slab, or X: never loaded (past the slab, or a level past NZ)
#pragma unroll
  for (int i = 0; i < PRE; ++i) {
    const int e = t + i * SP_BLOCK;
    const int p = e / slab, r = e - p * slab;
    const int xl = r / zc, zz = r - xl * zc;
    const bool ok = e < PLANES * slab && z0 + zz < NZ;
    sxl[i] = ok ? xl : X;
    src[i] = A + ((size_t)(b * PLANES + (ok ? p : 0)) * X * KY + ky) * NZ + (ok ? z0 + zz : 0);
  }
  const size_t xstride = (size_t)KY * NZ;
  for (int kx0 = 0; kx0 < X; kx0 += SP_KB * kxc) {
    int kx[SP_KB], idx[SP_KB];
    float fr[SP_KB][PLANES], fi[SP_KB][PLANES];
#pragma unroll
    for (int r = 0; r < SP_KB; ++r) {  // (a thread past the end repeats the last mode, not deposited)
      kx[r] = kx0 + r * kxc + kxl < X ? kx0 + r * kxc + kxl : X - 1;
      idx[r] = 0;
#pragma unroll
      for (int p = 0; p < PLANES; ++p) fr[r][p] = 0.f, fi[r][p] = 0.f;
    }
    float2 pre[PRE];
#pragma unroll
    for (int i = 0; i < PRE; ++i) pre[i] = sxl[i] < X ? src[i][(size_t)sxl[i] * xstride] : make_float2(0.f, 0.f);
    for (int xt0 = 0; xt0 < X; xt0 += SP_XT) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < PRE; ++i)
        if (t + i * SP_BLOCK < PLANES * slab) sA[t + i * SP_BLOCK] = pre[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < PRE; ++i) {  // the next slab: in flight during the loop below
        const int x = xt0 + SP_XT + sxl[i];
        pre[i] = x < X ? src[i][(size_t)x * xstride] : make_float2(0.f, 0.f);
      }
      const int nx = X - xt0 < SP_XT ? X - xt0 : SP_XT;
      if (live)
        for (int xl = 0; xl < nx; ++xl) {
          float2 w[SP_KB];
#pragma unroll
          for (int r = 0; r < SP_KB; ++r) w[r] = tw[idx[r]];
#pragma unroll
          for (int p = 0; p < PLANES; ++p) {  // a * (c - i s)
            const float2 a = sA[p * slab + xl * zc + zl];
#pragma unroll
            for (int r = 0; r < SP_KB; ++r) {
              fr[r][p] = fmaf(a.x, w[r].x, fr[r][p]);
              fr[r][p] = fmaf(a.y, w[r].y, fr[r][p]);
              fi[r][p] = fmaf(a.y, w[r].x, fi[r][p]);
              fi[r][p] = fmaf(-a.x, w[r].y, fi[r][p]);
            }
          }
#pragma unroll
          for (int r = 0; r < SP_KB; ++r) {
            idx[r] += kx[r];
            if (idx[r] >= X) idx[r] -= X;
          }
        }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < SP_KB; ++r) {
        const float* cr = fr[r];
        const float* ci = fi[r];
        float P[NS];
#pragma unroll
        for (int a = 0; a < NF; ++a) {  // e_hr, e_sr(, e_tl): the same expression
          const int o = 3 * a;
          P[a] = ((cr[o] * cr[o] + ci[o] * ci[o]) + (cr[o + 1] * cr[o + 1] + ci[o + 1] * ci[o + 1])) +
                 (cr[o + 2] * cr[o + 2] + ci[o + 2] * ci[o + 2]);
        }
        if constexpr (NF == 3) {
#pragma unroll
          for (int a = 1; a < 3; ++a) {  // c_sr, c_tl: the same expression with one factor from HR
            const int o = 3 * a;
            P[2 + a] = ((cr[0] * cr[o] + ci[0] * ci[o]) + (cr[1] * cr[o + 1] + ci[1] * ci[o + 1])) +
                       (cr[2] * cr[o + 2] + ci[2] * ci[o + 2]);
          }
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) prod[((r * kxc + kxl) * NS + q) * zc + zl] = P[q];
        const int kxr = kx0 + r * kxc + kxl;
        if (saved && kxr < X && z0 + zl < NZ) {
#pragma unroll
          for (int comp = 0; comp < 3; ++comp)
            saved[(((size_t)(b * 3 + comp) * X + kxr) * KY + ky) * NZ + z0 + zl] = make_float2(cr[3 + comp], ci[3 + comp]);
        }
      }
    }
    __syncthreads();
    if (t < NS * zc) {  // thread (sum q, level): the modes of this chunk in ascending kx, a run of one bin in a register
      const int q = t / zc, zz = t - q * zc;
      const int n = X - kx0 < SP_KB * kxc ? X - kx0 : SP_KB * kxc;
      int cur = sbin[kx0];
      float acc = binsum[(cur * NS + q) * zc + zz];
      for (int l = 0; l < n; ++l) {
        const int bin = sbin[kx0 + l];
        const float v = prod[(l * NS + q) * zc + zz];
        if (bin != cur) {
          binsum[(cur * NS + q) * zc + zz] = acc;
          cur = bin;
          acc = binsum[(cur * NS + q) * zc + zz];
        }
        acc += v;
      }
      binsum[(cur * NS + q) * zc + zz] = acc;
    }
  }
  __syncthreads();
  float* dst = part + (size_t)(b * KY + ky) * NK * NS * NZ;
  for (int e = t; e < NK * NS * zc; e += SP_BLOCK) {
    const int r = e / zc, zz = e - r * zc;
    if (z0 + zz < NZ) dst[(size_t)r * NZ + z0 + zz] = binsum[e];
  }
}

// ---- final: out[((b * NZ + z) * NK + bin) * NS + k] = scale * sum_ky h(ky) part[b][ky][bin][k][z], ascending, double ---
template <int NF>
__global__ __launch_bounds__(SP_BLOCK) void sp_final_kernel(SpGeom g, const float* __restrict__ part, double scale,
                                                            double* __restrict__ out) {
  constexpr int NS = sp_ns<NF>;
  const int b = blockIdx.y, items = g.NK * NS * g.NZ;
  const int e = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (e >= items) return;
  const int r = e / g.NZ, z = e - r * g.NZ;
  const float* src = part + (size_t)b * g.KY * items + e;
  double s = 0.0;
  for (int ky = 0; ky < g.KY; ++ky) {
    const double h = (ky == 0 || 2 * ky == g.Y) ? 1.0 : 2.0;
    s += h * (double)src[(size_t)ky * items];
  }
  out[((size_t)b * g.NZ + z) * g.NK * NS + r] = s * scale;
}

// ---- host side: the geometry of every pass and the workspace offsets, functions of the shape alone ---------------------
// floor(N / sqrt(2) + 1/2) + 1 in integers (wsr_level_spectra_bins): the largest k with (2k - 1)^2 <= 2 N^2, plus one
inline int sp_bins(int X, int Y) {
  const long N = X > Y ? X : Y;
  long k = (long)floor((double)N / sqrt(2.0) + 0.5);
  while (k > 0 && (2 * k - 1) * (2 * k - 1) > 2 * N * N) --k;
  while ((2 * k + 1) * (2 * k + 1) <= 2 * N * N) ++k;
  return (int)k + 1;
}

inline int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_spectra and wsr_spectral_energy document them.  nf: the field count;
// the passes of the loss's backward (zc4 .. MQ5, o_gf .. total_b) do not depend on it.
inline int sp_geom(SpGeom& g, int nf, int B, int X, int Y, int NZ) {
  const int planes = 3 * nf, ns = nf == 3 ? sp_ns<3> : sp_ns<2>;
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (X > SP_MAX_XY || Y > SP_MAX_XY || B > 65535 || NZ > 65535 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ;
  g.KY = Y / 2 + 1;
  g.NK = sp_bins(X, Y);
  g.zc1 = NZ < 64 ? NZ : 64;
  g.nzc1 = (NZ + g.zc1 - 1) / g.zc1;
  g.cpb1 = SP_BLOCK / g.zc1;
  const long chunks = ((long)X * Y + g.cpb1 - 1) / g.cpb1;
  g.rb = (int)(chunks < SP_MEAN_ROWS ? chunks : SP_MEAN_ROWS);
  int mmax = (SP_GMAX / Y) & ~3;  // (>= 8)
  if (mmax > 64) mmax = 64;
  g.zc2 = NZ < mmax ? NZ : mmax;
  g.nzc2 = (NZ + g.zc2 - 1) / g.zc2;
  g.xb = mmax / g.zc2 < 1 ? 1 : mmax / g.zc2;
  if (g.xb > X) g.xb = X;
  g.nxb = (X + g.xb - 1) / g.xb;
  g.M = g.xb * g.zc2;
  g.MQ = (g.M + 3) / 4;
  g.zc3 = SP_BMAX / (ns * g.NK);  // (>= 2: NK <= 726)
  if (g.zc3 > SP_ZC3) g.zc3 = SP_ZC3;
  if (g.zc3 > NZ) g.zc3 = NZ;
  g.nzc3 = (NZ + g.zc3 - 1) / g.zc3;
  g.kxc = SP_BLOCK / g.zc3;
  g.zc4 = NZ < SP_ZC3 ? NZ : SP_ZC3;
  g.nzc4 = (NZ + g.zc4 - 1) / g.zc4;
  g.xc4 = SP_BLOCK / g.zc4;
  int mmax5 = (SP_GMAX / (2 * g.KY)) & ~3;  // (>= 4: KY <= 513)
  if (mmax5 > 64) mmax5 = 64;
  g.zc5 = NZ < mmax5 ? NZ : mmax5;
  g.nzc5 = (NZ + g.zc5 - 1) / g.zc5;
  g.xb5 = mmax5 / g.zc5 < 1 ? 1 : mmax5 / g.zc5;
  if (g.xb5 > X) g.xb5 = X;
  g.nxb5 = (X + g.xb5 - 1) / g.xb5;
  g.M5 = g.xb5 * g.zc5;
  g.MQ5 = (g.M5 + 3) / 4;
  g.o_bins = 0;
  g.o_wx = up4((int64_t)X * g.KY);
  g.o_wy = g.o_wx + up4(X);
  const int64_t shared_end = g.o_wy + up4(Y);
  g.o_mean = shared_end;
  g.o_a = g.o_mean + up4((int64_t)B * planes * g.rb * NZ);
  g.o_part = g.o_a + up4((int64_t)B * planes * X * g.KY * NZ * 2);
  g.total_f = g.o_part + up4((int64_t)B * g.KY * g.NK * ns * NZ);
  g.o_gf = shared_end;
  g.o_c = g.o_gf + up4((int64_t)B * g.NK * NZ);
  g.o_mv = g.o_c + up4((int64_t)B * 3 * X * g.KY * NZ * 2);
  g.o_mf = g.o_mv + up4((int64_t)B * 3 * g.rb * NZ);
  g.total_b = g.o_mf + up4((int64_t)B * 3 * NZ);
  return 0;
}

// sum of the squared window over the plane, in double: (sum wx^2) * (sum wy^2)
inline double sp_w2(int X, int Y, int window) {
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
