// The backward kernels of csrc/spectral_loss.hip ([SPECTRAL_LOSS]), kept in a header of their own so that a host program
// can run them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/spectral_loss_host_check.cpp).  Nothing here needs more of HIP than spectrum_kernels.h does.  No thread leaves a
// kernel that has a barrier before the last barrier.
//
// The forward is the pipeline of spectrum_kernels.h with two fields; its column pass writes F_sr(b, comp, kx, ky, z),
// complex fp32, when asked to.  The backward is the adjoint, on the geometry sp_geom fills for it:
//
//   prep    bins and window as in the forward, and gbin (B, NZ, NK) double rounded ONCE to fp32 and laid out (B, NK, NZ)
//   icol    C(x, ky) = sum_kx G(bin(kx, ky)) F_sr(kx, ky) exp(+2 pi i kx x / X) per (b, comp, ky, chunk of <= 16 levels):
//           thread (x, z) holds SL_IKB values of x, G F comes through LDS in slabs of SL_IXT rows kx
//   irow    u(x, y) = sum_ky h Re(C exp(+2 pi i ky y / Y)), v = 2 scale wx wy u.  A workgroup owns M lines (rows x levels)
//           whose KY values h C it stages in LDS, re and im rows apart; a thread owns four consecutive lines of one y (two
//           float4 and one twiddle per eight fmaf) and writes v into dsr
//   mean    the plane sums of v (the forward's mean kernel on the three planes of dsr), mfin adds the partial rows in
//           double
//   sub     dsr -= mean_plane(v): the adjoint of the detrend
#pragma once

#include "spectrum_kernels.h"

namespace {

constexpr int SL_IXT = 64;         // rows kx of G F per LDS slab of the inverse column pass
constexpr int SL_IKB = 4;          // values of x per thread of the inverse column pass
constexpr int SL_IPRE = SL_IXT * SP_ZC3 / SP_BLOCK;

// ---- inverse column pass: Cw[(((b * 3 + comp) * X + x) * KY + ky) * NZ + z] = sum_kx gf(b, bin(kx, ky), z) F(kx, ky, z)
// exp(+2 pi i kx x / X), ascending kx.  The slab after the one in use is on its way into registers meanwhile. ----------
__global__ __launch_bounds__(SP_BLOCK) void sl_icol_kernel(SpGeom g, const int* __restrict__ bins,
                                                           const float* __restrict__ gf, const float2* __restrict__ F,
                                                           float2* __restrict__ Cw) {
  __shared__ float2 tw[SP_MAX_XY];
  __shared__ int sbin[SP_MAX_XY];
  __shared__ float2 sF[SL_IXT * SP_ZC3];
  const int t = threadIdx.x, ky = blockIdx.y, b = blockIdx.z;
  const int zci = blockIdx.x / 3, bp = b * 3 + (blockIdx.x - zci * 3);  // (the component: the fastest grid index)
  const int X = g.X, NZ = g.NZ, KY = g.KY, NK = g.NK, zc = g.zc4, xc = g.xc4;
  const int z0 = zci * zc;
  const int xl = t / zc, zl = t - xl * zc;
  const bool live = xl < xc;
  for (int i = t; i < X; i += SP_BLOCK) {
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
    const int e = t + i * SP_BLOCK;
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
        if (t + i * SP_BLOCK < slab) sF[t + i * SP_BLOCK] = pre[i];
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
__global__ __launch_bounds__(SP_BLOCK) void sl_irow_kernel(SpGeom g, const float2* __restrict__ Cw,
                                                           const float* __restrict__ wx, const float* __restrict__ wy,
                                                           float s2, float* __restrict__ dsr) {
  __shared__ __attribute__((aligned(16))) float sc[SP_GMAX];
  __shared__ float2 tw[SP_MAX_XY];
  const int t = threadIdx.x;
  const int comp = blockIdx.y, b = blockIdx.z, plane = b * 3 + comp;
  const int xbi = blockIdx.x / g.nzc5, zci = blockIdx.x - xbi * g.nzc5;
  const int X = g.X, Y = g.Y, NZ = g.NZ, KY = g.KY, M = g.M5, MQ = g.MQ5, MP = 4 * MQ, zc = g.zc5;
  const int x0 = xbi * g.xb5, z0 = zci * zc;
  for (int j = t; j < Y; j += SP_BLOCK) {
    double s, c;
    sincospi(2.0 * (double)j / (double)Y, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
  }
  const float2* src = Cw + (size_t)plane * X * KY * NZ;
  for (int e = t; e < KY * MP; e += SP_BLOCK) {
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
  for (int it = t; it < Y * MQ; it += SP_BLOCK) {
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
__global__ __launch_bounds__(SP_BLOCK) void sl_mfin_kernel(SpGeom g, const float* __restrict__ mpart,
                                                           float* __restrict__ mfin) {
  const long e = (long)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (e >= (long)g.B * 3 * g.NZ) return;
  const long plane = e / g.NZ;
  const int z = (int)(e - plane * g.NZ);
  const float* rows = mpart + plane * g.rb * g.NZ + z;
  double s = 0.0;
  for (int r = 0; r < g.rb; ++r) s += (double)rows[(long)r * g.NZ];
  mfin[e] = (float)(s / ((double)g.X * (double)g.Y));
}

// ---- sub: dsr(plane, col, z) -= mfin(plane, z); blockIdx.y the component, blockIdx.z the sample -----------------------
__global__ __launch_bounds__(SP_BLOCK) void sl_sub_kernel(SpGeom g, const float* __restrict__ mfin,
                                                          float* __restrict__ dsr) {
  const long vol = (long)g.X * g.Y * g.NZ;
  const long e = (long)blockIdx.x * SP_BLOCK + threadIdx.x;
  if (e >= vol) return;
  const long plane = (long)blockIdx.z * 3 + blockIdx.y;
  const int z = (int)(e % g.NZ);
  dsr[plane * vol + e] -= mfin[plane * g.NZ + z];
}

}  // namespace
