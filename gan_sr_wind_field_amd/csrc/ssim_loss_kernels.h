// The backward kernel of csrc/ssim_loss.hip ([SSIM_LOSS]), in a header of its own so that a host program can run it
// block by block on threads under the address and undefined-behaviour sanitisers (tools/ssim_loss_host_check.cpp), as
// ssim_kernels.h is.  No thread leaves a kernel that has a barrier before the last barrier.
//
// The forward is ssim_tile_kernel<2> and ssim_final_kernel<2> of ssim_kernels.h.
//
// ssl_bwd_kernel: one workgroup of 512 threads per (pixel tile, z chunk, component, sample); it recomputes,
// nothing is saved by the forward.  A tile is TX x TY OUTPUT PIXELS and ZC levels.  A pixel lies in the windows of the
// win x win positions up and left of it, and a position reads the win x win pixels down and right of it, so the tile
// needs MX x MY = (TX + win - 1) x (TY + win - 1) positions and JX x JY = (TX + 2 (win - 1)) x (TY + 2 (win - 1)) pixels,
// both clipped at the plane.  LDS indices are relative to the pixel (x0 - (win - 1), y0 - (win - 1)).
//
//   stage     HR and SR of the clipped pixel range, in[f][jx][jy][z]
//   x pass    for every (position column mx, pixel row jy, z) the five sums over k of g[k] q(mx + k, jy, z),
//             q = a, s, a a, s s, a s, into mid[q][mx][jy][z]
//   y pass    for every (mx, my, z) the five sums over k of g[k] mid[q][mx][my + k][z]: the moments of the forward, then
//             l, cs and their denominators by the forward's ss_l_cs; h = G0 l + G1 and
//                 alpha = G0 cs (2 mu_a - 2 mu_s l) / D1 + h (2 mu_s cs - 2 mu_a) / D2
//                 beta  = -h cs / D2,     gamma = 2 h / D2
//             into co[3][mx][my][z]; a position outside the plane's valid range holds three zeros
//   xT pass   for every (output column tx, my, z) the three sums over i of g[i] co[.][tx + win - 1 - i][my][z], into
//             adj (which takes the place of mid)
//   yT pass   for every output pixel the three sums over j of g[j] adj[.][tx][ty + win - 1 - j][z], then
//                 dsr = A + 2 s B + a C        with a, s from the staged tile
//
// Every dsr element is written by exactly one thread: no atomics, no zero fill, the grid a function of the shape.
#pragma once

#include "ssim_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int SSL_BW_LDS_FLOATS = 20000;  // in + mid + co; with the taps 80,064 B: two workgroups per CU
constexpr int SSL_MAX_T = 32;

struct SslBwdGeom {
  int B, X, Y, NZ, win;
  int PX, PY;         // valid positions per axis
  int TX, TY, ZC;     // output pixels of a tile, levels of a chunk
  int MX, MY;         // positions around a tile: TX + win - 1, TY + win - 1
  int JX, JY;         // pixels around a tile: TX + 2 (win - 1), TY + 2 (win - 1)
  int ntx, nty, nzc;  // tiles per axis (of pixels), z chunks
  int ntxy;
};

// floats of LDS of a backward tile shape: in (2 fields), mid (5 x-pass sums; later the 3 xT-pass sums), co (3 maps)
inline long ssl_bwd_lds_floats(int TX, int TY, int ZC, int win) {
  const long MX = TX + win - 1, MY = TY + win - 1, JX = MX + win - 1, JY = MY + win - 1;
  return (2 * JX * JY + (long)ss_nq<2> * MX * JY + 3 * MX * MY) * ZC;
}

// 0: fine; the refusals of ss_geom.  The tile: of the chunks min(NZ, 16), 8, 4, 2, 1 and the (TX, TY) up to 32 x 32 (and
// the plane) that fit the LDS, the one with the largest
//     run(ZC) * NZ / (nzc ZC) * TX TY / (JX JY)
// - output pixels per staged voxel, the levels past NZ in the last chunk counted as staged, times run = min(1, ZC / 4)
// (1 when the chunk is all of NZ): a chunk below 16 contiguous bytes per column is charged for the short runs of its
// global reads and writes.  Ties to the larger chunk, the larger tile, then the larger TY.  A function of
// (X, Y, NZ, win) alone.
inline int ssl_bwd_geom(SslBwdGeom& g, int B, int X, int Y, int NZ, int win) {
  SsGeom f{};
  if (const int rc = ss_geom(f, B, X, Y, NZ, win)) return rc;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.win = win;
  g.PX = f.PX, g.PY = f.PY;
  const int mx = X < SSL_MAX_T ? X : SSL_MAX_T, my = Y < SSL_MAX_T ? Y : SSL_MAX_T;
  const int zfull = NZ < 16 ? NZ : 16;
  const int cand[5] = {zfull, 8, 4, 2, 1};
  int bx = 0, by = 0, bz = 0;
  double best = -1.0;
  for (int ci = 0; ci < 5; ++ci) {
    const int zc = cand[ci];
    if (zc > zfull || (ci > 0 && zc == zfull)) continue;
    const double run = (zc == NZ || zc >= 4) ? 1.0 : (double)zc / 4.0;
    const double zuse = run * (double)NZ / (double)(((NZ + zc - 1) / zc) * zc);
    for (int tx = 1; tx <= mx; ++tx)
      for (int ty = 1; ty <= my; ++ty) {
        if (ssl_bwd_lds_floats(tx, ty, zc, win) > SSL_BW_LDS_FLOATS) break;
        const double eff = zuse * (double)(tx * ty) / (double)((tx + 2 * (win - 1)) * (ty + 2 * (win - 1)));
        if (eff > best || (eff == best && zc == bz && (tx * ty > bx * by || (tx * ty == bx * by && ty > by))))
          best = eff, bx = tx, by = ty, bz = zc;
      }
  }
  if (bx == 0) return WSR_EUNSUPPORTED;  // (never: a 1 x 1 x 1 tile of the largest window takes 4,532 floats)
  g.TX = bx, g.TY = by, g.ZC = bz;
  g.MX = bx + win - 1, g.MY = by + win - 1;
  g.JX = g.MX + win - 1, g.JY = g.MY + win - 1;
  g.ntx = (X + bx - 1) / bx, g.nty = (Y + by - 1) / by, g.nzc = (NZ + bz - 1) / bz;
  g.ntxy = g.ntx * g.nty;
  if ((long)g.ntxy * g.nzc > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

__global__ __launch_bounds__(SS_BLOCK) void ssl_bwd_kernel(const float* __restrict__ hr, int hr_c,
                                                           const float* __restrict__ sr, int sr_c,
                                                           const double* __restrict__ gout,
                                                           const float* __restrict__ taps, float c1, float c2,
                                                           SslBwdGeom g, float* __restrict__ dsr) {
  __shared__ float lds[SSL_BW_LDS_FLOATS];
  __shared__ float gt[SS_MAX_WIN + 1];
  const int t = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int tile = (int)(blockIdx.x / (unsigned)g.nzc), zchunk = (int)(blockIdx.x - (unsigned)tile * g.nzc);
  const int tix = tile / g.nty, tiy = tile - tix * g.nty;
  const int win = g.win, ZC = g.ZC, MY = g.MY, JY = g.JY, h1 = win - 1;
  const int x0 = tix * g.TX, y0 = tiy * g.TY, z0 = zchunk * ZC;
  const int nxo = g.X - x0 < g.TX ? g.X - x0 : g.TX;  // output pixels of this tile
  const int nyo = g.Y - y0 < g.TY ? g.Y - y0 : g.TY;
  const int nz = g.NZ - z0 < ZC ? g.NZ - z0 : ZC;
  const int ox0 = x0 - h1, oy0 = y0 - h1;             // the pixel (and position) LDS index 0 stands for
  // staged pixels [plo, phi) and computed positions [plo, qhi) per axis, as LDS indices; qhi + win - 1 <= phi
  const int pxlo = ox0 < 0 ? -ox0 : 0, pylo = oy0 < 0 ? -oy0 : 0;
  const int pxhi = (x0 + nxo + h1 < g.X ? x0 + nxo + h1 : g.X) - ox0;
  const int pyhi = (y0 + nyo + h1 < g.Y ? y0 + nyo + h1 : g.Y) - oy0;
  const int qxhi = (x0 + nxo < g.PX ? x0 + nxo : g.PX) - ox0;
  const int qyhi = (y0 + nyo < g.PY ? y0 + nyo : g.PY) - oy0;
  const int vol = g.X * g.Y * g.NZ;  // (< 2^31: checked on the host)
  const int fin = g.JX * JY * ZC;    // floats of one staged field
  const int fmid = g.MX * JY * ZC;   // ... of one x-pass sum
  const int fco = g.MX * MY * ZC;    // ... of one coefficient map
  const int fadj = g.TX * MY * ZC;   // ... of one xT-pass sum (3 fadj <= 5 fmid)
  float* mid = lds + 2 * fin;
  float* co = mid + ss_nq<2> * fmid;
  float* adj = mid;

  if (t < win) gt[t] = taps[t];
  {  // ---- stage
    const float* ph = hr + ((long)b * hr_c + c) * vol;
    const float* ps = sr + ((long)b * sr_c + c) * vol;
    const int ny = pyhi - pylo, run = ny * nz, n = (pxhi - pxlo) * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int ix = e / run, r = e - ix * run;
      const int iy = r / nz, z = r - iy * nz;
      const int jx = pxlo + ix, jy = pylo + iy;
      const int src = ((ox0 + jx) * g.Y + (oy0 + jy)) * g.NZ + z0 + z;
      const int dst = (jx * JY + jy) * ZC + z;
      lds[dst] = ph[src];
      lds[fin + dst] = ps[src];
    }
  }
  __syncthreads();
  {  // ---- x pass: positions [pxlo, qxhi) x pixel rows [pylo, pyhi)
    const int ny = pyhi - pylo, run = ny * nz, n = (qxhi - pxlo) * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int ix = e / run, r = e - ix * run;
      const int iy = r / nz, z = r - iy * nz;
      const int o = ((pxlo + ix) * JY + pylo + iy) * ZC + z;
      float ma = 0.f, ms = 0.f, aa = 0.f, ss = 0.f, as = 0.f;
      for (int k = 0; k < win; ++k) {
        const int i = o + k * JY * ZC;
        const float w = gt[k], a = lds[i], s = lds[fin + i];
        ma += w * a;
        ms += w * s;
        aa += w * (a * a);
        ss += w * (s * s);
        as += w * (a * s);
      }
      mid[o] = ma;
      mid[fmid + o] = ms;
      mid[2 * fmid + o] = aa;
      mid[3 * fmid + o] = ss;
      mid[4 * fmid + o] = as;
    }
  }
  __syncthreads();
  {  // ---- y pass: the three coefficient maps on all MX x MY positions, zero outside [pxlo, qxhi) x [pylo, qyhi)
    const int run = MY * nz, n = g.MX * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int mx = e / run, r = e - mx * run;
      const int my = r / nz, z = r - my * nz;
      float al = 0.f, be = 0.f, ga = 0.f;
      if (mx >= pxlo && mx < qxhi && my >= pylo && my < qyhi) {
        const int o = (mx * JY + my) * ZC + z;
        float q[ss_nq<2>];
#pragma unroll
        for (int j = 0; j < ss_nq<2>; ++j) q[j] = 0.f;
        for (int k = 0; k < win; ++k) {
          const float w = gt[k];
          const int i = o + k * ZC;
#pragma unroll
          for (int j = 0; j < ss_nq<2>; ++j) q[j] += w * mid[j * fmid + i];
        }
        const float ma = q[0], ms = q[1];
        float l, cs, d1, d2;
        ss_l_cs(ma, ms, q[2], q[3], q[4], c1, c2, l, cs, d1, d2);
        const long gi = ((((long)b * g.NZ + z0 + z) * 3 + c) * ss_ns<2>);
        const float g0 = (float)gout[gi], g1 = (float)gout[gi + 1];
        const float h = g0 * l + g1;
        al = (g0 * cs) * (2.f * ma - (2.f * ms) * l) / d1 + h * ((2.f * ms) * cs - 2.f * ma) / d2;
        be = -(h * cs) / d2;
        ga = (2.f * h) / d2;
      }
      const int o = (mx * MY + my) * ZC + z;
      co[o] = al;
      co[fco + o] = be;
      co[2 * fco + o] = ga;
    }
  }
  __syncthreads();  // (mid is dead from here: adj takes its place)
  {  // ---- xT pass: output columns [0, nxo) x position rows [0, MY)
    const int run = MY * nz, n = nxo * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int tx = e / run, r = e - tx * run;
      const int my = r / nz, z = r - my * nz;
      const int o = ((tx + h1) * MY + my) * ZC + z;
      float A = 0.f, Bq = 0.f, C = 0.f;
      for (int i = 0; i < win; ++i) {
        const float w = gt[i];
        const int k = o - i * MY * ZC;
        A += w * co[k];
        Bq += w * co[fco + k];
        C += w * co[2 * fco + k];
      }
      const int d = (tx * MY + my) * ZC + z;
      adj[d] = A;
      adj[fadj + d] = Bq;
      adj[2 * fadj + d] = C;
    }
  }
  __syncthreads();
  {  // ---- yT pass and the combination
    float* pd = dsr + ((long)b * 3 + c) * vol;
    const int run = nyo * nz, n = nxo * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int tx = e / run, r = e - tx * run;
      const int ty = r / nz, z = r - ty * nz;
      const int o = (tx * MY + ty + h1) * ZC + z;
      float A = 0.f, Bq = 0.f, C = 0.f;
      for (int j = 0; j < win; ++j) {
        const float w = gt[j];
        const int k = o - j * ZC;
        A += w * adj[k];
        Bq += w * adj[fadj + k];
        C += w * adj[2 * fadj + k];
      }
      const int p = ((tx + h1) * JY + ty + h1) * ZC + z;
      const float a = lds[p], s = lds[fin + p];
      pd[((x0 + tx) * g.Y + (y0 + ty)) * g.NZ + z0 + z] = (A + (2.f * s) * Bq) + a * C;
    }
  }
}

}  // namespace
