// The forward SSIM kernels ([SSIM], [SSIM_LOSS]), kept in a header of their own so that a host program can run them block
// by block on threads under the address and undefined-behaviour sanitisers (tools/ssim_host_check.cpp and
// tools/ssim_loss_host_check.cpp, on the shim of tools/host_shim.h: __global__, __shared__, threadIdx / blockIdx and
// __syncthreads).  Nothing here needs more of HIP than those.  No thread leaves a kernel that has a barrier before the
// last barrier.
//
// Both kernels are templates on the field count NF.  NF = 3 (csrc/ssim.hip) takes HR, SR and TL: eight window sums and
// four results per position, ssim_sr, cs_sr, ssim_tl, cs_tl.  NF = 2 (csrc/ssim_loss.hip) takes HR and SR: five window
// sums and the first two results; the TL field, its three moments and its two results are compiled out.  Both run on the
// tile geometry of ss_geom, which is sized for three fields, so a workgroup of either covers the same positions and the
// two results of NF = 2 carry the bits of the first two of NF = 3.
//
// ssim_tile_kernel: one workgroup of 512 threads per (tile, component, sample).  A tile is TX x TY valid positions and
// ZC consecutive levels; with the win - 1 halo it reads IX x IY = (TX + win - 1) x (TY + win - 1) columns.
//
//   stage    the tiles of the fields into LDS, in[f][ix][iy][z]; the loop runs over (ix, iy, z) with z fastest, so a
//            wave reads runs of the chunk's levels - and, when the chunk is all of NZ, the whole (y, z) run of a row of
//            the tile, which is contiguous in memory
//   x pass   for every (ox, iy, z) of the tile the sums over k of g[k] q(ox + k, iy, z), q = the fields, their squares
//            and HR times each other field (HR's two shared by the SR and the TL pair), into LDS, mid[q][ox][iy][z]
//   y pass   thread (slot, z) walks the positions slot, slot + nslots, ... of the tile: the sums over k of
//            g[k] mid[q][ox][oy + k][z] in registers, then l, cs and l cs of every pair, added to its fp32 sums
//   reduce   the slots of a level are added through LDS in slot order: ONE partial row of ZC x NS floats per workgroup
//
// ssim_final_kernel adds the partial rows of a (sample, component, z chunk) in a fixed order in double.  No atomics, no
// zero fill, the grid a function of the shape alone: two calls give the same bits.  Everything is evaluated without
// contraction, products before sums, taps ascending; every pair goes through ss_l_cs with HR first (mu_s like mu_a, S_ss
// and S_as like S_aa), so with SR bit-equal to HR numerator and denominator of l and of cs hold the same bits, both
// quotients are 1.0f and every ssim_sr and cs_sr sum is exactly npos.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int SS_BLOCK = 512;
template <int NF> constexpr int ss_ns = NF == 3 ? 4 : 2;  // results per position: ssim_sr, cs_sr(, ssim_tl, cs_tl)
template <int NF> constexpr int ss_nq = NF == 3 ? 8 : 5;  // windowed quantities per position
static_assert(ss_ns<3> == WSR_SSIM_SUMS, "the four sums of wsr_level_ssim");
constexpr int SS_MAX_WIN = WSR_SSIM_MAX_WIN;
constexpr int SS_MAX_NZ = 256;
constexpr int SS_LDS_FLOATS = 18400;          // in + mid; with 8 KiB of sums and the taps 81,856 B: two workgroups per CU
constexpr int SS_MAX_T = 32;                  // positions per tile and axis, at most
constexpr int SS_FBLOCK = 256, SS_FWAVES = SS_FBLOCK / 64;

struct SsGeom {
  int B, X, Y, NZ, win;
  int PX, PY;         // valid positions per axis
  int TX, TY, ZC;     // tile
  int IX, IY;         // TX + win - 1, TY + win - 1
  int ntx, nty, nzc;  // tiles per axis, z chunks
  int ntxy;           // ntx * nty
  int nslots;         // SS_BLOCK / ZC
};

// floats of LDS of a tile shape, with three fields
inline long ss_lds_floats(int TX, int TY, int ZC, int win) {
  const long IX = TX + win - 1, IY = TY + win - 1;
  return 3 * IX * IY * ZC + (long)ss_nq<3> * TX * IY * ZC;
}

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_ssim documents them.  The tile: a chunk of min(NZ, 16) levels or
// of 8 (4, 2, 1 only if neither fits); of the (TX, TY, ZC) that fit the LDS the one with the most valid positions per
// staged voxel, the levels past NZ in the last chunk counted as staged; ties to the larger chunk, the larger tile, then
// the larger TY.  A function of (X, Y, NZ, win) alone.
inline int ss_geom(SsGeom& g, int B, int X, int Y, int NZ, int win) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (win < 3 || win > SS_MAX_WIN || (win & 1) == 0 || X < win || Y < win) return WSR_EINVAL;
  if (NZ > SS_MAX_NZ || B > 65535 || X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.win = win;
  g.PX = X - win + 1, g.PY = Y - win + 1;
  const int mx = g.PX < SS_MAX_T ? g.PX : SS_MAX_T, my = g.PY < SS_MAX_T ? g.PY : SS_MAX_T;
  const int zfull = NZ < 16 ? NZ : 16;
  const int cand[5] = {zfull, 8, 4, 2, 1};
  int bx = 0, by = 0, bz = 0;
  double best = -1.0;
  for (int ci = 0; ci < 5; ++ci) {
    const int zc = cand[ci];
    if (zc > zfull || (ci > 0 && zc == zfull) || (ci > 1 && bx != 0)) continue;
    const double zuse = (double)NZ / (double)(((NZ + zc - 1) / zc) * zc);
    for (int tx = 1; tx <= mx; ++tx)
      for (int ty = 1; ty <= my; ++ty) {
        if (ss_lds_floats(tx, ty, zc, win) > SS_LDS_FLOATS) break;
        const double eff = zuse * (double)(tx * ty) / (double)((tx + win - 1) * (ty + win - 1));
        if (eff > best || (eff == best && zc == bz && (tx * ty > bx * by || (tx * ty == bx * by && ty > by))))
          best = eff, bx = tx, by = ty, bz = zc;
      }
  }
  if (bx == 0) return WSR_EUNSUPPORTED;  // (never: a 1 x 1 x 1 tile of the largest window takes 795 floats)
  g.TX = bx, g.TY = by, g.ZC = bz;
  g.IX = bx + win - 1, g.IY = by + win - 1;
  g.ntx = (g.PX + bx - 1) / bx, g.nty = (g.PY + by - 1) / by, g.nzc = (NZ + bz - 1) / bz;
  g.ntxy = g.ntx * g.nty;
  g.nslots = SS_BLOCK / bz;
  if ((long)g.ntxy * g.nzc > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

// floats of the partial rows: part[((b * 3 + c) * nzc + zchunk) * ntxy + tile][z][NS]
template <int NF> inline long ss_workspace_floats(const SsGeom& g) {
  return (long)g.B * 3 * g.nzc * g.ntxy * g.ZC * ss_ns<NF>;
}

// l, cs and their denominators d1, d2 of the pair (a, s) from the five window sums of a position: the means ma, ms and
// the second moments aa, ss, as.  The one operation sequence of the forward of both field counts and of the backward.
__device__ __forceinline__ void ss_l_cs(float ma, float ms, float aa, float ss, float as, float c1, float c2, float& l,
                                        float& cs, float& d1, float& d2) {
  const float maa = ma * ma, mss = ms * ms, mas = ma * ms;
  const float va = aa - maa, vs = ss - mss, cv = as - mas;
  d1 = (maa + mss) + c1;
  d2 = (va + vs) + c2;
  l = (2.f * mas + c1) / d1;
  cs = (2.f * cv + c2) / d2;
}

// tl, tl_c: read with NF = 3 only
template <int NF>
__global__ __launch_bounds__(SS_BLOCK) void ssim_tile_kernel(const float* __restrict__ hr, int hr_c,
                                                             const float* __restrict__ sr, int sr_c,
                                                             const float* __restrict__ tl, int tl_c,
                                                             const float* __restrict__ taps,
                                                             float c1, float c2, SsGeom g, float* __restrict__ part) {
  constexpr int NS = ss_ns<NF>, NQ = ss_nq<NF>;
  // mid[q]: the means of the fields, their second moments, then HR times SR (and HR times TL)
  constexpr int Q_MA = 0, Q_MS = 1, Q_MT = 2, Q_AA = NF, Q_SS = NF + 1, Q_TT = NF + 2, Q_AS = 2 * NF, Q_AT = 2 * NF + 1;
  __shared__ float lds[SS_LDS_FLOATS];
  __shared__ float sums[NS][SS_BLOCK];
  __shared__ float gt[SS_MAX_WIN + 1];
  const int t = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int tile = (int)(blockIdx.x / (unsigned)g.nzc), zchunk = (int)(blockIdx.x - (unsigned)tile * g.nzc);
  const int tx = tile / g.nty, ty = tile - tx * g.nty;
  const int win = g.win, ZC = g.ZC, IY = g.IY;
  const int x0 = tx * g.TX, y0 = ty * g.TY, z0 = zchunk * ZC;
  const int nxo = g.PX - x0 < g.TX ? g.PX - x0 : g.TX;  // valid positions of this tile
  const int nyo = g.PY - y0 < g.TY ? g.PY - y0 : g.TY;
  const int nz = g.NZ - z0 < ZC ? g.NZ - z0 : ZC;
  const int nxi = nxo + win - 1, nyi = nyo + win - 1;   // columns it reads: x0 + nxi <= X, y0 + nyi <= Y
  const int vol = g.X * g.Y * g.NZ;                     // (< 2^31: checked on the host)
  const int fin = g.IX * IY * ZC;                       // floats of one staged field
  float* mid = lds + NF * fin;
  const int fmid = g.TX * IY * ZC;

  if (t < win) gt[t] = taps[t];
  {  // ---- stage
    const float* ph = hr + ((long)b * hr_c + c) * vol;
    const float* ps = sr + ((long)b * sr_c + c) * vol;
    const int run = nyi * nz, n = nxi * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int ix = e / run, r = e - ix * run;
      const int iy = r / nz, z = r - iy * nz;
      const int src = ((x0 + ix) * g.Y + (y0 + iy)) * g.NZ + z0 + z;
      const int dst = (ix * IY + iy) * ZC + z;
      lds[dst] = ph[src];
      lds[fin + dst] = ps[src];
      if constexpr (NF == 3) lds[2 * fin + dst] = (tl + ((long)b * tl_c + c) * vol)[src];
    }
  }
  __syncthreads();
  {  // ---- x pass
    const int run = nyi * nz, n = nxo * run;
    for (int e = t; e < n; e += SS_BLOCK) {
      const int ox = e / run, r = e - ox * run;
      const int iy = r / nz, z = r - iy * nz;
      const int o = (ox * IY + iy) * ZC + z;
      float m[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) m[j] = 0.f;
      for (int k = 0; k < win; ++k) {
        const int i = o + k * IY * ZC;
        const float w = gt[k], a = lds[i], s = lds[fin + i];
        m[Q_MA] += w * a;
        m[Q_MS] += w * s;
        m[Q_AA] += w * (a * a);
        m[Q_SS] += w * (s * s);
        m[Q_AS] += w * (a * s);
        if constexpr (NF == 3) {
          const float u = lds[2 * fin + i];
          m[Q_MT] += w * u;
          m[Q_TT] += w * (u * u);
          m[Q_AT] += w * (a * u);
        }
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) mid[j * fmid + o] = m[j];
    }
  }
  __syncthreads();
  float acc[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j] = 0.f;
  const int slot = t / ZC, z = t - slot * ZC;
  if (slot < g.nslots && z < nz) {  // ---- y pass
    const int npos = nxo * nyo;
    for (int p = slot; p < npos; p += g.nslots) {
      const int ox = p / nyo, oy = p - ox * nyo;
      const int o = (ox * IY + oy) * ZC + z;
      float q[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) q[j] = 0.f;
      for (int k = 0; k < win; ++k) {
        const float w = gt[k];
        const int i = o + k * ZC;
#pragma unroll
        for (int j = 0; j < NQ; ++j) q[j] += w * mid[j * fmid + i];
      }
      float l, cs, d1, d2;
      ss_l_cs(q[Q_MA], q[Q_MS], q[Q_AA], q[Q_SS], q[Q_AS], c1, c2, l, cs, d1, d2);
      acc[0] += l * cs;
      acc[1] += cs;
      if constexpr (NF == 3) {
        ss_l_cs(q[Q_MA], q[Q_MT], q[Q_AA], q[Q_TT], q[Q_AT], c1, c2, l, cs, d1, d2);
        acc[2] += l * cs;
        acc[3] += cs;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) sums[j][t] = acc[j];
  __syncthreads();
  // ---- reduce: item (level, sum) over the slots in order
  float* row = part + ((((long)b * 3 + c) * g.nzc + zchunk) * g.ntxy + tile) * (ZC * NS);
  for (int item = t; item < nz * NS; item += SS_BLOCK) {
    const int lvl = item / NS, j = item - lvl * NS;
    float s = sums[j][lvl];
    for (int sl = 1; sl < g.nslots; ++sl) s += sums[j][sl * ZC + lvl];
    row[item] = s;
  }
}

// out[b][z][c][j] = the ntxy partial rows of (b, c, z chunk) in double: 64 (level, sum) items per workgroup of 4 waves,
// wave w adds rows w, w + 4, ... in order, the four wave sums are then added in order
template <int NF>
__global__ __launch_bounds__(SS_FBLOCK) void ssim_final_kernel(const float* __restrict__ part, SsGeom g,
                                                               double* __restrict__ out) {
  constexpr int NS = ss_ns<NF>;
  __shared__ double sh[SS_FWAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y % 3, zchunk = blockIdx.y / 3, b = blockIdx.z;
  const int item = blockIdx.x * 64 + lane;
  const int z0 = zchunk * g.ZC;
  const int nz = g.NZ - z0 < g.ZC ? g.NZ - z0 : g.ZC;
  const int stride = g.ZC * NS;
  const float* rows = part + (((long)b * 3 + c) * g.nzc + zchunk) * g.ntxy * stride;
  const bool live = item < nz * NS;
  double s = 0.0;
  if (live)
    for (int r = wave; r < g.ntxy; r += SS_FWAVES) s += (double)rows[(long)r * stride + item];
  sh[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && live) {
    double a = sh[0][lane];
#pragma unroll
    for (int w = 1; w < SS_FWAVES; ++w) a += sh[w][lane];
    const int lvl = item / NS, j = item - lvl * NS;
    out[(((long)b * g.NZ + z0 + lvl) * 3 + c) * NS + j] = a;
  }
}

}  // namespace
