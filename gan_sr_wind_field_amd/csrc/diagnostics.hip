// Per-level evaluation diagnostics ([DIAGNOSTICS]): 15 sums per z level of one sample over its X * Y columns, from ONE
// pass over HR, SR, the trilinear baseline TL and the raw altitude zc.  All tensors fp32 planar (B, C, X, Y, NZ), z
// innermost; only channels 0..2 of the three fields are read.
//
//   k = 0        ||HR||
//   1, 2         ||HR - SR||, ||HR - TL||
//   3, 4         ||SR|| - ||HR||, ||TL|| - ||HR||          (signed speed bias)
//   5, 6         | ||SR|| - ||HR|| |, | ||TL|| - ||HR|| |
//   7            h = sqrt(HR_u^2 + HR_v^2)
//   8, 9         h * theta(HR, SR), h * theta(HR, TL)      theta(a, b) = atan2f(|a_u b_v - a_v b_u|, a_u b_u + a_v b_v),
//                                                          0 when both arguments are 0
//   10, 11, 12   div(HR)^2, div(SR)^2, div(TL)^2           div = du/dx + dv/dy + dw/dz with deriv_row (stencil.h), as
//                                                          physics_stats_kernel forms div3
//   13, 14       zc, zc - zc at level 0 of the same column
//
// Threads as in column_interp_kernel: the 256 threads of a workgroup own cpb = floor(256 / NZ) consecutive columns x NZ
// levels, thread t = (column slot t / NZ, level t % NZ), so every load along z is coalesced; the x and y neighbours of
// the divergence come from global memory (the same lines a neighbouring workgroup reads: L2).  A workgroup strides over
// its column chunks and accumulates in fp32 at its fixed (column slot, level); the column slots of a level are then
// added through LDS in slot order: ONE partial row of NZ x 15 floats per workgroup.  A second kernel adds the rows of a
// sample in a fixed order in double.  No atomics, no zero fill: two calls give the same bits.  Everything is evaluated
// without contraction (a x b - b x a is exactly 0, the same field gives the same divergence bits).
#include "common.h"
#pragma clang fp contract(off)
#include "stencil.h"

namespace {

constexpr int LD_BLOCK = 256;
constexpr int LD_NS = WSR_LEVEL_DIAG_SUMS;
constexpr int LD_MAX_ROWS = WSR_LEVEL_DIAG_MAX_ROWS;

struct LdGeom {
  int X, Y, NZ;
  int cpb;      // columns per workgroup pass
  long ncols;   // X * Y
  long nchunks; // ceil(ncols / cpb)
};

// the coordinates deriv_row asks for at row i - c[i-1], c[i], c[i+1] - read beforehand, so that no load waits inside
// one of its branches (the index is clamped at the ends, where deriv_row does not ask for that neighbour)
struct Loc3 {
  float cm, c0, cp;
  int i;
  __device__ float operator()(int j) const { return j < i ? cm : (j > i ? cp : c0); }
};
__device__ __forceinline__ Loc3 load_loc3(const float* __restrict__ c, int i, int n) {
  return Loc3{c[i > 0 ? i - 1 : 0], c[i], c[i < n - 1 ? i + 1 : i], i};
}

// one field at a voxel: its value and the six neighbours of its divergence.  Every neighbour is loaded unconditionally
// from a clamped (in-bounds) offset and selected afterwards, so all loads of a voxel are in flight together.
struct Raw { float u, v, w, ulo, uhi, vlo, vhi, wlo, whi; };
struct Offs { int xlo, xhi, ylo, yhi, zlo, zhi; };

__device__ __forceinline__ Raw load_raw(const float* __restrict__ p, int vol, const Offs& o) {
  const float* pu = p;
  const float* pv = p + vol;
  const float* pw = pv + vol;
  return Raw{*pu, *pv, *pw, pu[o.xlo], pu[o.xhi], pv[o.ylo], pv[o.yhi], pw[o.zlo], pw[o.zhi]};
}

// du/dx + dv/dy + dw/dz, each row applied as physics_loss.hip's jacobian() applies it
__device__ __forceinline__ float divergence(const Raw& f, int i, int j, int k, int X, int Y, int NZ, const Row3& wx,
                                            const Row3& wy, const Row3& wz) {
  const float jx = (i > 0 ? wx.a * f.ulo : 0.f) + wx.b * f.u + (i < X - 1 ? wx.c * f.uhi : 0.f);
  const float jy = (j > 0 ? wy.a * f.vlo : 0.f) + wy.b * f.v + (j < Y - 1 ? wy.c * f.vhi : 0.f);
  const float jz = (k > 0 ? wz.a * f.wlo : 0.f) + wz.b * f.w + (k < NZ - 1 ? wz.c * f.whi : 0.f);
  return (jx + jy) + jz;
}

__device__ __forceinline__ float angle(float au, float av, float bu, float bv) {
  const float cr = fabsf(au * bv - av * bu), dt = au * bu + av * bv;
  return (cr == 0.f && dt == 0.f) ? 0.f : atan2f(cr, dt);
}

// partial rows: partials[((b * nb + blockIdx.x) * NZ + level) * 15 + k]
__global__ __launch_bounds__(LD_BLOCK) void level_diag_kernel(const float* __restrict__ hr, int hr_c,
                                                              const float* __restrict__ sr, int sr_c,
                                                              const float* __restrict__ tl, int tl_c,
                                                              const float* __restrict__ zc, const float* __restrict__ xs,
                                                              const float* __restrict__ ys, LdGeom g,
                                                              float* __restrict__ partials) {
  __shared__ float sh[LD_NS][LD_BLOCK];
  const int b = blockIdx.y, nb = gridDim.x, t = threadIdx.x;
  const int X = g.X, Y = g.Y, NZ = g.NZ;
  const int lc = t / NZ, k = t - lc * NZ;
  const bool owner = lc < g.cpb;
  const int vol = (int)(g.ncols * NZ);  // (< 2^31: checked on the host, so offsets inside a plane are 32-bit)
  const int sx = Y * NZ;
  const float* hp = hr + (long)b * hr_c * vol;
  const float* sp = sr + (long)b * sr_c * vol;
  const float* tp = tl + (long)b * tl_c * vol;
  const float* zp = zc + (long)b * vol;
  float acc[LD_NS];
#pragma unroll
  for (int q = 0; q < LD_NS; ++q) acc[q] = 0.f;
  const int ncols = (int)g.ncols, nchunks = (int)g.nchunks;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += nb) {
    const int col = chunk * g.cpb + lc;
    if (!owner || col >= ncols) continue;
    const int i = (int)((unsigned)col / (unsigned)Y), j = col - i * Y;
    const int e = col * NZ + k;
    const Offs o{i > 0 ? -sx : 0, i < X - 1 ? sx : 0, j > 0 ? -NZ : 0, j < Y - 1 ? NZ : 0, k > 0 ? -1 : 0, k < NZ - 1 ? 1 : 0};
    const Raw H = load_raw(hp + e, vol, o), S = load_raw(sp + e, vol, o), T = load_raw(tp + e, vol, o);
    const Loc3 cx = load_loc3(xs, i, X), cy = load_loc3(ys, j, Y), cz = load_loc3(zp + col * NZ, k, NZ);
    const float z = cz.c0, z0 = zp[col * NZ];
    const Row3 wx = deriv_row(cx, i, X), wy = deriv_row(cy, j, Y), wz = deriv_row(cz, k, NZ);
    const float divh = divergence(H, i, j, k, X, Y, NZ, wx, wy, wz);
    const float divs = divergence(S, i, j, k, X, Y, NZ, wx, wy, wz);
    const float divt = divergence(T, i, j, k, X, Y, NZ, wx, wy, wz);
    const float nh = sqrtf((H.u * H.u + H.v * H.v) + H.w * H.w);
    const float ns = sqrtf((S.u * S.u + S.v * S.v) + S.w * S.w);
    const float nt = sqrtf((T.u * T.u + T.v * T.v) + T.w * T.w);
    const float dsu = H.u - S.u, dsv = H.v - S.v, dsw = H.w - S.w;
    const float dtu = H.u - T.u, dtv = H.v - T.v, dtw = H.w - T.w;
    const float bs = ns - nh, bt = nt - nh;
    const float h = sqrtf(H.u * H.u + H.v * H.v);
    acc[0] += nh;
    acc[1] += sqrtf((dsu * dsu + dsv * dsv) + dsw * dsw);
    acc[2] += sqrtf((dtu * dtu + dtv * dtv) + dtw * dtw);
    acc[3] += bs;
    acc[4] += bt;
    acc[5] += fabsf(bs);
    acc[6] += fabsf(bt);
    acc[7] += h;
    acc[8] += h * angle(H.u, H.v, S.u, S.v);
    acc[9] += h * angle(H.u, H.v, T.u, T.v);
    acc[10] += divh * divh;
    acc[11] += divs * divs;
    acc[12] += divt * divt;
    acc[13] += z;
    acc[14] += z - z0;
  }
#pragma unroll
  for (int q = 0; q < LD_NS; ++q) sh[q][t] = acc[q];
  __syncthreads();
  float* row = partials + ((long)b * nb + blockIdx.x) * (NZ * LD_NS);
  for (int item = t; item < NZ * LD_NS; item += LD_BLOCK) {
    const int lvl = item / LD_NS, q = item - lvl * LD_NS;
    float s = sh[q][lvl];
    for (int slot = 1; slot < g.cpb; ++slot) s += sh[q][slot * NZ + lvl];
    row[item] = s;
  }
}

// sums[b][level][k] = the nb partial rows of sample b in double: 64 (level, k) items per workgroup of 16 waves, wave w
// adds rows w, w + 16, ... in order (eight independent loads at a time), the sixteen wave sums are then added in order
constexpr int LD_FBLOCK = 1024, LD_FWAVES = LD_FBLOCK / 64;
__global__ __launch_bounds__(LD_FBLOCK) void level_diag_final_kernel(const float* __restrict__ partials, int nb, int items,
                                                                     double* __restrict__ sums) {
  __shared__ double sh[LD_FWAVES][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = blockIdx.x * 64 + lane;
  const float* rows = partials + (long)b * nb * items;
  double s = 0.0;
  if (item < items) {
    int r = wave;
    for (; r + 7 * LD_FWAVES < nb; r += 8 * LD_FWAVES) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = rows[(long)(r + q * LD_FWAVES) * items + item];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += (double)v[q];
    }
    for (; r < nb; r += LD_FWAVES) s += (double)rows[(long)r * items + item];
  }
  sh[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && item < items) {
    double a = sh[0][lane];
#pragma unroll
    for (int w = 1; w < LD_FWAVES; ++w) a += sh[w][lane];
    sums[(long)b * items + item] = a;
  }
}

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_diagnostics documents them
inline int ld_geom(LdGeom& g, int B, int X, int Y, int NZ) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  if (NZ > LD_BLOCK || B > 65535 || X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  g.cpb = LD_BLOCK / NZ;
  g.ncols = (long)X * Y;
  g.nchunks = (g.ncols + g.cpb - 1) / g.cpb;
  return 0;
}

inline int ld_rows(const LdGeom& g) { return (int)(g.nchunks < LD_MAX_ROWS ? g.nchunks : LD_MAX_ROWS); }

}  // namespace

extern "C" int64_t wsr_level_diagnostics_workspace_floats(int32_t B, int32_t X, int32_t Y, int32_t NZ) {
  LdGeom g{};
  if (ld_geom(g, B, X, Y, NZ) != 0) return 0;
  return (int64_t)B * ld_rows(g) * NZ * LD_NS;
}

extern "C" int wsr_level_diagnostics(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl,
                                     int32_t tl_c, const float* zc, const float* xs, const float* ys, int32_t B, int32_t X,
                                     int32_t Y, int32_t NZ, float* workspace, double* sums, void* stream) {
  if (!hr || !sr || !tl || !zc || !xs || !ys || !workspace || !sums || hr_c < 3 || sr_c < 3 || tl_c < 3) return WSR_EINVAL;
  LdGeom g{};
  const int rc = ld_geom(g, B, X, Y, NZ);
  if (rc != 0) return rc;
  const int nb = ld_rows(g), items = NZ * LD_NS;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(level_diag_kernel, dim3((unsigned)nb, (unsigned)B), dim3(LD_BLOCK), 0, st, hr, hr_c, sr, sr_c, tl,
                     tl_c, zc, xs, ys, g, workspace);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(level_diag_final_kernel, dim3((unsigned)((items + 63) / 64), (unsigned)B), dim3(LD_FBLOCK), 0, st,
                     workspace, nb, items, sums);
  WSR_LAUNCH_CHECK();
  return 0;
}
