// The kernels of csrc/increments.hip ([INCREMENTS]; increments.py holds the definition), kept in a header of their own so
// that a host program can run them block by block on threads under the address and undefined-behaviour sanitisers
// (tools/increments_host_check.cpp: the shim of tools/host_shim.h).  Nothing here needs more of HIP than __global__,
// __shared__, threadIdx / blockIdx and __syncthreads.  No thread leaves a kernel that has a barrier before the last
// barrier.
//
// Every (direction, kind) of the definition reads ONE wind component (x: L = u, T = v; y: L = v, T = u; W = w in both), so
// a workgroup works on one component of one source and the kinds are sorted out when the rows are added.
//
// increments_kernel        grid (tiles x level chunks, sources x 3 components, B), 256 threads.  A workgroup owns a
//                          32 x 32 tile of the plane and nz <= ZC consecutive levels.  1. It stages the tile with a
//                          FORWARD halo of R = the largest separation along x and along y (increments look one way):
//                          the element loop runs over (staged row, staged column, z) with z fastest, so a wave reads runs
//                          of the chunk's levels - when the chunk is all of NZ, contiguous memory.  Cells outside the
//                          plane hold 0 and are never paired.  2. Thread t = (slot t / nz, level t % nz) walks the
//                          positions slot, slot + nslots, ... of the tile in this order; per position one LDS read of
//                          f(p) and, per separation, one of f(p + r e_x) and one of f(p + r e_y); delta, delta^2,
//                          delta^3, delta^4 as the definition rounds them, into 6 fp32 accumulators per separation that
//                          are plain registers (the loop over the separations is unrolled over the 8 possible ones).
//                          3. The accumulators go to LDS (over the staged tile, after a barrier); item (level,
//                          separation, direction, order) adds its slots in groups of 16 - inside a group in slot order,
//                          then the group sums in order - and is written into the workgroup's partial row.
// increments_final_kernel  one thread per element of out: the rows of the tiles in order, in double; the slices of an
//                          absent baseline are written as zeros.
//
// No atomics, no zero fill: every element of out is written and two calls give the same bits.  The three sources go
// through the same code on the same geometry.  The longest fp32 chain of a sum: 1024 / nslots <= 64 terms in a thread
// (nslots = 256 / nz >= 16), 16 in a group, 16 groups - at most 96 roundings whatever the plane, and never more than the
// entry has pairs (a zero partial adds exactly).
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int INC_BLOCK = 256;
constexpr int INC_TILE = 32;                            // positions of a workgroup: INC_TILE x INC_TILE
constexpr int INC_MAX_NR = WSR_INCREMENTS_MAX_SEPARATIONS;
constexpr int INC_MAX_R = WSR_INCREMENTS_MAX_SEPARATION;
constexpr int INC_MAX_ZC = 16;
constexpr int INC_ACC = 6;                              // (direction, order) per separation
constexpr int INC_LDS_FLOATS = INC_BLOCK * INC_MAX_NR * INC_ACC;  // 12288 floats = 48 KiB: the staged tile, then the slots
constexpr int INC_GROUP = 16;                           // slots per group of the workgroup's sum

struct IncGeom {
  int B, X, Y, NZ, nr;
  int sep[INC_MAX_NR];  // ascending
  int R, S;             // the largest separation; staged rows = columns = INC_TILE + R
  int ntx, nty;         // tiles along x and y
  int ZC, nzc;          // levels per chunk; chunks
};

// 0: fine; WSR_EINVAL / WSR_EUNSUPPORTED as wsr_level_increments documents them.  separations: host.  A function of the
// arguments alone (and the sums do not depend on the chunk): the chunk is what fits INC_LDS_FLOATS, at most INC_MAX_ZC
// levels, the levels spread evenly over the chunks.
inline int inc_geom(IncGeom& g, int B, int X, int Y, int NZ, const int* separations, int nr) {
  if (B <= 0 || X <= 0 || Y <= 0 || NZ <= 0 || !separations || nr < 1 || nr > INC_MAX_NR) return WSR_EINVAL;
  for (int k = 0; k < nr; ++k) {
    const int r = separations[k];
    if (r < 1 || r > INC_MAX_R || (k > 0 && r <= separations[k - 1])) return WSR_EINVAL;
  }
  if (B > 65535 || (long)X * Y > 0x7fffffffL || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B, g.X = X, g.Y = Y, g.NZ = NZ, g.nr = nr;
  for (int k = 0; k < INC_MAX_NR; ++k) g.sep[k] = k < nr ? separations[k] : 0;
  g.R = separations[nr - 1];
  g.S = INC_TILE + g.R;                                 // <= 64
  g.ntx = (X + INC_TILE - 1) / INC_TILE, g.nty = (Y + INC_TILE - 1) / INC_TILE;
  int zc = INC_LDS_FLOATS / (g.S * g.S);                // >= 3
  if (zc > INC_MAX_ZC) zc = INC_MAX_ZC;
  if (zc > NZ) zc = NZ;
  g.nzc = (NZ + zc - 1) / zc;
  g.ZC = (NZ + g.nzc - 1) / g.nzc;
  g.nzc = (NZ + g.ZC - 1) / g.ZC;
  if ((long)g.ntx * g.nty * g.nzc > 0x7fffffffL) return WSR_EUNSUPPORTED;
  if (((long)NZ * 3 * nr * 3 * INC_ACC + INC_BLOCK - 1) / INC_BLOCK > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

// floats of one partial row (a workgroup's) and of the whole workspace: always three sources
inline long inc_row_floats(const IncGeom& g) { return (long)g.ZC * g.nr * INC_ACC; }
inline long inc_workspace_floats(const IncGeom& g) {
  return (long)g.B * 9 * g.nzc * g.ntx * g.nty * inc_row_floats(g);
}

// partials[((((b * 9 + src * 3 + comp) * nzc + chunk) * ntiles + tile) * ZC + level in chunk) * nr * 6 + (k * 2 + dir) * 3
// + order]; f2 may be null (then gridDim.y is 6)
__global__ __launch_bounds__(INC_BLOCK) void increments_kernel(const float* __restrict__ f0, int c0,
                                                               const float* __restrict__ f1, int c1,
                                                               const float* __restrict__ f2, int c2, IncGeom g,
                                                               float* __restrict__ partials) {
  __shared__ float lds[INC_LDS_FLOATS];
  const int t = threadIdx.x, b = blockIdx.z;
  const int src = (int)blockIdx.y / 3, comp = (int)blockIdx.y - 3 * src;
  const int chunk = (int)(blockIdx.x % (unsigned)g.nzc), tile = (int)(blockIdx.x / (unsigned)g.nzc);
  const int ty = tile % g.nty, tx = tile / g.nty;
  const int x0 = tx * INC_TILE, y0 = ty * INC_TILE;
  const int z0 = chunk * g.ZC;
  const int nz = g.NZ - z0 < g.ZC ? g.NZ - z0 : g.ZC;
  const int S = g.S, nr = g.nr;
  const long vol = (long)g.X * g.Y * g.NZ;               // (< 2^31: checked on the host)
  const float* f = src == 0 ? f0 : (src == 1 ? f1 : f2);
  const int c = src == 0 ? c0 : (src == 1 ? c1 : c2);
  const float* p = f + ((long)b * c + comp) * vol;

  // 1. the staged tile: lds[(i * S + j) * nz + z]
  const int n_stage = S * S * nz;                        // <= INC_LDS_FLOATS
  for (int e = t; e < n_stage; e += INC_BLOCK) {
    const int col = e / nz, z = e - col * nz;
    const int i = col / S, j = col - i * S;
    const int x = x0 + i, y = y0 + j;
    lds[e] = (x < g.X && y < g.Y) ? p[((long)x * g.Y + y) * g.NZ + z0 + z] : 0.f;
  }
  __syncthreads();

  // 2. the increments of the thread's positions
  const int nslots = INC_BLOCK / nz;                     // >= 16
  const int slot = t / nz, zl = t - slot * nz;
  const int lim_x = g.X - x0, lim_y = g.Y - y0;          // the tile's rows / columns inside the plane (may exceed 32 + R)
  float acc[INC_MAX_NR][INC_ACC];
#pragma unroll
  for (int k = 0; k < INC_MAX_NR; ++k)
#pragma unroll
    for (int a = 0; a < INC_ACC; ++a) acc[k][a] = 0.f;
  if (slot < nslots) {
    for (int pos = slot; pos < INC_TILE * INC_TILE; pos += nslots) {
      const int lx = pos / INC_TILE, ly = pos - lx * INC_TILE;
      if (lx >= lim_x || ly >= lim_y) continue;
      const int at = (lx * S + ly) * nz + zl;
      const float v = lds[at];
#pragma unroll
      for (int k = 0; k < INC_MAX_NR; ++k) {
        if (k < nr) {
          const int r = g.sep[k];
          if (lx + r < lim_x) {
            const float d = lds[at + r * S * nz] - v;
            const float q = d * d;
            const float cu = q * d, fo = q * q;
            acc[k][0] += q, acc[k][1] += cu, acc[k][2] += fo;
          }
          if (ly + r < lim_y) {
            const float d = lds[at + r * nz] - v;
            const float q = d * d;
            const float cu = q * d, fo = q * q;
            acc[k][3] += q, acc[k][4] += cu, acc[k][5] += fo;
          }
        }
      }
    }
  }
  __syncthreads();                                       // the staged tile is read: its LDS now holds the slots

  // 3. lds[(k * 6 + a) * 256 + t]; a thread beyond the last slot holds zeros and is never added
#pragma unroll
  for (int k = 0; k < INC_MAX_NR; ++k)
#pragma unroll
    for (int a = 0; a < INC_ACC; ++a) lds[(k * INC_ACC + a) * INC_BLOCK + t] = acc[k][a];
  __syncthreads();
  const int nacc = nr * INC_ACC;
  const long ntiles = (long)g.ntx * g.nty;
  float* row = partials + ((((long)b * 9 + blockIdx.y) * g.nzc + chunk) * ntiles + tile) * ((long)g.ZC * nacc);
  for (int item = t; item < nz * nacc; item += INC_BLOCK) {
    const int z = item / nacc, ka = item - z * nacc;
    const float* s = lds + ka * INC_BLOCK + z;           // slot q at s[q * nz]
    float total = 0.f;
    for (int q0 = 0; q0 < nslots; q0 += INC_GROUP) {
      const int q1 = q0 + INC_GROUP < nslots ? q0 + INC_GROUP : nslots;
      float part = s[q0 * nz];
      for (int q = q0 + 1; q < q1; ++q) part += s[q * nz];
      total = q0 == 0 ? part : total + part;
    }
    row[item] = total;
  }
}

// out (B, NZ, 3, nr, 2, 3, 3) doubles; grid (ceil(NZ * 3 * nr * 18 / 256), B)
__global__ __launch_bounds__(INC_BLOCK) void increments_final_kernel(const float* __restrict__ partials, IncGeom g,
                                                                     int nsrc, double* __restrict__ out) {
  const int b = blockIdx.y;
  const long per_sample = (long)g.NZ * 3 * g.nr * 18;
  const long e = (long)blockIdx.x * INC_BLOCK + threadIdx.x;
  if (e >= per_sample) return;
  long i = e;
  const int order = (int)(i % 3); i /= 3;
  const int kind = (int)(i % 3); i /= 3;
  const int dir = (int)(i % 2); i /= 2;
  const int k = (int)(i % g.nr); i /= g.nr;
  const int src = (int)(i % 3); i /= 3;
  const int z = (int)i;
  double sum = 0.0;
  if (src < nsrc) {
    const int comp = kind == 2 ? 2 : (dir == 0 ? kind : 1 - kind);   // x: L = u, T = v; y: L = v, T = u
    const int chunk = z / g.ZC, zl = z - chunk * g.ZC;
    const int nacc = g.nr * INC_ACC;
    const long ntiles = (long)g.ntx * g.nty, rowf = (long)g.ZC * nacc;
    const float* rows = partials + ((((long)b * 9 + src * 3 + comp) * g.nzc + chunk) * ntiles) * rowf +
                        (long)zl * nacc + (k * 2 + dir) * 3 + order;
    for (long tile = 0; tile < ntiles; ++tile) sum += (double)rows[tile * rowf];
  }
  out[(long)b * per_sample + e] = sum;
}

}  // namespace
