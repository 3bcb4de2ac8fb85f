// Tiled whole-domain inference ([TILE]): overlapping (x, y) tiles cut out of a batch, and the generator's outputs on the
// tiles blended back into one field.  All tensors fp32 planar (.., C, X, Y, NZ), z innermost; z is never tiled.
//
// Thread layout of data_gather.hip / ensemble.hip: a workgroup covers a chunk of one plane, so tile, sample and channel
// are workgroup-uniform; a thread moves V consecutive floats (V | NZ: a piece never straddles two columns), consecutive
// threads move consecutive pieces - stores are fully coalesced, loads are runs of NZ floats.
//
// wsr_tile_gather is a pure copy.  wsr_tile_stitch is a gather-form blend: every output piece finds the tiles that cover
// its column, reads them and is written once - no atomics, no zero fill, no second launch, so two calls give the same
// bits.  The origins travel by value in the launch arguments; a workgroup first narrows both axes to the tiles that
// touch its chunk (scalar loops over workgroup-uniform values), a thread then walks only those.
//
// The blend weight of a tile on one axis is an integer ramp (the rule is stated in include/windsr_hip.h); the share of
// tile (ix, iy) is (wx / Wx) * (wy / Wy) with Wx, Wy the sums over the covering tiles of the axis - two correctly
// rounded quotients and their product.  Where one tile covers a column both quotients are 1.0f exactly: the tile's value
// comes back bit for bit and the seam is exactly 0.  Products and sums in tile order, without contraction.
#include "common.h"

namespace {

constexpr int TL_BLOCK = 256;
constexpr int TL_GATHER_MAX = 256;  // tiles per gather launch (their origins travel by value); more: several launches
constexpr int TL_MAXA = WSR_TILE_MAX_PER_AXIS;

template <int V> using uvec = unsigned int __attribute__((ext_vector_type(V)));
template <int V> using fvec = float __attribute__((ext_vector_type(V)));

struct TileGatherGeom {
  int BC, X, Y, NZ, tx, ty, nb;
  int x0[TL_GATHER_MAX], y0[TL_GATHER_MAX];
};

struct StitchGeom {
  int B, C, X, Y, NZ, Tx, Ty, Rx, Ry, nx, ny, nb;
  int xs[TL_MAXA], ys[TL_MAXA];
};

template <int V>
__global__ __launch_bounds__(TL_BLOCK) void tile_gather_kernel(const float* __restrict__ src, TileGatherGeom g,
                                                               float* __restrict__ dst) {
  // workgroup -> (tile, b * C + c, chunk): the planes of dst (n, B, C, tx, ty, NZ) in their own order
  const int plane_id = blockIdx.x / g.nb;
  const int chunk = blockIdx.x - plane_id * g.nb;
  const int k = plane_id / g.BC;
  const int bc = plane_id - k * g.BC;
  const int x0 = g.x0[k], y0 = g.y0[k];
  const long tplane = (long)g.tx * g.ty * g.NZ;
  const long e = ((long)chunk * TL_BLOCK + threadIdx.x) * V;
  if (e >= tplane) return;
  const unsigned eu = (unsigned)e;  // (tplane <= X * Y * NZ < 2^31: checked on the host)
  const int col = (int)(eu / (unsigned)g.NZ);
  const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
  const int i = col / g.ty, j = col - i * g.ty;
  const float* sp = src + ((long)bc * g.X + (x0 + i)) * ((long)g.Y * g.NZ) + (long)(y0 + j) * g.NZ + zz;
  const uvec<V> v = *reinterpret_cast<const uvec<V>*>(sp);
  *reinterpret_cast<uvec<V>*>(dst + (long)plane_id * tplane + e) = v;
}

// weight of the tile at origin a (side T, ramp R) on an axis of length N at coordinate i; 0 outside the tile
__device__ __forceinline__ int axis_weight(int i, int a, int T, int N, int R) {
  const int p = i - a;
  if (p < 0 || p >= T) return 0;
  const int l = a == 0 ? R + 1 : min(p + 1, R + 1);      // a domain border has no ramp
  const int r = a + T == N ? R + 1 : min(T - p, R + 1);
  return min(l, r);
}

// the tiles of a sorted axis that touch coordinates [c0, c1]: the first whose end lies past c0 .. the last starting <= c1
__device__ __forceinline__ void axis_range(const int* s, int n, int T, int c0, int c1, int& lo, int& hi) {
  lo = 0;
  hi = 0;
  for (int k = 0; k < n; ++k) {
    if (s[k] + T <= c0) lo = k + 1;
    if (s[k] <= c1) hi = k;
  }
}

template <int V, bool SEAM>
__global__ __launch_bounds__(TL_BLOCK) void tile_stitch_kernel(const float* __restrict__ tiles, StitchGeom g,
                                                               float* __restrict__ out, float* __restrict__ seam) {
#pragma clang fp contract(off)
  // workgroup -> (b, c, chunk) of the output
  const int plane_id = blockIdx.x / g.nb;
  const int chunk = blockIdx.x - plane_id * g.nb;
  const long plane = (long)g.X * g.Y * g.NZ;  // (< 2^31: checked on the host)
  // the columns of this chunk -> the tiles of each axis that can cover one of them (workgroup-uniform)
  const unsigned e0 = (unsigned)chunk * (unsigned)(TL_BLOCK * V);
  const unsigned e1 = (unsigned)min((long)e0 + TL_BLOCK * V, plane) - 1u;
  const int col0 = (int)(e0 / (unsigned)g.NZ), col1 = (int)(e1 / (unsigned)g.NZ);
  const int i0 = col0 / g.Y, i1 = col1 / g.Y;
  const int j0 = i0 == i1 ? col0 - i0 * g.Y : 0, j1 = i0 == i1 ? col1 - i1 * g.Y : g.Y - 1;
  int lox, hix, loy, hiy;
  axis_range(g.xs, g.nx, g.Tx, i0, i1, lox, hix);
  axis_range(g.ys, g.ny, g.Ty, j0, j1, loy, hiy);

  const long e = (long)e0 + (long)threadIdx.x * V;
  if (e >= plane) return;
  const unsigned eu = (unsigned)e;
  const int col = (int)(eu / (unsigned)g.NZ);
  const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
  const int i = col / g.Y, j = col - i * g.Y;
  int Wx = 0, Wy = 0;
  for (int ix = lox; ix <= hix; ++ix) Wx += axis_weight(i, g.xs[ix], g.Tx, g.X, g.Rx);
  for (int iy = loy; iy <= hiy; ++iy) Wy += axis_weight(j, g.ys[iy], g.Ty, g.Y, g.Ry);
  const float fWx = (float)Wx, fWy = (float)Wy;  // (>= 1: the host checked that the tiles cover each axis)
  const long tplane = (long)g.Tx * g.Ty * g.NZ;
  const float* base = tiles + (long)plane_id * tplane + zz;  // plane (b, c) of tile 0
  const long tile_stride = (long)g.B * g.C * tplane;

  fvec<V> acc = 0.0f;
  bool first = true;
  for (int ix = lox; ix <= hix; ++ix) {
    const int wx = axis_weight(i, g.xs[ix], g.Tx, g.X, g.Rx);
    if (wx == 0) continue;
    const float ax = (float)wx / fWx;
    for (int iy = loy; iy <= hiy; ++iy) {
      const int wy = axis_weight(j, g.ys[iy], g.Ty, g.Y, g.Ry);
      if (wy == 0) continue;
      const float alpha = ax * ((float)wy / fWy);
      const float* tp = base + (long)(ix * g.ny + iy) * tile_stride +
                        ((long)(i - g.xs[ix]) * g.Ty + (j - g.ys[iy])) * g.NZ;
      const fvec<V> p = *reinterpret_cast<const fvec<V>*>(tp) * alpha;
      acc = first ? p : acc + p;  // (the first product starts the sum: a single cover keeps the sign of zero)
      first = false;
    }
  }
  const long o = (long)plane_id * plane + e;
  *reinterpret_cast<fvec<V>*>(out + o) = acc;
  if (SEAM) {  // sum alpha (x_T - out)^2: the same tiles again (they sit in the cache this thread just filled)
    fvec<V> sacc = 0.0f;
    first = true;
    for (int ix = lox; ix <= hix; ++ix) {
      const int wx = axis_weight(i, g.xs[ix], g.Tx, g.X, g.Rx);
      if (wx == 0) continue;
      const float ax = (float)wx / fWx;
      for (int iy = loy; iy <= hiy; ++iy) {
        const int wy = axis_weight(j, g.ys[iy], g.Ty, g.Y, g.Ry);
        if (wy == 0) continue;
        const float alpha = ax * ((float)wy / fWy);
        const float* tp = base + (long)(ix * g.ny + iy) * tile_stride +
                          ((long)(i - g.xs[ix]) * g.Ty + (j - g.ys[iy])) * g.NZ;
        const fvec<V> d = *reinterpret_cast<const fvec<V>*>(tp) - acc;
        const fvec<V> p = (d * d) * alpha;
        sacc = first ? p : sacc + p;
        first = false;
      }
    }
    *reinterpret_cast<fvec<V>*>(seam + o) = sacc;
  }
}

template <int V>
int launch_gather(const float* src, TileGatherGeom g, int n, float* dst, hipStream_t st) {
  const long tplane = (long)g.tx * g.ty * g.NZ;
  g.nb = (int)((tplane / V + TL_BLOCK - 1) / TL_BLOCK);
  const long blocks = (long)n * g.BC * g.nb;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(tile_gather_kernel<V>, dim3((unsigned)blocks), dim3(TL_BLOCK), 0, st, src, g, dst);
  WSR_LAUNCH_CHECK();
  return 0;
}

template <int V>
int launch_stitch(const float* tiles, StitchGeom g, float* out, float* seam, hipStream_t st) {
  const long plane = (long)g.X * g.Y * g.NZ;
  g.nb = (int)((plane / V + TL_BLOCK - 1) / TL_BLOCK);
  const long blocks = (long)g.B * g.C * g.nb;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  if (seam)
    hipLaunchKernelGGL((tile_stitch_kernel<V, true>), dim3((unsigned)blocks), dim3(TL_BLOCK), 0, st, tiles, g, out, seam);
  else
    hipLaunchKernelGGL((tile_stitch_kernel<V, false>), dim3((unsigned)blocks), dim3(TL_BLOCK), 0, st, tiles, g, out,
                       seam);
  WSR_LAUNCH_CHECK();
  return 0;
}

// origins of one axis: first 0, strictly increasing, no gap wider than a tile, the last tile ending at N
inline int check_axis(const int32_t* s, int n, int T, int N, int R) {
  if (!s || n < 1 || T < 1 || T > N || R < 0 || R > 32768) return WSR_EINVAL;
  if (s[0] != 0) return WSR_EINVAL;
  for (int k = 1; k < n; ++k)
    if (s[k] <= s[k - 1] || s[k] - s[k - 1] > T) return WSR_EINVAL;
  if ((long)s[n - 1] + T != N) return WSR_EINVAL;
  return n > TL_MAXA ? WSR_EUNSUPPORTED : 0;
}

}  // namespace

extern "C" int wsr_tile_gather(const float* src, int32_t B, int32_t C, int32_t X, int32_t Y, int32_t NZ,
                               const int32_t* x0, const int32_t* y0, int32_t n, int32_t tx, int32_t ty, float* dst,
                               void* stream) {
  if (!src || !dst || !x0 || !y0 || B <= 0 || C <= 0 || X <= 0 || Y <= 0 || NZ <= 0 || n <= 0 || tx <= 0 || ty <= 0 ||
      tx > X || ty > Y)
    return WSR_EINVAL;
  for (int k = 0; k < n; ++k)  // every tile inside the domain, before anything is written
    if (x0[k] < 0 || y0[k] < 0 || x0[k] > X - tx || y0[k] > Y - ty) return WSR_EINVAL;
  if (X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL || (long)B * C > 0x7fffffffL) return WSR_EUNSUPPORTED;
  TileGatherGeom g{};
  g.BC = B * C;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  g.tx = tx;
  g.ty = ty;
  const hipStream_t st = as_stream(stream);
  const long per_tile = (long)B * C * tx * ty * NZ;
  const int v = piece_width(NZ, {src, dst});
  for (int k0 = 0; k0 < n; k0 += TL_GATHER_MAX) {  // (one launch up to TL_GATHER_MAX tiles)
    const int m = n - k0 < TL_GATHER_MAX ? n - k0 : TL_GATHER_MAX;
    for (int k = 0; k < m; ++k) {
      g.x0[k] = x0[k0 + k];
      g.y0[k] = y0[k0 + k];
    }
    float* d = dst + (long)k0 * per_tile;  // (a multiple of NZ floats: the alignment of dst carries over)
    const int rc = v == 4 ? launch_gather<4>(src, g, m, d, st)
                          : (v == 2 ? launch_gather<2>(src, g, m, d, st) : launch_gather<1>(src, g, m, d, st));
    if (rc) return rc;
  }
  return 0;
}

extern "C" int wsr_tile_stitch(const float* tiles, const int32_t* xs, int32_t nx, const int32_t* ys, int32_t ny,
                               int32_t B, int32_t C, int32_t X, int32_t Y, int32_t NZ, int32_t Tx, int32_t Ty,
                               int32_t Rx, int32_t Ry, float* out, float* seam, void* stream) {
  if (!tiles || !out || B <= 0 || C <= 0 || X <= 0 || Y <= 0 || NZ <= 0) return WSR_EINVAL;
  const int rx = check_axis(xs, nx, Tx, X, Rx), ry = check_axis(ys, ny, Ty, Y, Ry);
  if (rx == WSR_EINVAL || ry == WSR_EINVAL) return WSR_EINVAL;
  if (rx || ry) return WSR_EUNSUPPORTED;
  if (X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL || (long)B * C > 0x7fffffffL) return WSR_EUNSUPPORTED;
  StitchGeom g{};
  g.B = B;
  g.C = C;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  g.Tx = Tx;
  g.Ty = Ty;
  g.Rx = Rx;
  g.Ry = Ry;
  g.nx = nx;
  g.ny = ny;
  for (int k = 0; k < nx; ++k) g.xs[k] = xs[k];
  for (int k = 0; k < ny; ++k) g.ys[k] = ys[k];
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {tiles, out, seam})) {
    case 4: return launch_stitch<4>(tiles, g, out, seam, st);
    case 2: return launch_stitch<2>(tiles, g, out, seam, st);
    default: return launch_stitch<1>(tiles, g, out, seam, st);
  }
}
