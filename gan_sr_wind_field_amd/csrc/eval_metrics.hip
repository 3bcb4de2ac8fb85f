// Device-side evaluation ([EVAL] device_metrics): the trilinear baseline, the per-sample error sums behind the nine
// metrics of test.py / the validation PSNRs, and np.interp per column (back onto the raw terrain-following levels).
// All tensors fp32 planar (B, C, X, Y, NZ), z innermost.  Indexing as in data_gather.hip: a thread moves V consecutive
// floats of the flattened (xy, z) run of one plane (V | NZ: a piece never straddles two columns), consecutive threads
// move consecutive pieces, so loads and stores are coalesced for NZ = 10 as well as NZ = 128.
//
// The baseline is F.interpolate(LR[:, :3], scale_factor=(s, s, 1), mode="trilinear", align_corners=True): the z scale is
// 1, so an output column is a 4-corner blend of LR columns.  Output index o of an axis with `in` source and `out` output
// points sits at o * (in - 1) / (out - 1); index pair and weights are computed as ATen computes them (axis_map), so the
// baseline is the reference's baseline and not a slightly different one.  axis_map and blend4 are evaluated without
// contraction, so wsr_trilinear_xy and the on-the-fly form of wsr_field_metrics produce the same bits.
//
// The sums: fp32 partials per thread (fixed order: the pieces of its stride loop, the lanes of a piece), butterfly in each
// wave, the four wave sums in LDS, ONE partial row per workgroup; a second kernel adds the rows of a sample in a fixed
// order in double.  No atomics: two calls give the same bits (as grad_sqnorm_multi_kernel in elementwise.hip).
#include "common.h"

namespace {

constexpr int EV_BLOCK = 256;
constexpr int EV_MAX_ROWS = WSR_FIELD_METRICS_MAX_ROWS;
constexpr int EV_NSUMS = WSR_FIELD_METRICS_SUMS;

template <int V> using fvec = float __attribute__((ext_vector_type(V)));

// source pair and upper weight of output index o on an axis of `in` -> `out` points (align_corners), in ATen's own
// fp32 arithmetic (area_pixel_compute_scale / compute_source_index_and_lambda): scale = (in - 1) / (out - 1) rounded
// once, src = scale * o rounded once, lower index = trunc(src), upper weight = src - lower index (exact)
__device__ __forceinline__ void axis_map(int o, int in, int out, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  if (out <= 1) {
    i0 = i1 = 0;
    l1 = 0.f;
    return;
  }
  const float scale = (float)(in - 1) / (float)(out - 1);
  const float src = scale * (float)o;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// lx0 * (ly0 * v00 + ly1 * v01) + lx1 * (ly0 * v10 + ly1 * v11): the nesting of ATen's separable kernel, x outermost
template <int V>
__device__ __forceinline__ fvec<V> blend4(fvec<V> v00, fvec<V> v01, fvec<V> v10, fvec<V> v11, float lx1, float ly1) {
#pragma clang fp contract(off)
  const float lx0 = 1.f - lx1, ly0 = 1.f - ly1;
  const fvec<V> a = ly0 * v00 + ly1 * v01;
  const fvec<V> b = ly0 * v10 + ly1 * v11;
  return lx0 * a + lx1 * b;
}

struct TlGeom {
  int Cin, Xl, Yl, X, Y, NZ;
  long lplane;  // Xl * Yl * NZ
};

// the V baseline values of channel c at flat position e = (i * Y + j) * NZ + zz of sample b
template <int V>
__device__ __forceinline__ fvec<V> baseline_piece(const float* __restrict__ lr, const TlGeom& g, int b, int c, int i0,
                                                  int i1, int j0, int j1, float lx1, float ly1, int zz) {
  const float* p = lr + ((long)b * g.Cin + c) * g.lplane + zz;
  const long r0 = (long)i0 * g.Yl, r1 = (long)i1 * g.Yl;
  const fvec<V> v00 = *reinterpret_cast<const fvec<V>*>(p + (r0 + j0) * g.NZ);
  const fvec<V> v01 = *reinterpret_cast<const fvec<V>*>(p + (r0 + j1) * g.NZ);
  const fvec<V> v10 = *reinterpret_cast<const fvec<V>*>(p + (r1 + j0) * g.NZ);
  const fvec<V> v11 = *reinterpret_cast<const fvec<V>*>(p + (r1 + j1) * g.NZ);
  return blend4<V>(v00, v01, v10, v11, lx1, ly1);
}

template <int V>
__global__ __launch_bounds__(EV_BLOCK) void trilinear_xy_kernel(const float* __restrict__ lr, TlGeom g, int nb,
                                                                float* __restrict__ tl) {
  const int plane_id = blockIdx.x / nb;  // (b, c), c in 0..2
  const int chunk = blockIdx.x - plane_id * nb;
  const int b = plane_id / 3, c = plane_id - b * 3;
  const long plane = (long)g.X * g.Y * g.NZ;
  const long e = ((long)chunk * EV_BLOCK + threadIdx.x) * V;
  if (e >= plane) return;
  const unsigned eu = (unsigned)e;  // (plane < 2^31: checked on the host)
  const int col = (int)(eu / (unsigned)g.NZ);
  const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
  const int i = col / g.Y, j = col - i * g.Y;
  int i0, i1, j0, j1;
  float lx1, ly1;
  axis_map(i, g.Xl, g.X, i0, i1, lx1);
  axis_map(j, g.Yl, g.Y, j0, j1, ly1);
  const fvec<V> v = baseline_piece<V>(lr, g, b, c, i0, i1, j0, j1, lx1, ly1, zz);
  *reinterpret_cast<fvec<V>*>(tl + ((long)b * 3 + c) * plane + e) = v;
}

template <int V> __device__ __forceinline__ float lane_of(const fvec<V>& v, int k) { return v[k]; }
template <> __device__ __forceinline__ float lane_of<1>(const fvec<1>& v, int) { return v[0]; }

// partial rows: partials[(b * nb + blockIdx.x) * 7 + k], k = sq_sr, sq_tl, abs_sr, abs_tl, len_sr, len_tl, len_hr
template <int V, bool FLY>
__global__ __launch_bounds__(EV_BLOCK) void field_metrics_kernel(const float* __restrict__ hr, int hr_c,
                                                                 const float* __restrict__ sr, int sr_c,
                                                                 const float* __restrict__ tl, int tl_c, TlGeom g,
                                                                 float* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ float sh[EV_NSUMS][EV_BLOCK / 64];
  const int b = blockIdx.y, nb = gridDim.x;
  const long plane = (long)g.X * g.Y * g.NZ;
  const long pieces = plane / V;
  const float* hp = hr + (long)b * hr_c * plane;
  const float* sp = sr + (long)b * sr_c * plane;
  const float* tp = FLY ? nullptr : tl + (long)b * tl_c * plane;
  float acc[EV_NSUMS];
#pragma unroll
  for (int k = 0; k < EV_NSUMS; ++k) acc[k] = 0.f;
  for (long p = (long)blockIdx.x * EV_BLOCK + threadIdx.x; p < pieces; p += (long)nb * EV_BLOCK) {
    const long e = p * V;  // (< 2^31: checked on the host, so the column split below is 32-bit arithmetic)
    fvec<V> h[3], r[3], t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      h[c] = *reinterpret_cast<const fvec<V>*>(hp + c * plane + e);
      r[c] = *reinterpret_cast<const fvec<V>*>(sp + c * plane + e);
    }
    if (FLY) {
      const unsigned eu = (unsigned)e;
      const int col = (int)(eu / (unsigned)g.NZ);
      const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
      const int i = col / g.Y, j = col - i * g.Y;
      int i0, i1, j0, j1;
      float lx1, ly1;
      axis_map(i, g.Xl, g.X, i0, i1, lx1);
      axis_map(j, g.Yl, g.Y, j0, j1, ly1);
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] = baseline_piece<V>(tl, g, b, c, i0, i1, j0, j1, lx1, ly1, zz);  // (tl = LR here)
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) t[c] = *reinterpret_cast<const fvec<V>*>(tp + c * plane + e);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float qs = 0.f, qt = 0.f, qh = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float hv = lane_of<V>(h[c], k);
        const float ds = hv - lane_of<V>(r[c], k), dt = hv - lane_of<V>(t[c], k);
        qs += ds * ds;
        qt += dt * dt;
        qh += hv * hv;
        acc[2] += fabsf(ds);
        acc[3] += fabsf(dt);
      }
      acc[0] += qs;
      acc[1] += qt;
      acc[4] += sqrtf(qs);
      acc[5] += sqrtf(qt);
      acc[6] += sqrtf(qh);
    }
  }
#pragma unroll
  for (int k = 0; k < EV_NSUMS; ++k) {
    float s = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < EV_NSUMS) {
    const int k = threadIdx.x;
    partials[((long)b * nb + blockIdx.x) * EV_NSUMS + k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
  }
}

// sums[b][k] = the nb partial rows of sample b, added in double in a fixed order (thread-strided, butterfly, LDS)
__global__ __launch_bounds__(EV_BLOCK) void field_metrics_final_kernel(const float* __restrict__ partials, int nb,
                                                                       double* __restrict__ sums) {
  __shared__ double sh[EV_NSUMS][EV_BLOCK / 64];
  const int b = blockIdx.x;
  const float* rows = partials + (long)b * nb * EV_NSUMS;
#pragma unroll
  for (int k = 0; k < EV_NSUMS; ++k) {
    double s = 0.0;
    for (int r = threadIdx.x; r < nb; r += EV_BLOCK) s += (double)rows[(long)r * EV_NSUMS + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < EV_NSUMS) {
    const int k = threadIdx.x;
    sums[(long)b * EV_NSUMS + k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
  }
}

// np.interp(z_dst[col], z_src[col], vals[c][col]) for every column: a workgroup stages `cpb` consecutive columns
// (cpb * NZ <= 256 floats of levels, then of each channel's values) in LDS; a thread owns one query, searches its
// column's levels once and evaluates every channel with numpy's double arithmetic, rounded once to fp32.
__global__ __launch_bounds__(EV_BLOCK) void column_interp_kernel(const float* __restrict__ vals,
                                                                 const float* __restrict__ zs,
                                                                 const float* __restrict__ zd, int C, long ncols, int NZ,
                                                                 int cpb, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float s_z[EV_BLOCK], s_v[EV_BLOCK];
  const int b = blockIdx.y, t = threadIdx.x;
  const int lc = t / NZ, k = t - lc * NZ;
  const long col = (long)blockIdx.x * cpb + lc;
  const bool active = lc < cpb && col < ncols;
  const long plane = ncols * NZ;
  const long off = col * NZ + k;
  float q = 0.f;
  if (active) {
    s_z[t] = zs[(long)b * plane + off];
    q = zd[(long)b * plane + off];
  }
  __syncthreads();
  const float* xp = s_z + lc * NZ;
  int j = 0;
  bool knot = true;  // the result is fp[j] itself: outside the range, on a knot, or in the last interval's end
  const bool nanq = q != q;  // np.interp gives NaN for a NaN query
  if (active && !nanq) {
    if (q > xp[NZ - 1]) {
      j = NZ - 1;
    } else if (q < xp[0]) {
      j = 0;
    } else {
      int lo = 0, hi = NZ - 1;  // largest j with xp[j] <= q
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (xp[mid] <= q) lo = mid; else hi = mid - 1;
      }
      j = lo;
      knot = j == NZ - 1 || xp[j] == q;
    }
  }
  for (int c = 0; c < C; ++c) {
    const long base = ((long)b * C + c) * plane;
    __syncthreads();  // (the previous channel's reads of s_v are done)
    if (active) s_v[t] = vals[base + off];
    __syncthreads();
    if (!active) continue;
    const float* fp = s_v + lc * NZ;
    float res;
    if (nanq) {
      res = q;
    } else if (knot) {
      res = fp[j];
    } else {
      const double x = (double)q, x0 = (double)xp[j], x1 = (double)xp[j + 1];
      const double y0 = (double)fp[j], y1 = (double)fp[j + 1];
      const double slope = (y1 - y0) / (x1 - x0);
      double d = slope * (x - x0) + y0;
      if (d != d) {
        d = slope * (x - x1) + y1;
        if (d != d && y0 == y1) d = y0;
      }
      res = (float)d;
    }
    out[base + off] = res;
  }
}

inline bool tl_geom(TlGeom& g, int Cin, int Xl, int Yl, int NZ, int s) {
  if (Cin < 3 || Xl <= 0 || Yl <= 0 || NZ <= 0 || s <= 0) return false;
  const long X = (long)Xl * s, Y = (long)Yl * s;
  if (X > 32768 || Y > 32768 || X * Y * NZ > 0x7fffffffL) return false;
  g.Cin = Cin;
  g.Xl = Xl;
  g.Yl = Yl;
  g.X = (int)X;
  g.Y = (int)Y;
  g.NZ = NZ;
  g.lplane = (long)Xl * Yl * NZ;
  return true;
}

template <int V>
int launch_trilinear(const float* lr, const TlGeom& g, int B, float* tl, hipStream_t st) {
  const long plane = (long)g.X * g.Y * g.NZ;
  const int nb = (int)((plane / V + EV_BLOCK - 1) / EV_BLOCK);
  const long blocks = (long)B * 3 * nb;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(trilinear_xy_kernel<V>, dim3((unsigned)blocks), dim3(EV_BLOCK), 0, st, lr, g, nb, tl);
  WSR_LAUNCH_CHECK();
  return 0;
}

template <int V, bool FLY>
int launch_metrics(const float* hr, int hr_c, const float* sr, int sr_c, const float* tl, int tl_c, const TlGeom& g,
                   int B, float* partials, double* sums, hipStream_t st) {
  const long pieces = (long)g.X * g.Y * g.NZ / V;
  long nb = (pieces + EV_BLOCK - 1) / EV_BLOCK;
  if (nb > EV_MAX_ROWS) nb = EV_MAX_ROWS;
  hipLaunchKernelGGL((field_metrics_kernel<V, FLY>), dim3((unsigned)nb, (unsigned)B), dim3(EV_BLOCK), 0, st, hr, hr_c,
                     sr, sr_c, tl, tl_c, g, partials);
  WSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(field_metrics_final_kernel, dim3((unsigned)B), dim3(EV_BLOCK), 0, st, partials, (int)nb, sums);
  WSR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int wsr_trilinear_xy(const float* lr, int32_t B, int32_t Cin, int32_t Xl, int32_t Yl, int32_t NZ, int32_t s,
                                float* tl, void* stream) {
  TlGeom g{};
  if (!lr || !tl || B <= 0 || Cin < 3 || Xl <= 0 || Yl <= 0 || NZ <= 0 || s <= 0) return WSR_EINVAL;
  if (!tl_geom(g, Cin, Xl, Yl, NZ, s)) return WSR_EUNSUPPORTED;
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {lr, tl})) {
    case 4: return launch_trilinear<4>(lr, g, B, tl, st);
    case 2: return launch_trilinear<2>(lr, g, B, tl, st);
    default: return launch_trilinear<1>(lr, g, B, tl, st);
  }
}

extern "C" int wsr_field_metrics(const float* hr, int32_t hr_c, const float* sr, int32_t sr_c, const float* tl,
                                 int32_t tl_c, const float* lr, int32_t lr_c, int32_t s, int32_t B, int32_t X, int32_t Y,
                                 int32_t NZ, float* partials, double* sums, void* stream) {
  if (!hr || !sr || !partials || !sums || hr_c < 3 || sr_c < 3 || B <= 0 || X <= 0 || Y <= 0 || NZ <= 0)
    return WSR_EINVAL;
  if ((tl != nullptr) == (lr != nullptr)) return WSR_EINVAL;  // the baseline: a tensor, or LR and s - one of the two
  if (B > 65535) return WSR_EUNSUPPORTED;
  TlGeom g{};
  const hipStream_t st = as_stream(stream);
  if (lr) {
    if (lr_c < 3 || s <= 0 || X % s || Y % s) return WSR_EINVAL;
    if (!tl_geom(g, lr_c, X / s, Y / s, NZ, s)) return WSR_EUNSUPPORTED;
    switch (piece_width(NZ, {hr, sr, lr})) {
      case 4: return launch_metrics<4, true>(hr, hr_c, sr, sr_c, lr, 0, g, B, partials, sums, st);
      case 2: return launch_metrics<2, true>(hr, hr_c, sr, sr_c, lr, 0, g, B, partials, sums, st);
      default: return launch_metrics<1, true>(hr, hr_c, sr, sr_c, lr, 0, g, B, partials, sums, st);
    }
  }
  if (tl_c < 3) return WSR_EINVAL;
  if (X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  switch (piece_width(NZ, {hr, sr, tl})) {
    case 4: return launch_metrics<4, false>(hr, hr_c, sr, sr_c, tl, tl_c, g, B, partials, sums, st);
    case 2: return launch_metrics<2, false>(hr, hr_c, sr, sr_c, tl, tl_c, g, B, partials, sums, st);
    default: return launch_metrics<1, false>(hr, hr_c, sr, sr_c, tl, tl_c, g, B, partials, sums, st);
  }
}

extern "C" int wsr_column_interp(const float* vals, const float* z_src, const float* z_dst, int32_t B, int32_t C,
                                 int64_t ncols, int32_t NZ, float* out, void* stream) {
  if (!vals || !z_src || !z_dst || !out || B <= 0 || C <= 0 || ncols <= 0 || NZ <= 0) return WSR_EINVAL;
  if (NZ > 128 || B > 65535 || ncols * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  const int cpb = EV_BLOCK / NZ;
  const long nb = (ncols + cpb - 1) / cpb;
  if (nb > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(column_interp_kernel, dim3((unsigned)nb, (unsigned)B), dim3(EV_BLOCK), 0, as_stream(stream), vals,
                     z_src, z_dst, C, (long)ncols, NZ, cpb, out);
  WSR_LAUNCH_CHECK();
  return 0;
}
