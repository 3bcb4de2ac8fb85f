// The kernel of csrc/data_gather.hip, kept in a header of its own so that a host program can run it block by block on
// threads under the address and undefined-behaviour sanitisers (tools/degradation_host_check.cpp, on the shim of
// tools/host_shim.h with min and max added).  Nothing here needs more of HIP than __global__, threadIdx / blockIdx, min,
// max and clang's vector types.  No barriers, no LDS.
//
// gather_batch_kernel<V, FILTERED>: a thread moves V consecutive floats of one output column.  FILTERED = false is the
// plain batch gather (wsr_gather_batch): every plane is a copy with a sign.  FILTERED = true (wsr_gather_batch_filtered,
// [DEGRADATION]) also evaluates the anti-aliasing filter on the LR channels below n_filt; its HR and Z planes and the LR
// channels that stay point-sampled go through the statements of the plain gather.  With FILTERED = false no plane is
// filtered at compile time: gb_filtered and every use of wx, wy, R and n_filt are compiled out.
#pragma once

#pragma clang fp contract(off)

namespace {

constexpr int GB_BLOCK = 256;
constexpr int GB_MAX_R = WSR_DEGRADE_MAX_R;

template <int V> using uvec = unsigned int __attribute__((ext_vector_type(V)));
template <int V> using fvec = float __attribute__((ext_vector_type(V)));

struct GatherGeom {
  int B, Cin, s, W, H, Wc, Hc, X, Y, NZ;  // W x H: slice (pre-rotation) on the HR grid; Wc x Hc: the same, coarsened
  int nb_lr, nb_hr;                       // workgroups per LR / per HR-or-Z plane
  int R, n_filt;                          // tap radius; LR channels [0, n_filt) are filtered (both 0 in the plain gather)
  long n_samples;
};

// the geometry of a call from the arguments of wsr_gather_batch (R = n_filt = 0) or wsr_gather_batch_filtered: 0, or the
// error the export returns
inline int gb_geom(GatherGeom& g, long n_samples, int B, int Cin, int s, int S, int X, int Y, int NZ, int R, int n_filt) {
  if (n_samples <= 0 || B <= 0 || Cin < 3 || s <= 0 || S < 0 || X <= 0 || Y <= 0 || NZ <= 0 || S > X || S > Y)
    return WSR_EINVAL;
  if (R < 0 || R > GB_MAX_R || n_filt < 0 || n_filt > Cin) return WSR_EINVAL;
  g.B = B;
  g.Cin = Cin;
  g.s = s;
  g.W = S ? S : X;
  g.H = S ? S : Y;
  g.Wc = (g.W + s - 1) / s;
  g.Hc = (g.H + s - 1) / s;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  g.R = R;
  g.n_filt = n_filt;
  g.n_samples = n_samples;
  if ((long)g.W * g.H * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  return 0;
}

// workgroups of the launch at V floats per thread (V | NZ); fills the per-plane counts
template <int V> inline long gb_plan(GatherGeom& g) {
  const long lr_plane = (long)g.Wc * g.Hc * g.NZ, hr_plane = (long)g.W * g.H * g.NZ;
  g.nb_lr = (int)((lr_plane / V + GB_BLOCK - 1) / GB_BLOCK);
  g.nb_hr = (int)((hr_plane / V + GB_BLOCK - 1) / GB_BLOCK);
  return (long)g.B * g.Cin * g.nb_lr + (long)g.B * 4 * g.nb_hr;
}

// V consecutive levels of a filtered LR plane at the sample point (s a, s bb) of the pre-rotation slice whose origin in
// the store is (x0, y0): the x pass then the y pass, taps ascending from +0.0f, every product and sum rounded to fp32
template <int V>
__device__ __forceinline__ uvec<V> gb_filtered(const float* __restrict__ chan, const float* __restrict__ wx,
                                               const float* __restrict__ wy, const GatherGeom& g, int a, int bb, int x0,
                                               int y0, int zz) {
  const long row = (long)g.Y * g.NZ;  // floats per store x-plane
  const int R = g.R, T = 2 * R + 1;
  const int xc = g.s * a, yc = g.s * bb;  // the sample point in the slice: xc < W, yc < H
  // taps inside the slice: 0 <= xc + dx - R < W, 0 <= yc + dy - R < H (never empty: the centre tap is inside)
  const int dx0 = max(0, R - xc), dx1 = min(T, g.W + R - xc);
  const int dy0 = max(0, R - yc), dy1 = min(T, g.H + R - yc);
  const float* wxa = wx + (long)a * T;
  const float* wyb = wy + (long)bb * T;
  const long xt = x0 + xc - R, yt = y0 + yc - R;  // store coordinates of tap (0, 0); may lie outside, never read there
  fvec<V> acc = 0.0f;
  for (int dy = dy0; dy < dy1; ++dy) {
    const float* p = chan + (yt + dy) * g.NZ + zz;
    fvec<V> gx = 0.0f;
    for (int dx = dx0; dx < dx1; ++dx) {
      const fvec<V> f = *reinterpret_cast<const fvec<V>*>(p + (xt + dx) * row);
      const fvec<V> prod = wxa[dx] * f;
      gx = gx + prod;
    }
    const fvec<V> prod = wyb[dy] * gx;
    acc = acc + prod;
  }
  return __builtin_bit_cast(uvec<V>, acc);
}

// wx, wy: read with FILTERED only
template <int V, bool FILTERED>
__global__ __launch_bounds__(GB_BLOCK) void gather_batch_kernel(const float* __restrict__ store,
                                                                const int* __restrict__ desc,
                                                                const float* __restrict__ wx,
                                                                const float* __restrict__ wy, GatherGeom g,
                                                                float* __restrict__ lr, float* __restrict__ hr,
                                                                float* __restrict__ zo) {
  // workgroup -> (plane, chunk): the B*Cin LR planes first, then B*4 planes of HR channels 0..2 and Z
  int blk = blockIdx.x;
  const int lr_blocks = g.B * g.Cin * g.nb_lr;
  const bool is_lr = blk < lr_blocks;
  int b, c, chunk;
  if (is_lr) {
    const int plane = blk / g.nb_lr;
    chunk = blk - plane * g.nb_lr;
    b = plane / g.Cin;
    c = plane - b * g.Cin;
  } else {
    blk -= lr_blocks;
    const int plane = blk / g.nb_hr;
    chunk = blk - plane * g.nb_hr;
    b = plane >> 2;
    c = plane & 3;  // 3 = Z
  }
  const int* d = desc + 6 * b;
  const int n = d[0], x0 = d[1], y0 = d[2], k = d[3], fx = d[4], fy = d[5];
  if (n < 0 || n >= g.n_samples || k < 0 || k > 3 || x0 < 0 || y0 < 0 || x0 + g.W > g.X || y0 + g.H > g.Y ||
      ((k & 1) && g.W != g.H))
    return;  // (the host validates descriptors; this keeps a bad one from reading outside the store)

  const int sc = is_lr ? g.s : 1;
  const int P = is_lr ? g.Wc : g.W, Q = is_lr ? g.Hc : g.H;  // output plane = pre-rotation plane (square if k odd)
  // rot90 moves u into -v ... (_rotate_wind), then each mirror negates its component
  int src = c;
  unsigned sign = 0u;
  if (!is_lr && c == 3) {
    src = g.Cin;
  } else if (c == 0) {
    src = (k & 1) ? 1 : 0;
    sign = ((k == 1 || k == 2) ^ (fx != 0)) ? 0x80000000u : 0u;
  } else if (c == 1) {
    src = (k & 1) ? 0 : 1;
    sign = ((k >= 2) ^ (fy != 0)) ? 0x80000000u : 0u;
  }
  const long plane_elems = (long)P * Q * g.NZ;
  const long e = ((long)chunk * GB_BLOCK + threadIdx.x) * V;
  if (e >= plane_elems) return;
  const int col = (int)(e / g.NZ);
  const int zz = (int)(e - (long)col * g.NZ);
  const int i = col / Q, j = col - i * Q;
  const int i1 = fx ? P - 1 - i : i, j1 = fy ? Q - 1 - j : j;  // undo the mirrors ...
  int a, bb;                                                   // ... and the rotation: torch.rot90(t, k, [1, 2])
  switch (k) {
    case 0: a = i1; bb = j1; break;
    case 1: a = j1; bb = Q - 1 - i1; break;
    case 2: a = P - 1 - i1; bb = Q - 1 - j1; break;
    default: a = P - 1 - j1; bb = i1; break;
  }
  const long row = (long)g.Y * g.NZ;  // floats per store x-plane
  const float* chan = store + ((long)n * (g.Cin + 1) + src) * g.X * row;
  float* dp;
  if (is_lr)
    dp = lr + ((long)b * g.Cin + c) * plane_elems;
  else if (c < 3)
    dp = hr + ((long)b * 3 + c) * plane_elems;
  else
    dp = zo + (long)b * plane_elems;

  bool filtered = false;  // (workgroup-uniform; the filter belongs to the pre-rotation channel the plane reads)
  if constexpr (FILTERED) filtered = is_lr && src < g.n_filt;
  uvec<V> v;
  if (filtered) {
    v = gb_filtered<V>(chan, wx, wy, g, a, bb, x0, y0, zz);
  } else {
    const long xs = x0 + (long)sc * a, ys = y0 + (long)sc * bb;
    v = *reinterpret_cast<const uvec<V>*>(chan + xs * row + ys * g.NZ + zz);
  }
  v ^= sign;
  *reinterpret_cast<uvec<V>*>(dp + e) = v;
}

}  // namespace
