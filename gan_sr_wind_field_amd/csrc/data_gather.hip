// One training batch out of the device-resident store (device_data.py): the slice / coarsen / rot90 / mirror
// augmentation of CustomizedDataset.__getitem__ as a gather.  Rotation and mirrors only permute (x, y), so every
// output column (b, c, i, j, 0..NZ) is a contiguous run of NZ floats from ONE store column, copied or with its sign
// flipped.  Each workgroup covers a chunk of one output plane (b, c): the plane's descriptor, source channel, sign and
// index map are workgroup-uniform; a thread moves V consecutive floats (V | NZ, so a piece never straddles two
// columns), consecutive threads move consecutive pieces: stores are fully coalesced, loads are contiguous runs of NZ
// floats.  No arithmetic on the values besides the sign bit, which keeps the batch bit-identical to the CPU path.
#include "common.h"

namespace {

constexpr int GB_BLOCK = 256;

template <int V> using uvec = unsigned int __attribute__((ext_vector_type(V)));

struct GatherGeom {
  int B, Cin, s, W, H, Wc, Hc, X, Y, NZ;  // W x H: slice (pre-rotation) on the HR grid; Wc x Hc: the same, coarsened
  int nb_lr, nb_hr;                       // workgroups per LR / per HR-or-Z plane
  long n_samples;
};

template <int V>
__global__ __launch_bounds__(GB_BLOCK) void gather_batch_kernel(const float* __restrict__ store,
                                                                const int* __restrict__ desc, GatherGeom g,
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
  const long xs = x0 + (long)sc * a, ys = y0 + (long)sc * bb;
  const float* sp = store + (((long)n * (g.Cin + 1) + src) * g.X + xs) * ((long)g.Y * g.NZ) + ys * g.NZ + zz;
  float* dp;
  if (is_lr)
    dp = lr + ((long)b * g.Cin + c) * plane_elems;
  else if (c < 3)
    dp = hr + ((long)b * 3 + c) * plane_elems;
  else
    dp = zo + (long)b * plane_elems;
  uvec<V> v = *reinterpret_cast<const uvec<V>*>(sp);
  v ^= sign;
  *reinterpret_cast<uvec<V>*>(dp + e) = v;
}

template <int V>
int launch(const float* store, const int32_t* desc, GatherGeom g, float* lr, float* hr, float* z, hipStream_t st) {
  const long lr_plane = (long)g.Wc * g.Hc * g.NZ, hr_plane = (long)g.W * g.H * g.NZ;
  g.nb_lr = (int)((lr_plane / V + GB_BLOCK - 1) / GB_BLOCK);
  g.nb_hr = (int)((hr_plane / V + GB_BLOCK - 1) / GB_BLOCK);
  const long blocks = (long)g.B * g.Cin * g.nb_lr + (long)g.B * 4 * g.nb_hr;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(gather_batch_kernel<V>, dim3((unsigned)blocks), dim3(GB_BLOCK), 0, st, store, desc, g, lr, hr, z);
  WSR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int wsr_gather_batch(const float* store, int64_t n_samples, const int32_t* desc, int32_t B, int32_t Cin,
                                int32_t s, int32_t S, int32_t X, int32_t Y, int32_t NZ, float* lr, float* hr, float* z,
                                void* stream) {
  if (!store || !desc || !lr || !hr || !z || n_samples <= 0 || B <= 0 || Cin < 3 || s <= 0 || S < 0 || X <= 0 ||
      Y <= 0 || NZ <= 0 || S > X || S > Y)
    return WSR_EINVAL;
  GatherGeom g{};
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
  g.n_samples = n_samples;
  if ((long)g.W * g.H * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  const hipStream_t st = as_stream(stream);
  if (NZ % 4 == 0) return launch<4>(store, desc, g, lr, hr, z, st);
  if (NZ % 2 == 0) return launch<2>(store, desc, g, lr, hr, z, st);
  return launch<1>(store, desc, g, lr, hr, z, st);
}
