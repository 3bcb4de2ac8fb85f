// Geometric self-ensemble ([ENSEMBLE]): the eight symmetries of the square applied to a batch, and the reduction of the
// generator's outputs on the transformed copies back to one field.  All tensors fp32 planar (B, C, X, Y, NZ), z innermost.
//
// A member is (k, fx), code k + 4 * fx: k quarter turns as process_data._rotate_wind does them (torch.rot90 in the
// (x, y) plane, the horizontal wind components turning with the grid), then, if fx, a mirror along x with u negated -
// the order of CustomizedDataset.__getitem__.  Its inverse: undo the mirror, then _rotate_wind by (4 - k) % 4.  Both only
// permute (x, y) and flip sign bits, so every output column (.., i, j, 0..NZ) is a contiguous run of NZ floats of ONE
// source column.  Thread layout of data_gather.hip: a workgroup covers a chunk of one output plane, so member, source
// channel and sign are workgroup-uniform; a thread moves V consecutive floats (V | NZ: a piece never straddles two
// columns), consecutive threads move consecutive pieces - stores are fully coalesced, loads are runs of NZ floats.
//
// wsr_ensemble_reduce reads its K source pieces into registers, adds them as the pairwise tree ((m0 + m1) + (m2 + m3)) + ...
// in member order and multiplies by 1 / K (K a power of two: exact), so K identical members give the member back bit for
// bit; the variance is the same tree over (m_k - mean)^2, from the registers.  No atomics, no second pass: two calls give
// the same bits.  Evaluated without contraction, so the mean is the fp32 tree as any IEEE machine evaluates it.
#include "common.h"

namespace {

constexpr int EN_BLOCK = 256;
constexpr int EN_MAXK = WSR_ENSEMBLE_MAX_MEMBERS;

template <int V> using uvec = unsigned int __attribute__((ext_vector_type(V)));
template <int V> using fvec = float __attribute__((ext_vector_type(V)));

struct EnsGeom {
  int B, C, X, Y, NZ;  // the un-transformed tensor; a member with odd k is (Y, X) in (x, y) - X == Y then (host-checked)
  int K, nb, is_vector;
  int code[EN_MAXK];
};

// torch.rot90(t, k, [x, y]): the source (a, b) of output (i, j); P x Q = the SOURCE plane
__device__ __forceinline__ void rot_source(int k, int i, int j, int P, int Q, int& a, int& b) {
  switch (k) {
    case 0: a = i; b = j; break;
    case 1: a = j; b = Q - 1 - i; break;
    case 2: a = P - 1 - i; b = Q - 1 - j; break;
    default: a = P - 1 - j; b = i; break;
  }
}

// _rotate_wind: the source channel and sign bit of horizontal wind component c (0 = u, 1 = v) after k quarter turns
__device__ __forceinline__ void rot_component(int k, int c, int& src, unsigned& sign) {
  src = (k & 1) ? 1 - c : c;
  sign = (c == 0 ? (k == 1 || k == 2) : (k >= 2)) ? 0x80000000u : 0u;
}

template <int V>
__global__ __launch_bounds__(EN_BLOCK) void dihedral_members_kernel(const float* __restrict__ src, EnsGeom g,
                                                                    float* __restrict__ dst) {
  // workgroup -> (member, b, c, chunk)
  const int plane_id = blockIdx.x / g.nb;
  const int chunk = blockIdx.x - plane_id * g.nb;
  const int m = plane_id / (g.B * g.C);
  const int bc = plane_id - m * (g.B * g.C);
  const int b = bc / g.C, c = bc - b * g.C;
  const int k = g.code[m] & 3, fx = g.code[m] >> 2;
  const int Xo = (k & 1) ? g.Y : g.X, Yo = (k & 1) ? g.X : g.Y;  // the member's plane
  int sc = c;
  unsigned sign = 0u;
  if (g.is_vector && c < 2) {
    rot_component(k, c, sc, sign);
    if (fx && c == 0) sign ^= 0x80000000u;
  }
  const long plane = (long)g.X * g.Y * g.NZ;
  const long e = ((long)chunk * EN_BLOCK + threadIdx.x) * V;
  if (e >= plane) return;
  const unsigned eu = (unsigned)e;  // (plane < 2^31: checked on the host)
  const int col = (int)(eu / (unsigned)g.NZ);
  const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
  const int i = col / Yo, j = col - i * Yo;
  const int i1 = fx ? Xo - 1 - i : i;  // undo the mirror, then the rotation
  int a, bb;
  rot_source(k, i1, j, g.X, g.Y, a, bb);
  const float* sp = src + ((long)b * g.C + sc) * plane + ((long)a * g.Y + bb) * g.NZ + zz;
  uvec<V> v = *reinterpret_cast<const uvec<V>*>(sp);
  v ^= sign;
  *reinterpret_cast<uvec<V>*>(dst + (((long)m * g.B + b) * g.C + c) * plane + e) = v;
}

template <int V, int K> __device__ __forceinline__ fvec<V> tree_sum(const fvec<V>* t) {
#pragma clang fp contract(off)
  fvec<V> s[K];
#pragma unroll
  for (int q = 0; q < K; ++q) s[q] = t[q];
#pragma unroll
  for (int n = K; n > 1; n >>= 1) {
#pragma unroll
    for (int q = 0; q < n / 2; ++q) s[q] = s[2 * q] + s[2 * q + 1];
  }
  return s[0];
}

template <int V, int K>
__global__ __launch_bounds__(EN_BLOCK) void ensemble_reduce_kernel(const float* __restrict__ members, EnsGeom g,
                                                                   float* __restrict__ mean, float* __restrict__ var) {
#pragma clang fp contract(off)
  // workgroup -> (b, c, chunk) of the output; c in 0..2
  const int plane_id = blockIdx.x / g.nb;
  const int chunk = blockIdx.x - plane_id * g.nb;
  const int b = plane_id / 3, c = plane_id - b * 3;
  const long plane = (long)g.X * g.Y * g.NZ;
  const long e = ((long)chunk * EN_BLOCK + threadIdx.x) * V;
  if (e >= plane) return;
  const unsigned eu = (unsigned)e;  // (plane < 2^31: checked on the host)
  const int col = (int)(eu / (unsigned)g.NZ);
  const int zz = (int)(eu - (unsigned)col * (unsigned)g.NZ);
  const int i = col / g.Y, j = col - i * g.Y;
  fvec<V> mv[K];
#pragma unroll
  for (int m = 0; m < K; ++m) {
    const int k = g.code[m] & 3, fx = g.code[m] >> 2;
    const int kinv = (4 - k) & 3;
    const int Xm = (k & 1) ? g.Y : g.X, Ym = (k & 1) ? g.X : g.Y;  // the member's plane
    // output = _rotate_wind(unmirror(member), kinv): channel and sign of the rotation, then of the mirror it reads through
    int sc = c;
    unsigned sign = 0u;
    if (c < 2) {
      rot_component(kinv, c, sc, sign);
      if (fx && sc == 0) sign ^= 0x80000000u;
    }
    int a, bb;
    rot_source(kinv, i, j, Xm, Ym, a, bb);
    if (fx) a = Xm - 1 - a;
    const float* sp = members + (((long)m * g.B + b) * 3 + sc) * plane + ((long)a * Ym + bb) * g.NZ + zz;
    uvec<V> v = *reinterpret_cast<const uvec<V>*>(sp);
    v ^= sign;
    mv[m] = __builtin_bit_cast(fvec<V>, v);
  }
  const float inv_k = 1.0f / (float)K;
  const fvec<V> mu = tree_sum<V, K>(mv) * inv_k;
  const long o = ((long)b * 3 + c) * plane + e;
  *reinterpret_cast<fvec<V>*>(mean + o) = mu;
  if (var) {
#pragma unroll
    for (int m = 0; m < K; ++m) {
      const fvec<V> d = mv[m] - mu;
      mv[m] = d * d;
    }
    *reinterpret_cast<fvec<V>*>(var + o) = tree_sum<V, K>(mv) * inv_k;
  }
}

// K in {1, 2, 4, 8}, every code in 0..7, odd quarter turns only on a square plane
inline int fill_geom(EnsGeom& g, const int32_t* codes, int K, int B, int C, int X, int Y, int NZ) {
  if (!codes || (K != 1 && K != 2 && K != 4 && K != 8) || B <= 0 || C <= 0 || X <= 0 || Y <= 0 || NZ <= 0)
    return WSR_EINVAL;
  for (int m = 0; m < K; ++m) {
    if (codes[m] < 0 || codes[m] > 7) return WSR_EINVAL;
    if ((codes[m] & 1) && X != Y) return WSR_EINVAL;
    g.code[m] = codes[m];
  }
  if (X > 32768 || Y > 32768 || (long)X * Y * NZ > 0x7fffffffL) return WSR_EUNSUPPORTED;
  g.B = B;
  g.C = C;
  g.X = X;
  g.Y = Y;
  g.NZ = NZ;
  g.K = K;
  return 0;
}

template <int V>
int launch_members(const float* src, EnsGeom g, float* dst, hipStream_t st) {
  const long plane = (long)g.X * g.Y * g.NZ;
  g.nb = (int)((plane / V + EN_BLOCK - 1) / EN_BLOCK);
  const long blocks = (long)g.K * g.B * g.C * g.nb;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  hipLaunchKernelGGL(dihedral_members_kernel<V>, dim3((unsigned)blocks), dim3(EN_BLOCK), 0, st, src, g, dst);
  WSR_LAUNCH_CHECK();
  return 0;
}

template <int V, int K>
int launch_reduce_k(const float* members, const EnsGeom& g, long blocks, float* mean, float* var, hipStream_t st) {
  hipLaunchKernelGGL((ensemble_reduce_kernel<V, K>), dim3((unsigned)blocks), dim3(EN_BLOCK), 0, st, members, g, mean,
                     var);
  WSR_LAUNCH_CHECK();
  return 0;
}

template <int V>
int launch_reduce(const float* members, EnsGeom g, float* mean, float* var, hipStream_t st) {
  const long plane = (long)g.X * g.Y * g.NZ;
  g.nb = (int)((plane / V + EN_BLOCK - 1) / EN_BLOCK);
  const long blocks = (long)g.B * 3 * g.nb;
  if (blocks > 0x7fffffffL) return WSR_EUNSUPPORTED;
  switch (g.K) {
    case 1: return launch_reduce_k<V, 1>(members, g, blocks, mean, var, st);
    case 2: return launch_reduce_k<V, 2>(members, g, blocks, mean, var, st);
    case 4: return launch_reduce_k<V, 4>(members, g, blocks, mean, var, st);
    default: return launch_reduce_k<V, 8>(members, g, blocks, mean, var, st);
  }
}

}  // namespace

extern "C" int wsr_dihedral_members(const float* src, int32_t B, int32_t C, int32_t X, int32_t Y, int32_t NZ,
                                    const int32_t* codes, int32_t K, int32_t is_vector, float* dst, void* stream) {
  if (!src || !dst) return WSR_EINVAL;
  if (is_vector && C < 2) return WSR_EINVAL;
  EnsGeom g{};
  const int rc = fill_geom(g, codes, K, B, C, X, Y, NZ);
  if (rc) return rc;
  g.is_vector = is_vector ? 1 : 0;
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {src, dst})) {
    case 4: return launch_members<4>(src, g, dst, st);
    case 2: return launch_members<2>(src, g, dst, st);
    default: return launch_members<1>(src, g, dst, st);
  }
}

extern "C" int wsr_ensemble_reduce(const float* members, const int32_t* codes, int32_t K, int32_t B, int32_t X,
                                   int32_t Y, int32_t NZ, float* mean, float* var, void* stream) {
  if (!members || !mean) return WSR_EINVAL;
  EnsGeom g{};
  const int rc = fill_geom(g, codes, K, B, 3, X, Y, NZ);
  if (rc) return rc;
  g.is_vector = 1;
  const hipStream_t st = as_stream(stream);
  switch (piece_width(NZ, {members, mean, var})) {
    case 4: return launch_reduce<4>(members, g, mean, var, st);
    case 2: return launch_reduce<2>(members, g, mean, var, st);
    default: return launch_reduce<1>(members, g, mean, var, st);
  }
}
