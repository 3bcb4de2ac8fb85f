// Runs the filtered kernel of csrc/data_gather.hip (wsr_gather_batch_filtered) block by block on 256 host threads, for
// the address and undefined-behaviour sanitisers, on the shim of tools/host_shim.h with min and max added.  Every buffer
// is a heap allocation of exactly the size the C ABI documents - the store, the descriptor table, the two weight tables
// and the three outputs - so a read outside the store or a table and a write outside an output are reported.  The
// kernel's vector types are clang's.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/degradation_host_check.cpp -o degradation_host_check
//   ./degradation_host_check Cin s S X Y NZ R n_filt [dump.bin]
//
// S = 0: the whole X x Y domain (then the odd rotations are left out unless X == Y).  The batch holds every rotation x
// mirror combination once, at slice origins that touch both ends of the domain.  The weights are a normalised triangle,
// zero outside the slice like degradation.axis_weights; the store is random with negative zeros sprinkled in.  With a
// last argument the operands and results are written as raw arrays - desc (int32), store, wx, wy, lr, hr, z (float32) -
// for a comparison with degradation.degrade_lr and the rotation / mirror code of CustomizedDataset.__getitem__.
#include <algorithm>

#include "host_shim.h"

using std::max;
using std::min;

#include "../gan_sr_wind_field_amd/csrc/data_gather_kernels.h"

namespace {

std::vector<float> triangle_weights(int n, int s, int R) {
  const int rows = (n + s - 1) / s, T = 2 * R + 1;
  std::vector<float> w((size_t)rows * T);
  for (int i = 0; i < rows; ++i) {
    double sum = 0.0;
    for (int d = 0; d < T; ++d) {
      const int pos = s * i + d - R;
      if (pos >= 0 && pos < n) sum += R + 1 - abs(d - R);
    }
    for (int d = 0; d < T; ++d) {
      const int pos = s * i + d - R;
      w[(size_t)i * T + d] = pos >= 0 && pos < n ? (float)((R + 1 - abs(d - R)) / sum) : 0.0f;
    }
  }
  return w;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: %s Cin s S X Y NZ R n_filt [dump.bin]\n", argv[0]);
    return 2;
  }
  const int Cin = atoi(argv[1]), s = atoi(argv[2]), S = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]);
  const int NZ = atoi(argv[6]), R = atoi(argv[7]), n_filt = atoi(argv[8]);
  const int n_samples = 3;
  std::vector<int32_t> desc;
  const int W = S ? S : X, H = S ? S : Y;
  const int x0s[5] = {1, X - W, 5, 0, 13}, y0s[5] = {0, 7, Y - H, 2, 9};
  int m = 0;
  for (int k = 0; k < 4; ++k)
    for (int fx = 0; fx < 2; ++fx)
      for (int fy = 0; fy < 2; ++fy, ++m) {
        if ((k & 1) && W != H) continue;
        const int x0 = S ? std::min(x0s[m % 5], X - W) : 0, y0 = S ? std::min(y0s[(3 * m + 1) % 5], Y - H) : 0;
        const int32_t row[6] = {(5 * m) % n_samples, x0, y0, k, fx, fy};
        desc.insert(desc.end(), row, row + 6);
      }
  const int B = (int)(desc.size() / 6);
  GatherGeom g{};
  if (gb_geom(g, n_samples, B, Cin, s, S, X, Y, NZ, R, n_filt) != 0) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> store((size_t)n_samples * (Cin + 1) * X * Y * NZ);
  for (size_t i = 0; i < store.size(); ++i) store[i] = i % 97 == 0 ? -0.0f : (float)uniform();
  const std::vector<float> wx = triangle_weights(W, s, R), wy = triangle_weights(H, s, R);
  std::vector<float> lr((size_t)B * Cin * g.Wc * g.Hc * NZ, nan), hr((size_t)B * 3 * W * H * NZ, nan);
  std::vector<float> z((size_t)B * W * H * NZ, nan);

  const auto run = [&](auto vtag) {
    constexpr int V = decltype(vtag)::value;
    const long blocks = gb_plan<V>(g);
    launch(GB_BLOCK, (unsigned)blocks, 1, 1, [&] {
      gather_batch_kernel<V, true>(store.data(), desc.data(), wx.data(), wy.data(), g, lr.data(), hr.data(), z.data());
    });
  };
  if (NZ % 4 == 0)
    run(std::integral_constant<int, 4>{});
  else if (NZ % 2 == 0)
    run(std::integral_constant<int, 2>{});
  else
    run(std::integral_constant<int, 1>{});

  size_t bad = 0;  // every output element written, and finite
  for (float v : lr) bad += !isfinite(v);
  for (float v : hr) bad += !isfinite(v);
  for (float v : z) bad += !isfinite(v);
  if (argc > 9) {
    FILE* fp = fopen(argv[9], "wb");
    if (!fp) return 3;
    dump(fp, desc.data(), desc.size());
    dump(fp, store.data(), store.size());
    dump(fp, wx.data(), wx.size());
    dump(fp, wy.data(), wy.size());
    dump(fp, lr.data(), lr.size());
    dump(fp, hr.data(), hr.size());
    dump(fp, z.data(), z.size());
    fclose(fp);
  }
  printf("Cin %d s %d S %d X %d Y %d NZ %d R %d n_filt %d: B %d, %zu unwritten or non-finite outputs\n", Cin, s, S, X, Y,
         NZ, R, n_filt, B, bad);
  return bad ? 1 : 0;
}
