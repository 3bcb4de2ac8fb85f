//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/consistency_loss_host_check.cpp -o consistency_loss_host_check
//   ./consistency_loss_host_check                          (the built-in shapes)
//   ./consistency_loss_host_check B C X Y NZ s gaussian(0|1) sigma
//
// Runs the kernels of csrc/consistency_loss.hip block by block on host threads, for the address and undefined-behaviour
// sanitisers: the shim of tools/host_shim.h (__global__, threadIdx / blockIdx, __syncthreads as a pthread barrier), with
// the LDS strip a heap buffer of exactly the floats the launch asks for (CL_LDS).  Every buffer is a heap allocation of
// exactly the size the C ABI documents - the two fields, the two weight tables, r, the upstream gradient and dsr - so an
// access outside one of them is reported.
//
// The launches are those of wsr_coarse_residual and wsr_coarse_residual_bwd, at every piece width V that divides NZ.  The
// weight tables are built as degradation.axis_weights builds them (float64, rounded once).  r and dsr are filled with NaN
// before the launch.  The program computes both with a plain loop over the definition of consistency_loss.py and exits
// non-zero on any element that differs bit for bit or was not written.
#include "host_shim.h"

#include <string.h>

namespace {
float* g_lds = nullptr;  // the strip of the running launch: exactly its size
}
#define CL_LDS(name) float* const name = g_lds

#include "../gan_sr_wind_field_amd/csrc/consistency_loss_kernels.h"

namespace {

std::vector<double> make_taps(bool gaussian, int s, double sigma) {
  if (!gaussian) {
    const int R = s / 2;
    std::vector<double> t((size_t)2 * R + 1, 1.0);
    if (s % 2 == 0) t.front() = t.back() = 0.5;
    return t;
  }
  const int R = (int)ceil(3.0 * sigma);
  std::vector<double> t((size_t)2 * R + 1);
  for (int d = -R; d <= R; ++d) t[(size_t)(d + R)] = exp(-(double)d * d / (2.0 * sigma * sigma));
  return t;
}

std::vector<float> axis_weights(int n, int s, const std::vector<double>& t) {
  const int K = (int)t.size(), R = (K - 1) / 2, n_out = (n + s - 1) / s;
  std::vector<float> w((size_t)n_out * K);
  for (int i = 0; i < n_out; ++i) {
    double sum = 0.0;
    for (int d = 0; d < K; ++d) {
      const int p = s * i + d - R;
      if (p >= 0 && p < n) sum += t[(size_t)d];
    }
    for (int d = 0; d < K; ++d) {
      const int p = s * i + d - R;
      w[(size_t)i * K + d] = (float)((p >= 0 && p < n ? t[(size_t)d] : 0.0) / sum);
    }
  }
  return w;
}

bool same(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

template <int V>
void run_fwd(const std::vector<float>& hr, const std::vector<float>& sr, int C, const std::vector<float>& wx,
             const std::vector<float>& wy, const ClGeom& g, std::vector<float>& r) {
  std::vector<float> lds((size_t)g.fwd_lds);
  g_lds = lds.data();
  launch(CL_BLOCK, (unsigned)g.njr, (unsigned)g.XL, (unsigned)(3 * g.B),
         [&] { cl_fwd_kernel<V>(hr.data(), C, sr.data(), C, wx.data(), wy.data(), g, r.data()); });
  g_lds = nullptr;
}

template <int V>
void run_bwd(const std::vector<float>& G, int C, const std::vector<float>& wx, const std::vector<float>& wy,
             const ClGeom& g, std::vector<float>& dsr) {
  std::vector<float> lds((size_t)(g.bwd_lds > 0 ? g.bwd_lds : 1));
  g_lds = lds.data();
  launch(CL_BLOCK, (unsigned)g.nyr, (unsigned)g.X, (unsigned)(C * g.B),
         [&] { cl_bwd_kernel<V>(G.data(), wx.data(), wy.data(), g, C, dsr.data()); });
  g_lds = nullptr;
}

// 0: fine
int run(int B, int C, int X, int Y, int NZ, int s, bool gaussian, double sigma) {
  const std::vector<double> t = make_taps(gaussian, s, sigma);
  const int K = (int)t.size(), R = (K - 1) / 2;
  ClGeom g{};
  if (cl_geom(g, s, R, B, X, Y, NZ) != 0 || C < 3) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const std::vector<float> wx = axis_weights(X, s, t), wy = axis_weights(Y, s, t);
  const int XL = g.XL, YL = g.YL;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const size_t vol = (size_t)X * Y * NZ, cvol = (size_t)XL * YL * NZ;
  std::vector<float> hr((size_t)B * C * vol), sr(hr.size()), G((size_t)B * 3 * cvol);
  for (auto& v : hr) v = (float)uniform();
  for (auto& v : sr) v = (float)uniform();
  for (auto& v : G) v = (float)uniform();

  // the definition, forward
  std::vector<float> want_r((size_t)B * 3 * cvol), gx((size_t)Y * NZ);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < XL; ++i) {
        const size_t base = ((size_t)b * C + c) * vol;
        for (int m = 0; m < Y * NZ; ++m) {
          float acc = 0.f;
          for (int d = 0; d < K; ++d) {
            const int x = s * i + d - R;
            if (x < 0 || x >= X) continue;
            const size_t at = base + (size_t)x * Y * NZ + m;
            const float e = sr[at] - hr[at];
            const float p = wx[(size_t)i * K + d] * e;
            acc = acc + p;
          }
          gx[(size_t)m] = acc;
        }
        for (int j = 0; j < YL; ++j)
          for (int z = 0; z < NZ; ++z) {
            float acc = 0.f;
            for (int d = 0; d < K; ++d) {
              const int y = s * j + d - R;
              if (y < 0 || y >= Y) continue;
              const float p = wy[(size_t)j * K + d] * gx[(size_t)y * NZ + z];
              acc = acc + p;
            }
            want_r[((((size_t)b * 3 + c) * XL + i) * YL + j) * NZ + z] = acc;
          }
      }
  // the definition, backward
  std::vector<float> want_d((size_t)B * C * vol, 0.f), tx((size_t)YL * NZ);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < 3; ++c)
      for (int x = 0; x < X; ++x) {
        for (int j = 0; j < YL; ++j)
          for (int z = 0; z < NZ; ++z) {
            float acc = 0.f;
            for (int i = 0; i < XL; ++i) {
              const int d = x - s * i + R;
              if (d < 0 || d > 2 * R) continue;
              const float p = wx[(size_t)i * K + d] * G[((((size_t)b * 3 + c) * XL + i) * YL + j) * NZ + z];
              acc = acc + p;
            }
            tx[(size_t)j * NZ + z] = acc;
          }
        for (int y = 0; y < Y; ++y)
          for (int z = 0; z < NZ; ++z) {
            float acc = 0.f;
            for (int j = 0; j < YL; ++j) {
              const int d = y - s * j + R;
              if (d < 0 || d > 2 * R) continue;
              const float p = wy[(size_t)j * K + d] * tx[(size_t)j * NZ + z];
              acc = acc + p;
            }
            want_d[((((size_t)b * C + c) * X + x) * Y + y) * NZ + z] = acc;
          }
      }

  int rc = 0;
  for (int V = 4; V >= 1; V >>= 1) {
    if (NZ % V) continue;
    std::vector<float> r(want_r.size(), nan), dsr(want_d.size(), nan);
    if (V == 4) run_fwd<4>(hr, sr, C, wx, wy, g, r), run_bwd<4>(G, C, wx, wy, g, dsr);
    if (V == 2) run_fwd<2>(hr, sr, C, wx, wy, g, r), run_bwd<2>(G, C, wx, wy, g, dsr);
    if (V == 1) run_fwd<1>(hr, sr, C, wx, wy, g, r), run_bwd<1>(G, C, wx, wy, g, dsr);
    size_t rdiffer = 0, ddiffer = 0, unwritten = 0;
    for (size_t k = 0; k < r.size(); ++k) rdiffer += !same(r[k], want_r[k]), unwritten += std::isnan(r[k]);
    for (size_t k = 0; k < dsr.size(); ++k) ddiffer += !same(dsr[k], want_d[k]), unwritten += std::isnan(dsr[k]);
    printf("B %d C %d X %d Y %d NZ %d s %d %s R %d V %d: forward %d rows x %d runs, %d floats of LDS; backward %d rows x %d "
           "runs, %d floats of LDS; %zu of %zu residuals differ, %zu of %zu gradient elements differ, %zu unwritten\n",
           B, C, X, Y, NZ, s, gaussian ? "gaussian" : "box", R, V, g.TJ, g.njr, g.fwd_lds, g.TY, g.nyr, g.bwd_lds, rdiffer,
           r.size(), ddiffer, dsr.size(), unwritten);
    rc |= rdiffer || ddiffer || unwritten ? 1 : 0;
  }
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 9)
    return run(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]) != 0,
               atof(argv[8]));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [B C X Y NZ s gaussian(0|1) sigma]\n", argv[0]);
    return 2;
  }
  // the shapes of tests/test_consistency_loss_gpu.py: odd extents and half end taps; the reference's patch with a surplus
  // channel; R = 6 with the widest level count; odd s; R = 30, larger than the domain; several workgroups per plane; and
  // one more with two runs per row in both launches
  struct Case {
    int B, C, X, Y, NZ, s;
    bool gaussian;
    double sigma;
  };
  const Case cases[] = {{2, 3, 5, 7, 3, 2, false, 0.0},  {1, 4, 16, 16, 10, 4, false, 0.0}, {1, 3, 8, 8, 128, 4, true, 2.0},
                        {2, 3, 6, 5, 4, 3, false, 0.0},  {1, 3, 16, 12, 2, 8, true, 10.0},  {1, 3, 64, 64, 10, 4, false, 0.0},
                        {1, 3, 12, 40, 128, 4, false, 0.0}};
  int rc = 0;
  for (const auto& c : cases) rc |= run(c.B, c.C, c.X, c.Y, c.NZ, c.s, c.gaussian, c.sigma);
  return rc;
}
