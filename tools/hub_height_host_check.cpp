//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/hub_height_host_check.cpp -o hub_height_host_check
//   ./hub_height_host_check B X Y NZ hr_c sr_c tl_c nh log_mode with_cols      (tl_c 0: no baseline; nh heights 1 .. 8)
//
// Runs the two kernels of csrc/hub_height.hip block by block on host threads, for the address and undefined-behaviour
// sanitisers: the shim of tools/host_shim.h (__global__, __shared__ as a static array, one block at a time, threadIdx /
// blockIdx, __syncthreads as a pthread barrier) with the NaN flag of a column stored atomically (several threads store
// the same 1).  Every buffer is a heap allocation of exactly the size the C ABI documents - the three fields, the
// altitudes, the terrain, the workspace, the sums and the planes - so an access outside one of them is reported; the LDS
// arrays are statics of the kernels' own sizes.
//
// The launches are those of wsr_hub_height with UVW_MAX 32, the heights 10, 50, 100, 150, 200, ... m and the default
// power curve of [HUB_HEIGHT].  The terrain is smooth in 0 .. 400 m (multiples of 0.25 m), the columns reach 120 .. 600 m
// above ground from 2 m with quadratically stretched levels, the fields are random around a logarithmic profile, the
// surplus channels NaN.  The special columns of the tests are planted at the first and the last column, on both sides
// of the first staging boundary and at every fifth column: a height exactly on a level and on the top level, the top
// or the lowest level one fp32 step on either side of a height, a column that begins above two heights, a lowest level
// at and below the ground, a NaN altitude at the lowest and at an inner level.  The program computes the same
// quantities with a plain loop over the definition of hub_height.py (the interval by a linear scan, the same fp32
// roundings per column, double sums) and exits non-zero when a plane element or a count differs, when a sum is
// further away than 16 sqrt(n) 2^-24 times the sum of its terms' magnitudes, or when a sum of the absent baseline is not
// zero.
#include "host_shim.h"

#include <string.h>

#define HH_FLAG_SET(p) __atomic_store_n((p), 1, __ATOMIC_RELAXED)

#include "../gan_sr_wind_field_amd/csrc/hub_height_kernels.h"

namespace {

constexpr int KINDS = 11;

// the heights above ground of a special column (levels 0.25 m apart, or spread over lo .. hi); true: its terrain is 0,
// so that the altitude is the height itself, bit for bit
bool special_column(int kind, float q, int NZ, float* h) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const int m = NZ / 2;
  float step = floorf(q / (2.f * (m + 1)) * 4.f) / 4.f;
  if (step < 0.25f) step = 0.25f;
  auto spread = [&](float lo, float hi) {
    for (int k = 0; k < NZ; ++k) h[k] = lo + (hi - lo) * (float)k / (float)(NZ - 1);
  };
  switch (kind) {
    case 0: for (int k = 0; k < NZ; ++k) h[k] = q + (float)(k - m) * step; return false;        // on level m
    case 1: for (int k = 0; k < NZ; ++k) h[k] = q - (float)(NZ - 1 - k) * step; return false;   // on the top level
    case 2: spread(1.f, q), h[NZ - 1] = nextafterf(q, 0.f); return true;                         // the top one step below
    case 3: spread(1.f, q), h[NZ - 1] = nextafterf(q, 1e9f); return true;                        // ... one step above
    case 4: spread(q, 4.f * q), h[0] = nextafterf(q, 1e9f); return true;                         // the bottom one step above
    case 5: spread(q, 4.f * q), h[0] = nextafterf(q, 0.f); return true;                          // ... one step below
    case 6: spread(60.f, 500.f); return false;                                                   // begins above 10 and 50 m
    case 7: spread(0.f, 400.f); return false;                                                    // the lowest level on the ground
    case 8: spread(-1.f, 400.f); return false;                                                   // ... below it
    case 9: spread(2.f, 400.f), h[0] = nan; return true;
    default: spread(2.f, 400.f), h[NZ > 2 ? NZ / 2 : 1] = nan; return true;
  }
}

float curve_plain(float V, const float* cv, const float* cp, int nk) {  // np.interp
  if (V != V) return V;
  if (V <= cv[0]) return cp[0];
  if (V >= cv[nk - 1]) return cp[nk - 1];
  int i = 0;
  while (!(cv[i] <= V && V < cv[i + 1])) ++i;
  const double slope = ((double)cp[i + 1] - (double)cp[i]) / ((double)cv[i + 1] - (double)cv[i]);
  return (float)(slope * ((double)V - (double)cv[i]) + (double)cp[i]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s B X Y NZ hr_c sr_c tl_c nh log_mode with_cols\n", argv[0]);
    return 2;
  }
  const int B = atoi(argv[1]), X = atoi(argv[2]), Y = atoi(argv[3]), NZ = atoi(argv[4]);
  const int chan[3] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
  const int nh = atoi(argv[8]), log_mode = atoi(argv[9]), with_cols = atoi(argv[10]);
  const float heights[HH_MAX_NH] = {10.f, 50.f, 100.f, 150.f, 200.f, 300.f, 400.f, 500.f};
  const int nk = 12;
  const double uvw = 32.0;
  float cv[nk], cp[nk];
  for (int k = 0; k < nk; ++k) {
    const double v = k < 10 ? 3.0 + k : (k == 10 ? 25.0 : 26.0);
    cv[k] = (float)(v / uvw);
    cp[k] = (float)(k == 0 || k == 11 ? 0.0 : (k == 10 ? 1.0 : (v * v * v - 27.0) / (1728.0 - 27.0)));
  }
  HhGeom g{};
  if (hh_geom(g, B, X, Y, NZ, heights, nh, cv, nk, log_mode) != 0 || chan[0] < 3 || chan[1] < 3 ||
      (chan[2] != 0 && chan[2] < 3)) {
    fprintf(stderr, "refused\n");
    return 2;
  }
  const int nsrc = chan[2] ? 3 : 2;
  const int ncols = X * Y;
  const size_t vol = (size_t)ncols * NZ;
  const float nan = std::numeric_limits<float>::quiet_NaN();

  // exact-size heap buffers; the surplus channels hold NaN and are never read
  std::vector<float> terrain((size_t)ncols), z((size_t)B * vol);
  for (int i = 0; i < X; ++i)
    for (int j = 0; j < Y; ++j) {
      const double t = 200.0 + 200.0 * sin(6.2831853 * (1.3 * i / X + 0.2)) * cos(6.2831853 * (0.9 * j / Y + 0.1));
      terrain[(size_t)i * Y + j] = (float)(floor(t * 4.0) / 4.0);
    }
  std::vector<float> hcol((size_t)NZ);
  std::vector<std::vector<float>> f((size_t)nsrc);
  for (int s = 0; s < nsrc; ++s) f[s].assign((size_t)B * chan[s] * vol, nan);
  const int marks[4] = {0, g.cps - 1, g.cps, ncols - 1};
  auto kind_of = [&](int b, int c) {  // the special column planted at column c of sample b, -1: none
    int kind = c % 5 == 0 ? (c / 5 + b) % KINDS : -1;
    for (int i = 0; i < 4; ++i)
      if (c == marks[i]) kind = (b * 4 + i + (c == 0 ? 0 : 3)) % KINDS;
    return kind;
  };
  auto height_of = [&](int b, int c) { return heights[(c + b) % (nh < 2 ? 1 : 2)]; };
  for (int b = 0; b < B; ++b)  // (one terrain for all samples)
    for (int c = 0; c < ncols; ++c)
      if (kind_of(b, c) >= 0 && special_column(kind_of(b, c), height_of(b, c), NZ, hcol.data())) terrain[c] = 0.f;
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < ncols; ++c) {
      const int kind = kind_of(b, c);
      if (kind >= 0) {
        special_column(kind, height_of(b, c), NZ, hcol.data());
      } else {
        const double top = 360.0 + 240.0 * uniform();
        for (int k = 0; k < NZ; ++k) hcol[k] = (float)(2.0 + (top - 2.0) * ((double)k / (NZ - 1)) * ((double)k / (NZ - 1)));
      }
      for (int k = 0; k < NZ; ++k) {
        z[(size_t)b * vol + (size_t)c * NZ + k] = terrain[c] + hcol[k];
        const double hh = hcol[k] == hcol[k] && hcol[k] > 0.05f ? hcol[k] : 0.06;
        const double prof = 0.3 * log(hh / 0.05) / log(600.0 / 0.05);
        for (int s = 0; s < nsrc; ++s) {
          const double dir = 0.6 + 0.2 * s + 0.3 * uniform();
          f[s][((size_t)b * chan[s] + 0) * vol + (size_t)c * NZ + k] = (float)(prof * cos(dir) + 0.03 * uniform());
          f[s][((size_t)b * chan[s] + 1) * vol + (size_t)c * NZ + k] = (float)(prof * sin(dir) + 0.03 * uniform());
        }
      }
    }

  HhTables tab{};
  for (int k = 0; k < nh; ++k) tab.q[k] = heights[k];
  for (int k = 0; k < nk; ++k) tab.cv[k] = cv[k], tab.cp[k] = cp[k];
  const size_t n_ws = (size_t)hh_workspace_floats(g, B), n_out = (size_t)B * nh * HH_NS;
  const size_t n_cols = (size_t)B * nh * HH_PLANES * ncols;
  std::vector<float> ws(n_ws, nan), cols(with_cols ? n_cols : 0, nan);
  std::vector<double> out(n_out, (double)nan);
  launch(HH_BLOCK, (unsigned)g.nb, (unsigned)B, 1, [&] {
    hub_height_kernel(f[0].data(), chan[0], f[1].data(), chan[1], nsrc == 3 ? f[2].data() : nullptr, chan[2], z.data(),
                      terrain.data(), tab, g, ws.data(), with_cols ? cols.data() : nullptr);
  });
  const int items = nh * HH_NS;
  launch(HH_FBLOCK, (unsigned)((items + 63) / 64), (unsigned)B, 1,
         [&] { hub_height_final_kernel(ws.data(), g.nb, items, out.data()); });

  // the definition, column by column
  std::vector<double> want(n_out, 0.0), mag(n_out, 0.0);
  std::vector<float> wcols(n_cols, 0.f);
  size_t n_valid_total = 0, n_invalid_total = 0;
  for (int b = 0; b < B; ++b)
    for (int qi = 0; qi < nh; ++qi)
      for (int c = 0; c < ncols; ++c) {
        const float q = heights[qi];
        bool valid = true, any_nan = false;
        for (int k = 0; k < NZ; ++k) {
          hcol[k] = z[(size_t)b * vol + (size_t)c * NZ + k] - terrain[c];
          any_nan = any_nan || hcol[k] != hcol[k];
        }
        valid = hcol[0] <= q && q <= hcol[NZ - 1] && !any_nan && (!log_mode || hcol[0] > 0.f);
        float V[3] = {0, 0, 0}, P[3] = {0, 0, 0}, cc[6] = {0, 0, 0, 0, 0, 0};
        if (valid) {
          int j = 0;
          for (int k = 0; k < NZ; ++k)
            if (hcol[k] <= q) j = k;
          double w = 0.0;
          const int j1 = j < NZ - 1 ? j + 1 : j;
          if (j < NZ - 1)
            w = log_mode ? log((double)q / (double)hcol[j]) / log((double)hcol[j1] / (double)hcol[j])
                         : ((double)q - (double)hcol[j]) / ((double)hcol[j1] - (double)hcol[j]);
          for (int s = 0; s < nsrc; ++s) {
            for (int d = 0; d < 2; ++d) {
              const float* p = f[s].data() + ((size_t)b * chan[s] + d) * vol + (size_t)c * NZ;
              cc[2 * s + d] = (float)((double)p[j] + w * ((double)p[j1] - (double)p[j]));
            }
            const float uu = cc[2 * s] * cc[2 * s], vv = cc[2 * s + 1] * cc[2 * s + 1];
            V[s] = sqrtf(uu + vv);
            P[s] = curve_plain(V[s], cv, cp, nk);
          }
          double term[HH_NS] = {0};
          term[0] = 1;
          for (int s = 0; s < nsrc; ++s) {
            term[1 + s] = V[s], term[8 + s] = (V[s] * V[s]) * V[s], term[11 + s] = P[s];
            if (s) {
              const float dv = V[s] - V[0], dp = P[s] - P[0];
              const float cr = fabsf(cc[0] * cc[2 * s + 1] - cc[1] * cc[2 * s]), dt = cc[0] * cc[2 * s] + cc[1] * cc[2 * s + 1];
              const float ang = (cr == 0.f && dt == 0.f) ? 0.f : atan2f(cr, dt);
              term[3 + s] = fabsf(dv), term[5 + s] = dv * dv, term[13 + s] = fabsf(dp), term[15 + s] = V[0] * ang;
            }
          }
          for (int k = 0; k < HH_NS; ++k) {
            want[((size_t)b * nh + qi) * HH_NS + k] += term[k];
            mag[((size_t)b * nh + qi) * HH_NS + k] += fabs(term[k]);
          }
        }
        (valid ? n_valid_total : n_invalid_total) += 1;
        float* o = wcols.data() + (((size_t)b * nh + qi) * HH_PLANES) * ncols + c;
        for (int s = 0; s < 3; ++s) o[(size_t)s * ncols] = V[s], o[(size_t)(3 + s) * ncols] = P[s];
        o[(size_t)6 * ncols] = valid ? 1.f : 0.f;
      }
  size_t bad_sums = 0, bad_cols = 0;
  double worst = 0.0;
  for (size_t i = 0; i < n_out; ++i) {
    const int k = (int)(i % HH_NS);
    const double n = want[i - k];
    const double bound = k == 0 ? 0.0 : 16.0 * sqrt(n > 1 ? n : 1) * ldexp(1.0, -24) * mag[i] + ldexp(1.0, -100);
    const double err = fabs(out[i] - want[i]);
    if (!(err <= bound)) {
      if (bad_sums++ < 8) fprintf(stderr, "sum %zu (k = %d): got %.17g want %.17g bound %.3g\n", i, k, out[i], want[i], bound);
    } else if (bound > 0 && mag[i] > 0) {
      worst = err / bound > worst ? err / bound : worst;
    }
  }
  if (with_cols)
    for (size_t i = 0; i < n_cols; ++i)
      if (memcmp(&cols[i], &wcols[i], sizeof(float)) != 0 && !(cols[i] != cols[i] && wcols[i] != wcols[i])) {
        if (bad_cols++ < 8) fprintf(stderr, "plane element %zu: got %.9g want %.9g\n", i, cols[i], wcols[i]);
      }
  printf("B %d X %d Y %d NZ %d channels %d %d %d heights %d %s%s: %d columns per chunk, %d x %d workgroups, %zu valid and "
         "%zu invalid (column, height) pairs, %zu of %zu sums outside the bound (worst error / bound %.3g), %zu plane "
         "elements differ\n", B, X, Y, NZ, chan[0], chan[1], chan[2], nh, log_mode ? "log" : "linear",
         with_cols ? " with planes" : "", g.cps, g.nb, B, n_valid_total, n_invalid_total, bad_sums, n_out, worst, bad_cols);
  return bad_sums || bad_cols || n_valid_total == 0 || n_invalid_total == 0 ? 1 : 0;
}
