// tests/test_margins_kernel_on_host.py: csrc/hmpc_margins.h -- everything of the margins kernel behind the assembly, and the penalty kernel --
// compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop: h = 1, 5, 10, 20 and NC = 2, 3;
// leg-steps in swing (gait byte 0, and a cap of 1e-4f: below the double literal of the stance rule), all legs in swing, a NaN force, equal
// minima in two rows (small-integer data and a repeated step: the lowest index wins), Fz <= 0 (no friction headroom fraction); then the
// penalty: NaN floors, NaN summaries, no penalty_in, in place.  Everything is compared as bit patterns.
#include "hmpc_margins.h"
#include <cmath>
#include <cstdio>
#include <random>

template <int NC>
__global__ void margins_test_kernel(const float *Fc, const float *u, const unsigned char *gait, const float *cap, int h, double *slack_out,
                                    double *summary, int32_t *where) {
  __shared__ double slack[10 * NC * 20];
  __shared__ hmpc::MarginMin wave_min[hmpc::MARGINS_WAVES][hmpc::MARGIN_CLASSES];
  hmpc::margins_of_instance<NC, hmpc::MARGINS_NT>(Fc, u, gait, cap, h, slack, wave_min, slack_out, summary, where);
}

static bool in_stance(float cap, unsigned char g) {
  const double ub = (double)(cap * (float)g);
  return !(ub < 0.0001 && ub > -.0001);
}

template <int NC>
static int run(std::mt19937 &rng) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  int bad = 0;
  for (int h : {1, 5, 10, 20})
    for (int variant = 0; variant < 6; ++variant) {
      std::vector<float> Fc(C8 * U), u(U * h), cap(NC, 500.f);
      std::vector<unsigned char> gait(NC * h);
      std::vector<double> slack(10 * NC * h, -7.0), want(10 * NC * h), summary(6, -7.0);
      std::vector<int32_t> where(6, -7);
      const bool small = variant == 3;  // small integers: many equal values
      for (auto &v : Fc) v = (rng() % 3 == 0) ? 0.f : (small ? (float)((int)(rng() % 5) - 2) : ((int)(rng() % 2001) - 1000) / 512.f);
      for (auto &v : u) v = small ? (float)(rng() % 4) : ((int)(rng() % 20001) - 10000) / 64.f;
      for (auto &g : gait) g = (variant == 1) ? 0 : (rng() % 4 != 0);
      if (variant == 0 && NC == 3) cap[2] = 1e-4f;  // not in stance: (float)1e-4 lies below the double literal
      if (variant == 2) u[rng() % u.size()] = NAN, gait.assign(NC * h, 1);
      if (variant == 3 && h > 1) {  // two steps with the same forces and gait: every minimum is met twice
        for (int k = 0; k < U; ++k) u[U * (h - 1) + k] = u[k];
        for (int c = 0; c < NC; ++c) gait[NC * (h - 1) + c] = gait[c] = 1;
      }
      if (variant == 4) {  // rows 7 with Fz <= 0 for half of the leg-steps
        for (int r = 0; r < C8; ++r)
          for (int k = 0; k < U; ++k) Fc[r * U + k] = (r % 8 == 7) ? ((k == 3 * (r / 8) + 2) ? 2.f : 0.f) : Fc[r * U + k];
        for (int i = 0; i < h; ++i)
          for (int c = 0; c < NC; ++c) u[U * i + 3 * c + 2] = (i + c) % 2 ? -std::fabs(u[U * i + 3 * c + 2]) * (i % 3 == 0 ? 0.f : 1.f) : 40.f + i;
      }
      if (variant == 5) gait.assign(NC * h, 1);
      hipLaunchKernelGGL(margins_test_kernel<NC>, dim3(1), dim3(hmpc::MARGINS_NT), 0, nullptr, Fc.data(), u.data(), gait.data(), cap.data(), h,
                         slack.data(), summary.data(), where.data());
      // the plain loop
      double ws[6];
      int32_t ww[6];
      for (int k = 0; k < 6; ++k) ws[k] = INFINITY, ww[k] = -1;
      auto cand = [&](int k, double v, int idx) {
        if (v < ws[k] || (v == ws[k] && ww[k] < 0)) ws[k] = v, ww[k] = idx;  // (ascending index: an equal value keeps the earlier one)
      };
      for (int i = 0; i < h; ++i)
        for (int c = 0; c < NC; ++c) {
          double *s = &want[10 * (NC * i + c)];
          if (!in_stance(cap[c], gait[NC * i + c])) {
            for (int j = 0; j < 10; ++j) s[j] = INFINITY;
            continue;
          }
          double row[8];
          for (int j = 0; j < 8; ++j) {
            double acc = 0.0;
            for (int k = 0; k < U; ++k) acc = std::fma((double)Fc[(8 * c + j) * U + k], (double)u[U * i + k], acc);
            row[j] = acc;
          }
          for (int j = 0; j < 4; ++j) s[j] = row[j];
          s[4] = row[4], s[5] = (double)0.01f - row[4], s[6] = 0.0 - row[5], s[7] = 0.0 - row[6], s[8] = row[7];
          s[9] = (double)(cap[c] * (float)gait[NC * i + c]) - row[7];
          const int base = 10 * (NC * i + c);
          double m = INFINITY;
          for (int j = 0; j < 4; ++j) { cand(0, s[j], base + j); if (s[j] < m) m = s[j]; }
          cand(1, s[4], base + 4), cand(1, s[5], base + 5), cand(2, s[6], base + 6), cand(2, s[7], base + 7);
          cand(3, s[8], base + 8), cand(4, s[9], base + 9);
          if (s[8] > 0.0) cand(5, m / (0.5 * s[8]), base);
        }
      bool ok = memcmp(slack.data(), want.data(), sizeof(double) * want.size()) == 0;
      if (!ok) printf("NC %d h %d variant %d: slacks differ\n", NC, h, variant);
      for (int k = 0; k < 6; ++k)
        if (memcmp(&summary[k], &ws[k], 8) != 0 || where[k] != ww[k]) {
          ok = false;
          printf("NC %d h %d variant %d class %d: got %.17g at %d, want %.17g at %d\n", NC, h, variant, k, summary[k], where[k], ws[k], ww[k]);
        }
      if (variant == 1 && !(where[0] == -1 && where[5] == -1 && std::isinf(summary[3]))) ok = false, printf("all swing: a candidate\n");
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(11);
  int bad = run<2>(rng) + run<3>(rng);
  // the penalty
  for (int variant = 0; variant < 4; ++variant) {
    const int B = 700;
    std::vector<double> summary(6 * B), pen(B), out(B, -7.0);
    hmpc::MarginFloor f;
    for (int k = 0; k < 6; ++k) f.v[k] = (variant == 0 || rng() % 2) ? NAN : (double)(rng() % 5);
    if (variant == 2) f.v[5] = 2.0;
    for (auto &v : summary) { const int r = rng() % 12; v = r == 0 ? NAN : r == 1 ? INFINITY : (double)(rng() % 9) - 1.0; }
    for (auto &v : pen) v = (double)(rng() % 100);
    const bool in_place = variant == 3, no_pen = variant == 1;
    if (in_place) out = pen;
    const std::vector<double> pen0 = pen;
    hipLaunchKernelGGL((hmpc::margin_penalty_kernel<hmpc::PENALTY_NT>), dim3((B + hmpc::PENALTY_NT - 1) / hmpc::PENALTY_NT), dim3(hmpc::PENALTY_NT), 0,
                       nullptr, summary.data(), f, no_pen ? nullptr : (in_place ? out.data() : pen.data()), out.data(), B);
    for (int i = 0; i < B; ++i) {
      bool masked = false;
      for (int k = 0; k < 6; ++k)
        if (!std::isnan(f.v[k]) && !(summary[6 * i + k] >= f.v[k])) masked = true;
      const double w = masked ? INFINITY : (no_pen ? 0.0 : pen0[i]);
      if (memcmp(&out[i], &w, 8) != 0) { ++bad; printf("penalty variant %d instance %d: got %g want %g\n", variant, i, out[i], w); break; }
    }
  }
  printf("%d problems\n", bad);
  return bad != 0;
}
