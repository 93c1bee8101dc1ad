// tests/test_certificate_kernel_on_host.py: csrc/hmpc_certificate.h -- everything of the certificate kernel behind the assembly, and the
// penalty kernel -- compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop: h = 1, 5, 10, 20
// and NC = 2, 3.  States, costate, gradient, slacks and the maxima are compared as bit patterns; the multipliers by what defines them
// (lambda >= 0 and 0 off the active set, e = r - N lambda bit for bit, and the optimality conditions of the projection: N_A' e <= 0,
// lambda' N' e = 0), which fixes e.  Variants: random data (active sets of up to ten rows, opposite normals among them), an eight-row
// active set of rank 5, an empty active set, swing leg-steps, all legs in swing, a NaN force (the run must end; summary[0] = +inf).  Then
// the penalty: NaN ceilings, NaN summaries, no penalty_in, in place.
#include "hmpc_certificate.h"
#include <cmath>
#include <cstdio>
#include <random>

constexpr int HM = 20;

template <int NC>
__global__ void certificate_test_kernel(const float *Acd, const float *Bcd, const float *x0, const float *W, const float *traj, const float *alpha,
                                        const float *Fc, const float *u, const unsigned char *gait, const float *cap, int h, double act_tol,
                                        double *grad, double *lam, double *res, double *summary, int32_t *where) {
  __shared__ hmpc::CertScratch<NC, HM> T;
  hmpc::certificate_of_instance<NC, HM, hmpc::CERT_NT>(Acd, Bcd, x0, W, traj, alpha, Fc, u, gait, cap, h, act_tol, T, grad, lam, res, summary, where);
}

static bool in_stance(float cap, unsigned char g) {
  const double ub = (double)(cap * (float)g);
  return !(ub < 0.0001 && ub > -.0001);
}
static const int SRC[10] = {0, 1, 2, 3, 4, 4, 5, 6, 7, 7};
static const double SIG[10] = {1, 1, 1, 1, 1, -1, -1, -1, 1, -1};
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

template <int NC>
static int run(std::mt19937 &rng) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  for (int h : {1, 5, 10, 20})
    for (int variant = 0; variant < 6; ++variant) {
      std::vector<float> Acd(169), Bcd(13 * U), x0(13), W(13), traj(12 * h), alpha(U), Fc(C8 * U, 0.f), u(U * h), cap(NC, 500.f);
      std::vector<unsigned char> gait(NC * h);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.02, 0.02);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : traj) v = uni(-1, 1);
      for (auto &v : alpha) v = uni(1e-6, 1e-3);
      for (auto &v : u) v = uni(-50, 150);
      for (auto &g : gait) g = (variant == 3) ? 0 : (rng() % 4 != 0);
      auto col = [&](int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); };
      for (int c = 0; c < NC; ++c)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) Fc[(8 * c + j) * U + col(c, k)] = (rng() % 4 == 0) ? 0.f : uni(-1, 1);
      double act_tol = 1e-3;
      if (variant == 1) {  // contact 0: eight rows spanning five dimensions; zero forces at step 0 make rows 0-4, 6, 7, 8 active
        float basis[5][6], mix;
        for (auto &b : basis)
          for (auto &v : b) v = (float)((int)(rng() % 9) - 4);
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) {
            float acc = 0.f;
            for (int b = 0; b < 5; ++b) mix = (float)((int)((j * 7 + b * 3) % 5) - 2), acc += mix * basis[b][k];
            Fc[j * U + col(0, k)] = acc;  // (small integers: exactly of rank <= 5)
          }
        for (int k = 0; k < U; ++k) u[k] = 0.f;
        gait.assign(NC * h, 1);
      }
      if (variant == 2) act_tol = -1e30, gait.assign(NC * h, 1);  // nothing is active
      if (variant == 4) u[rng() % u.size()] = NAN, gait.assign(NC * h, 1);
      if (variant == 5 && NC == 3) cap[2] = 1e-4f;  // not in stance
      std::vector<double> grad(U * h, -7.0), lam(10 * NC * h, -7.0), res(6 * NC * h, -7.0), summary(4, -7.0);
      std::vector<int32_t> where(2, -7);
      hipLaunchKernelGGL(certificate_test_kernel<NC>, dim3(1), dim3(hmpc::CERT_NT), 0, nullptr, Acd.data(), Bcd.data(), x0.data(), W.data(),
                         traj.data(), alpha.data(), Fc.data(), u.data(), gait.data(), cap.data(), h, act_tol, grad.data(), lam.data(), res.data(),
                         summary.data(), where.data());
      // the plain loop: states, costate, gradient
      bool ok = true;
      std::vector<double> x(13 * (h + 1)), p(13 * (h + 2), 0.0), want(U * h);
      for (int s = 0; s < 13; ++s) x[s] = (double)x0[s];
      for (int i = 0; i < h; ++i)
        for (int s = 0; s < 13; ++s) {
          double acc = 0.0;
          for (int k = 0; k < 13; ++k) acc = std::fma((double)Acd[s * 13 + k], x[13 * i + k], acc);
          for (int c = 0; c < U; ++c) acc = std::fma((double)Bcd[s * U + c], (double)u[U * i + c], acc);
          x[13 * (i + 1) + s] = acc;
        }
      for (int i = h; i >= 1; --i)
        for (int s = 0; s < 13; ++s) {
          double q = 0.0;
          if (s < 12) q = ((double)W[s] + (double)W[s]) * (x[13 * i + s] - (double)traj[12 * (i - 1) + s]);
          if (i < h) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma((double)Acd[k * 13 + s], p[13 * (i + 1) + k], acc);
            q = q + acc;
          }
          p[13 * i + s] = q;
        }
      for (int i = 0; i < h; ++i)
        for (int c = 0; c < U; ++c) {
          double acc = 0.0;
          for (int k = 0; k < 13; ++k) acc = std::fma((double)Bcd[k * U + c], p[13 * (i + 1) + k], acc);
          want[U * i + c] = std::fma((double)alpha[c] + (double)alpha[c], (double)u[U * i + c], acc);
        }
      if (memcmp(grad.data(), want.data(), sizeof(double) * want.size()) != 0) ok = false, printf("NC %d h %d variant %d: gradients differ\n", NC, h, variant);
      // leg-steps: slacks, the multipliers' defining properties, the maxima
      double ws[4] = {-1, -1, -1, -1};
      int32_t ww[4] = {-1, -1, -1, -1};
      auto cand = [&](int k, double v, int idx) {
        if (std::isnan(v)) v = INFINITY;
        if (v > ws[k]) ws[k] = v, ww[k] = idx;  // (ascending index: an equal value keeps the earlier one)
      };
      for (int i = 0; i < h && ok; ++i)
        for (int c = 0; c < NC && ok; ++c) {
          const int ls = NC * i + c;
          const double *l = &lam[10 * ls], *e = &res[6 * ls];
          if (!in_stance(cap[c], gait[ls])) {
            for (int j = 0; j < 10; ++j) ok = ok && same(l[j], 0.0);
            for (int k = 0; k < 6; ++k) ok = ok && same(e[k], 0.0);
            if (!ok) printf("NC %d h %d variant %d: a swing leg-step with a multiplier or a residual\n", NC, h, variant);
            continue;
          }
          double row[8], s[10], r[6], N[10][6];
          for (int j = 0; j < 8; ++j) {
            double acc = 0.0;
            for (int k = 0; k < U; ++k) acc = std::fma((double)Fc[(8 * c + j) * U + k], (double)u[U * i + k], acc);
            row[j] = acc;
          }
          for (int j = 0; j < 4; ++j) s[j] = row[j];
          s[4] = row[4], s[5] = (double)0.01f - row[4], s[6] = 0.0 - row[5], s[7] = 0.0 - row[6], s[8] = row[7];
          s[9] = (double)(cap[c] * (float)gait[ls]) - row[7];
          double nn = 0.0, rn = 0.0;
          for (int k = 0; k < 6; ++k) r[k] = grad[U * i + col(c, k)], rn += r[k] * r[k];
          for (int j = 0; j < 10; ++j)
            for (int k = 0; k < 6; ++k) N[j][k] = SIG[j] * (double)Fc[(8 * c + SRC[j]) * U + col(c, k)], nn += N[j][k] * N[j][k];
          const bool nan_in = std::isnan(rn);
          const double tol = 1e-9 * std::sqrt(nn) * std::fmax(1.0, std::sqrt(rn));
          int nact = 0;
          for (int j = 0; j < 10; ++j) {
            const bool act = s[j] <= act_tol;
            nact += act;
            if (!(l[j] >= 0.0) || (!act && !same(l[j], 0.0))) ok = false, printf("NC %d h %d variant %d leg-step %d: lambda[%d] = %g, slack %g\n", NC, h, variant, ls, j, l[j], s[j]);
          }
          for (int k = 0; k < 6; ++k) {
            double acc = 0.0;
            for (int j = 0; j < 10; ++j) acc = std::fma(N[j][k], l[j], acc);
            if (!same(e[k], r[k] - acc)) ok = false, printf("NC %d h %d variant %d leg-step %d: e[%d] is not r - N lambda\n", NC, h, variant, ls, k);
          }
          if (variant == 2 && nact != 0) ok = false, printf("variant 2: an active row\n");
          if (variant == 1 && ls == 0 && nact != 8) ok = false, printf("variant 1: %d active rows, not 8\n", nact);
          if (!nan_in)
            for (int j = 0; j < 10; ++j) {
              if (!(s[j] <= act_tol)) continue;
              double w = 0.0;
              for (int k = 0; k < 6; ++k) w += N[j][k] * e[k];
              if (w > tol || (l[j] > 0.0 && std::fabs(w) > tol))
                ok = false, printf("NC %d h %d variant %d leg-step %d: column %d has n.e = %g (lambda %g, tolerance %g)\n", NC, h, variant, ls, j, w, l[j], tol);
            }
          for (int k = 0; k < 6; ++k) cand(0, std::fabs(e[k]), 6 * ls + k), cand(3, std::fabs(r[k]), 6 * ls + k);
          for (int j = 0; j < 10; ++j) {
            if (s[j] <= act_tol) cand(1, l[j] * (s[j] > 0.0 ? s[j] : 0.0), 10 * ls + j);
            cand(2, s[j] < 0.0 ? 0.0 - s[j] : (std::isnan(s[j]) ? s[j] : 0.0), 10 * ls + j);
          }
        }
      for (int k = 0; k < 4; ++k) {
        const double v = ww[k] < 0 ? 0.0 : ws[k];
        if (!same(summary[k], v) || (k < 2 && where[k] != ww[k])) {
          ok = false;
          printf("NC %d h %d variant %d summary %d: got %.17g at %d, want %.17g at %d\n", NC, h, variant, k, summary[k], k < 2 ? where[k] : 0, v, ww[k]);
        }
      }
      if (variant == 3 && !(where[0] == -1 && where[1] == -1 && same(summary[0], 0.0) && same(summary[3], 0.0))) ok = false, printf("all swing: a candidate\n");
      if (variant == 4 && !(std::isinf(summary[0]) && summary[0] > 0)) ok = false, printf("NaN force: summary[0] = %g\n", summary[0]);
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(13);
  int bad = run<2>(rng) + run<3>(rng);
  // the penalty
  for (int variant = 0; variant < 4; ++variant) {
    const int B = 700;
    std::vector<double> summary(4 * B), pen(B), out(B, -7.0);
    hmpc::CertCeil f;
    for (int k = 0; k < 3; ++k) f.v[k] = (variant == 0 || rng() % 2) ? NAN : (double)(rng() % 5);
    if (variant == 2) f.v[0] = 2.0;
    for (auto &v : summary) { const int r = rng() % 12; v = r == 0 ? NAN : r == 1 ? INFINITY : (double)(rng() % 9) - 1.0; }
    for (auto &v : pen) v = (double)(rng() % 100);
    const bool in_place = variant == 3, no_pen = variant == 1;
    if (in_place) out = pen;
    const std::vector<double> pen0 = pen;
    hipLaunchKernelGGL((hmpc::certificate_penalty_kernel<hmpc::PENALTY_NT>), dim3((B + hmpc::PENALTY_NT - 1) / hmpc::PENALTY_NT), dim3(hmpc::PENALTY_NT),
                       0, nullptr, summary.data(), f, no_pen ? nullptr : (in_place ? out.data() : pen.data()), out.data(), B);
    for (int i = 0; i < B; ++i) {
      bool masked = false;
      for (int k = 0; k < 3; ++k)
        if (!std::isnan(f.v[k]) && !(summary[4 * i + k] <= f.v[k])) masked = true;
      const double w = masked ? INFINITY : (no_pen ? 0.0 : pen0[i]);
      if (memcmp(&out[i], &w, 8) != 0) { ++bad; printf("penalty variant %d instance %d: got %g want %g\n", variant, i, out[i], w); break; }
    }
  }
  printf("%d problems\n", bad);
  return bad != 0;
}
