// tests/test_feedback_kernel_on_host.py: csrc/hmpc_feedback.h -- everything of the feedback-gain kernel and of the first-order kernel behind
// the assembly -- compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop that states the
// definition once more, sequentially: h = 1, 3, 20 and NC = 2, 3, every output compared as bit patterns.  Variants: random data; every
// limit active (ten normals of rank 6: no free direction, gains exactly 0); an unloaded foot (eight active rows of rank 5: one free
// direction); nothing active; all legs in swing; a NaN force (the run must end); a hand that is not in stance.
#include "hmpc_feedback.h"
#include <cmath>
#include <cstdio>
#include <random>

constexpr int HM = 20;

template <int NC>
__global__ void feedback_test_kernel(const float *Acd, const float *Bcd, const float *W, const float *alpha, const float *Fc, const float *u,
                                     const unsigned char *gait, const float *cap, int h, double act_tol, double *gain, double *ref, int32_t *fr,
                                     double *summary) {
  __shared__ hmpc::FeedbackKeep<NC, HM> Kp;
  __shared__ hmpc::FeedbackWork<NC, HM> Wk;
  hmpc::feedback_of_instance<NC, HM, hmpc::FB_NT>(Acd, Bcd, W, alpha, Fc, u, gait, cap, h, act_tol, Kp, Wk, gain, ref, fr, summary);
}

template <int NC>
__global__ void first_order_test_kernel(const double *gain, const double *ref, const double *dx, const double *dt, const float *u0, const float *Fc,
                                        const unsigned char *gait, const float *cap, int h, float *wrench, double *worst) {
  __shared__ hmpc::FirstOrderScratch<NC> T;
  hmpc::first_order_of_instance<NC, hmpc::FB_NT>(gain, ref, dx, dt, u0, Fc, gait, cap, h, T, wrench, worst);
}

static bool in_stance(float cap, unsigned char g) {
  const double ub = (double)(cap * (float)g);
  return !(ub < 0.0001 && ub > -.0001);
}
static const int SRC[10] = {0, 1, 2, 3, 4, 4, 5, 6, 7, 7};
static const double SIG[10] = {1, 1, 1, 1, 1, -1, -1, -1, 1, -1};
static bool same(const double *a, const double *b, size_t n) { return memcmp(a, b, 8 * n) == 0; }

// the ten slacks of leg-step (i, c), as hmpc_margins.h has them
template <int NC>
static void slacks(const std::vector<float> &Fc, const std::vector<float> &u, int i, int c, float ub7, double *s) {
  constexpr int U = 6 * NC;
  double row[8];
  for (int j = 0; j < 8; ++j) {
    double acc = 0.0;
    for (int k = 0; k < U; ++k) acc = std::fma((double)Fc[(8 * c + j) * U + k], (double)u[U * i + k], acc);
    row[j] = acc;
  }
  for (int j = 0; j < 4; ++j) s[j] = row[j];
  s[4] = row[4], s[5] = (double)0.01f - row[4], s[6] = 0.0 - row[5], s[7] = 0.0 - row[6], s[8] = row[7], s[9] = (double)ub7 - row[7];
}

// the plain loop: the definition, sequentially
template <int NC>
struct Plain {
  static constexpr int U = 6 * NC;
  std::vector<double> gain, ref, summary;
  std::vector<int32_t> fr;
  std::vector<int> held;  // per leg-step
  static int col(int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); }
  static int directions(const std::vector<float> &Fc, int c, const double *s, double act_tol, double *q) {
    int m = 0;
    auto reduce = [&](double *v) {
      for (int pass = 0; pass < 2; ++pass)
        for (int a = 0; a < m; ++a) {
          double d = 0.0;
          for (int k = 0; k < 6; ++k) d = std::fma(q[6 * a + k], v[k], d);
          for (int k = 0; k < 6; ++k) v[k] = std::fma(0.0 - d, q[6 * a + k], v[k]);
        }
    };
    auto norm2 = [](const double *v) {
      double acc = 0.0;
      for (int k = 0; k < 6; ++k) acc = std::fma(v[k], v[k], acc);
      return acc;
    };
    auto hold = [&](const double *v, double rem2) {
      const double len = std::sqrt(rem2);
      for (int k = 0; k < 6; ++k) q[6 * m + k] = v[k] / len;
      ++m;
    };
    for (int j = 0; j < 10; ++j) {
      if (!(s[j] <= act_tol)) continue;
      double v[6];
      for (int k = 0; k < 6; ++k) v[k] = SIG[j] * (double)Fc[(8 * c + SRC[j]) * U + col(c, k)];
      const double len2 = norm2(v);
      reduce(v);
      const double rem2 = norm2(v);
      if (m < 6 && rem2 > 0.0 && rem2 >= 1e-12 * len2) hold(v, rem2);
    }
    const int normals = m;
    bool taken[6] = {false, false, false, false, false, false};
    while (m < 6) {
      int best = -1;
      double vb[6] = {0, 0, 0, 0, 0, 0}, rb = 0.0;
      for (int k = 0; k < 6; ++k) {
        if (taken[k]) continue;
        double v[6] = {0, 0, 0, 0, 0, 0};
        v[k] = 1.0;
        reduce(v);
        const double rem2 = norm2(v);
        if (best < 0 || rem2 > rb) {
          best = k, rb = rem2;
          for (int kk = 0; kk < 6; ++kk) vb[kk] = v[kk];
        }
      }
      taken[best] = true;
      hold(vb, rb);
    }
    return normals;
  }
  Plain(const std::vector<float> &Acd, const std::vector<float> &Bcd, const std::vector<float> &W, const std::vector<float> &alpha,
        const std::vector<float> &Fc, const std::vector<float> &u, const std::vector<unsigned char> &gait, const std::vector<float> &cap, int h,
        double act_tol)
      : gain(U * 13), ref((size_t)h * U * 12), summary(2), fr(h), held(NC * h) {
    std::vector<double> A(169), B(13 * U), q2(13, 0.0), r2(U), Zq(36 * NC * h, 0.0);
    for (int t = 0; t < 169; ++t) A[t] = (double)Acd[t];
    for (int t = 0; t < 13 * U; ++t) B[t] = (double)Bcd[t];
    for (int s = 0; s < 12; ++s) q2[s] = (double)W[s] + (double)W[s];
    for (int c = 0; c < U; ++c) r2[c] = (double)alpha[c] + (double)alpha[c];
    for (int i = 0; i < h; ++i) {
      fr[i] = 0;
      for (int c = 0; c < NC; ++c) {
        const int ls = NC * i + c;
        held[ls] = 6;
        if (in_stance(cap[c], gait[ls])) {
          double s[10];
          slacks<NC>(Fc, u, i, c, cap[c] * (float)gait[ls], s);
          held[ls] = directions(Fc, c, s, act_tol, &Zq[36 * ls]);
        }
        fr[i] += 6 - held[ls];
      }
    }
    std::vector<double> P(169, 0.0), PA(169), PB(13 * U), Mall((size_t)(h > 1 ? h - 1 : 1) * 169), K(13 * U, 0.0), S(13 * U, 0.0);
    for (int s = 0; s < 13; ++s) P[14 * s] = q2[s];
    double pivmin = 1.0;
    for (int i = h - 1; i >= 0; --i) {
      // Z_i as a dense U x r matrix, and each column's contact
      const int r = fr[i];
      std::vector<double> Z((size_t)U * (r > 0 ? r : 1), 0.0);
      std::vector<int> zc(r > 0 ? r : 1), first(NC);
      int b = 0;
      for (int c = 0; c < NC; ++c) {
        first[c] = b;
        for (int a = held[NC * i + c]; a < 6; ++a, ++b) {
          zc[b] = c;
          for (int k = 0; k < 6; ++k) Z[col(c, k) * r + b] = Zq[36 * (NC * i + c) + 6 * a + k];
        }
      }
      for (int k = 0; k < 13; ++k)
        for (int s = 0; s < 13; ++s) {
          double acc = 0.0;
          for (int l = 0; l < 13; ++l) acc = std::fma(P[k * 13 + l], A[l * 13 + s], acc);
          PA[k * 13 + s] = acc;
        }
      for (int k = 0; k < 13; ++k)
        for (int c = 0; c < U; ++c) {
          double acc = 0.0;
          for (int l = 0; l < 13; ++l) acc = std::fma(P[k * 13 + l], B[l * U + c], acc);
          PB[k * U + c] = acc;
        }
      if (r > 0) {
        std::vector<double> Wm(U * U), WZ(U * r), G(r * r), L(r * r, 0.0), X(r * 13);
        for (int c = 0; c < U; ++c)
          for (int d = 0; d < U; ++d) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(B[k * U + c], PB[k * U + d], acc);
            Wm[c * U + d] = (c == d) ? r2[c] + acc : acc;
          }
        for (int c = 0; c < U; ++c)
          for (int bb = 0; bb < r; ++bb) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = std::fma(Wm[c * U + col(zc[bb], k)], Z[col(zc[bb], k) * r + bb], acc);
            WZ[c * r + bb] = acc;
          }
        for (int a = 0; a < r; ++a)
          for (int bb = 0; bb < r; ++bb) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = std::fma(Z[col(zc[a], k) * r + a], WZ[col(zc[a], k) * r + bb], acc);
            G[a * r + bb] = acc;
          }
        for (int a = 0; a < r; ++a)
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = std::fma(Z[col(zc[a], k) * r + a], B[s * U + col(zc[a], k)], acc);
            X[a * 13 + s] = acc;
          }
        for (int j = 0; j < r; ++j) {
          double ss = 0.0;
          for (int bb = 0; bb < j; ++bb) ss = std::fma(L[j * r + bb], L[j * r + bb], ss);
          const double d = G[j * r + j] - ss, p = d / G[j * r + j], v = (p == p) ? p : 0.0;
          pivmin = (v < pivmin) ? v : pivmin;
          L[j * r + j] = std::sqrt(d);
          for (int a = j + 1; a < r; ++a) {
            double acc = 0.0;
            for (int bb = 0; bb < j; ++bb) acc = std::fma(L[a * r + bb], L[j * r + bb], acc);
            L[a * r + j] = (G[a * r + j] - acc) / L[j * r + j];
          }
        }
        for (int s = 0; s < 13; ++s) {
          for (int a = 0; a < r; ++a) {
            double acc = 0.0;
            for (int bb = 0; bb < a; ++bb) acc = std::fma(L[a * r + bb], X[bb * 13 + s], acc);
            X[a * 13 + s] = (X[a * 13 + s] - acc) / L[a * r + a];
          }
          for (int a = r - 1; a >= 0; --a) {
            double acc = 0.0;
            for (int bb = a + 1; bb < r; ++bb) acc = std::fma(L[bb * r + a], X[bb * 13 + s], acc);
            X[a * 13 + s] = (X[a * 13 + s] - acc) / L[a * r + a];
          }
        }
        for (int c = 0; c < U; ++c) {
          const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int bb = first[cc]; bb < first[cc] + 6 - held[NC * i + cc]; ++bb) acc = std::fma(Z[c * r + bb], X[bb * 13 + s], acc);
            S[c * 13 + s] = acc;
          }
        }
        for (int c = 0; c < U; ++c)
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(S[c * 13 + k], PA[k * 13 + s], acc);
            K[c * 13 + s] = 0.0 - acc;
          }
      } else {
        for (auto &v : S) v = 0.0;
        for (auto &v : K) v = 0.0;
      }
      if (i > 0) {
        double *M = &Mall[(size_t)169 * (i - 1)];
        for (int k = 0; k < 13; ++k)
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int c = 0; c < U; ++c) acc = std::fma(B[k * U + c], K[c * 13 + s], acc);
            M[k * 13 + s] = A[k * 13 + s] + acc;
          }
        for (int s = 0; s < 13; ++s)
          for (int t = s; t < 13; ++t) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(PA[k * 13 + s], M[k * 13 + t], acc);
            const double v = (s == t) ? q2[s] + acc : acc;
            P[s * 13 + t] = v, P[t * 13 + s] = v;
          }
      }
    }
    gain = K;
    double kmax = 0.0;
    for (double kv : K) {
      const double a = std::fabs(kv), v = (a == a) ? a : INFINITY;
      kmax = (v > kmax) ? v : kmax;
    }
    summary[0] = pivmin, summary[1] = kmax;
    std::vector<double> Psi = S, nxt(13 * U);
    for (int j = 1; j <= h; ++j) {
      for (int c = 0; c < U; ++c)
        for (int s = 0; s < 12; ++s) ref[((size_t)(j - 1) * U + c) * 12 + s] = Psi[c * 13 + s] * q2[s];
      if (j < h) {
        const double *M = &Mall[(size_t)169 * (j - 1)];
        for (int c = 0; c < U; ++c)
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(Psi[c * 13 + k], M[s * 13 + k], acc);
            nxt[c * 13 + s] = acc;
          }
        Psi = nxt;
      }
    }
  }
};

template <int NC>
static int run(std::mt19937 &rng) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  auto col = [&](int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); };
  for (int h : {1, 3, 20})
    for (int variant = 0; variant < 7; ++variant) {
      std::vector<float> Acd(169), Bcd(13 * U), W(13), alpha(U), Fc(C8 * U, 0.f), u(U * h), cap(NC, 500.f);
      std::vector<unsigned char> gait(NC * h);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.02, 0.02);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : alpha) v = uni(1e-6, 1e-3);
      for (auto &v : u) v = uni(-50, 150);
      for (auto &g : gait) g = (variant == 3) ? 0 : (rng() % 4 != 0);
      for (int c = 0; c < NC; ++c)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) Fc[(8 * c + j) * U + col(c, k)] = (rng() % 4 == 0) ? 0.f : uni(-1, 1);
      double act_tol = 1e-3;
      if (variant == 0) act_tol = 40.0;  // random data: active sets of every size
      if (variant == 1) {                // the unloaded foot: eight rows spanning five dimensions; zero forces make rows 0-4, 6, 7, 8 active
        float basis[5][6];
        for (int b = 0; b < 5; ++b)
          for (int k = 0; k < 6; ++k) basis[b][k] = (k == b ? 1.f : 0.f) + (k == 5 ? (float)(b + 1) : 0.f);  // (of rank 5 exactly)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k)
            Fc[j * U + col(0, k)] = j < 5 ? basis[j][k] : (j == 5 ? basis[0][k] + basis[1][k] : (j == 6 ? basis[1][k] - basis[2][k] : basis[3][k] + basis[4][k]));
        for (int k = 0; k < U; ++k) u[k] = 0.f;
        gait.assign(NC * h, 1);
      }
      if (variant == 2) act_tol = -1e30, gait.assign(NC * h, 1);  // nothing is active
      if (variant == 4) u[rng() % u.size()] = NAN, gait.assign(NC * h, 1);
      if (variant == 5 && NC == 3) cap[2] = 1e-4f;               // not in stance
      if (variant == 6) act_tol = 1e30, gait.assign(NC * h, 1);  // all ten limits active on every leg-step: rank 6, nothing free
      std::vector<double> gain(U * 13, -7.0), ref((size_t)h * U * 12, -7.0), summary(2, -7.0);
      std::vector<int32_t> fr(h, -7);
      hipLaunchKernelGGL(feedback_test_kernel<NC>, dim3(1), dim3(hmpc::FB_NT), 0, nullptr, Acd.data(), Bcd.data(), W.data(), alpha.data(), Fc.data(),
                         u.data(), gait.data(), cap.data(), h, act_tol, gain.data(), ref.data(), fr.data(), summary.data());
      Plain<NC> want(Acd, Bcd, W, alpha, Fc, u, gait, cap, h, act_tol);
      bool ok = true;
      if (memcmp(fr.data(), want.fr.data(), 4 * h) != 0) ok = false, printf("NC %d h %d variant %d: free_dims differ\n", NC, h, variant);
      if (!same(gain.data(), want.gain.data(), gain.size())) ok = false, printf("NC %d h %d variant %d: gains differ\n", NC, h, variant);
      if (!same(ref.data(), want.ref.data(), ref.size())) ok = false, printf("NC %d h %d variant %d: reference gains differ\n", NC, h, variant);
      if (!same(summary.data(), want.summary.data(), 2))
        ok = false, printf("NC %d h %d variant %d: summary %.17g %.17g, want %.17g %.17g\n", NC, h, variant, summary[0], summary[1], want.summary[0], want.summary[1]);
      if (variant == 1 && want.held[0] != 5) ok = false, printf("variant 1: %d normals held, not 5\n", want.held[0]);
      if (variant == 1 && fr[0] != 1) ok = false, printf("variant 1: free_dims[0] = %d, not 1 (the other contacts' eight random normals span R^6)\n", fr[0]);
      if (variant == 2)
        for (int i = 0; i < h; ++i)
          if (fr[i] != U) ok = false, printf("variant 2: free_dims[%d] = %d\n", i, fr[i]);
      if (variant == 3 || variant == 6) {
        for (int i = 0; i < h; ++i)
          if (fr[i] != 0) ok = false, printf("variant %d: free_dims[%d] = %d\n", variant, i, fr[i]);
        for (double v : gain)
          if (v != 0.0) ok = false;
        for (double v : ref)
          if (v != 0.0) ok = false;
        if (!(summary[0] == 1.0 && summary[1] == 0.0)) ok = false;
        if (!ok) printf("NC %d h %d variant %d: no free direction, yet a gain or a pivot\n", NC, h, variant);
      }
      if (variant != 4 && !(summary[0] > 0.0 && std::isfinite(summary[1]))) ok = false, printf("NC %d h %d variant %d: summary %g %g\n", NC, h, variant, summary[0], summary[1]);
      if (variant != 4 && variant != 3 && variant != 6) {  // N_A' K_0 = 0 on the stance leg-steps of step 0; swing rows exactly 0
        for (int c = 0; c < NC; ++c) {
          if (!in_stance(cap[c], gait[c])) {
            for (int k = 0; k < 6; ++k)
              for (int s = 0; s < 13; ++s)
                if (gain[col(c, k) * 13 + s] != 0.0) ok = false, printf("NC %d h %d variant %d: a swing row of the gain is not 0\n", NC, h, variant);
            continue;
          }
          double s10[10];
          slacks<NC>(Fc, u, 0, c, cap[c] * (float)gait[c], s10);
          for (int j = 0; j < 10; ++j) {
            if (!(s10[j] <= act_tol)) continue;
            double nn = 0.0;
            for (int k = 0; k < 6; ++k) nn += (double)Fc[(8 * c + SRC[j]) * U + col(c, k)] * (double)Fc[(8 * c + SRC[j]) * U + col(c, k)];
            for (int s = 0; s < 13; ++s) {
              double acc = 0.0;
              for (int k = 0; k < 6; ++k) acc += SIG[j] * (double)Fc[(8 * c + SRC[j]) * U + col(c, k)] * gain[col(c, k) * 13 + s];
              if (std::fabs(acc) > 1e-9 * std::sqrt(nn) * std::fmax(1.0, summary[1]))
                ok = false, printf("NC %d h %d variant %d: normal %d of contact %d times the gain = %g\n", NC, h, variant, j, c, acc);
            }
          }
        }
      }
      // the first-order wrench: zero deltas give u0 bit for bit; random deltas against the plain chain
      if (variant != 4) {
        for (int pass = 0; pass < 2; ++pass) {
          std::vector<double> dx(13, 0.0), dt(12 * h, 0.0);
          if (pass == 1) {
            for (auto &v : dx) v = (double)uni(-1e-3, 1e-3);
            for (auto &v : dt) v = (double)uni(-1e-3, 1e-3);
          }
          std::vector<float> wrench(U, -7.f);
          double worst = -7.0;
          hipLaunchKernelGGL(first_order_test_kernel<NC>, dim3(1), dim3(hmpc::FB_NT), 0, nullptr, gain.data(), ref.data(), dx.data(), dt.data(), u.data(),
                             Fc.data(), gait.data(), cap.data(), h, wrench.data(), &worst);
          std::vector<float> ww(U);
          for (int c = 0; c < U; ++c) {
            double acc = 0.0;
            for (int s = 0; s < 13; ++s) acc = std::fma(gain[c * 13 + s], dx[s], acc);
            for (int j = 0; j < h; ++j)
              for (int s = 0; s < 12; ++s) acc = std::fma(ref[((size_t)j * U + c) * 12 + s], dt[12 * j + s], acc);
            ww[c] = (float)((double)u[c] + acc);
          }
          if (memcmp(ww.data(), wrench.data(), 4 * U) != 0) ok = false, printf("NC %d h %d variant %d pass %d: first-order wrenches differ\n", NC, h, variant, pass);
          if (pass == 0 && memcmp(u.data(), wrench.data(), 4 * U) != 0) ok = false, printf("NC %d h %d variant %d: zero deltas do not return u0\n", NC, h, variant);
          double wmin = INFINITY;
          std::vector<float> u1(ww);
          u1.resize(U * h, 0.f);
          for (int c = 0; c < NC; ++c)
            if (in_stance(cap[c], gait[c])) {
              double s10[10];
              slacks<NC>(Fc, u1, 0, c, cap[c] * (float)gait[c], s10);
              for (int j = 0; j < 10; ++j) wmin = (s10[j] < wmin) ? s10[j] : wmin;
            }
          if (memcmp(&wmin, &worst, 8) != 0) ok = false, printf("NC %d h %d variant %d pass %d: worst slack %g, want %g\n", NC, h, variant, pass, worst, wmin);
        }
      }
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(29);
  const int bad = run<2>(rng) + run<3>(rng);
  printf("%d problems\n", bad);
  return bad != 0;
}
