// tests/test_adjoint_kernel_on_host.py: csrc/hmpc_adjoint.h -- everything of the adjoint kernel behind the assembly -- compiled for the CPU
// against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop that states the definition once more, sequentially:
// h = 1, 3, 20 and NC = 2, 3, every output compared as bit patterns.  Variants: random data and a random seed; a zero seed (zeros out);
// an unloaded foot (eight active rows of rank 5: one free direction); nothing active; all legs in swing; a NaN force (the run must end);
// a NaN seed (the run must end); every limit active (no free direction: dir and every gradient exactly 0); a seed on swing contacts
// alone (zeros out, and finite entries there change no bit of the outputs of a random seed).
#include "hmpc_adjoint.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

constexpr int HM = 20;

template <int NC>
__global__ void adjoint_test_kernel(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj, const float *alpha,
                                    const float *Fc, const float *u, const unsigned char *gait, const float *cap, const double *seed, int h,
                                    double act_tol, double *gx0, double *gtraj, double *gw, double *galpha, double *dir, double *summary) {
  __shared__ hmpc::FeedbackKeep<NC, HM> Kp;
  __shared__ hmpc::AdjointKeep<NC, HM> Ak;
  __shared__ hmpc::AdjointWork<NC, HM> Wk;
  hmpc::adjoint_of_instance<NC, HM, hmpc::FB_NT>(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, seed, h, act_tol, Kp, Ak, Wk, gx0, gtraj, gw, galpha,
                                                 dir, summary);
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
  std::vector<double> gx0, gtraj, gw, galpha, dir, summary;
  std::vector<int> fr, held;  // free directions per step, normals held per leg-step
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
  Plain(const std::vector<float> &x0, const std::vector<float> &Acd, const std::vector<float> &Bcd, const std::vector<float> &W,
        const std::vector<float> &traj, const std::vector<float> &alpha, const std::vector<float> &Fc, const std::vector<float> &u,
        const std::vector<unsigned char> &gait, const std::vector<float> &cap, const std::vector<double> &ell, int h, double act_tol)
      : gx0(13), gtraj((size_t)h * 12), gw(12), galpha(U), dir((size_t)h * U), summary(2), fr(h), held(NC * h) {
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
    std::vector<double> P(169, 0.0), PA(169), PB(13 * U), M(169), Kall((size_t)h * 13 * U, 0.0), kall((size_t)h * U, 0.0), S(13 * U, 0.0), p(13, 0.0), pn(13);
    for (int s = 0; s < 13; ++s) P[14 * s] = q2[s];
    double pivmin = 1.0;
    for (int i = h - 1; i >= 0; --i) {
      const int r = fr[i];
      double *K = &Kall[(size_t)13 * U * i], *kv = &kall[(size_t)U * i];
      const double *li = &ell[(size_t)U * i];
      std::vector<double> Z((size_t)U * (r > 0 ? r : 1), 0.0), v(U);
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
      for (int c = 0; c < U; ++c) {
        double acc = 0.0;
        for (int k = 0; k < 13; ++k) acc = std::fma(B[k * U + c], p[k], acc);
        v[c] = li[c] + acc;
      }
      if (r > 0) {
        std::vector<double> Wm(U * U), WZ(U * r), G(r * r), L(r * r, 0.0), X(r * 14);  // (column 13 of X: the vector y)
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
        for (int a = 0; a < r; ++a) {
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = std::fma(Z[col(zc[a], k) * r + a], B[s * U + col(zc[a], k)], acc);
            X[a * 14 + s] = acc;
          }
          double acc = 0.0;
          for (int k = 0; k < 6; ++k) acc = std::fma(Z[col(zc[a], k) * r + a], v[col(zc[a], k)], acc);
          X[a * 14 + 13] = acc;
        }
        for (int j = 0; j < r; ++j) {
          double ss = 0.0;
          for (int bb = 0; bb < j; ++bb) ss = std::fma(L[j * r + bb], L[j * r + bb], ss);
          const double d = G[j * r + j] - ss, pr = d / G[j * r + j], pv = (pr == pr) ? pr : 0.0;
          pivmin = (pv < pivmin) ? pv : pivmin;
          L[j * r + j] = std::sqrt(d);
          for (int a = j + 1; a < r; ++a) {
            double acc = 0.0;
            for (int bb = 0; bb < j; ++bb) acc = std::fma(L[a * r + bb], L[j * r + bb], acc);
            L[a * r + j] = (G[a * r + j] - acc) / L[j * r + j];
          }
        }
        for (int s = 0; s < 14; ++s) {
          for (int a = 0; a < r; ++a) {
            double acc = 0.0;
            for (int bb = 0; bb < a; ++bb) acc = std::fma(L[a * r + bb], X[bb * 14 + s], acc);
            X[a * 14 + s] = (X[a * 14 + s] - acc) / L[a * r + a];
          }
          for (int a = r - 1; a >= 0; --a) {
            double acc = 0.0;
            for (int bb = a + 1; bb < r; ++bb) acc = std::fma(L[bb * r + a], X[bb * 14 + s], acc);
            X[a * 14 + s] = (X[a * 14 + s] - acc) / L[a * r + a];
          }
        }
        for (int c = 0; c < U; ++c) {
          const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
          for (int s = 0; s < 14; ++s) {
            double acc = 0.0;
            for (int bb = first[cc]; bb < first[cc] + 6 - held[NC * i + cc]; ++bb) acc = std::fma(Z[c * r + bb], X[bb * 14 + s], acc);
            if (s < 13) S[c * 13 + s] = acc;
            else kv[c] = 0.0 - acc;
          }
        }
        for (int c = 0; c < U; ++c)
          for (int s = 0; s < 13; ++s) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(S[c * 13 + k], PA[k * 13 + s], acc);
            K[c * 13 + s] = 0.0 - acc;
          }
      }
      for (int k = 0; k < 13; ++k)
        for (int s = 0; s < 13; ++s) {
          double acc = 0.0;
          for (int c = 0; c < U; ++c) acc = std::fma(B[k * U + c], K[c * 13 + s], acc);
          M[k * 13 + s] = A[k * 13 + s] + acc;
        }
      for (int s = 0; s < 13; ++s) {
        double acc = 0.0;
        for (int k = 0; k < 13; ++k) acc = std::fma(M[k * 13 + s], p[k], acc);
        for (int c = 0; c < U; ++c) acc = std::fma(K[c * 13 + s], li[c], acc);
        pn[s] = acc;
      }
      p = pn;
      if (i > 0)
        for (int s = 0; s < 13; ++s)
          for (int t = s; t < 13; ++t) {
            double acc = 0.0;
            for (int k = 0; k < 13; ++k) acc = std::fma(PA[k * 13 + s], M[k * 13 + t], acc);
            const double val = (s == t) ? q2[s] + acc : acc;
            P[s * 13 + t] = val, P[t * 13 + s] = val;
          }
    }
    gx0 = p;
    std::vector<double> dx(13, 0.0), x(13), nx(13), ndx(13);
    for (int s = 0; s < 13; ++s) x[s] = (double)x0[s];
    for (int s = 0; s < 12; ++s) gw[s] = 0.0;
    for (int i = 0; i < h; ++i) {
      double *du = &dir[(size_t)U * i];
      for (int c = 0; c < U; ++c) {
        double acc = 0.0;
        for (int s = 0; s < 13; ++s) acc = std::fma(Kall[(size_t)13 * U * i + c * 13 + s], dx[s], acc);
        du[c] = acc + kall[(size_t)U * i + c];
      }
      for (int s = 0; s < 13; ++s) {
        double acc = 0.0;
        for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], dx[k], acc);
        for (int c = 0; c < U; ++c) acc = std::fma(B[s * U + c], du[c], acc);
        ndx[s] = acc;
        acc = 0.0;
        for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], x[k], acc);
        for (int c = 0; c < U; ++c) acc = std::fma(B[s * U + c], (double)u[U * i + c], acc);
        nx[s] = acc;
      }
      dx = ndx, x = nx;
      for (int s = 0; s < 12; ++s) {
        gtraj[(size_t)12 * i + s] = 0.0 - q2[s] * dx[s];
        const double e = x[s] - (double)traj[12 * i + s];
        gw[s] = std::fma(e + e, dx[s], gw[s]);
      }
    }
    double dmax = 0.0;
    for (double dv : dir) {
      const double a = std::fabs(dv), val = (a == a) ? a : INFINITY;
      dmax = (val > dmax) ? val : dmax;
    }
    for (int c = 0; c < U; ++c) {
      double acc = 0.0;
      for (int i = 0; i < h; ++i) {
        const double uv = (double)u[U * i + c];
        acc = std::fma(uv + uv, dir[(size_t)U * i + c], acc);
      }
      galpha[c] = acc;
    }
    summary[0] = pivmin, summary[1] = dmax;
  }
};

template <int NC>
struct Got {
  static constexpr int U = 6 * NC;
  std::vector<double> gx0, gtraj, gw, galpha, dir, summary;
  explicit Got(int h) : gx0(13, -7.0), gtraj((size_t)h * 12, -7.0), gw(12, -7.0), galpha(U, -7.0), dir((size_t)h * U, -7.0), summary(2, -7.0) {}
  bool equals(const Got &o) const {
    return same(gx0.data(), o.gx0.data(), 13) && same(gtraj.data(), o.gtraj.data(), gtraj.size()) && same(gw.data(), o.gw.data(), 12) &&
           same(galpha.data(), o.galpha.data(), U) && same(dir.data(), o.dir.data(), dir.size()) && same(summary.data(), o.summary.data(), 2);
  }
  bool zeros() const {
    for (const auto *v : {&gx0, &gtraj, &gw, &galpha, &dir})
      for (double e : *v)
        if (e != 0.0) return false;
    return summary[1] == 0.0;
  }
};

template <int NC>
static int run(std::mt19937 &rng) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  auto col = [&](int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); };
  for (int h : {1, 3, 20})
    for (int variant = 0; variant < 9; ++variant) {
      std::vector<float> x0(13), Acd(169), Bcd(13 * U), W(13), traj(12 * h), alpha(U), Fc(C8 * U, 0.f), u(U * h), cap(NC, 500.f);
      std::vector<unsigned char> gait(NC * h);
      std::vector<double> ell((size_t)U * h);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : traj) v = uni(-1, 1);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.02, 0.02);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : alpha) v = uni(1e-6, 1e-3);
      for (auto &v : u) v = uni(-50, 150);
      for (auto &v : ell) v = (double)uni(-1, 1);
      for (auto &g : gait) g = (variant == 3) ? 0 : (rng() % 4 != 0);
      for (int c = 0; c < NC; ++c)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) Fc[(8 * c + j) * U + col(c, k)] = (rng() % 4 == 0) ? 0.f : uni(-1, 1);
      double act_tol = 1e-3;
      if (variant == 0 || variant == 8) act_tol = 40.0;  // random data: active sets of every size
      if (variant == 1) {                                // the unloaded foot: eight rows spanning five dimensions; zero forces make rows 0-4, 6, 7, 8 active
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
      if (variant == 5) ell[rng() % ell.size()] = NAN;             // a NaN seed
      if (variant == 6) act_tol = 1e30, gait.assign(NC * h, 1);  // all ten limits active on every leg-step: rank 6, nothing free
      if (variant == 7) for (auto &v : ell) v = 0.0;             // a zero seed
      if (variant == 8) {                                        // contact 0 swings at every step; the seed lives on it alone
        for (int i = 0; i < h; ++i) gait[NC * i] = 0, gait[NC * i + 1] = 1;
        for (int i = 0; i < h; ++i)
          for (int c = 0; c < U; ++c) {
            const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
            if (cc != 0) ell[(size_t)U * i + c] = 0.0;
          }
      }
      auto launch = [&](const std::vector<double> &seed) {
        Got<NC> g(h);
        hipLaunchKernelGGL(adjoint_test_kernel<NC>, dim3(1), dim3(hmpc::FB_NT), 0, nullptr, x0.data(), Acd.data(), Bcd.data(), W.data(), traj.data(),
                           alpha.data(), Fc.data(), u.data(), gait.data(), cap.data(), seed.data(), h, act_tol, g.gx0.data(), g.gtraj.data(), g.gw.data(),
                           g.galpha.data(), g.dir.data(), g.summary.data());
        return g;
      };
      const Got<NC> got = launch(ell);
      Plain<NC> want(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, ell, h, act_tol);
      Got<NC> w(h);
      w.gx0 = want.gx0, w.gtraj = want.gtraj, w.gw = want.gw, w.galpha = want.galpha, w.dir = want.dir, w.summary = want.summary;
      bool ok = true;
      if (!got.equals(w)) {
        ok = false;
        printf("NC %d h %d variant %d: differ from the plain loop (x0 %d traj %d weights %d alpha %d dir %d summary %d: %.17g %.17g, want %.17g %.17g)\n", NC,
               h, variant, same(got.gx0.data(), w.gx0.data(), 13), same(got.gtraj.data(), w.gtraj.data(), w.gtraj.size()), same(got.gw.data(), w.gw.data(), 12),
               same(got.galpha.data(), w.galpha.data(), U), same(got.dir.data(), w.dir.data(), w.dir.size()), same(got.summary.data(), w.summary.data(), 2),
               got.summary[0], got.summary[1], w.summary[0], w.summary[1]);
      }
      if (variant == 1 && (want.held[0] != 5 || want.fr[0] != 1)) ok = false, printf("variant 1: %d normals held, %d free\n", want.held[0], want.fr[0]);
      if (variant == 2)
        for (int i = 0; i < h; ++i)
          if (want.fr[i] != U) ok = false, printf("variant 2: free_dims[%d] = %d\n", i, want.fr[i]);
      if ((variant == 3 || variant == 6 || variant == 7 || variant == 8) && !got.zeros())
        ok = false, printf("NC %d h %d variant %d: outputs that must be exactly 0 are not\n", NC, h, variant);
      if ((variant == 3 || variant == 6) && got.summary[0] != 1.0) ok = false, printf("NC %d h %d variant %d: a pivot without a free direction\n", NC, h, variant);
      if (variant != 4 && variant != 5 && !(got.summary[0] > 0.0 && std::isfinite(got.summary[1])))
        ok = false, printf("NC %d h %d variant %d: summary %g %g\n", NC, h, variant, got.summary[0], got.summary[1]);
      if (variant == 5 && !(got.summary[1] == INFINITY || got.zeros())) ok = false, printf("NC %d h %d variant 5: a NaN seed and max|dir| = %g\n", NC, h, got.summary[1]);
      if (variant == 0 || variant == 8) {
        // rows of dir on swing contacts are exactly 0, and other finite seed entries there change no bit
        std::vector<double> ell2(ell);
        for (int i = 0; i < h; ++i)
          for (int c = 0; c < U; ++c) {
            const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
            if (in_stance(cap[cc], gait[NC * i + cc])) continue;
            if (got.dir[(size_t)U * i + c] != 0.0) ok = false, printf("NC %d h %d variant %d: a swing row of dir is not 0\n", NC, h, variant);
            ell2[(size_t)U * i + c] = (double)uni(-5, 5);
          }
        if (!launch(ell2).equals(got)) ok = false, printf("NC %d h %d variant %d: seed entries on swing contacts changed an output\n", NC, h, variant);
      }
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(31);
  const int bad = run<2>(rng) + run<3>(rng);
  printf("%d problems\n", bad);
  return bad != 0;
}
