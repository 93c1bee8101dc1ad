// tests/test_limit_adjoint_kernel_on_host.py: csrc/hmpc_limit_adjoint.h -- everything of the limit-gradient kernel behind the assembly --
// compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop that states the definition once
// more, sequentially: h = 1, 3, 10 (HMAX = 10) and h = 11, 20 (HMAX = 20), NC = 2, 3, every output compared as bit patterns.  Variants:
// random data with limits made active; a zero seed and dir (zeros out but lambda); a contact that is swing at every step (exact zeros
// there); ten active limits on every leg-step (five admitted: the block's rank, nothing limits the moment about the normal); an unloaded foot (eight active rows of rank 5: five admitted); a NaN force
// (the run must end); a NaN seed (the run must end); lt = 0 (IEEE division, the rest as before).  On every leg-step of every case the
// admitted set of admitted_normals, and of the plain loop, must be free_directions' (hmpc_feedback.h): the same count, the same vectors.
#include "hmpc_limit_adjoint.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

template <int NC, int HM>
__global__ void limit_adjoint_test_kernel(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj, const float *alpha,
                                          const float *Fc, const float *u, const unsigned char *gait, const float *cap, const double *dir,
                                          const double *seed, int h, double act_tol, double lt, double lh, double *glim, double *gFc, double *gb,
                                          double *lam, double *nu, double *summary) {
  __shared__ hmpc::LimitAdjointKeep<NC, HM> Kp;
  __shared__ hmpc::LimitAdjointWork<NC, HM> Wk;
  hmpc::limit_adjoint_of_instance<NC, HM, hmpc::LADJ_NT>(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, dir, seed, h, act_tol, lt, lh, Kp, Wk, glim,
                                                         gFc, gb, lam, nu, summary);
}

static bool in_stance(float cap, unsigned char g) {
  const double ub = (double)(cap * (float)g);
  return !(ub < 0.0001 && ub > -.0001);
}
static const int SRC[10] = {0, 1, 2, 3, 4, 4, 5, 6, 7, 7};
static const double SIG[10] = {1, 1, 1, 1, 1, -1, -1, -1, 1, -1};
static bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), 8 * a.size()) == 0; }
static double mag(double v) { return std::isnan(v) ? INFINITY : std::fabs(v); }

template <int NC>
struct Out {
  static constexpr int U = 6 * NC;
  std::vector<double> lim, G, gb, lam, nu, summary;
  explicit Out(int h) : lim(3 + NC, -7.0), G(8 * NC * U, -7.0), gb(10 * NC * h, -7.0), lam(10 * NC * h, -7.0), nu(10 * NC * h, -7.0), summary(3, -7.0) {}
  bool equals(const Out &o) const { return same(lim, o.lim) && same(G, o.G) && same(gb, o.gb) && same(lam, o.lam) && same(nu, o.nu) && same(summary, o.summary); }
};

template <int NC>
static int col(int c, int k) {
  return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3);
}

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

// the admitted normals of one leg-step, sequentially: rows[] ascending, q the orthonormal vectors; returns m
template <int NC>
static int admitted(const std::vector<float> &Fc, int c, const double *s, double act_tol, double *q, int *rows) {
  constexpr int U = 6 * NC;
  int m = 0;
  for (int j = 0; j < 10; ++j) {
    if (!(s[j] <= act_tol)) continue;
    double v[6], len2 = 0.0, rem2 = 0.0;
    for (int k = 0; k < 6; ++k) v[k] = SIG[j] * (double)Fc[(8 * c + SRC[j]) * U + col<NC>(c, k)];
    for (int k = 0; k < 6; ++k) len2 = std::fma(v[k], v[k], len2);
    for (int pass = 0; pass < 2; ++pass)
      for (int a = 0; a < m; ++a) {
        double d = 0.0;
        for (int k = 0; k < 6; ++k) d = std::fma(q[6 * a + k], v[k], d);
        for (int k = 0; k < 6; ++k) v[k] = std::fma(0.0 - d, q[6 * a + k], v[k]);
      }
    for (int k = 0; k < 6; ++k) rem2 = std::fma(v[k], v[k], rem2);
    if (m < 6 && rem2 > 0.0 && rem2 >= 1e-12 * len2) {
      const double len = std::sqrt(rem2);
      for (int k = 0; k < 6; ++k) q[6 * m + k] = v[k] / len;
      rows[m++] = j;
    }
  }
  return m;
}

// the plain loop: the definition, sequentially; *pinned counts the leg-steps whose admitted set is not free_directions'
template <int NC>
static Out<NC> plain(const std::vector<float> &x0, const std::vector<float> &Acd, const std::vector<float> &Bcd, const std::vector<float> &W,
                     const std::vector<float> &traj, const std::vector<float> &alpha, const std::vector<float> &Fc, const std::vector<float> &u,
                     const std::vector<unsigned char> &gait, const std::vector<float> &cap, const std::vector<double> &dir,
                     const std::vector<double> &ell, int h, double act_tol, double lt, double lh, int *unpinned, int *most_admitted) {
  constexpr int U = 6 * NC;
  Out<NC> o(h);
  std::vector<double> A(169), B(13 * U), q2(13, 0.0), a2(U);
  for (int t = 0; t < 169; ++t) A[t] = (double)Acd[t];
  for (int t = 0; t < 13 * U; ++t) B[t] = (double)Bcd[t];
  for (int s = 0; s < 12; ++s) q2[s] = (double)W[s] + (double)W[s];
  for (int c = 0; c < U; ++c) a2[c] = (double)alpha[c] + (double)alpha[c];
  std::vector<double> x(13 * (h + 1)), dx(13 * (h + 1), 0.0), c(13 * (h + 2), 0.0), d(13 * (h + 2), 0.0);
  for (int s = 0; s < 13; ++s) x[s] = (double)x0[s];
  for (int i = 0; i < h; ++i)
    for (int s = 0; s < 13; ++s) {
      double acc = 0.0;
      for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], x[13 * i + k], acc);
      for (int cc = 0; cc < U; ++cc) acc = std::fma(B[s * U + cc], (double)u[U * i + cc], acc);
      x[13 * (i + 1) + s] = acc;
      acc = 0.0;
      for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], dx[13 * i + k], acc);
      for (int cc = 0; cc < U; ++cc) acc = std::fma(B[s * U + cc], dir[U * i + cc], acc);
      dx[13 * (i + 1) + s] = acc;
    }
  for (int j = h; j >= 1; --j)  // rows j at 13 j
    for (int s = 0; s < 13; ++s) {
      double tc = 0.0, td = 0.0;
      for (int k = 0; k < 13; ++k) tc = std::fma(A[k * 13 + s], c[13 * (j + 1) + k], tc), td = std::fma(A[k * 13 + s], d[13 * (j + 1) + k], td);
      if (s < 12) {
        tc = std::fma(q2[s], x[13 * j + s] - (double)traj[12 * (j - 1) + s], tc);
        td = std::fma(q2[s], dx[13 * j + s], td);
      }
      c[13 * j + s] = tc, d[13 * j + s] = td;
    }
  std::vector<double> grad(U * h), rho(U * h);
  for (int i = 0; i < h; ++i)
    for (int k = 0; k < U; ++k) {
      double ac = 0.0, ad = 0.0;
      for (int a = 0; a < 13; ++a) ac = std::fma(B[a * U + k], c[13 * (i + 1) + a], ac), ad = std::fma(B[a * U + k], d[13 * (i + 1) + a], ad);
      grad[U * i + k] = std::fma(a2[k], (double)u[U * i + k], ac);
      rho[U * i + k] = ell[U * i + k] + std::fma(a2[k], dir[U * i + k], ad);
    }
  std::fill(o.lam.begin(), o.lam.end(), 0.0), std::fill(o.nu.begin(), o.nu.end(), 0.0);
  double worst[2] = {0.0, 0.0};
  for (int i = 0; i < h; ++i)
    for (int cc = 0; cc < NC; ++cc) {
      const int ls = NC * i + cc;
      if (!in_stance(cap[cc], gait[ls])) continue;
      double s[10], q[36], qf[36];
      int rows[6];
      slacks<NC>(Fc, u, i, cc, cap[cc] * (float)gait[ls], s);
      const int m = admitted<NC>(Fc, cc, s, act_tol, q, rows);
      *most_admitted = m > *most_admitted ? m : *most_admitted;
      {  // the pin: free_directions' count and vectors, and admitted_normals' rows
        unsigned list = 0;
        double qa[36];
        const int mf = hmpc::free_directions<NC>(Fc.data(), cc, s, act_tol, qf), ma = hmpc::admitted_normals<NC>(Fc.data(), cc, s, act_tol, qa, list);
        bool ok = mf == m && ma == m && memcmp(qf, q, 48 * m) == 0 && memcmp(qa, q, 48 * m) == 0;
        for (int b = 0; b < m && ok; ++b) ok = (int)((list >> (4 * b)) & 15u) == rows[b];
        *unpinned += !ok;
      }
      auto N = [&](int j, int k) { return SIG[j] * (double)Fc[(8 * cc + SRC[j]) * U + col<NC>(cc, k)]; };
      for (int which = 0; which < 2; ++which) {
        const std::vector<double> &rhs = which ? rho : grad;
        double xs[6] = {0, 0, 0, 0, 0, 0};
        for (int a = m - 1; a >= 0; --a) {
          double taa = 0.0, y = 0.0, sum = 0.0;
          for (int k = 0; k < 6; ++k) taa = std::fma(q[6 * a + k], N(rows[a], k), taa);
          for (int k = 0; k < 6; ++k) y = std::fma(q[6 * a + k], rhs[U * i + col<NC>(cc, k)], y);
          for (int b = a + 1; b < m; ++b) {
            double tab = 0.0;
            for (int k = 0; k < 6; ++k) tab = std::fma(q[6 * a + k], N(rows[b], k), tab);
            sum = std::fma(tab, xs[b], sum);
          }
          xs[a] = (y - sum) / taa;
        }
        for (int b = 0; b < m; ++b) (which ? o.nu : o.lam)[10 * ls + rows[b]] = xs[b];
        for (int k = 0; k < 6; ++k) {
          double acc = 0.0;
          for (int b = 0; b < m; ++b) acc = std::fma(N(rows[b], k), xs[b], acc);
          const double v = mag(rhs[U * i + col<NC>(cc, k)] - acc);
          worst[which] = v > worst[which] ? v : worst[which];
        }
      }
    }
  std::fill(o.G.begin(), o.G.end(), 0.0);
  double worst_g = 0.0;
  for (int cc = 0; cc < NC; ++cc)
    for (int r = 0; r < 8; ++r)
      for (int k = 0; k < 6; ++k) {
        double acc = 0.0;
        for (int i = 0; i < h; ++i)
          for (int j = 0; j < 10; ++j) {
            if (SRC[j] != r) continue;
            acc = std::fma(0.0 - SIG[j] * o.lam[10 * (NC * i + cc) + j], dir[U * i + col<NC>(cc, k)], acc);
            acc = std::fma(0.0 - SIG[j] * o.nu[10 * (NC * i + cc) + j], (double)u[U * i + col<NC>(cc, k)], acc);
          }
        o.G[(8 * cc + r) * U + col<NC>(cc, k)] = acc;
        worst_g = mag(acc) > worst_g ? mag(acc) : worst_g;
      }
  for (size_t t = 0; t < o.gb.size(); ++t) o.gb[t] = 0.0 - o.nu[t];
  double gm = 0.0, glt = 0.0, glh = 0.0;
  for (int cc = 0; cc < NC; ++cc) {
    gm = gm + o.G[(8 * cc + 1) * U + 3 * cc];
    gm = gm - o.G[(8 * cc + 0) * U + 3 * cc];
    gm = gm + o.G[(8 * cc + 3) * U + 3 * cc + 1];
    gm = gm - o.G[(8 * cc + 2) * U + 3 * cc + 1];
    for (int k = 0; k < 3; ++k) {
      glt = std::fma(o.G[(8 * cc + 5) * U + 3 * cc + k], (double)Fc[(8 * cc + 5) * U + 3 * cc + k], glt);
      glh = std::fma(o.G[(8 * cc + 6) * U + 3 * cc + k], (double)Fc[(8 * cc + 6) * U + 3 * cc + k], glh);
    }
    double acc = 0.0;
    for (int i = 0; i < h; ++i) acc = std::fma(o.gb[10 * (NC * i + cc) + 9], (double)(float)gait[NC * i + cc], acc);
    o.lim[3 + cc] = acc;
  }
  o.lim[0] = gm, o.lim[1] = glt / lt, o.lim[2] = glh / lh;
  o.summary[0] = worst[0], o.summary[1] = worst[1], o.summary[2] = worst_g;
  return o;
}

template <int NC, int HM>
static int run(std::mt19937 &rng, std::initializer_list<int> horizons) {
  constexpr int U = 6 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  for (int h : horizons)
    for (int variant = 0; variant < 8; ++variant) {
      std::vector<float> x0(13), Acd(169), Bcd(13 * U), W(13), traj(12 * h), alpha(U), Fc(8 * NC * U, 0.f), u(U * h), cap(NC);
      std::vector<unsigned char> gait(NC * h);
      std::vector<double> dir((size_t)U * h), ell((size_t)U * h);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : traj) v = uni(-1, 1);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.4, 0.4);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : alpha) v = uni(1e-6, 1e-3);
      for (auto &v : cap) v = uni(100, 300);
      for (auto &v : gait) v = (rng() % 5 == 0) ? 0 : 1;
      const float mu = uni(0.3, 2.0), lt32 = uni(0.05, 0.1), lh32 = uni(0.03, 0.08);
      for (int c = 0; c < NC; ++c) {  // a block of the assembly's shape, the contact frame tilted a little
        float *row = Fc.data() + 8 * c * U;
        const int cf = 3 * c, cm = 3 * NC + 3 * c;
        row[0 * U + cf] = -mu, row[1 * U + cf] = mu, row[2 * U + cf + 1] = -mu, row[3 * U + cf + 1] = mu;
        for (int r = 0; r < 4; ++r) row[r * U + cf + 2] = 1.f;
        const float t0[3] = {1.f + uni(-0.02, 0.02), uni(-0.1, 0.1), uni(-0.1, 0.1)}, t1[3] = {uni(-0.1, 0.1), 1.f + uni(-0.02, 0.02), uni(-0.1, 0.1)};
        const float n[3] = {uni(-0.1, 0.1), uni(-0.1, 0.1), 1.f + uni(-0.02, 0.02)};
        for (int j = 0; j < 3; ++j) {
          row[4 * U + cm + j] = t0[j];
          row[5 * U + cf + j] = -lt32 * n[j], row[5 * U + cm + j] = t1[j];
          row[6 * U + cf + j] = -lh32 * n[j], row[6 * U + cm + j] = (c != 1) ? -t1[j] : t1[j];
        }
        row[7 * U + cf + 2] = 2.f;
      }
      for (int i = 0; i < h; ++i)
        for (int c = 0; c < NC; ++c) {
          float *v = u.data() + U * i;
          const bool st = gait[NC * i + c] != 0;
          const float fz = st ? uni(20, 90) : 0.f;
          v[3 * c] = st ? uni(-5, 5) : 0.f, v[3 * c + 1] = st ? uni(-5, 5) : 0.f, v[3 * c + 2] = fz;
          for (int k = 0; k < 3; ++k) v[3 * NC + 3 * c + k] = st ? uni(-0.004, 0.004) * (k == 0 ? 1.f : 100.f) : 0.f;
          if (st && rng() % 3 == 0) v[3 * c] = fz / mu;             // a friction row at its limit, up to rounding
          if (st && rng() % 4 == 0) v[3 * c + 2] = 0.5f * cap[c];   // the Fz cap
          if (st && rng() % 4 == 0) v[3 * NC + 3 * c] = 0.f;        // the Mx floor
        }
      for (auto &v : dir) v = (double)uni(-1, 1);
      for (auto &v : ell) v = (double)uni(-1, 1);
      for (int i = 0; i < h; ++i)  // no direction and no force on swing leg-steps
        for (int c = 0; c < NC; ++c)
          if (!gait[NC * i + c])
            for (int k = 0; k < 6; ++k) dir[U * i + col<NC>(c, k)] = 0.0;
      double act_tol = 1e-3, lt = (double)lt32, lh = (double)lh32;
      if (variant == 1) for (size_t t = 0; t < dir.size(); ++t) dir[t] = 0.0, ell[t] = 0.0;
      if (variant == 2)
        for (int i = 0; i < h; ++i) {
          gait[NC * i] = 0;
          for (int k = 0; k < 6; ++k) u[U * i + col<NC>(0, k)] = 0.f, dir[U * i + col<NC>(0, k)] = 0.0;
        }
      if (variant == 3) act_tol = 1e30;  // every limit of every stance leg-step is active
      if (variant == 4) {                // an unloaded foot at step 0
        gait[0] = 1;
        for (int k = 0; k < 6; ++k) u[col<NC>(0, k)] = 0.f;
      }
      if (variant == 5) u[rng() % u.size()] = NAN;
      if (variant == 6) ell[rng() % ell.size()] = NAN;
      if (variant == 7) lt = 0.0;
      Out<NC> got(h);
      hipLaunchKernelGGL((limit_adjoint_test_kernel<NC, HM>), dim3(1), dim3(hmpc::LADJ_NT), 0, nullptr, x0.data(), Acd.data(), Bcd.data(), W.data(),
                         traj.data(), alpha.data(), Fc.data(), u.data(), gait.data(), cap.data(), dir.data(), ell.data(), h, act_tol, lt, lh,
                         got.lim.data(), got.G.data(), got.gb.data(), got.lam.data(), got.nu.data(), got.summary.data());
      int unpinned = 0, most = 0;
      const Out<NC> want = plain<NC>(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, dir, ell, h, act_tol, lt, lh, &unpinned, &most);
      bool ok = true;
      if (!got.equals(want))
        ok = false, printf("NC %d HMAX %d h %d variant %d: differ from the plain loop (limits %d Fc %d bound %d lambda %d nu %d summary %d)\n", NC, HM, h,
                           variant, same(got.lim, want.lim), same(got.G, want.G), same(got.gb, want.gb), same(got.lam, want.lam), same(got.nu, want.nu),
                           same(got.summary, want.summary));
      if (unpinned) ok = false, printf("NC %d HMAX %d h %d variant %d: %d leg-steps whose admitted set is not free_directions'\n", NC, HM, h, variant, unpinned);
      if (variant == 1) {
        bool z = true;
        for (const auto *v : {&got.lim, &got.G, &got.gb, &got.nu})
          for (double e : *v) z = z && e == 0.0;
        if (!z) ok = false, printf("NC %d HMAX %d h %d: a zero seed and outputs that are not 0\n", NC, HM, h);
      }
      if (variant == 2)
        for (int i = 0; i < h; ++i)
          for (int j = 0; j < 10; ++j)
            if (got.lam[10 * NC * i + j] != 0.0 || got.nu[10 * NC * i + j] != 0.0 || got.gb[10 * NC * i + j] != 0.0)
              ok = false, printf("NC %d HMAX %d h %d: multipliers on a swing contact are not 0\n", NC, HM, h);
      if (variant == 2) {
        for (int r = 0; r < 8; ++r)
          for (int k = 0; k < U; ++k)
            if (got.G[r * U + k] != 0.0) ok = false;
        if (got.lim[3] != 0.0) ok = false;
      }
      if (variant == 3 && most != 5) ok = false, printf("NC %d HMAX %d h %d: ten active limits and %d admitted\n", NC, HM, h, most);
      if (variant == 4) {  // rows 0 1 2 3 4 6 7 8 are active on the unloaded foot: rank 5
        int nz = 0;
        for (int j = 0; j < 10; ++j) nz += got.lam[j] != 0.0 || got.nu[j] != 0.0;
        if (nz > 5) ok = false, printf("NC %d HMAX %d h %d: an unloaded foot with %d multipliers\n", NC, HM, h, nz);
      }
      if (variant == 7 && !(std::isnan(got.lim[1]) || std::isinf(got.lim[1]))) ok = false, printf("NC %d HMAX %d h %d: lt = 0 and a finite grad_lt\n", NC, HM, h);
      if (variant == 0 || variant == 4)
        for (const auto *v : {&got.lim, &got.G, &got.gb, &got.lam, &got.nu, &got.summary})
          for (double e : *v)
            if (!std::isfinite(e)) ok = false;
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(41);
  const int bad = run<2, 10>(rng, {1, 3, 10}) + run<2, 20>(rng, {11, 20}) + run<3, 10>(rng, {1, 5, 10});
  printf("%d problems\n", bad);
  return bad != 0;
}
