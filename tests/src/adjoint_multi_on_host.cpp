// tests/test_adjoint_multi_kernel_on_host.py: csrc/hmpc_adjoint_multi.h -- everything of the multi-seed adjoint kernel behind the assembly
// -- compiled for the CPU against tests/src/hip_lane_shim (one thread per lane).  The oracle is adjoint_of_instance of csrc/hmpc_adjoint.h
// under each seed alone (itself pinned to a plain loop by tests/src/adjoint_on_host.cpp): every output of every seed of a tile compared
// as bit patterns.  Shapes: (h 10, NC 2) standing, (10, 2) walking with a swing foot at step 0, (11 in HMAX 20, 2), (10, 3); S = 1, 2 and
// the whole tile.  Variants: random seeds; a zero seed among them (zeros out); a seed that lives on a swing contact alone (zeros out); a
// NaN in one seed only (the other seeds' bits are the single-seed ones all the same); all ten limits active (every output exactly 0); an
// unloaded foot (eight active rows of rank 5).  Slots of the outputs behind the last seed must stay untouched.
#include "hmpc_adjoint_multi.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

template <int NC, int HM>
__global__ void single_kernel(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj, const float *alpha,
                              const float *Fc, const float *u, const unsigned char *gait, const float *cap, const double *seed, int h,
                              double act_tol, double *gx0, double *gtraj, double *gw, double *galpha, double *dir, double *summary) {
  __shared__ hmpc::FeedbackKeep<NC, HM> Kp;
  __shared__ hmpc::AdjointKeep<NC, HM> Ak;
  __shared__ hmpc::AdjointWork<NC, HM> Wk;
  hmpc::adjoint_of_instance<NC, HM, hmpc::FB_NT>(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, seed, h, act_tol, Kp, Ak, Wk, gx0, gtraj, gw, galpha,
                                                 dir, summary);
}

template <int NC, int HM>
__global__ void multi_kernel(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj, const float *alpha,
                             const float *Fc, const float *u, const unsigned char *gait, const float *cap, const double *seed, int ns,
                             hmpc::AdjointMultiStride St, int h, double act_tol, double *gx0, double *gtraj, double *gw, double *galpha,
                             double *dir, double *summary) {
  constexpr int ST = hmpc::adjoint_seed_tile<NC>();
  __shared__ hmpc::FeedbackKeep<NC, HM> Kp;
  __shared__ hmpc::AdjointMultiKeep<HM> Ak;
  __shared__ hmpc::AdjointMultiWork<NC, HM, ST> Wk;
  hmpc::adjoint_multi_of_instance<NC, HM, hmpc::FB_NT, ST>(x0, Acd, Bcd, W, traj, alpha, Fc, u, gait, cap, seed, ns, St, h, act_tol, Kp, Ak, Wk, gx0,
                                                           gtraj, gw, galpha, dir, summary);
}

static bool same(const double *a, const double *b, size_t n) { return memcmp(a, b, 8 * n) == 0; }
static const double UNTOUCHED = -7.0;

enum Variant { RANDOM, ZERO_SEED, SWING_SEED, NAN_SEED, ALL_ACTIVE, UNLOADED, N_VARIANTS };
enum Gait { STANDING, WALKING };

template <int NC, int HM>
static int run(std::mt19937 &rng, const int h, const Gait gaitkind) {
  constexpr int U = 6 * NC, C8 = 8 * NC, ST = hmpc::adjoint_seed_tile<NC>();
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  auto col = [&](int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); };
  for (int variant = 0; variant < N_VARIANTS; ++variant)
    for (int S : {1, 2, ST}) {
      std::vector<float> x0(13), Acd(169), Bcd(13 * U), W(13), traj(12 * h), alpha(U), Fc(C8 * U, 0.f), u(U * h), cap(NC, 500.f);
      std::vector<unsigned char> gait(NC * h, 1);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : traj) v = uni(-1, 1);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.02, 0.02);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : alpha) v = uni(1e-6, 1e-3);
      for (auto &v : u) v = uni(-50, 150);
      if (gaitkind == WALKING)  // contact 0 swings at steps 0 .. 4, contact 1 at steps 5 .. 9, and so on
        for (int i = 0; i < h; ++i) gait[NC * i + (i / 5) % 2] = 0;
      for (int c = 0; c < NC; ++c)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) Fc[(8 * c + j) * U + col(c, k)] = (rng() % 4 == 0) ? 0.f : uni(-1, 1);
      double act_tol = 40.0;  // random data: active sets of every size
      if (variant == ALL_ACTIVE) act_tol = 1e30, gait.assign(NC * h, 1);  // rank 6 on every leg-step: nothing free
      if (variant == UNLOADED) {  // eight rows spanning five dimensions; zero forces make rows 0-4, 6, 7, 8 active
        float basis[5][6];
        for (int b = 0; b < 5; ++b)
          for (int k = 0; k < 6; ++k) basis[b][k] = (k == b ? 1.f : 0.f) + (k == 5 ? (float)(b + 1) : 0.f);
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k)
            Fc[j * U + col(0, k)] = j < 5 ? basis[j][k] : (j == 5 ? basis[0][k] + basis[1][k] : (j == 6 ? basis[1][k] - basis[2][k] : basis[3][k] + basis[4][k]));
        for (int k = 0; k < U; ++k) u[k] = 0.f;
        gait[0] = 1;
        act_tol = 1e-3;
      }
      // seeds [S][h][U], outputs [S][..] with one instance per slice (the strides of a batch of one), one slice of slack behind them
      const size_t nseed = (size_t)h * U;
      std::vector<double> seeds((size_t)S * nseed);
      for (auto &v : seeds) v = (double)uni(-1, 1);
      const int special = (S > 1) ? 1 : 0;  // the seed the variant is about
      double *sp = &seeds[special * nseed];
      if (variant == ZERO_SEED) for (size_t t = 0; t < nseed; ++t) sp[t] = 0.0;
      if (variant == NAN_SEED) {  // on a contact in stance, where the seed is read
        const int i = (int)(rng() % (unsigned)h), cc = gait[NC * i] ? 0 : 1;
        sp[(size_t)U * i + col(cc, (int)(rng() % 6))] = NAN;
      }
      if (variant == SWING_SEED) {  // contact 0 swings at every step; the seed lives on it alone
        for (int i = 0; i < h; ++i) gait[NC * i] = 0, gait[NC * i + 1] = 1;
        for (int i = 0; i < h; ++i)
          for (int c = 0; c < U; ++c) {
            const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
            if (cc != 0) sp[(size_t)U * i + c] = 0.0;
          }
      }
      const hmpc::AdjointMultiStride St = {nseed, 13, (size_t)h * 12, 12, (size_t)U, nseed, 2};
      std::vector<double> gx0((S + 1) * St.x0, UNTOUCHED), gtraj((S + 1) * St.traj, UNTOUCHED), gw((S + 1) * St.weights, UNTOUCHED),
          galpha((S + 1) * St.alpha, UNTOUCHED), dir((S + 1) * St.dir, UNTOUCHED), summary((S + 1) * St.summary, UNTOUCHED);
      hipLaunchKernelGGL((multi_kernel<NC, HM>), dim3(1), dim3(hmpc::FB_NT), 0, nullptr, x0.data(), Acd.data(), Bcd.data(), W.data(), traj.data(),
                         alpha.data(), Fc.data(), u.data(), gait.data(), cap.data(), seeds.data(), S, St, h, act_tol, gx0.data(), gtraj.data(), gw.data(),
                         galpha.data(), dir.data(), summary.data());
      bool ok = true;
      for (int s = 0; s < S; ++s) {
        std::vector<double> x(13, UNTOUCHED), t((size_t)h * 12, UNTOUCHED), w(12, UNTOUCHED), a(U, UNTOUCHED), d(nseed, UNTOUCHED), sm(2, UNTOUCHED);
        hipLaunchKernelGGL((single_kernel<NC, HM>), dim3(1), dim3(hmpc::FB_NT), 0, nullptr, x0.data(), Acd.data(), Bcd.data(), W.data(), traj.data(),
                           alpha.data(), Fc.data(), u.data(), gait.data(), cap.data(), &seeds[s * nseed], h, act_tol, x.data(), t.data(), w.data(), a.data(),
                           d.data(), sm.data());
        const bool e[6] = {same(&gx0[s * St.x0], x.data(), 13),       same(&gtraj[s * St.traj], t.data(), t.size()), same(&gw[s * St.weights], w.data(), 12),
                           same(&galpha[s * St.alpha], a.data(), U), same(&dir[s * St.dir], d.data(), d.size()),    same(&summary[s * St.summary], sm.data(), 2)};
        if (!(e[0] && e[1] && e[2] && e[3] && e[4] && e[5]))
          ok = false, printf("NC %d h %d gait %d variant %d S %d seed %d: differs from the single-seed adjoint (x0 %d traj %d weights %d alpha %d dir %d summary %d)\n",
                             NC, h, (int)gaitkind, variant, S, s, e[0], e[1], e[2], e[3], e[4], e[5]);
        if (summary[s * St.summary] != summary[0]) ok = false, printf("NC %d h %d variant %d S %d: summary[0] differs between seeds\n", NC, h, variant, S);
        const bool zero_expected = variant == ALL_ACTIVE || (s == special && (variant == ZERO_SEED || variant == SWING_SEED));
        if (zero_expected) {
          bool z = summary[s * St.summary + 1] == 0.0;
          for (size_t k = 0; k < 13; ++k) z = z && gx0[s * St.x0 + k] == 0.0;
          for (size_t k = 0; k < nseed; ++k) z = z && dir[s * St.dir + k] == 0.0;
          for (size_t k = 0; k < (size_t)U; ++k) z = z && galpha[s * St.alpha + k] == 0.0;
          if (!z) ok = false, printf("NC %d h %d variant %d S %d seed %d: outputs that must be exactly 0 are not\n", NC, h, variant, S, s);
        }
        if (variant == NAN_SEED && s != special && !std::isfinite(summary[s * St.summary + 1]))
          ok = false, printf("NC %d h %d S %d seed %d: a NaN in seed %d reached this one\n", NC, h, S, s, special);
      }
      for (const auto *v : {&gx0, &gtraj, &gw, &galpha, &dir, &summary})  // the slice behind the last seed
        for (size_t k = v->size() - v->size() / (S + 1); k < v->size(); ++k)
          if ((*v)[k] != UNTOUCHED) ok = false, printf("NC %d h %d variant %d S %d: wrote behind the last seed\n", NC, h, variant, S), k = v->size();
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(47);
  const int bad = run<2, 10>(rng, 10, STANDING) + run<2, 10>(rng, 10, WALKING) + run<2, 20>(rng, 11, WALKING) + run<3, 10>(rng, 10, STANDING);
  printf("%d problems\n", bad);
  return bad != 0;
}
