// tests/test_rollout_score_kernel_on_host.py: the kernels of csrc/hmpc_rollout_score.h compiled for the CPU against tests/src/hip_lane_shim (one
// thread per lane) and run (a) without arguments, against plain loops written here from the comment of include/hector_mpc.h: the score over
// tick counts either side of a wave and of two passes with NaN, fallen and unsolved rows and every NULL member, the selection over group
// sizes either side of a wave and of the workgroup with NaN / +-inf penalties, ties, a wholly masked group and every subset of outputs; (b)
// with "in out", on one recorded case of tests/rollout_score_mirror.py, whose results the Python test compares with the mirror bit for bit.
#include "hmpc_rollout_score.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

// the contract, one instance: a plain loop with the 64 partial sums in an array
void plain_score(const hmpc_tick_inputs &tk, const hmpc_rollout_cost &c, int n, const double *state, const float *wrench, const double *tau,
                 const int32_t *summary, double *cost, double *score) {
  const double TWO_PI = 6.283185307179586;
  double vdw[2];
  for (int a = 0; a < 2; ++a) vdw[a] = (tk.rBody[a] * tk.v_des_robot[0] + tk.rBody[3 + a] * tk.v_des_robot[1]) + tk.rBody[6 + a] * 0.0;
  double P[2][64], e[12];
  for (int l = 0; l < 64; ++l) P[0][l] = P[1][l] = 0.0;
  for (int k = 0; k < n; ++k) {
    const double t = (double)(k + 1) * c.dt_tick;
    const double ref[12] = {tk.roll_des, tk.pitch_des, tk.rpy[2] + t * tk.yaw_rate_des, tk.position[0] + t * vdw[0], tk.position[1] + t * vdw[1],
                            c.height, 0.0, 0.0, tk.yaw_rate_des, vdw[0], vdw[1], 0.0};
    for (int s = 0; s < 12; ++s) e[s] = state[12 * k + s] - ref[s];
    e[2] = e[2] - TWO_PI * std::nearbyint(e[2] / TWO_PI);
    double trk = 0.0, eff = 0.0;
    for (int s = 0; s < 12; ++s) trk = trk + (c.w_state[s] * e[s]) * e[s];
    if (wrench)
      for (int j = 0; j < 12; ++j) { const double u = (double)wrench[12 * k + j]; eff = eff + (c.w_wrench[j] * u) * u; }
    if (tau)
      for (int j = 0; j < 10; ++j) { const double u = tau[10 * k + j]; eff = eff + (c.w_tau[j] * u) * u; }
    P[0][k % 64] = P[0][k % 64] + trk, P[1][k % 64] = P[1][k % 64] + eff;
  }
  for (int q = 0; q < 2; ++q)
    for (int off = 32; off > 0; off >>= 1) {
      double N[64];
      for (int l = 0; l < 64; ++l) N[l] = P[q][l] + P[q][l ^ off];
      for (int l = 0; l < 64; ++l) P[q][l] = N[l];
    }
  cost[0] = P[0][0], cost[1] = P[1][0], cost[2] = 0.0;
  for (int s = 0; s < 12; ++s) cost[2] = cost[2] + (c.w_terminal[s] * e[s]) * e[s];
  cost[3] = 0.0;
  if (summary) cost[3] = (summary[1] >= 0 ? c.fall_penalty : 0.0) + (summary[2] > 0 ? (double)summary[2] * c.unsolved_penalty : 0.0);
  *score = ((cost[0] + cost[1]) + cost[2]) + cost[3];
}

template <class T> bool same_bits(const T &a, const T &b) { return memcmp(&a, &b, sizeof(T)) == 0; }

int self_check() {
  std::mt19937 rng(11);
  std::normal_distribution<double> nd(0.0, 1.0);
  int bad = 0;
  // ---- score
  for (int n : {1, 2, 63, 64, 65, 128, 130}) {
    for (int variant = 0; variant < 5; ++variant) {
      const int B = 6;  // (two workgroups, the second with two idle waves)
      std::vector<hmpc_tick_inputs> t(B);
      std::vector<double> state((size_t)B * n * 12), tau((size_t)B * n * 10), cost(4 * B + 2, 5.0), score(B + 2, 5.0);
      std::vector<float> wrench((size_t)B * n * 12);
      std::vector<int32_t> summary(4 * B);
      hmpc_rollout_cost c;
      memset(&c, 0, sizeof(c));
      for (int s = 0; s < 12; ++s) c.w_state[s] = 1 + s, c.w_terminal[s] = 0.5 * s, c.w_wrench[s] = 1e-3 * (s + 1);
      for (int j = 0; j < 10; ++j) c.w_tau[j] = 1e-2 * (10 - j);
      c.height = 0.55, c.dt_tick = 0.005, c.fall_penalty = variant == 1 ? 250.0 : INFINITY, c.unsolved_penalty = variant == 2 ? INFINITY : 2.0;
      memset(t.data(), 0, sizeof(hmpc_tick_inputs) * B);
      for (int i = 0; i < B; ++i) {
        for (int k = 0; k < 9; ++k) t[i].rBody[k] = nd(rng);
        for (int k = 0; k < 3; ++k) t[i].position[k] = nd(rng), t[i].rpy[k] = nd(rng);
        t[i].v_des_robot[0] = nd(rng), t[i].v_des_robot[1] = nd(rng), t[i].yaw_rate_des = nd(rng), t[i].roll_des = 0.1 * nd(rng), t[i].pitch_des = 0.1 * nd(rng);
        summary[4 * i] = n, summary[4 * i + 1] = (rng() % 3 == 0) ? (int)(rng() % n) : -1, summary[4 * i + 2] = variant == 2 ? 0 : (int)(rng() % 3), summary[4 * i + 3] = rng() % 30;
      }
      for (auto &v : state) v = 4.0 * nd(rng);  // (yaw errors well beyond pi)
      for (auto &v : tau) v = 3.0 * nd(rng);
      for (auto &v : wrench) v = (float)(20.0 * nd(rng));
      if (variant == 3) state[(size_t)(2 * n + n / 2) * 12 + 5] = NAN;
      hmpc::RolloutScoreArgs a;
      memset(&a, 0, sizeof(a));
      a.cost = c, a.ticks0 = t.data(), a.batch = B, a.n_ticks = n, a.out_cost = cost.data() + 1, a.out_score = score.data() + 1;
      a.log.state = state.data();
      a.log.wrench = variant == 4 ? nullptr : wrench.data(), a.log.tau = (variant == 4 || variant == 1) ? nullptr : tau.data();
      a.log.summary = variant == 4 ? nullptr : summary.data();
      if (hmpc::launch_rollout_score(a, nullptr) != hipSuccess) return 2;
      for (int i = 0; i < B; ++i) {
        double wc[4], ws;
        plain_score(t[i], c, n, state.data() + (size_t)i * n * 12, a.log.wrench ? wrench.data() + (size_t)i * n * 12 : nullptr,
                    a.log.tau ? tau.data() + (size_t)i * n * 10 : nullptr, a.log.summary ? summary.data() + 4 * i : nullptr, wc, &ws);
        bool ok = same_bits(ws, score[1 + i]);
        for (int q = 0; q < 4; ++q) ok = ok && same_bits(wc[q], cost[1 + 4 * i + q]);
        if (variant == 3 && i == 2) ok = ok && std::isnan(score[1 + i]);
        if (variant == 2) ok = ok && (std::isfinite(score[1 + i]) || summary[4 * i + 1] >= 0);
        if (!ok) { ++bad; printf("score n %d variant %d instance %d: got %.17g want %.17g\n", n, variant, i, score[1 + i], ws); }
      }
      if (cost[0] != 5.0 || cost[4 * B + 1] != 5.0 || score[0] != 5.0 || score[B + 1] != 5.0) { ++bad; printf("score n %d: wrote outside\n", n); }
      // either output may be left out
      a.out_cost = nullptr;
      std::vector<double> again(score);
      if (hmpc::launch_rollout_score(a, nullptr) != hipSuccess || memcmp(again.data(), score.data(), again.size() * 8)) { ++bad; printf("score without cost differs\n"); }
    }
  }
  // ---- selection
  for (int K : {1, 3, 64, 65, 130, 300}) {
    const int G = 3, B = G * K, n = 2;
    std::vector<double> sc(B), pen(B), tau((size_t)B * n * 10), oscore(G), otau(G * 10);
    std::vector<float> wrench((size_t)B * n * 12), owrench(G * 12);
    std::vector<int32_t> summary(4 * B), oidx(G), osum(G * 4);
    for (int variant = 0; variant < 5; ++variant) {
      for (int i = 0; i < B; ++i) {
        sc[i] = std::round((rng() % 1000) / 10.0) / 10.0;
        const int r = rng() % 20;
        if (r == 0) sc[i] = NAN; else if (r == 1) sc[i] = INFINITY; else if (r == 2) sc[i] = -0.0;
        const int p = rng() % 20;
        pen[i] = p == 0 ? NAN : p == 1 ? INFINITY : p == 2 ? -INFINITY : (rng() % 3) * 0.5;
        if (variant == 2 && i / K == 1) pen[i] = NAN;
        for (int q = 0; q < 4; ++q) summary[4 * i + q] = rng() % 50;
      }
      for (auto &v : tau) v = nd(rng);
      for (auto &v : wrench) v = (float)nd(rng);
      std::fill(oscore.begin(), oscore.end(), 5.0), std::fill(otau.begin(), otau.end(), 5.0), std::fill(owrench.begin(), owrench.end(), 5.f);
      std::fill(oidx.begin(), oidx.end(), 5), std::fill(osum.begin(), osum.end(), 5);
      hmpc::RolloutSelectArgs a;
      memset(&a, 0, sizeof(a));
      a.score = sc.data(), a.penalty = variant == 3 ? nullptr : pen.data(), a.groups = G, a.group_size = K, a.n_ticks = n;
      a.log.wrench = wrench.data(), a.log.tau = tau.data(), a.log.summary = summary.data();
      const bool part = variant == 4;  // only index and tau asked for
      a.choice.index = oidx.data(), a.choice.tau = otau.data();
      if (!part) a.choice.score = oscore.data(), a.choice.wrench = owrench.data(), a.choice.summary = osum.data();
      if (hmpc::launch_rollout_select(a, nullptr) != hipSuccess) return 2;
      for (int g = 0; g < G; ++g) {
        int best = -1; double bs = INFINITY;
        for (int k = 0; k < K; ++k) {
          const int i = g * K + k; double s = sc[i]; if (a.penalty) s = s + pen[i];
          if (std::isfinite(s) && (best < 0 || s < bs)) best = k, bs = s;
        }
        const int w = g * K + (best < 0 ? 0 : best);
        bool ok = oidx[g] == best;
        for (int q = 0; q < 10; ++q) { const double v = best < 0 ? 0.0 : tau[(size_t)w * n * 10 + q]; ok = ok && same_bits(v, otau[g * 10 + q]); }
        if (!part) {
          ok = ok && same_bits(bs, oscore[g]);
          for (int q = 0; q < 12; ++q) { const float v = best < 0 ? 0.f : wrench[(size_t)w * n * 12 + q]; ok = ok && same_bits(v, owrench[g * 12 + q]); }
          for (int q = 0; q < 4; ++q) ok = ok && osum[g * 4 + q] == (best < 0 ? (q == 1 ? -1 : 0) : summary[4 * w + q]);
        } else {
          ok = ok && oscore[g] == 5.0 && owrench[g * 12] == 5.f && osum[g * 4] == 5;
        }
        if (!ok) { ++bad; printf("select K %d variant %d group %d: got %d want %d\n", K, variant, g, oidx[g], best); }
      }
    }
    // an output whose log member is missing is refused
    hmpc::RolloutSelectArgs a;
    memset(&a, 0, sizeof(a));
    a.score = sc.data(), a.groups = G, a.group_size = K, a.n_ticks = n, a.choice.index = oidx.data(), a.choice.wrench = owrench.data();
    if (hmpc::launch_rollout_select(a, nullptr) != hipErrorInvalidValue) { ++bad; printf("select: a wrench without a log was launched\n"); }
  }
  printf("%d problems\n", bad);
  return bad != 0;
}

template <class T> std::vector<T> take(FILE *f, size_t count, bool present = true) {
  std::vector<T> v(present ? count : 0);
  if (present && count && fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "short case file\n"); exit(3); }
  return v;
}

template <class T> void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int run_case(const char *in, const char *out) {
  FILE *f = fopen(in, "rb");
  if (!f) return 3;
  const std::vector<int32_t> hd = take<int32_t>(f, 8);
  const int kind = hd[0], B = hd[1], n = hd[2], K = hd[6];
  const bool has_w = hd[3], has_t = hd[4], has_s = hd[5], has_p = hd[7];
  const size_t rows = (size_t)B * n;
  FILE *o = fopen(out, "wb");
  if (!o) return 3;
  if (kind == 0) {
    auto c = take<hmpc_rollout_cost>(f, 1);
    auto t = take<hmpc_tick_inputs>(f, B);
    auto state = take<double>(f, rows * 12);
    auto wrench = take<float>(f, rows * 12, has_w);
    auto tau = take<double>(f, rows * 10, has_t);
    auto summary = take<int32_t>(f, (size_t)B * 4, has_s);
    std::vector<double> cost((size_t)B * 4), score(B);
    hmpc::RolloutScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.cost = c[0], a.ticks0 = t.data(), a.batch = B, a.n_ticks = n, a.out_cost = cost.data(), a.out_score = score.data();
    a.log.state = state.data(), a.log.wrench = has_w ? wrench.data() : nullptr, a.log.tau = has_t ? tau.data() : nullptr;
    a.log.summary = has_s ? summary.data() : nullptr;
    if (hmpc::launch_rollout_score(a, nullptr) != hipSuccess) return 2;
    put(o, cost), put(o, score);
  } else {
    const int G = B / K;
    auto sc = take<double>(f, B);
    auto pen = take<double>(f, B, has_p);
    auto wrench = take<float>(f, rows * 12, has_w);
    auto tau = take<double>(f, rows * 10, has_t);
    auto summary = take<int32_t>(f, (size_t)B * 4, has_s);
    std::vector<int32_t> oidx(G), osum(has_s ? G * 4 : 0);
    std::vector<double> oscore(G), otau(has_t ? G * 10 : 0);
    std::vector<float> owrench(has_w ? G * 12 : 0);
    hmpc::RolloutSelectArgs a;
    memset(&a, 0, sizeof(a));
    a.score = sc.data(), a.penalty = has_p ? pen.data() : nullptr, a.groups = G, a.group_size = K, a.n_ticks = n;
    a.log.wrench = has_w ? wrench.data() : nullptr, a.log.tau = has_t ? tau.data() : nullptr, a.log.summary = has_s ? summary.data() : nullptr;
    a.choice.index = oidx.data(), a.choice.score = oscore.data();
    a.choice.wrench = has_w ? owrench.data() : nullptr, a.choice.tau = has_t ? otau.data() : nullptr, a.choice.summary = has_s ? osum.data() : nullptr;
    if (hmpc::launch_rollout_select(a, nullptr) != hipSuccess) return 2;
    put(o, oidx), put(o, oscore), put(o, owrench), put(o, otau), put(o, osum);
  }
  fclose(f), fclose(o);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 3) return run_case(argv[1], argv[2]);
  return self_check();
}
