// tests/test_select_kernel_on_host.py: csrc/hmpc_select.hip compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run
// against a plain loop: group sizes either side of a wave and of the workgroup, NaN / +-inf penalties, ineligible status codes, ties (the
// costs are rounded), a group with every command masked, no penalty at all; then the tick expansion against a field-by-field copy.
#include "hmpc_select.hip"
#include <cmath>
#include <cstdio>
#include <random>
int main() {
  std::mt19937 rng(7);
  int bad = 0;
  const int FW = 120, SW = 130;
  for (int K : {1, 3, 64, 65, 130, 300}) {
    const int G = 3, B = G * K;
    std::vector<double> cost(2 * B), pen(B), score(G); std::vector<float> st(B * SW), f(B * FW), of(G * FW, 5.f), os(G * SW, 5.f);
    std::vector<uint32_t> status(B), ostat(G); std::vector<int32_t> idx(G);
    for (int variant = 0; variant < 4; ++variant) {
      for (int i = 0; i < B; ++i) {
        cost[2 * i] = std::round((rng() % 1000) / 10.0) / 10.0, cost[2 * i + 1] = (rng() % 5) / 2.0;
        const int r = rng() % 20;
        pen[i] = r == 0 ? NAN : r == 1 ? INFINITY : r == 2 ? -INFINITY : (rng() % 3) * 0.5;
        if (variant == 2 && i / K == 1) pen[i] = NAN;
        const int c = rng() % 10;
        status[i] = (c < 6 ? 0 : c == 6 ? 6 : c == 7 ? 7 : c == 8 ? 3 : 1) | ((rng() % 40) << 8);
        for (int t = 0; t < FW; ++t) f[i * FW + t] = (float)(rng() % 1000) - 500;
        for (int t = 0; t < SW; ++t) st[i * SW + t] = (float)(rng() % 1000) - 500;
      }
      hmpc::SelectArgs a{cost.data(), st.data(), status.data(), f.data(), variant == 3 ? nullptr : pen.data(), G, K, FW, SW, idx.data(), score.data(), of.data(), ostat.data(), os.data()};
      if (hmpc::launch_select(a, nullptr) != hipSuccess) return 2;
      for (int g = 0; g < G; ++g) {
        int best = -1; double bs = INFINITY;
        for (int k = 0; k < K; ++k) {
          const int i = g * K + k; double s = cost[2 * i] + cost[2 * i + 1]; if (a.penalty) s = s + pen[i];
          const uint32_t c = status[i] & 0xff;
          if ((c == 0 || c == 6) && std::isfinite(s) && (best < 0 || s < bs)) best = k, bs = s;
        }
        bool ok = idx[g] == best && memcmp(&score[g], &bs, 8) == 0 && ostat[g] == (best < 0 ? 0xffffffffu : status[g * K + best]);
        for (int t = 0; t < FW; ++t) { float w = best < 0 ? 0.f : f[(g * K + best) * FW + t]; ok = ok && memcmp(&of[g * FW + t], &w, 4) == 0; }
        for (int t = 0; t < SW; ++t) { float w = best < 0 ? 0.f : st[(g * K + best) * SW + t]; ok = ok && memcmp(&os[g * SW + t], &w, 4) == 0; }
        if (!ok) { ++bad; printf("K %d variant %d group %d: got %d want %d\n", K, variant, g, idx[g], best); }
      }
    }
  }
  // expansion
  {
    const int G = 5, K = 7;
    std::vector<hmpc_tick_inputs> t(G), out(G * K); std::vector<hmpc_command> c(G * K); std::vector<double> wpd(2 * G);
    unsigned char *p = (unsigned char *)t.data();
    for (size_t i = 0; i < sizeof(hmpc_tick_inputs) * G; ++i) p[i] = rng();
    for (int g = 0; g < G; ++g) { t[g].position[0] = g * 0.1, t[g].position[1] = -g * 0.1; t[g].world_position_desired[0] = g * 0.1 + (g - 2) * 0.04; t[g].world_position_desired[1] = -g * 0.1 - (g - 2) * 0.04; }
    p = (unsigned char *)c.data();
    for (size_t i = 0; i < sizeof(hmpc_command) * G * K; ++i) p[i] = rng();
    if (hmpc::launch_expand_ticks(t.data(), G, c.data(), K, out.data(), wpd.data(), nullptr) != hipSuccess) return 2;
    for (int i = 0; i < G * K; ++i) {
      hmpc_tick_inputs w = t[i / K];
      memcpy(w.v_des_robot, c[i].v_des_robot, 16); memcpy(&w.yaw_rate_des, &c[i].yaw_rate_des, 8); memcpy(&w.roll_des, &c[i].roll_des, 8); memcpy(&w.pitch_des, &c[i].pitch_des, 8);
      if (memcmp(&w, &out[i], sizeof(w))) { ++bad; printf("expand %d differs\n", i); }
    }
    for (int g = 0; g < G; ++g) {
      double x = t[g].world_position_desired[0], p0 = t[g].position[0];
      if (x - p0 > .05) x = p0 + .05; if (p0 - x > .05) x = p0 - .05;
      if (wpd[2 * g] != x) { ++bad; printf("wpd %d\n", g); }
    }
  }
  printf("%d problems\n", bad);
  return bad != 0;
}
