// tests/test_chains_on_host.py: csrc/hmpc_chains.h -- the power recurrences over the compact table, the Phi and e items -- compiled for the CPU
// against tests/src/hip_lane_shim and compared BIT FOR BIT with the dense chains written out below: every entry of every power
// Acd^k (k <= h, all 169 through the slot map), of Phi_k = Acd^k Bcd (k < h) and of e_k = Acd^(k+1) x0 - X_d (k < h), each a 13-term k-ascending
// fmaf chain from +0 over the full matrices, started at the identity.  The lanes are run the way stage_a_chains (hmpc_kernel.h) runs them:
// lane L < 14 carries its entry (and its partner's) through h steps and stores its slot of every power; an item reads its four slots.
//
// File (little endian): int32 n_cases; per case: int32 h, nc, nb; float32 Acd [nb][169], Bcd [nb][13 * 6 nc], x0 [nb][13], traj [nb][12 h].
#include <cmath>
#include "hmpc_chains.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hmpc;

static int bad = 0;
static long compared = 0, live_bits = 0;
static void differ(const char *what, int cs, int i, int k, int t, float got, float want) {
  ++compared;
  if (memcmp(&got, &want, 4) != 0) {
    if (++bad <= 20) printf("case %d instance %d %s step %d [%d]: got %.9g want %.9g\n", cs, i, what, k, t, got, want);
  }
}

template <int NC>
static void run_instance(int cs, int inst, int h, const float *Acd, const float *Bcd, const float *x0, const float *traj) {
  constexpr int U = 6 * NC, PS = 13 * U;
  // ---- the dense statement
  std::vector<float> Pd((size_t)(h + 1) * 169), Phid((size_t)h * PS), ed((size_t)h * 13);
  for (int t = 0; t < 169; ++t) Pd[t] = (t % 14 == 0) ? 1.0f : 0.0f;
  for (int k = 0; k < h; ++k)
    for (int i = 0; i < 13; ++i)
      for (int j = 0; j < 13; ++j) {
        float acc = 0.0f;
        for (int m = 0; m < 13; ++m) acc = std::fmaf(Pd[k * 169 + i * 13 + m], Acd[m * 13 + j], acc);
        Pd[(k + 1) * 169 + i * 13 + j] = acc;
      }
  for (int k = 0; k < h; ++k) {
    for (int i = 0; i < 13; ++i)
      for (int j = 0; j < U; ++j) {
        float acc = 0.0f;
        for (int m = 0; m < 13; ++m) acc = std::fmaf(Pd[k * 169 + i * 13 + m], Bcd[m * U + j], acc);
        Phid[k * PS + i * U + j] = acc;
      }
    for (int s = 0; s < 13; ++s) {
      float acc = 0.0f;
      for (int m = 0; m < 13; ++m) acc = std::fmaf(Pd[(k + 1) * 169 + s * 13 + m], x0[m], acc);
      const float xd = (s < 12) ? traj[12 * k + s] : 0.0f;
      ed[k * 13 + s] = acc - xd;
    }
  }
  // ---- the header's: phase P ...
  std::vector<float> Pw((size_t)(h + 1) * CH_SLOTS);
  for (int t = 0; t < CH_SLOTS; ++t) Pw[t] = chains_identity_slot(t);
  for (int L = 0; L < CH_SLOTS; ++L) {
    ChainsPowerLane P;
    chains_power_setup(P, L < CH_LIVE ? L : 0, Acd);
    for (int k = 0; k < h; ++k) {
      chains_power_step(P);
      Pw[(k + 1) * CH_SLOTS + L] = (L < CH_LIVE) ? P.v[0] : chains_identity_slot(L);
    }
  }
  for (int k = 0; k <= h; ++k)
    for (int i = 0; i < 13; ++i)
      for (int j = 0; j < 13; ++j) {
        const float want = Pd[k * 169 + i * 13 + j], idv = (i == j) ? 1.0f : 0.0f;
        differ("power", cs, inst, k, i * 13 + j, Pw[k * CH_SLOTS + chains_slot(i, j)], want);
        if (memcmp(&want, &idv, 4) != 0) ++live_bits;
      }
  // ... and phase F
  for (int r = 0; r < PS; ++r) {
    ChainsItem it;
    chains_phi_item<NC>(it, r, Bcd);
    for (int k = 0; k < h; ++k) differ("Phi", cs, inst, k, r, chains_item_value(it, &Pw[k * CH_SLOTS]), Phid[k * PS + r]);
  }
  for (int s = 0; s < 13; ++s) {
    ChainsItem it;
    chains_e_item(it, s, x0);
    for (int k = 0; k < h; ++k) {
      const float xd = (s < 12) ? traj[12 * k + s] : 0.0f;
      differ("e", cs, inst, k, s, chains_item_value(it, &Pw[(k + 1) * CH_SLOTS]) - xd, ed[k * 13 + s]);
    }
  }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](void *p, size_t n) { if (fread(p, 1, n, f) != n) { printf("short file\n"); exit(2); } };
  int n_cases = 0;
  rd(&n_cases, 4);
  for (int cs = 0; cs < n_cases; ++cs) {
    int hd[3];
    rd(hd, sizeof(hd));
    const int h = hd[0], nc = hd[1], nb = hd[2], U = 6 * nc;
    if (h < 1 || h > 20 || (nc != 2 && nc != 3)) { printf("case %d: bad header\n", cs); return 2; }
    std::vector<float> Acd((size_t)nb * 169), Bcd((size_t)nb * 13 * U), x0((size_t)nb * 13), traj((size_t)nb * 12 * h);
    rd(Acd.data(), 4 * Acd.size()), rd(Bcd.data(), 4 * Bcd.size()), rd(x0.data(), 4 * x0.size()), rd(traj.data(), 4 * traj.size());
    for (int i = 0; i < nb; ++i) {
      if (nc == 2) run_instance<2>(cs, i, h, &Acd[(size_t)i * 169], &Bcd[(size_t)i * 13 * U], &x0[(size_t)i * 13], &traj[(size_t)i * 12 * h]);
      else run_instance<3>(cs, i, h, &Acd[(size_t)i * 169], &Bcd[(size_t)i * 13 * U], &x0[(size_t)i * 13], &traj[(size_t)i * 12 * h]);
    }
  }
  printf("%ld values compared, %ld entries of the powers off the identity's bits\n", compared, live_bits);
  printf("%d problems\n", bad);
  return bad != 0;
}
