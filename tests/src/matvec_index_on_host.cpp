// tests/test_matvec_index.py: csrc/hmpc_matvec_index.h -- the lane constants and the coefficient of gather_w -- compiled for the CPU
// and run against the plain per-use expressions they replace (gather_w as it stood before: restated below).
//   coefficient: ac in {-1, 0, +1} in every one of the eight byte positions of the packed word (the other bytes filled with all three
//     values), sgn in {-1, +1} handed in as a literal the way the kernel hands it in, cf over +-0, denormals, +-inf, NaNs and random bit
//     patterns: equal BIT FOR BIT;
//   addresses: every thread index below NMAX of every shape (NMAX = 60, 120, 180, 240; two or three contacts): the column of Cn, the
//     eight rows, the act / slot words and the slot bytes against S.Cn[leg][rr][t % 6], Q.act[8 * (t / 6)], (sm >> 8 rr) & 0xff.
// Prints the number of problems found.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hmpc_matvec_index.h"

using namespace hmpc;

static long problems = 0, checked = 0;
#define EXPECT(cond, ...)                                      \
  do {                                                         \
    ++checked;                                                 \
    if (!(cond)) {                                             \
      if (++problems <= 20) printf(__VA_ARGS__), printf("\n"); \
    }                                                          \
  } while (0)

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return b;
}
static double from_bits(uint64_t b) {
  double v;
  memcpy(&v, &b, sizeof v);
  return v;
}

// ---- the plain expressions ---------------------------------------------------------------------------------------------------------
// (sgn arrives as a literal after inlining, in the kernel and here: sgn * cf and -sgn * cf are then cf or its negation)
template <int SGN>
static double plain_coef(unsigned long long am, int rr, double cf) {
  const double sgn = (double)SGN;
  const int ac = (int)(signed char)((am >> (8 * rr)) & 0xff);
  return (ac == 0) ? 0.0 : ((ac > 0) ? sgn * cf : -sgn * cf);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static void check_coef() {
  const uint64_t special[] = {
      0x0000000000000000ull, 0x8000000000000000ull,  // +-0
      0x0000000000000001ull, 0x8000000000000001ull,  // smallest denormals
      0x000fffffffffffffull, 0x800fffffffffffffull,  // largest denormals
      0x0010000000000000ull, 0x8010000000000000ull,  // smallest normals
      0x7fefffffffffffffull, 0xffefffffffffffffull,  // largest finite
      0x7ff0000000000000ull, 0xfff0000000000000ull,  // +-inf
      0x7ff8000000000000ull, 0xfff8000000000000ull,  // quiet NaNs
      0x7ff8000000000abcull, 0xfff80000deadbeefull,  // ... with payloads
      0x3ff0000000000000ull, 0xbff0000000000000ull,  // +-1
  };
  const int nspecial = (int)(sizeof special / sizeof special[0]);
  const signed char acs[3] = {-1, 0, 1};
  for (int i = 0; i < nspecial + 4000; ++i) {
    const uint64_t cb = i < nspecial ? special[i] : next_u64();
    const double cf = from_bits(cb);
    if (i >= nspecial && cf != cf) continue;  // (random NaN patterns may be signalling: the plain expression's literal fold is for quiet values)
    for (int rr = 0; rr < 8; ++rr)
      for (int a = 0; a < 3; ++a)
        for (int fill = 0; fill < 3; ++fill) {
          unsigned long long am = 0;
          for (int b = 0; b < 8; ++b) am |= (unsigned long long)(unsigned char)(b == rr ? acs[a] : acs[(fill + b) % 3]) << (8 * b);
          const uint64_t wp = bits_of(plain_coef<1>(am, rr, cf)), gp = bits_of(mv_coef(am, rr, false, cf));
          const uint64_t wn = bits_of(plain_coef<-1>(am, rr, cf)), gn = bits_of(mv_coef(am, rr, true, cf));
          EXPECT(wp == gp, "coef sgn +1: cf %016llx ac %d row %d: plain %016llx, new %016llx", (unsigned long long)cb, acs[a], rr,
                 (unsigned long long)wp, (unsigned long long)gp);
          EXPECT(wn == gn, "coef sgn -1: cf %016llx ac %d row %d: plain %016llx, new %016llx", (unsigned long long)cb, acs[a], rr,
                 (unsigned long long)wn, (unsigned long long)gn);
        }
  }
}

// ---- addresses: a mock of the shared-memory members gather_w reads -----------------------------------------------------------------
template <int NMAX, int NC>
static void check_shape() {
  constexpr int NG = NMAX / 6, MMAX = 8 * NG;
  static double Cn[NC][8][6];
  static unsigned char ls_leg[NG];
  alignas(8) static signed char act[MMAX];
  alignas(8) static unsigned char slot[MMAX];
  for (int round = 0; round < 3; ++round) {
    for (int e = 0; e < NG; ++e) ls_leg[e] = (unsigned char)(next_u64() % NC);
    for (int c = 0; c < MMAX; ++c) act[c] = (signed char)((int)(next_u64() % 3) - 1), slot[c] = (unsigned char)next_u64();
    for (int t = 0; t < NMAX; ++t) {
      const int v_e = t / 6, v_k = t % 6;  // the plain expressions
      const int vleg = ls_leg[v_e];
      EXPECT(mv_var_e(t) == v_e && mv_var_k(t) == v_k, "NMAX %d: t %d -> e %d k %d", NMAX, t, mv_var_e(t), mv_var_k(t));
      const MvLane L = mv_lane(mv_var_e(t), mv_var_k(t), ls_leg[mv_var_e(t)]);
      const double *cncol = &Cn[0][0][0] + L.cn_col;
      unsigned long long am, sm, am_plain, sm_plain;
      memcpy(&am, &act[L.row0], 8), memcpy(&sm, &slot[L.row0], 8);
      memcpy(&am_plain, &act[8 * v_e], 8), memcpy(&sm_plain, &slot[8 * v_e], 8);
      EXPECT(L.row0 + 8 <= MMAX && &act[L.row0] == &act[8 * v_e] && am == am_plain && sm == sm_plain, "NMAX %d: t %d act / slot word", NMAX, t);
      for (int rr = 0; rr < 8; ++rr) {
        EXPECT(cncol + mv_cn_row(rr) == &Cn[vleg][rr][v_k], "NMAX %d NC %d: t %d row %d: Cn offset %d, plain %d", NMAX, NC, t, rr,
               (int)(cncol + mv_cn_row(rr) - &Cn[0][0][0]), (int)(&Cn[vleg][rr][v_k] - &Cn[0][0][0]));
        EXPECT(mv_slot(sm, rr) == (int)((sm_plain >> (8 * rr)) & 0xff) && mv_slot(sm, rr) == slot[8 * v_e + rr], "NMAX %d: t %d row %d slot", NMAX, t, rr);
      }
    }
  }
}

int main() {
  for (int t = 0; t < MV_TID_MAX; ++t)
    EXPECT(mv_div6(t) == t / 6 && mv_var_k(t) == t % 6, "t %d: mv_div6 %d, k %d", t, mv_div6(t), mv_var_k(t));
  check_coef();
  check_shape<60, 2>();
  check_shape<120, 2>();
  check_shape<180, 3>();
  check_shape<240, 2>();
  printf("matvec index: %ld checks, %ld problems\n", checked, problems);
  return problems ? 1 : 0;
}
