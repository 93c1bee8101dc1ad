// tests/test_schur_tile_index.py: csrc/hmpc_schur_tiles.h -- the lane-constant index arithmetic of the block start's Schur tiles --
// compiled for the CPU and run against the plain per-entry expressions it replaces (schur_load / schur_store as they stood before:
// restated below), for NTG = 3 .. 6, the wave counts the variants use (4 and 8), every wave, lane, tile slot and r, and every k0
// from 0 to 16 NTG.  Prints the number of problems found.
#include <stdio.h>

#include <vector>

#include "hmpc_schur_tiles.h"

using namespace hmpc;

static long problems = 0, checked = 0;
#define EXPECT(cond, ...)                                    \
  do {                                                       \
    ++checked;                                               \
    if (!(cond)) {                                           \
      if (++problems <= 20) printf(__VA_ARGS__), printf("\n"); \
    }                                                        \
  } while (0)

// ---- the plain expressions (per entry) ------------------------------------------------------------------------------------------
// high word of a positive double with binary exponent ex (what the loader reads from the diagonal of S0)
static int hi_word(int ex) { return ((1023 + ex) << 20) | 0x5a5a5; }
struct Plain {
  int k0;
  const std::vector<int> &diag_hi;  // high word of S0_ii, i < k0; rows >= k0 hold whatever was there before
  int kof(int i) const {
    if (i >= k0) return 0;
    const int ex = ((diag_hi[i] >> 20) & 2047) - 1023;
    return -(ex >> 1);
  }
  // schur_load: entry (i, j) of the grid
  bool load_valid(int i, int j) const { return (i < j ? j : i) < k0; }
  int load_offset(int i, int j) const {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return hi * (hi + 1) / 2 + lo;
  }
  int load_exp(int i, int j) const { return kof(i) + kof(j); }
  // schur_store: kexp[i] = kof(i) for every i < 16 NTG (schur_scale_exponents)
  bool store_valid(int i, int j) const { return i <= j && j < k0; }
  int store_offset(int i, int j) const { return j * (j + 1) / 2 + i; }
};

template <int NTG, int NWV, int WV>
static void check_wave(const Plain &P) {
  if constexpr (mfs_count(NTG, NWV, WV) > 0) {  // (six tiles on eight waves: two waves hold none)
  constexpr MfsTiles<NTG, NWV, WV> T;
  constexpr int CNT = mfs_count(NTG, NWV, WV);
  static_assert(CNT <= MfsGrid<NTG, NWV>::TPW, "tiles per wave");
  for (int t = 0; t < CNT; ++t) {
    const int I = T.i[t], J = T.j[t];
    EXPECT(I <= J && J < NTG && mfs_owner(NTG, NWV, I, J) == WV, "deal: NTG %d NWV %d wave %d slot %d", NTG, NWV, WV, t);
    bool any_valid = false;
    for (int lane = 0; lane < 64; ++lane) {
      const SchurLane L = schur_lane(lane);
      EXPECT(L.g == lane / 16 && L.c == lane % 16, "lane %d", lane);
      const int j = 16 * J + L.c;
      const int ct = schur_col_tri(L, J);
      const bool cv = schur_col_valid(L, J, P.k0);
      EXPECT(ct == j * (j + 1) / 2, "tri(j): J %d lane %d", J, lane);
      const int kc = schur_exponent(P.diag_hi[j], cv);
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + 4 * r + L.g;
        const int rt = schur_row_tri(L, I, r);
        const bool rv = schur_row_valid(L, I, r, P.k0);
        const int kr = schur_exponent(P.diag_hi[i], rv);
        EXPECT(rt == i * (i + 1) / 2, "tri(i): I %d r %d lane %d", I, r, lane);
        // load
        const bool lv = schur_load_valid(I, J, cv, rv);
        EXPECT(lv == P.load_valid(i, j), "load validity: NTG %d k0 %d (%d, %d)", NTG, P.k0, i, j);
        const int off = schur_offset(L, I, J, r, ct, rt);
        EXPECT(off == P.load_offset(i, j), "load offset: NTG %d (%d, %d): %d", NTG, i, j, off);
        EXPECT(off >= 0 && off < 16 * NTG * (16 * NTG + 1) / 2, "load offset outside the triangle: NTG %d (%d, %d): %d", NTG, i, j, off);
        EXPECT(kr + kc == P.load_exp(i, j), "exponent sum: NTG %d k0 %d (%d, %d): %d", NTG, P.k0, i, j, kr + kc);
        EXPECT(schur_on_diagonal(L, I, J, r) == (i == j), "diagonal: (%d, %d)", i, j);
        any_valid = any_valid || lv;
        // store (exponents from kexp: kof of both, which is what the load's pair gives for a valid entry)
        const bool sv = cv && schur_store_valid(L, I, J, r, true);
        EXPECT(sv == P.store_valid(i, j), "store validity: NTG %d k0 %d (%d, %d)", NTG, P.k0, i, j);
        if (sv) EXPECT(schur_offset_upper(L, I, r, ct) == P.store_offset(i, j), "store offset: (%d, %d)", i, j);
        if (sv) EXPECT(schur_tile_live(J, P.k0), "a dead tile stores: k0 %d (%d, %d)", P.k0, i, j);
      }
    }
    EXPECT(schur_tile_live(J, P.k0) == any_valid, "liveness: NTG %d k0 %d tile (%d, %d)", NTG, P.k0, I, J);
    if (schur_tile_live(J, P.k0)) EXPECT(schur_tile_live(I, P.k0), "J live, I dead: k0 %d tile (%d, %d)", P.k0, I, J);
  }
  }
}

template <int NTG, int NWV, int WV = 0>
static void check_waves(const Plain &P) {
  if constexpr (WV < NWV) {
    check_wave<NTG, NWV, WV>(P);
    check_waves<NTG, NWV, WV + 1>(P);
  }
}

template <int NTG>
static void check_grid() {
  // every tile of the grid has exactly one owner among the waves
  for (int nwv : {4, 8})
    for (int I = 0; I < NTG; ++I)
      for (int J = I; J < NTG; ++J) EXPECT(mfs_owner(NTG, nwv, I, J) >= 0 && mfs_owner(NTG, nwv, I, J) < nwv, "owner: NTG %d (%d, %d)", NTG, I, J);
  std::vector<int> diag(16 * NTG);
  for (int k0 = 0; k0 <= 16 * NTG; ++k0) {
    // exponents of S0_ii from 2^-9 to 2^13, odd and even, varied with the row and with k0; rows >= k0: anything at all
    for (int i = 0; i < 16 * NTG; ++i) diag[i] = i < k0 ? hi_word(((i * 7 + k0 * 3) % 23) - 9) : (int)(0x7ff80000u ^ (unsigned)(i * 2654435761u));
    const Plain P{k0, diag};
    check_waves<NTG, 4>(P);
    check_waves<NTG, 8>(P);
    // the pivot steps: never inside a dead tile row
    EXPECT(schur_steps(k0) == (k0 + 3) / 4, "steps: k0 %d", k0);
    for (int s = 0; s < schur_steps(k0); ++s) EXPECT(schur_tile_live(s >> 2, k0), "step %d of k0 %d pivots in dead tile row %d", s, k0, s >> 2);
  }
}

int main() {
  check_grid<3>();
  check_grid<4>();
  check_grid<5>();
  check_grid<6>();
  printf("%ld checks, %ld problems\n", checked, problems);
  return problems != 0;
}
