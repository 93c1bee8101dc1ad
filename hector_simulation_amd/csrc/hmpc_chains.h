// hmpc_chains.h -- the chains of stages A3 / A4 (powers of Acd, Phi_k = Acd^k Bcd, tracking error e), defined once over a compact table of the powers.
//
// Acd = I + dt A_ct has the structure  rows 0..2: columns 6..8 (dt Rbi);  row 3 + i: column 9 + i (dt);  row 11: column 12 (-dt);  the diagonal 1.
// In every power Acd^k exactly FOURTEEN entries ever differ from the identity's bits:
//     (i, j), i = 0..2, j = 6..8        slots 0..8   (3 i + j - 6)
//     (3, 9), (4, 10)                   slots 9, 10
//     (5, 11), (5, 12)                  slots 11, 12
//     (11, 12)                          slot 13
// every other entry is exactly 1.0f (diagonal) or +0.0f: its four-term chain adds products with an exact structural zero to a sum started at +0,
// which round-to-nearest leaves at +0 whatever the sign of the product (HMPC-A1).  A power is therefore kept as 16 floats
// (CH_SLOTS): the fourteen live entries, one slot holding 1.0f (CH_ONE) and one holding +0.0f (CH_ZERO); chains_slot maps (row, column) of the
// 13 x 13 power to its slot, so that every operand of a chain reads the same bits from the compact table as from the full matrix.
//
// The chains themselves are the four-term ones of the items they replace -- the same ffma, operands and order, padding terms included:
//   * power step: entry (i, j) of Acd^(k+1) from row i of Acd^k and column j of Acd (chains_power_terms).  A live entry's chain reads identity
//     constants and the entry itself; the two entries of row 5 also read each other ((5, 12) in its first term, (5, 11) in its padding terms),
//     so a lane carries a pair: its own entry and its partner's (itself for the twelve entries that have none).  The powers are then fourteen
//     scalar recurrences in registers: no LDS read and no barrier between steps;
//   * Phi item (i, j) of Phi_k and e item s of e_k: four operands of Acd^k / Acd^(k+1) through the slot map, four right-hand factors (a column
//     of Bcd, x0) that do not depend on k.
// A lane finds its terms and slots in tables of 4-bit entries packed into 64-bit constants, built at compile time from the plain statements
// of the structure below (chains_*_term, chains_slot): a shift and a mask per entry, no branch -- and a power operand is picked by bit masks,
// not by a select the compiler may turn into a branch in the loop.
// Plain functions over values and pointers to the caller's arrays; stage_a_chains (hmpc_kernel.h) calls them from its lanes.  Compiles under
// hipcc and, for tests/test_chains_on_host.py, as plain C++ against tests/src/hip_lane_shim.
#pragma once
#include "hmpc_math.h"

namespace hmpc {

constexpr int CH_LIVE = 14, CH_ONE = 14, CH_ZERO = 15, CH_SLOTS = 16;

// ---- the structure, stated plainly (evaluated at compile time only)
// the table of the live entries: slot L -> (row, column)
constexpr int chains_live_row(const int L) { return L < 9 ? L / 3 : (L == 9 ? 3 : (L == 10 ? 4 : (L < 13 ? 5 : 11))); }
constexpr int chains_live_col(const int L) { return L < 9 ? 6 + L % 3 : (L < 12 ? L : 12); }
// (row, column) of a power -> its slot in the compact table
constexpr int chains_slot(const int r, const int m) {
  return (r < 3 && m >= 6 && m < 9) ? 3 * r + m - 6
         : ((r == 3 || r == 4) && m == r + 6) ? r + 6
         : (r == 5 && (m == 11 || m == 12)) ? m
         : (r == 11 && m == 12) ? 13
         : (r == m ? CH_ONE : CH_ZERO);
}
// the lane that carries the other entry of row 5 (itself for the entries that have none)
constexpr int chains_partner(const int L) { return L == 11 ? 12 : (L == 12 ? 11 : L); }
// slots [0, CH_SLOTS) of the identity
constexpr float chains_identity_slot(const int t) { return t == CH_ONE ? 1.0f : 0.0f; }

// Term t < 4 of a chain sum_m P(row, m) C(m, col): the index m, ascending over the structurally non-zero ones; a chain with fewer live terms
// pads with a term whose right-hand factor is a structural zero (row 12 / row 0 of Acd, row 0 of Bcd; column 0 of the power for e).
// entry (., j) of the next power: column j of Acd has its diagonal and rows 0..2 (j = 6..8), row j - 6 (j = 9..11), row 11 (j = 12)
constexpr int chains_power_term(const int j, const int t) {
  const int pad = (j == 12) ? 0 : 12;
  const bool w3 = j >= 6 && j < 9;
  return t == 3 ? j : (w3 ? t : (t == 0 ? ((j >= 9 && j < 12) ? j - 6 : (j == 12 ? 11 : pad)) : pad));
}
// entry (., j) of Phi_k: the column of a force component has rows 6..8 and row 9 + j % 3 of Bcd, a moment column rows 6..8.
// c = j % 3 for a force column, 3 for a moment column
constexpr int chains_phi_term(const int c, const int t) { return t < 3 ? 6 + t : (c < 3 ? 9 + c : 0); }
// entry s of Acd^(k+1) x0: row s of a power has its diagonal and columns 6..8 (s < 3), s + 6 (s = 3, 4), 11 and 12 (s = 5), 12 (s = 11)
constexpr int chains_e_term(const int s, const int t) {
  return t == 0 ? s
         : t == 1 ? ((s < 3) ? 6 : ((s < 5) ? s + 6 : ((s == 5) ? 11 : ((s == 11) ? 12 : 0))))
         : t == 2 ? ((s < 3) ? 7 : ((s == 5) ? 12 : 0))
                  : ((s < 3) ? 8 : 0);
}

// ---- the same as tables: sixteen 4-bit entries in a 64-bit constant
typedef unsigned long long chains_word;
constexpr chains_word chains_pack(int (*f)(int)) {
  chains_word w = 0;
  for (int i = 0; i < 16; ++i) w |= (chains_word)(f(i) & 15) << (4 * i);
  return w;
}
__device__ __forceinline__ int chains_entry(const chains_word w, const int i) { return (int)(w >> (4 * i)) & 15; }
// lane L of the power phase: term and slot of its chain's term T; item s of e; row i of a power under the terms of a Phi column of class C
template <int T> constexpr int chains_lane_term(const int L) { return chains_power_term(chains_live_col(L), T); }
template <int T> constexpr int chains_lane_slot(const int L) { return chains_slot(chains_live_row(L), chains_lane_term<T>(L)); }
template <int T> constexpr int chains_e_term_of(const int s) { return chains_e_term(s, T); }
template <int T> constexpr int chains_e_slot_of(const int s) { return chains_slot(s, chains_e_term(s, T)); }
template <int T, int C> constexpr int chains_phi_slot_of(const int i) { return chains_slot(i, chains_phi_term(C, T)); }

__device__ __forceinline__ unsigned chains_bits(const float x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ float chains_float(const unsigned b) { return __builtin_bit_cast(float, b); }

__device__ __forceinline__ float chains_chain4(const float (&p)[4], const float (&c)[4]) {
  float acc = ffma(p[0], c[0], 0.0f);
  acc = ffma(p[1], c[1], acc);
  acc = ffma(p[2], c[2], acc);
  return ffma(p[3], c[3], acc);
}

// ---- the power recurrences: one lane per live entry
// What the loop relies on, proved from the statements above: the last term of a live entry's chain reads the entry itself (times the diagonal
// of Acd), its first three terms read identity constants or -- row 5 -- the partner's entry, never the entry itself or a third one.
constexpr bool chains_power_shape_ok() {
  for (int L = 0; L < CH_LIVE; ++L) {
    const int i = chains_live_row(L), j = chains_live_col(L);
    if (chains_slot(i, chains_power_term(j, 3)) != L) return false;
    for (int t = 0; t < 3; ++t) {
      const int s = chains_slot(i, chains_power_term(j, t));
      if (s < CH_LIVE && (s == L || s != chains_partner(L))) return false;
    }
  }
  return true;
}
static_assert(chains_power_shape_ok(), "a power lane carries its own entry and its partner's, nothing else");
struct ChainsPowerLane {
  float f[2][4];        // the Acd factors of the lane's own chain [0] and of its partner's [1]
  unsigned other[2][3]; // the power operand of term t < 3 = (the pair's other entry & other) | one: all ones where the term reads that entry,
  unsigned one[2][3];   //   the bits of the identity constant where it reads one (1.0f; +0.0f is no bit at all)
  float v[2];           // the two entries of the current power
};
template <int T>
__device__ __forceinline__ void chains_power_setup_term(ChainsPowerLane &P, const int w, const int Lw, const int Lo, const float *Acd) {
  constexpr chains_word TERM = chains_pack(&chains_lane_term<T>), SLOT = chains_pack(&chains_lane_slot<T>), COL = chains_pack(&chains_live_col);
  P.f[w][T] = Acd[chains_entry(TERM, Lw) * 13 + chains_entry(COL, Lw)];
  if constexpr (T < 3) {
    const int s = chains_entry(SLOT, Lw);
    P.other[w][T] = (s == Lo) ? ~0u : 0u;
    P.one[w][T] = (s == CH_ONE) ? chains_bits(1.0f) : 0u;
  }
}
// L < CH_LIVE; Acd: the 13 x 13 matrix.  Leaves the lane at the identity (every live entry is off the diagonal: +0).
__device__ __forceinline__ void chains_power_setup(ChainsPowerLane &P, const int L, const float *Acd) {
  const int Lp = ((L == 11) | (L == 12)) ? (L ^ 7) : L;  // chains_partner
  static_assert(chains_partner(11) == (11 ^ 7) && chains_partner(12) == (12 ^ 7) && chains_partner(13) == 13 && chains_partner(0) == 0, "");
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int Lw = w ? Lp : L, Lo = w ? L : Lp;
    chains_power_setup_term<0>(P, w, Lw, Lo, Acd);
    chains_power_setup_term<1>(P, w, Lw, Lo, Acd);
    chains_power_setup_term<2>(P, w, Lw, Lo, Acd);
    chains_power_setup_term<3>(P, w, Lw, Lo, Acd);
    P.v[w] = 0.0f;
  }
}
// Acd^k -> Acd^(k+1) for the lane's pair
__device__ __forceinline__ void chains_power_step(ChainsPowerLane &P) {
  const unsigned vb[2] = {chains_bits(P.v[0]), chains_bits(P.v[1])};
  float nv[2];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    float p[4];
#pragma unroll
    for (int t = 0; t < 3; ++t) p[t] = chains_float((vb[1 - w] & P.other[w][t]) | P.one[w][t]);
    p[3] = P.v[w];
    nv[w] = chains_chain4(p, P.f[w]);
  }
  P.v[0] = nv[0], P.v[1] = nv[1];
}

// ---- the Phi and e items: four slots of a power, four right-hand factors
struct ChainsItem {
  int s[4];
  float c[4];
};
template <int T>
__device__ __forceinline__ void chains_phi_item_term(ChainsItem &it, const int i, const int j, const int c, const int U, const float *Bcd) {
  constexpr chains_word S0 = chains_pack(&chains_phi_slot_of<T, 0>), S1 = chains_pack(&chains_phi_slot_of<T, 1>),
                        S2 = chains_pack(&chains_phi_slot_of<T, 2>), S3 = chains_pack(&chains_phi_slot_of<T, 3>);
  const chains_word sw = (T < 3) ? S0 : (c == 0 ? S0 : (c == 1 ? S1 : (c == 2 ? S2 : S3)));  // (terms 0..2 are the same for every column)
  const int m = (T < 3) ? 6 + T : (c < 3 ? 9 + c : 0);
  it.s[T] = chains_entry(sw, i);
  it.c[T] = Bcd[m * U + j];
}
// entry r = i U + j of Phi_k = Acd^k Bcd (Bcd: 13 x U, U = 6 NC)
template <int NC>
__device__ __forceinline__ void chains_phi_item(ChainsItem &it, const int r, const float *Bcd) {
  constexpr int U = 6 * NC;
  const int i = r / U, j = r % U, c = (j < 3 * NC) ? j % 3 : 3;
  static_assert(chains_phi_term(0, 3) == 9 && chains_phi_term(2, 3) == 11 && chains_phi_term(3, 3) == 0 && chains_phi_term(3, 1) == 7, "the m of chains_phi_item_term");
  chains_phi_item_term<0>(it, i, j, c, U, Bcd);
  chains_phi_item_term<1>(it, i, j, c, U, Bcd);
  chains_phi_item_term<2>(it, i, j, c, U, Bcd);
  chains_phi_item_term<3>(it, i, j, c, U, Bcd);
}
template <int T>
__device__ __forceinline__ void chains_e_item_term(ChainsItem &it, const int s, const float *x0) {
  constexpr chains_word TERM = chains_pack(&chains_e_term_of<T>), SLOT = chains_pack(&chains_e_slot_of<T>);
  it.s[T] = chains_entry(SLOT, s);
  it.c[T] = x0[chains_entry(TERM, s)];
}
// entry s < 13 of Acd^(k+1) x0
__device__ __forceinline__ void chains_e_item(ChainsItem &it, const int s, const float *x0) {
  chains_e_item_term<0>(it, s, x0);
  chains_e_item_term<1>(it, s, x0);
  chains_e_item_term<2>(it, s, x0);
  chains_e_item_term<3>(it, s, x0);
}
// the item's value from one power (pw: its CH_SLOTS floats)
__device__ __forceinline__ float chains_item_value(const ChainsItem &it, const float *pw) {
  const float p[4] = {pw[it.s[0]], pw[it.s[1]], pw[it.s[2]], pw[it.s[3]]};
  return chains_chain4(p, it.c);
}

}  // namespace hmpc
