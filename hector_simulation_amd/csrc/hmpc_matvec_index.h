// Lane constants of the solver's mat-vec path (gather_w of hmpc_kernel.h): everything here is plain C++ (no HIP type or builtin),
// so that it compiles for the device inside hmpc_kernel.h and on the host for tests/test_matvec_index.py, which checks it against
// the plain per-use expressions it replaces (tests/src/matvec_index_on_host.cpp).
//
//  (1) variable t = 6 e + k of leg-step e: e and k by one multiply and one shift, formed ONCE per call; from them the offset of
//      column k of the leg's constraint normals in Smem::Cn (rows are then compile-time offsets of 6 doubles) and the offset of the
//      leg-step's eight act / slot bytes;
//  (2) the coefficient of an active row from the packed act word: sgn * cf, its negation or +0.0 by integer operations on the
//      bits of cf -- no compare, no select, no multiply.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define HMPC_MV_FN __host__ __device__ __forceinline__
#else
#define HMPC_MV_FN inline
#endif

namespace hmpc {

constexpr int MV_GS = 6;          // variables per leg-step
constexpr int MV_TID_MAX = 1024;  // mv_div6 is exact for 0 <= t < 32768; the kernel has at most 1024 threads

// t / 6 for 0 <= t < MV_TID_MAX: 10923 / 65536 = 1/6 + 5.1e-6, so the quotient is exact while 5.1e-6 t < 1/6.  The mask changes no thread
// index; it shows the compiler that the product stays below 2^24 (a full-rate 24-bit multiply instead of the quarter-rate 32-bit one)
HMPC_MV_FN int mv_div6(int t) { return (int)((((unsigned)t & (MV_TID_MAX - 1)) * 10923u) >> 16); }

// what a lane of gather_w keeps for the length of ONE call
struct MvLane {
  int e, k;    // leg-step and position of the variable
  int cn_col;  // offset (doubles) of Cn[leg][0][k] from Cn[0][0][0]; row rr adds mv_cn_row(rr)
  int row0;    // first of the leg-step's eight constraint rows: offset (bytes) of its packed act and slot words
};
HMPC_MV_FN int mv_var_e(int t) { return mv_div6(t); }
HMPC_MV_FN int mv_var_k(int t) { return t - MV_GS * mv_div6(t); }
constexpr int mv_cn_row(int rr) { return MV_GS * rr; }
HMPC_MV_FN int mv_cn_col(int leg, int k) { return 8 * MV_GS * leg + k; }
HMPC_MV_FN MvLane mv_lane(int e, int k, int leg) { return MvLane{e, k, mv_cn_col(leg, k), 8 * e}; }

// Coefficient of row rr (0..7) of a leg-step whose eight act bytes (-1, 0, +1) are packed in `am`, for the multiplier cf:
//     ac == 0: +0.0;   ac > 0: sgn * cf;   ac < 0: -sgn * cf        with sgn = +1 (neg = false) or -1 (neg = true)
// sgn * cf with sgn = +-1 is cf or cf with its sign bit turned over, for every cf (zeros, denormals, infinities and NaNs included:
// no arithmetic instruction touches the value).  Bit 0 of the byte says "active" (+-1 are both odd), bit 7 is the sign of ac.
HMPC_MV_FN double mv_coef(unsigned long long am, int rr, bool neg, double cf) {
  const uint32_t w = (uint32_t)(am >> (32 * (rr >> 2)));
  const int b = 8 * (rr & 3);
  const uint32_t on = (uint32_t)((int32_t)(w << (31 - b)) >> 31);  // all ones when the row is active
  uint32_t flip = w << (24 - b);                                   // bit 31: ac < 0
  if (neg) flip = ~flip;
  uint64_t bits;
  __builtin_memcpy(&bits, &cf, sizeof bits);
  const uint32_t lo = (uint32_t)bits & on;
  const uint32_t hi = (((uint32_t)(bits >> 32)) ^ (flip & 0x80000000u)) & on;
  bits = ((uint64_t)hi << 32) | lo;
  double r;
  __builtin_memcpy(&r, &bits, sizeof r);
  return r;
}
// the slot (index into the multiplier vector) of row rr from the packed slot bytes
HMPC_MV_FN int mv_slot(unsigned long long sm, int rr) { return (int)((sm >> (8 * rr)) & 0xff); }

}  // namespace hmpc
