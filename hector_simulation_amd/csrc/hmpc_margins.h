// hmpc_margins.h -- the constraint margins of every solved instance (hmpc_constraint_margins): everything BEHIND
// the assembly, as device functions over plain LDS arrays, and the penalty kernel that turns the summaries into a mask for
// hmpc_sweep_select.  The kernel that assembles (hmpc_margins.hip) calls margins_of_instance with the constraint block the solve kernel's own
// stage function left in LDS; tests/src/margins_on_host.cpp compiles this header for the CPU (one thread per lane) against a plain loop.
//
// Definition (fixed in include/hector_mpc.h; tests/margins_mirror.py restates it in numpy).  Per instance, U = 6 NC, C8 = 8 NC:
//   c_{i,r} = sum_{k < U} Fc[r][k] u_i[k]        binary64, one ascending chain of explicit fma started at +0, dense
//   contact c is in stance at step i iff stance(cap_c, gait[NC i + c]) (hmpc_record.h); ub7 = fl32(cap_c * (float)gait[NC i + c])
//   slack[i][c][0..3] = c_{8c+0..3}                       friction pyramid
//   slack[i][c][4]    = c_{8c+4}, [5] = (double)0.01f - c_{8c+4}        Mx
//   slack[i][c][6]    = 0.0 - c_{8c+5}, [7] = 0.0 - c_{8c+6}            line contact (toe, heel)
//   slack[i][c][8]    = c_{8c+7}, [9] = (double)ub7 - c_{8c+7}          Fz floor (the row is 2 Fz), Fz cap
//   all ten +inf for a swing leg-step.
//   summary[k], where[k], k < 6: lexicographic (value, index) minima over the stance leg-steps, index = 10 NC i + 10 c + j'.
// Mapping: lane t of the workgroup takes rows t, t + NT, ... of the C8 h (step, row) pairs, then leg-steps t, t + NT, ... of the NC h for
// the minima; pairs are reduced by butterfly shuffles inside a wave and one LDS step across the waves (the scheme of hmpc_select.hip: the
// minimum under a total order does not depend on how the set is split).  No atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_record.h"

namespace hmpc {
constexpr int MARGINS_NT = DERIVED_NT;  // threads per workgroup (one workgroup per instance)
constexpr int MARGINS_WAVES = MARGINS_NT / 64;
constexpr int MARGIN_CLASSES = 6;  // friction, Mx, line contact, Fz floor, Fz cap, friction headroom fraction
constexpr int PENALTY_NT = 256;

struct MarginMin {
  double v;
  int idx;
};

__device__ __forceinline__ double margins_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// a candidate replaces the incumbent iff its value is < the incumbent's, or == with a lower index: NaN never enters
__device__ __forceinline__ MarginMin margin_min(const MarginMin inc, const MarginMin cand) {
  const bool take = cand.v < inc.v || (cand.v == inc.v && cand.idx < inc.idx);
  return take ? cand : inc;
}

// Rows, slacks and reductions of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): Fc[8 NC][6 NC],
// u[h][6 NC], gait[NC h] bytes, cap[NC] (f_max for the feet, the record's own cap for the hand).  Scratch: slack[10 NC h] doubles,
// wave_min[NT / 64][6].  Out: slack_out[h][NC][10], summary_out[6], where_out[6] (each may be nullptr).  Every lane of the workgroup
// calls it; begins and ends with a barrier.
template <int NC, int NT>
__device__ __forceinline__ void margins_of_instance(const float *Fc, const float *u, const unsigned char *gait, const float *cap, const int h,
                                                    double *slack, MarginMin (*wave_min)[MARGIN_CLASSES], double *slack_out,
                                                    double *summary_out, int32_t *where_out) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  const int tid = threadIdx.x;
  const double inf = margins_inf();
  __syncthreads();
  for (int t = tid; t < C8 * h; t += NT) {
    const int i = t / C8, r = t % C8, c = r / 8, j = r % 8;
    const float *row = Fc + r * U, *ui = u + U * i;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < U; ++k) acc = __builtin_fma((double)row[k], (double)ui[k], acc);
    const unsigned char gb = gait[NC * i + c];
    const bool st = stance(cap[c], gb);
    double *s = slack + 10 * (NC * i + c);
    if (j < 4) {
      s[j] = st ? acc : inf;
    } else if (j == 4) {
      s[4] = st ? acc : inf;
      s[5] = st ? (double)0.01f - acc : inf;
    } else if (j < 7) {
      s[j + 1] = st ? 0.0 - acc : inf;
    } else {
      const float ub7 = cap[c] * (float)gb;
      s[8] = st ? acc : inf;
      s[9] = st ? (double)ub7 - acc : inf;
    }
  }
  __syncthreads();
  if (slack_out)
    for (int t = tid; t < 10 * NC * h; t += NT) slack_out[t] = slack[t];
  MarginMin best[MARGIN_CLASSES];
#pragma unroll
  for (int k = 0; k < MARGIN_CLASSES; ++k) best[k] = {inf, INT_MAX};
  for (int ls = tid; ls < NC * h; ls += NT) {
    if (!stance(cap[ls % NC], gait[ls])) continue;
    const double *s = slack + 10 * ls;
    const int base = 10 * ls;
    double m4 = inf;  // the minimum of the four friction rows by <, started at +inf
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      best[0] = margin_min(best[0], {s[j], base + j});
      m4 = (s[j] < m4) ? s[j] : m4;
    }
    best[1] = margin_min(margin_min(best[1], {s[4], base + 4}), {s[5], base + 5});
    best[2] = margin_min(margin_min(best[2], {s[6], base + 6}), {s[7], base + 7});
    best[3] = margin_min(best[3], {s[8], base + 8});
    best[4] = margin_min(best[4], {s[9], base + 9});
    if (s[8] > 0.0) best[5] = margin_min(best[5], {m4 / (0.5 * s[8]), base});
  }
#pragma unroll
  for (int k = 0; k < MARGIN_CLASSES; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      MarginMin other;
      other.v = __shfl_xor(best[k].v, off, 64);
      other.idx = __shfl_xor(best[k].idx, off, 64);
      best[k] = margin_min(best[k], other);
    }
    if ((tid & 63) == 0) wave_min[tid >> 6][k] = best[k];
  }
  __syncthreads();
  if (tid < MARGIN_CLASSES) {
    MarginMin win = wave_min[0][tid];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) win = margin_min(win, wave_min[w][tid]);
    if (summary_out) summary_out[tid] = win.v;  // (+inf when there was no candidate)
    if (where_out) where_out[tid] = (win.idx == INT_MAX) ? -1 : win.idx;
  }
  __syncthreads();
}

// out[i] = +inf if for some k with a non-NaN floor[k] the test summary[i][k] >= floor[k] is false (a NaN summary masks), else
// penalty_in ? penalty_in[i] : +0.0.  One thread per instance; out may be penalty_in.
struct MarginFloor {
  double v[MARGIN_CLASSES];
};
template <int NT>
__global__ __launch_bounds__(NT) void margin_penalty_kernel(const double *summary, const MarginFloor floor, const double *penalty_in,
                                                            double *out, const int batch) {
  const int i = (int)(blockIdx.x * NT + threadIdx.x);
  if (i >= batch) return;
  bool pass = true;
#pragma unroll
  for (int k = 0; k < MARGIN_CLASSES; ++k) {
    const double f = floor.v[k];
    if (f == f) pass = pass && (summary[(size_t)MARGIN_CLASSES * i + k] >= f);
  }
  out[i] = pass ? (penalty_in ? penalty_in[i] : 0.0) : margins_inf();
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants, mu_inst) and `forces`; it writes slack[batch][horizon][nc][10], summary[batch][6] (binary64) and where[batch][6] and
// nothing else.  Shapes: derived_shape (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_margins(int nc, const KernelArgs &args, double *slack, double *summary, int32_t *where, hipStream_t stream);
// out[batch] from summary[batch][6] and floor[6]; penalty_in may be nullptr or out.
hipError_t launch_margin_penalty(const double *summary, const double floor[MARGIN_CLASSES], const double *penalty_in, double *out, int batch,
                                 hipStream_t stream);
}  // namespace hmpc
#endif
