// hmpc_rollout_score.h -- what a closed-loop command sweep adds behind the rollout: the cost of every instance's log
// (rollout_score_kernel) and the cheapest instance of every group (rollout_select_kernel), with their launches.  hmpc_rollout_score.hip holds
// the C entry points; no kernel of the solve, of the plant or of hmpc_select.hip is touched.
// THE ARITHMETIC OF THE SCORE IS A CONTRACT: binary64, correctly rounded IEEE operations only, no contraction (the unit is built with
// -ffp-contract=off, HMPC-A1 of DESIGN.md section 3), in the operation order the comment of include/hector_mpc.h above struct
// hmpc_rollout_cost writes out.  tests/rollout_score_mirror.py restates that comment in numpy and is compared with these kernels bit for bit:
// there is no libm call in it (rint is one instruction, exact).
// Score mapping: a wave owns an instance, lane l owns the ticks l, l + 64, ... of its log in ascending order, so at every pass the wave reads
// 64 consecutive rows of each log array -- 6 KB of state, 3 KB of wrench, 5 KB of torques, whole cache lines but for the two ends.  Each lane
// chains its ticks' terms, then the 64 partial sums are added up by a butterfly of __shfl_xor exchanges: every lane adds the same two
// numbers its partner adds, so all lanes end with the same bits and the sum is a function of the inputs only.  Four waves per workgroup, the
// tail guarded per wave; no LDS, no atomics, no inline assembly.
// Selection mapping: hmpc_select.hip's -- one workgroup of 256 threads per group, each thread strides over its group in ascending order and
// keeps its best (value, position), eligibility tested first; butterfly inside a wave, one LDS step across the four waves.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"

namespace hmpc {

constexpr int RSCORE_W = 64;                  // W of the contract: partial sums per instance
constexpr int RSCORE_WAVES = 4;               // instances per workgroup
constexpr int RSCORE_NT = RSCORE_W * RSCORE_WAVES;
constexpr int RSELECT_NT = 256;               // threads per workgroup of the selection (one workgroup per group)
constexpr int RSELECT_WAVES = RSELECT_NT / 64;
static_assert(RSELECT_NT % 64 == 0, "whole waves");
constexpr double RSCORE_TWO_PI = 6.283185307179586;

// what one launch of the score reads and writes (by value: the host's hmpc_rollout_cost, the log's pointers)
struct RolloutScoreArgs {
  hmpc_rollout_cost cost;
  const hmpc_tick_inputs *ticks0;  // [batch], as they were before the rollout
  hmpc_rollout_log log;            // state is read; wrench, tau, summary when set; status never
  int batch, n_ticks;
  double *out_cost;                // [batch][4] or nullptr
  double *out_score;               // [batch] or nullptr
};

// what one launch of the selection reads and writes
struct RolloutSelectArgs {
  const double *score;    // [groups * group_size]
  const double *penalty;  // the same, or nullptr
  int groups, group_size;
  int n_ticks;            // rows per instance of log.wrench and log.tau (row 0 is copied)
  hmpc_rollout_log log;
  hmpc_rollout_choice choice;
};

// the reference of one instance: what of `ref` does not change from row to row, and the three rates of what does
struct RolloutRef {
  double roll, pitch, yaw0, x0, y0, yaw_rate, vdw[2];
};

__device__ __forceinline__ RolloutRef rollout_ref_of(const hmpc_tick_inputs &tk) {
  RolloutRef r;
  const double *R0 = tk.rBody;
  const double cx = tk.v_des_robot[0], cy = tk.v_des_robot[1];
#pragma unroll
  for (int a = 0; a < 2; ++a) r.vdw[a] = (R0[a] * cx + R0[3 + a] * cy) + R0[6 + a] * 0.0;
  r.roll = tk.roll_des, r.pitch = tk.pitch_des, r.yaw0 = tk.rpy[2], r.x0 = tk.position[0], r.y0 = tk.position[1];
  r.yaw_rate = tk.yaw_rate_des;
  return r;
}

// e of row k (the contract's "Row k"), from the 12 doubles of its state row
__device__ __forceinline__ void rollout_row_error(const double *state_row, const RolloutRef &r, double height, double dt_tick, int k, double *e) {
  const double t = (double)(k + 1) * dt_tick;
  const double ref[12] = {r.roll, r.pitch, r.yaw0 + t * r.yaw_rate, r.x0 + t * r.vdw[0], r.y0 + t * r.vdw[1], height,
                          0.0,    0.0,     r.yaw_rate,              r.vdw[0],            r.vdw[1],            0.0};
#pragma unroll
  for (int s = 0; s < 12; ++s) e[s] = state_row[s] - ref[s];
  e[2] = e[2] - RSCORE_TWO_PI * rint(e[2] / RSCORE_TWO_PI);
}

__device__ __forceinline__ double rollout_weighted_square(const double *w, const double *e) {
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < 12; ++s) acc = acc + (w[s] * e[s]) * e[s];
  return acc;
}

// P[l] = P[l] + P[l ^ off], off = 32 .. 1: every lane ends with the sum of the 64
__device__ __forceinline__ double rollout_wave_sum(double p) {
#pragma unroll
  for (int off = RSCORE_W / 2; off > 0; off >>= 1) p = p + __shfl_xor(p, off, RSCORE_W);
  return p;
}

__global__ __launch_bounds__(RSCORE_NT) void rollout_score_kernel(RolloutScoreArgs a) {
  const int lane = threadIdx.x & (RSCORE_W - 1);
  const int i = blockIdx.x * RSCORE_WAVES + (int)(threadIdx.x / RSCORE_W);
  if (i >= a.batch) return;  // (a whole wave: the exchanges below are the wave's own)
  const hmpc_rollout_cost &c = a.cost;
  const RolloutRef ref = rollout_ref_of(a.ticks0[i]);
  const size_t row0 = (size_t)i * (size_t)a.n_ticks;
  double trk = 0.0, eff = 0.0, e[12];
  for (int k = lane; k < a.n_ticks; k += RSCORE_W) {
    const size_t row = row0 + (size_t)k;
    rollout_row_error(a.log.state + row * 12, ref, c.height, c.dt_tick, k, e);
    trk = trk + rollout_weighted_square(c.w_state, e);
    double eff_k = 0.0;
    if (a.log.wrench) {
      const float *u = a.log.wrench + row * 12;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const double v = (double)u[j];
        eff_k = eff_k + (c.w_wrench[j] * v) * v;
      }
    }
    if (a.log.tau) {
      const double *u = a.log.tau + row * 10;
#pragma unroll
      for (int j = 0; j < 10; ++j) eff_k = eff_k + (c.w_tau[j] * u[j]) * u[j];
    }
    eff = eff + eff_k;
  }
  trk = rollout_wave_sum(trk);
  eff = rollout_wave_sum(eff);
  if (lane != 0) return;
  rollout_row_error(a.log.state + (row0 + (size_t)(a.n_ticks - 1)) * 12, ref, c.height, c.dt_tick, a.n_ticks - 1, e);
  const double term = rollout_weighted_square(c.w_terminal, e);
  double pen = 0.0;
  if (a.log.summary) {
    const int32_t *sm = a.log.summary + (size_t)4 * i;
    const int32_t fell = sm[1], unsolved = sm[2];
    pen = (fell >= 0 ? c.fall_penalty : 0.0) + (unsolved > 0 ? (double)unsolved * c.unsolved_penalty : 0.0);
  }
  if (a.out_cost) {
    double *o = a.out_cost + (size_t)4 * i;
    o[0] = trk, o[1] = eff, o[2] = term, o[3] = pen;
  }
  if (a.out_score) a.out_score[i] = ((trk + eff) + term) + pen;
}

struct RolloutBest {
  double s;
  int pos;
};

// lexicographic (value, position) minimum.  Values here are finite or +inf, never NaN, so == and < are a total order (-0 == +0)
__device__ __forceinline__ RolloutBest rollout_best_of(const RolloutBest a, const RolloutBest b) {
  const bool take_b = b.s < a.s || (b.s == a.s && b.pos < a.pos);
  return take_b ? b : a;
}

__device__ __forceinline__ bool rollout_finite64(const double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__global__ __launch_bounds__(RSELECT_NT) void rollout_select_kernel(RolloutSelectArgs a) {
  __shared__ RolloutBest wave_best[RSELECT_WAVES];
  const int tid = threadIdx.x, g = blockIdx.x, K = a.group_size;
  if (g >= a.groups) return;  // uniform
  const size_t first = (size_t)g * K;
  RolloutBest mine = {__longlong_as_double(0x7ff0000000000000ll), INT_MAX};
  for (int k = tid; k < K; k += RSELECT_NT) {
    const size_t i = first + k;
    double s = a.score[i];
    if (a.penalty) s = s + a.penalty[i];
    if (rollout_finite64(s) && s < mine.s) mine.s = s, mine.pos = k;  // (k ascending: an equal value keeps the lower position)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    RolloutBest other;
    other.s = __shfl_xor(mine.s, off, 64);
    other.pos = __shfl_xor(mine.pos, off, 64);
    mine = rollout_best_of(mine, other);
  }
  if ((tid & 63) == 0) wave_best[tid >> 6] = mine;
  __syncthreads();
  RolloutBest win = wave_best[0];
#pragma unroll
  for (int w = 1; w < RSELECT_WAVES; ++w) win = rollout_best_of(win, wave_best[w]);
  const bool none = win.pos == INT_MAX;
  const size_t src = first + (none ? 0 : win.pos);
  const hmpc_rollout_choice &o = a.choice;
  if (tid == 0) {
    if (o.index) o.index[g] = none ? -1 : win.pos;
    if (o.score) o.score[g] = win.s;  // (+inf when nothing was eligible)
  }
  // bit copies, word by word: the winner's row of tick 0 (12 floats, 10 doubles) and its summary row
  if (o.wrench && tid < 12) {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(a.log.wrench) + src * (size_t)a.n_ticks * 12;
    reinterpret_cast<uint32_t *>(o.wrench)[(size_t)g * 12 + tid] = none ? 0u : from[tid];
  }
  if (o.tau && tid >= 64 && tid < 64 + 20) {
    const int t = tid - 64;
    const uint32_t *from = reinterpret_cast<const uint32_t *>(a.log.tau) + src * (size_t)a.n_ticks * 20;
    reinterpret_cast<uint32_t *>(o.tau)[(size_t)g * 20 + t] = none ? 0u : from[t];
  }
  if (o.summary && tid >= 128 && tid < 128 + 4) {
    const int t = tid - 128;
    o.summary[(size_t)g * 4 + t] = none ? (t == 1 ? -1 : 0) : a.log.summary[src * 4 + t];
  }
}

// One launch of ceil(batch / 4) workgroups; hipErrorInvalidValue (nothing launched) for a null ticks0 or state or a size below 1.
inline hipError_t launch_rollout_score(const RolloutScoreArgs &a, hipStream_t stream) {
  if (a.batch < 1 || a.n_ticks < 1 || !a.ticks0 || !a.log.state) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_score_kernel, dim3((unsigned)((a.batch + RSCORE_WAVES - 1) / RSCORE_WAVES)), dim3(RSCORE_NT), 0, stream, a);
  return hipGetLastError();
}

// One launch of `groups` workgroups; hipErrorInvalidValue (nothing launched) for a null score, a size below 1, or an output whose log
// member is null.
inline hipError_t launch_rollout_select(const RolloutSelectArgs &a, hipStream_t stream) {
  if (a.groups < 1 || a.group_size < 1 || !a.score) return hipErrorInvalidValue;
  if ((a.choice.wrench && (!a.log.wrench || a.n_ticks < 1)) || (a.choice.tau && (!a.log.tau || a.n_ticks < 1)) ||
      (a.choice.summary && !a.log.summary))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_select_kernel, dim3((unsigned)a.groups), dim3(RSELECT_NT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace hmpc
