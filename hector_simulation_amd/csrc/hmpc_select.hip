// hmpc_select.hip -- the best command of every sweep group, picked on the device (hmpc_sweep_select), and the
// expansion of ticks x commands into the ticks of a command sweep (hmpc_tick_sweep_device).
//
// A command sweep solves one robot state under K commands and the prediction scores each of them (cost[batch][2]); what was missing is
// the planner's last step: the argmin per group and the winner's row of the force buffer, without a trip to the host.  A launch of its
// own (never part of hmpc_kernel, not a row of hmpc_variants.h), over whatever the status, force and prediction buffers hold.
//
// Definition (fixed in include/hector_mpc.h; tests/selection_mirror.py restates it in numpy).  Group g = instances g K .. g K + K - 1:
//   score_i  = (cost[i][0] + cost[i][1]) + penalty[i]      two binary64 additions in that order (the second only with a penalty)
//   eligible = status code OK or OK_RELAXED, and score_i finite
//   winner   = the eligible instance of smallest score, equal scores (==) broken by the lowest index
// Mapping: one workgroup of 256 threads per group.  Lane t looks at instances t, t + 256, ... of its group in ascending order and keeps
// its best (score, position) -- eligibility is tested first, so no NaN and no infinity of an instance ever enters a comparison; a lane
// without an eligible instance holds (+inf, INT_MAX), which loses to every eligible pair.  The pairs are then reduced with the
// lexicographic minimum, a total order on them: butterfly shuffles inside a wave, one LDS step across the four waves (every lane
// reads the four wave results in the same order).  The minimum of a set under a total order does not depend on how the set is split,
// so the result is a pure function of the inputs, whatever the workgroup size.  All lanes then copy the winner's force and state rows
// in coalesced bursts (zeros when the group has no winner).  No atomics, no inline assembly, nothing kept between launches.
// Traffic: 20 B per instance (28 with a penalty) in, one force row + one state row (at most 2 KB) in and out per group.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>

#include "hmpc_select.h"

namespace hmpc {
namespace {

constexpr int SELECT_WAVES = SELECT_NT / 64;
static_assert(SELECT_NT % 64 == 0, "whole waves");

struct Best {
  double score;
  int pos;
};

// lexicographic (score, position) minimum.  Scores here are finite or +inf, never NaN, so == and < are a total order (-0 == +0)
__device__ __forceinline__ Best best_of(const Best a, const Best b) {
  const bool take_b = b.score < a.score || (b.score == a.score && b.pos < a.pos);
  return take_b ? b : a;
}

__device__ __forceinline__ bool finite64(const double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__global__ __launch_bounds__(SELECT_NT) void hmpc_select_kernel(SelectArgs a) {
  __shared__ Best wave_best[SELECT_WAVES];
  const int tid = threadIdx.x, g = blockIdx.x, K = a.group_size;
  if (g >= a.groups) return;  // uniform
  const size_t first = (size_t)g * K;
  Best mine = {__longlong_as_double(0x7ff0000000000000ll), INT_MAX};
  for (int k = tid; k < K; k += SELECT_NT) {
    const size_t i = first + k;
    const uint32_t code = a.status[i] & 0xffu;
    double s = a.cost[2 * i] + a.cost[2 * i + 1];
    if (a.penalty) s = s + a.penalty[i];
    const bool eligible = (code == HMPC_S_OK || code == HMPC_S_OK_RELAXED) && finite64(s);
    if (eligible && s < mine.score) mine.score = s, mine.pos = k;  // (k ascending: an equal score keeps the lower position)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best other;
    other.score = __shfl_xor(mine.score, off, 64);
    other.pos = __shfl_xor(mine.pos, off, 64);
    mine = best_of(mine, other);
  }
  if ((tid & 63) == 0) wave_best[tid >> 6] = mine;
  __syncthreads();
  Best win = wave_best[0];
#pragma unroll
  for (int w = 1; w < SELECT_WAVES; ++w) win = best_of(win, wave_best[w]);
  const bool none = win.pos == INT_MAX;
  const size_t src = first + (none ? 0 : win.pos);
  if (tid == 0) {
    a.index[g] = none ? -1 : win.pos;
    a.score[g] = win.score;  // (+inf when nothing was eligible)
    a.out_status[g] = none ? HMPC_SELECT_NONE : a.status[src];
  }
  {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(a.forces) + src * a.force_words;
    uint32_t *to = reinterpret_cast<uint32_t *>(a.out_forces) + (size_t)g * a.force_words;
    for (int t = tid; t < a.force_words; t += SELECT_NT) to[t] = none ? 0u : from[t];
  }
  {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(a.states) + src * a.state_words;
    uint32_t *to = reinterpret_cast<uint32_t *>(a.out_states) + (size_t)g * a.state_words;
    for (int t = tid; t < a.state_words; t += SELECT_NT) to[t] = none ? 0u : from[t];
  }
}

// ---- ticks x commands -> the ticks of a sweep.  struct hmpc_command is the five command fields of hmpc_tick_inputs, in their order:
// a tick is copied word by word and the words of those fields come from the command instead.
constexpr int TICK_WORDS = (int)(sizeof(hmpc_tick_inputs) / 4), CMD_WORDS = (int)(sizeof(hmpc_command) / 4);
constexpr int CMD_FIRST = (int)(offsetof(hmpc_tick_inputs, v_des_robot) / 4);
static_assert(sizeof(hmpc_tick_inputs) % 4 == 0 && sizeof(hmpc_command) == 40, "hector_mpc.h");
static_assert(offsetof(hmpc_tick_inputs, yaw_rate_des) - offsetof(hmpc_tick_inputs, v_des_robot) == offsetof(hmpc_command, yaw_rate_des) &&
                  offsetof(hmpc_tick_inputs, roll_des) - offsetof(hmpc_tick_inputs, v_des_robot) == offsetof(hmpc_command, roll_des) &&
                  offsetof(hmpc_tick_inputs, pitch_des) - offsetof(hmpc_tick_inputs, v_des_robot) == offsetof(hmpc_command, pitch_des) &&
                  offsetof(hmpc_tick_inputs, world_position_desired) - offsetof(hmpc_tick_inputs, v_des_robot) == sizeof(hmpc_command),
              "hmpc_command = the command fields of hmpc_tick_inputs, contiguous and in order");

__global__ __launch_bounds__(256) void expand_ticks_kernel(const hmpc_tick_inputs *ticks, int n_ticks, const hmpc_command *commands,
                                                           int group_size, hmpc_tick_inputs *out, double *wpd_out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n_ticks * group_size * TICK_WORDS;
  if (t >= total) return;
  const size_t inst = t / TICK_WORDS;
  const int w = (int)(t % TICK_WORDS), g = (int)(inst / group_size);
  const uint32_t *tick = reinterpret_cast<const uint32_t *>(ticks + g);
  const uint32_t *cmd = reinterpret_cast<const uint32_t *>(commands + inst);
  const bool from_cmd = w >= CMD_FIRST && w < CMD_FIRST + CMD_WORDS;
  reinterpret_cast<uint32_t *>(out)[t] = from_cmd ? cmd[w - CMD_FIRST] : tick[w];
  if (wpd_out && w == 0 && inst % group_size == 0) {
    // the clamp of ConvexMPCLocomotion.cpp:336-346 as build_records_kernel has it (comparisons and one addition each: the same bits)
    const hmpc_tick_inputs &tk = ticks[g];
    const double *p = tk.position;
    const double max_pos_error = .05;
    double xStart = tk.world_position_desired[0], yStart = tk.world_position_desired[1];
    if (xStart - p[0] > max_pos_error) xStart = p[0] + max_pos_error;
    if (p[0] - xStart > max_pos_error) xStart = p[0] - max_pos_error;
    if (yStart - p[1] > max_pos_error) yStart = p[1] + max_pos_error;
    if (p[1] - yStart > max_pos_error) yStart = p[1] - max_pos_error;
    wpd_out[2 * g + 0] = xStart;
    wpd_out[2 * g + 1] = yStart;
  }
}

}  // namespace

hipError_t launch_select(const SelectArgs &a, hipStream_t stream) {
  if (a.groups < 1 || a.group_size < 1 || a.force_words < 1 || a.state_words < 1) return hipErrorInvalidValue;
  if (!a.cost || !a.states || !a.status || !a.forces || !a.index || !a.score || !a.out_forces || !a.out_status || !a.out_states)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hmpc_select_kernel, dim3(a.groups), dim3(SELECT_NT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_expand_ticks(const hmpc_tick_inputs *ticks, int n_ticks, const hmpc_command *commands, int group_size,
                               hmpc_tick_inputs *out, double *wpd_out, hipStream_t stream) {
  if (!ticks || !commands || !out || n_ticks < 1 || group_size < 1) return hipErrorInvalidValue;
  const size_t total = (size_t)n_ticks * group_size * TICK_WORDS;
  hipLaunchKernelGGL(expand_ticks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ticks, n_ticks, commands,
                     group_size, out, wpd_out);
  return hipGetLastError();
}

}  // namespace hmpc
