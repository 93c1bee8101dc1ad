// hmpc_select.h -- host-visible side of the selection kernels (hmpc_select.hip): the best command of every sweep group
// (hmpc_sweep_select) and the expansion of ticks x commands into the ticks of a sweep (hmpc_tick_sweep_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"

namespace hmpc {
constexpr int SELECT_NT = 256;  // threads per workgroup (one workgroup per group)

// Everything one selection launch reads and writes.  Inputs: cost[batch][2], states[batch][h][13] (the last prediction), status[batch]
// and forces[batch][nu*h] (the last solve), penalty[batch] or nullptr.  Outputs, one row per group of group_size consecutive instances:
// index[groups], score[groups], out_forces[groups][nu*h], out_status[groups], out_states[groups][h][13].
struct SelectArgs {
  const double *cost;
  const float *states;
  const uint32_t *status;
  const float *forces;
  const double *penalty;
  int groups, group_size;
  int force_words, state_words;  // nu * h, 13 * h
  int32_t *index;
  double *score;
  float *out_forces;
  uint32_t *out_status;
  float *out_states;
};

// One launch of `groups` workgroups on `stream`; hipErrorInvalidValue (nothing launched) for a null pointer other than penalty or a
// size below 1.
hipError_t launch_select(const SelectArgs &args, hipStream_t stream);

// out[g * group_size + k] = ticks[g] with the five command fields of commands[g * group_size + k]; wpd_out (may be nullptr)
// [n_ticks][2] = the clamped world_position_desired of ticks[g], the value build_records_kernel writes for it.
hipError_t launch_expand_ticks(const hmpc_tick_inputs *ticks, int n_ticks, const hmpc_command *commands, int group_size,
                               hmpc_tick_inputs *out, double *wpd_out, hipStream_t stream);

}  // namespace hmpc
