// hmpc_rollout_score.hip -- the unit that compiles the kernels of hmpc_rollout_score.h (the cost of a rollout's log, the cheapest instance of
// every group) and holds the C entry points of closed-loop command sweeps: hmpc_default_rollout_cost,
// hmpc_rollout_score_device, hmpc_rollout_select_device, hmpc_rollout_sweep_device and hmpc_get_device_rollout_sweep.  Built, like
// hmpc_plant.hip, under the no-contraction contract (-ffp-contract=off, HMPC-A1): the score is compared bit for bit with a numpy restatement
// of the header comment.  The chain enqueues what hmpc_select.hip's expansion and hmpc_rollout_device enqueue, then two launches of its own.
#include "hmpc_rollout_score.h"

#include <string.h>

#include "hmpc_handle.h"
#include "hmpc_select.h"

// the log and its shape behind a score or a selection that passes log == NULL: the last rollout's
static bool last_rollout(const hmpc_handle *h, int batch, hmpc_rollout_log *lg, int *n_ticks) {
  if (h->roll_last_ticks < 1 || batch != h->roll_last_batch) return false;
  *lg = h->roll_last, *n_ticks = h->roll_last_ticks;
  return true;
}

extern "C" {

void hmpc_default_rollout_cost(struct hmpc_rollout_cost *c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  const double q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  const double alpha[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  for (int s = 0; s < 12; ++s) c->w_state[s] = q[s], c->w_wrench[s] = alpha[s];
  c->height = 0.55, c->dt_tick = 0.005;
  c->fall_penalty = (double)INFINITY;
}

int hmpc_rollout_score_device(hmpc_handle *h, const void *device_ticks0, int batch, int n_ticks, const struct hmpc_rollout_cost *cost,
                              const struct hmpc_rollout_log *log, double *device_cost, double *device_score, void *stream) {
  if (!h || !device_ticks0 || !cost || batch < 0 || n_ticks < 1) return HMPC_E_ARG;
  hmpc::RolloutScoreArgs a;
  memset(&a, 0, sizeof(a));
  if (log) a.log = *log;
  else {
    int ticks = 0;
    if (!last_rollout(h, batch, &a.log, &ticks) || ticks != n_ticks) return HMPC_E_ARG;
  }
  if (!a.log.state) return HMPC_E_ARG;
  a.cost = *cost;
  a.ticks0 = (const hmpc_tick_inputs *)device_ticks0;
  a.batch = batch, a.n_ticks = n_ticks;
  a.out_cost = device_cost, a.out_score = device_score;
  h->rscore_batch = batch, h->rscore_ticks = n_ticks;
  if (batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_rollout_score(a, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_rollout_select_device(hmpc_handle *h, const double *device_score, const double *device_penalty, int batch, int group_size,
                               const struct hmpc_rollout_log *log, const struct hmpc_rollout_choice *choice, void *stream) {
  if (!h || !device_score || !choice || batch < 0 || group_size < 1 || batch % group_size != 0) return HMPC_E_ARG;
  hmpc::RolloutSelectArgs a;
  memset(&a, 0, sizeof(a));
  if (log) {
    if (h->rscore_ticks < 1 || batch != h->rscore_batch) return HMPC_E_ARG;
    a.log = *log, a.n_ticks = h->rscore_ticks;
  } else if (!last_rollout(h, batch, &a.log, &a.n_ticks)) return HMPC_E_ARG;
  a.choice = *choice;
  if ((a.choice.wrench && !a.log.wrench) || (a.choice.tau && !a.log.tau) || (a.choice.summary && !a.log.summary)) return HMPC_E_ARG;
  a.score = device_score, a.penalty = device_penalty;
  a.groups = batch / group_size, a.group_size = group_size;
  if (batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_rollout_select(a, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_rollout_sweep_device(hmpc_handle *h, const void *device_ticks, int n_states, const struct hmpc_command *device_commands, int K,
                              int n_ticks, double dtMPC, int ticks_per_step, int subtick0, const struct hmpc_plant *plant,
                              const struct hmpc_rollout_cost *cost, const double *device_penalty, const struct hmpc_rollout_choice *choice,
                              void *stream) {
  if (!h || !device_ticks || !device_commands || !plant || !cost || !choice || n_states < 1 || K < 1) return HMPC_E_ARG;
  if (n_ticks < 1 || ticks_per_step < 1 || subtick0 < 0 || plant->substeps < 1 || h->nc != 2) return HMPC_E_ARG;
  if ((long long)n_states * (long long)K > (long long)h->max_batch) return HMPC_E_BATCH;
  const int batch = n_states * K;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->d_rsw_ticks.get()) HIP_TRY(h->d_rsw_ticks.alloc((size_t)h->max_batch * sizeof(hmpc_tick_inputs)));
  if (!h->d_rsw_ticks0.get()) HIP_TRY(h->d_rsw_ticks0.alloc((size_t)h->max_batch * sizeof(hmpc_tick_inputs)));
  if (!h->d_rsw_cost.get()) HIP_TRY(h->d_rsw_cost.alloc((size_t)h->max_batch * 4));
  if (!h->d_rsw_score.get()) HIP_TRY(h->d_rsw_score.alloc((size_t)h->max_batch));
  const hipStream_t s = (hipStream_t)stream;
  RC_TRY(enter_stream(h, s));  // (before the expansions: they write the handle's tick buffers, which the previous sweep's rollout may still read)
  hmpc_tick_inputs *now = (hmpc_tick_inputs *)h->d_rsw_ticks.get(), *before = (hmpc_tick_inputs *)h->d_rsw_ticks0.get();
  HIP_TRY(hmpc::launch_expand_ticks((const hmpc_tick_inputs *)device_ticks, n_states, device_commands, K, now, nullptr, s));
  HIP_TRY(hmpc::launch_expand_ticks((const hmpc_tick_inputs *)device_ticks, n_states, device_commands, K, before, nullptr, s));
  int rc = hmpc_rollout_device(h, now, batch, n_ticks, dtMPC, ticks_per_step, subtick0, plant, /*log=*/nullptr, stream);
  if (rc != HMPC_OK) return rc;
  h->rsw_batch = batch;
  rc = hmpc_rollout_score_device(h, before, batch, n_ticks, cost, nullptr, h->d_rsw_cost.get(), h->d_rsw_score.get(), stream);
  if (rc != HMPC_OK) return rc;
  return hmpc_rollout_select_device(h, h->d_rsw_score.get(), device_penalty, batch, K, nullptr, choice, stream);
}

int hmpc_get_device_rollout_sweep(hmpc_handle *h, void **ticks_final, double **cost, double **score) {
  if (!h || h->rsw_batch < 1) return HMPC_E_ARG;
  if (ticks_final) *ticks_final = h->d_rsw_ticks.get();
  if (cost) *cost = h->d_rsw_cost.get();
  if (score) *score = h->d_rsw_score.get();
  return HMPC_OK;
}

}  // extern "C"
