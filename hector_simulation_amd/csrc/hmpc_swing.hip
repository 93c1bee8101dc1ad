// hmpc_swing.hip -- the unit that compiles the kernels of hmpc_swing.h (swing update, state start) and holds their launches and the C entry
// points of the swing legs on the device: hmpc_default_swing, hmpc_swing_state_init_device, hmpc_swing_legs_device,
// hmpc_tick_command_device, hmpc_set_rollout_swing, and the launch a rollout enqueues per tick while that setting is on
// (rollout_swing_tick, called by hmpc_plant.hip).  Built, like hmpc_plant.hip, under the no-contraction contract (-ffp-contract=off,
// HMPC-A1): the swing arithmetic is compared with a numpy restatement of the header comment.  No kernel of the solve is touched.
#include "hmpc_swing.h"

#include <string.h>

#include "hmpc_handle.h"

namespace hmpc {
namespace {

dim3 swing_grid(int batch) { return dim3((2 * batch + SWING_NT - 1) / SWING_NT); }

hipError_t launch_swing_legs(const hmpc_tick_inputs *ticks, const SwingArgs &a, hipStream_t stream) {
  if (a.batch < 1) return hipSuccess;
  if (!ticks || !a.state || a.horizon < 1 || a.cfg.updates < 1 || a.cfg.ticks_per_step < 1 || a.cfg.subtick < 0 ||
      a.cfg.subtick >= a.cfg.ticks_per_step || a.cmd_stride < 1 || a.cmd_row < 0 || a.cmd_row >= a.cmd_stride)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(swing_legs_kernel, swing_grid(a.batch), dim3(SWING_NT), 0, stream, ticks, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace hmpc

static bool swing_cfg_ok(const hmpc_swing *cfg) {
  return cfg && cfg->updates >= 1 && cfg->ticks_per_step >= 1 && cfg->subtick >= 0 && cfg->subtick < cfg->ticks_per_step;
}

// the arguments every swing entry refuses (include/hector_mpc.h): nothing is enqueued for them
static bool swing_args_ok(const hmpc_handle *h, const void *ticks, int batch, const hmpc_swing *cfg, const void *state, const void *cmd) {
  return h && ticks && state && cmd && swing_cfg_ok(cfg) && batch >= 0 && batch <= h->max_batch && h->nc == 2;
}

static void swing_args(const hmpc_handle *h, int batch, const hmpc_swing &cfg, hmpc_swing_state *state, const double *tau, hmpc_motor_cmd *cmd,
                       double *detail, hmpc::SwingArgs *a) {
  memset(a, 0, sizeof(*a));
  a->cfg = cfg;
  a->batch = batch, a->horizon = h->setup.horizon;
  a->state = state, a->tau = tau, a->cmd = cmd, a->cmd_stride = 1, a->cmd_row = 0, a->detail = detail;
}

// tick k of a rollout with hmpc_set_rollout_swing on: the swing launch behind the tick's torque launch (d_roll_tau), before the plant step
int rollout_swing_tick(hmpc_handle *h, const void *device_ticks, int batch, int k, int n_ticks, int ticks_per_step, int subtick0,
                       hipStream_t stream) {
  if (!h->swing_on || batch < 1) return HMPC_OK;
  hmpc::SwingArgs a;
  swing_args(h, batch, h->swing_cfg, h->swing_state, h->d_roll_tau.get(), h->swing_cmd_log, nullptr, &a);
  a.cfg.ticks_per_step = ticks_per_step, a.cfg.subtick = (subtick0 + k) % ticks_per_step;
  a.cmd_stride = n_ticks, a.cmd_row = k;
  HIP_TRY(hmpc::launch_swing_legs((const hmpc_tick_inputs *)device_ticks, a, stream));
  return HMPC_OK;
}

extern "C" {

void hmpc_default_swing(struct hmpc_swing *c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->dt_update = 0.001, c->dtMPC = 0.04;
  c->updates = 2, c->ticks_per_step = 40, c->subtick = 0;
  c->height = 0.15, c->place_gain_v = 1.75, c->place_gain_err = 0.1, c->place_max = 0.3;
  for (int leg = 0; leg < 2; ++leg) {
    c->hip_yaw[leg][0] = -0.005, c->hip_yaw[leg][1] = leg == 0 ? -0.057 : 0.057, c->hip_yaw[leg][2] = -0.126;
    c->hip_width_offset[leg][0] = -0.015, c->hip_width_offset[leg][1] = leg == 0 ? 0.055 : -0.055, c->hip_width_offset[leg][2] = 0.0;
  }
  c->hip_roll[0] = 0.0465, c->hip_roll[1] = 0.015, c->hip_roll[2] = -0.0705;
  c->ik_link = 0.22, c->ik_horizontal = 0.0205, c->ik_hip_x = 0.06;
  for (int k = 0; k < 5; ++k) c->kp[k] = k < 4 ? 30.0 : 20.0, c->kd[k] = 1.0;
}

int hmpc_swing_state_init_device(hmpc_handle *h, struct hmpc_swing_state *device_state, int batch, void *stream) {
  if (!h || !device_state || batch < 0) return HMPC_E_ARG;
  if (batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  hipLaunchKernelGGL(hmpc::swing_state_init_kernel, hmpc::swing_grid(batch), dim3(hmpc::SWING_NT), 0, (hipStream_t)stream, device_state, batch);
  HIP_TRY(hipGetLastError());
  return HMPC_OK;
}

int hmpc_swing_legs_device(hmpc_handle *h, const void *device_ticks, int batch, const struct hmpc_swing *cfg,
                           struct hmpc_swing_state *device_state, const double *device_tau, struct hmpc_motor_cmd *device_cmd,
                           double *device_detail, void *stream) {
  if (!swing_args_ok(h, device_ticks, batch, cfg, device_state, device_cmd)) return HMPC_E_ARG;
  if (batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  hmpc::SwingArgs a;
  swing_args(h, batch, *cfg, device_state, device_tau, device_cmd, device_detail, &a);
  HIP_TRY(hmpc::launch_swing_legs((const hmpc_tick_inputs *)device_ticks, a, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_tick_command_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, const struct hmpc_swing *cfg,
                             struct hmpc_swing_state *device_state, double *device_wpd_out, double *device_f_ff,
                             struct hmpc_motor_cmd *device_cmd, void *stream) {
  if (!swing_args_ok(h, device_ticks, batch, cfg, device_state, device_cmd)) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));  // (first: the torque buffer is allocated once, outside the solve)
  if (!h->d_roll_tau.get()) HIP_TRY(h->d_roll_tau.alloc((size_t)h->max_batch * 10));
  RC_TRY(hmpc_tick_solve_device(h, device_ticks, batch, dtMPC, device_wpd_out, device_f_ff, h->d_roll_tau.get(), stream));
  if (batch == 0) return HMPC_OK;
  hmpc::SwingArgs a;
  swing_args(h, batch, *cfg, device_state, h->d_roll_tau.get(), device_cmd, nullptr, &a);
  HIP_TRY(hmpc::launch_swing_legs((const hmpc_tick_inputs *)device_ticks, a, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_set_rollout_swing(hmpc_handle *h, const struct hmpc_swing *cfg, void *device_state, struct hmpc_motor_cmd *device_cmd_log) {
  if (!h) return HMPC_E_ARG;
  if (!cfg) {
    h->swing_on = false, h->swing_state = nullptr, h->swing_cmd_log = nullptr;
    return HMPC_OK;
  }
  if (!device_state || cfg->updates < 1 || h->nc != 2) return HMPC_E_ARG;
  h->swing_cfg = *cfg;
  h->swing_state = (hmpc_swing_state *)device_state, h->swing_cmd_log = device_cmd_log;
  h->swing_on = true;
  return HMPC_OK;
}

}  // extern "C"
