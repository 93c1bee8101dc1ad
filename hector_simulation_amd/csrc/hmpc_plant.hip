// hmpc_plant.hip -- the unit that compiles the kernels of hmpc_plant.h (plant step, summary start) and holds their launches and the C entry
// points of the closed loop on the device: hmpc_default_plant, hmpc_plant_step_device, hmpc_rollout_device and the
// rollout's log buffers.  Built, like hmpc_builder.hip, under the no-contraction contract (-ffp-contract=off, HMPC-A1): the plant's
// arithmetic is compared bit for bit with a numpy restatement of the header comment.  No kernel of the solve is touched: a rollout
// enqueues exactly what hmpc_tick_solve_device enqueues, then one launch of the plant step, per tick -- and between the two, while
// hmpc_set_rollout_swing is on, the swing launch of hmpc_swing.hip.
#include "hmpc_plant.h"

#include <string.h>

#include "hmpc_handle.h"

namespace hmpc {
namespace {

dim3 plant_grid(int items) { return dim3((items + PLANT_NT - 1) / PLANT_NT); }

hipError_t launch_plant_step(hmpc_tick_inputs *ticks, const PlantArgs &a, hipStream_t stream) {
  if (a.batch < 1) return hipSuccess;
  if (!ticks || !a.forces || !a.status || a.force_stride < 12 || a.horizon < 1 || a.plant.substeps < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plant_step_kernel, plant_grid(a.batch), dim3(PLANT_NT), 0, stream, ticks, a);
  return hipGetLastError();
}

hipError_t launch_summary_init(int32_t *summary, int batch, hipStream_t stream) {
  if (batch < 1 || !summary) return hipSuccess;
  hipLaunchKernelGGL(plant_summary_init_kernel, plant_grid(batch), dim3(PLANT_NT), 0, stream, summary, batch);
  return hipGetLastError();
}

}  // namespace
}  // namespace hmpc

// what one plant launch of this handle reads: the caller's forces / status or the handle's own
static int plant_args(hmpc_handle *h, int batch, const hmpc_plant *plant, const float *forces, int force_stride, const uint32_t *status,
                      const double *wpd, int32_t *summary, hmpc::PlantArgs *a) {
  memset(a, 0, sizeof(*a));
  a->plant = *plant;
  a->batch = batch, a->horizon = h->setup.horizon;
  a->forces = forces ? forces : h->d_forces.get();
  a->force_stride = forces ? force_stride : 12 * h->setup.horizon;
  a->status = status ? status : h->d_status.get();
  a->wpd = wpd, a->summary = summary;
  a->n_ticks = 1;
  if ((!forces || !status) && batch > h->max_batch) return HMPC_E_ARG;  // (the handle's own buffers hold max_batch rows)
  return (a->force_stride < 12) ? HMPC_E_ARG : HMPC_OK;
}

// whether any member of `lg` is one of the handle's own log buffers
static bool logs_into_own_buffers(const hmpc_handle *h, const hmpc_rollout_log &lg) {
  return (lg.state && lg.state == h->d_roll_state.get()) || (lg.wrench && lg.wrench == h->d_roll_wrench.get()) ||
         (lg.status && lg.status == h->d_roll_status.get()) || (lg.tau && lg.tau == h->d_roll_taulog.get()) ||
         (lg.summary && lg.summary == h->d_roll_summary.get());
}

// the handle's own log buffers, for max_batch x n_ticks (kept when they already hold as many ticks).  A growth frees the old buffers, so
// a last rollout that logged into any of them is forgotten first -- whatever happens after: hmpc_download_rollout and the score and
// selection with log == NULL answer as before the first rollout instead of reading freed memory.  One that logged wholly into the
// caller's buffers stays.
static int own_rollout_buffers(hmpc_handle *h, int n_ticks) {
  const size_t rows = (size_t)h->max_batch * (size_t)n_ticks;
  if (n_ticks > h->roll_own_ticks) {
    if (logs_into_own_buffers(h, h->roll_last)) h->roll_last = {}, h->roll_last_ticks = 0, h->roll_last_batch = 0;
    RC_TRY(grow(h, h->d_roll_state, rows * 12 * sizeof(double)));
    RC_TRY(grow(h, h->d_roll_wrench, rows * 12 * sizeof(float)));
    RC_TRY(grow(h, h->d_roll_status, rows * sizeof(uint32_t)));
    RC_TRY(grow(h, h->d_roll_taulog, rows * 10 * sizeof(double)));
    h->roll_own_ticks = n_ticks;
  }
  if (!h->d_roll_summary.get()) HIP_TRY(h->d_roll_summary.alloc((size_t)h->max_batch * 4));
  return HMPC_OK;
}

// where a rollout that passes log == NULL writes: the caller's buffers of hmpc_set_device_rollout, else the handle's own
static int default_rollout_log(hmpc_handle *h, int n_ticks, hmpc_rollout_log *out) {
  const hmpc_rollout_log &c = h->roll_caller;
  if (!(c.state && c.wrench && c.status && c.tau && c.summary)) {
    const int rc = own_rollout_buffers(h, n_ticks);
    if (rc != HMPC_OK) return rc;
  }
  out->state = c.state ? c.state : h->d_roll_state.get();
  out->wrench = c.wrench ? c.wrench : h->d_roll_wrench.get();
  out->status = c.status ? c.status : h->d_roll_status.get();
  out->tau = c.tau ? c.tau : h->d_roll_taulog.get();
  out->summary = c.summary ? c.summary : h->d_roll_summary.get();
  return HMPC_OK;
}

extern "C" {

void hmpc_default_plant(struct hmpc_plant *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->dt_tick = 0.005, p->dtMPC = 0.04;
  p->substeps = 1;
  p->mass = 9.0, p->inertia[0] = 0.5413, p->inertia[1] = 0.5200, p->inertia[2] = 0.0691, p->gravity = 9.81;
  for (int leg = 0; leg < 2; ++leg) p->hip[leg][0] = -0.005, p->hip[leg][1] = leg == 0 ? -0.057 : 0.057, p->hip[leg][2] = -0.126;
  p->fall_cos = 0.5;
}

int hmpc_plant_step_device(hmpc_handle *h, void *device_ticks, int batch, const struct hmpc_plant *plant, const float *device_forces,
                           int force_stride, const uint32_t *device_status, const double *device_wpd, int32_t *device_summary,
                           void *stream) {
  if (!h || !device_ticks || !plant || batch < 0 || plant->substeps < 1 || h->nc != 2) return HMPC_E_ARG;
  hmpc::PlantArgs a;
  const int rc = plant_args(h, batch, plant, device_forces, force_stride, device_status, device_wpd, device_summary, &a);
  if (rc != HMPC_OK) return rc;
  if (batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_plant_step((hmpc_tick_inputs *)device_ticks, a, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_set_device_rollout(hmpc_handle *h, const struct hmpc_rollout_log *log) {
  if (!h) return HMPC_E_ARG;
  if (log) h->roll_caller = *log;
  else memset(&h->roll_caller, 0, sizeof(h->roll_caller));
  return HMPC_OK;
}

int hmpc_get_device_rollout(hmpc_handle *h, int n_ticks, struct hmpc_rollout_log *log) {
  if (!h || n_ticks < 1 || !log) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const int rc = own_rollout_buffers(h, n_ticks);
  if (rc != HMPC_OK) return rc;
  *log = {h->d_roll_state.get(), h->d_roll_wrench.get(), h->d_roll_status.get(), h->d_roll_taulog.get(), h->d_roll_summary.get()};
  return HMPC_OK;
}

int hmpc_rollout_device(hmpc_handle *h, void *device_ticks, int batch, int n_ticks, double dtMPC, int ticks_per_step, int subtick0,
                        const struct hmpc_plant *plant, const struct hmpc_rollout_log *log, void *stream) {
  if (!h || !device_ticks || !plant) return HMPC_E_ARG;
  if (n_ticks < 1 || ticks_per_step < 1 || subtick0 < 0 || plant->substeps < 1 || h->nc != 2 || batch < 0 || batch > h->max_batch) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));  // (first: a log that has to grow then waits for this stream alone)
  hmpc_rollout_log lg;
  if (log) lg = *log;
  else {
    const int rc = default_rollout_log(h, n_ticks, &lg);
    if (rc != HMPC_OK) return rc;
  }
  // a tick's clamped world_position_desired and torques, between its solve and its plant step
  if (!h->d_roll_wpd.get()) HIP_TRY(h->d_roll_wpd.alloc((size_t)h->max_batch * 2));
  if (!h->d_roll_tau.get()) HIP_TRY(h->d_roll_tau.alloc((size_t)h->max_batch * 10));
  h->roll_last = lg, h->roll_last_batch = batch, h->roll_last_ticks = n_ticks;
  if (batch == 0) return HMPC_OK;
  const hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hmpc::launch_summary_init(lg.summary, batch, s));
  hmpc_plant pl = *plant;
  pl.dtMPC = dtMPC;
  int shift = 0;  // gait steps the table advanced between the previous tick's solve and this one's
  for (int k = 0; k < n_ticks; ++k) {
    if (h->tick_warm) h->tick_shift = shift;
    int rc = hmpc_tick_solve_device(h, device_ticks, batch, dtMPC, h->d_roll_wpd.get(), /*f_ff=*/nullptr, h->d_roll_tau.get(), stream);
    if (rc != HMPC_OK) return rc;
    if (h->swing_on) RC_TRY(rollout_swing_tick(h, device_ticks, batch, k, n_ticks, ticks_per_step, subtick0, s));  // (hmpc_set_rollout_swing)
    pl.advance_gait =((subtick0 + k + 1) % ticks_per_step == 0) ? 1 : 0;
    hmpc::PlantArgs a;
    rc = plant_args(h, batch, &pl, nullptr, 0, nullptr, h->d_roll_wpd.get(), lg.summary, &a);
    if (rc != HMPC_OK) return rc;
    a.log = lg, a.tau = h->d_roll_tau.get(), a.tick = k, a.n_ticks = n_ticks;
    HIP_TRY(hmpc::launch_plant_step((hmpc_tick_inputs *)device_ticks, a, s));
    shift = pl.advance_gait;
  }
  return HMPC_OK;
}

int hmpc_download_rollout(hmpc_handle *h, double *state, float *wrench, uint32_t *status, double *tau, int32_t *summary) {
  if (!h || h->roll_last_ticks < 1) return HMPC_E_ARG;
  const hmpc_rollout_log &lg = h->roll_last;
  if ((state && !lg.state) || (wrench && !lg.wrench) || (status && !lg.status) || (tau && !lg.tau) || (summary && !lg.summary)) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  const size_t rows = (size_t)h->roll_last_batch * (size_t)h->roll_last_ticks;
  if (rows == 0) return HMPC_OK;
  if (state) HIP_TRY(hipMemcpy(state, lg.state, rows * 12 * sizeof(double), hipMemcpyDeviceToHost));
  if (wrench) HIP_TRY(hipMemcpy(wrench, lg.wrench, rows * 12 * sizeof(float), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, lg.status, rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (tau) HIP_TRY(hipMemcpy(tau, lg.tau, rows * 10 * sizeof(double), hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, lg.summary, (size_t)h->roll_last_batch * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

}  // extern "C"
