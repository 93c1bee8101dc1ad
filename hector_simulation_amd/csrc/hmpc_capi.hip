// hmpc_capi.hip -- the batched C ABI of include/hector_mpc.h over the gfx950 kernels: handles, batches, settings, downloads, the debug
// hooks, the caller-side rows f1-f3 and the device-resident ticks, and the results derived from a solve (prediction, margins, certificate,
// selection).  What a solve launches is hmpc_launch.hip's; the reference's own process-global interface is hmpc_legacy.hip's.
// There is NO CPU fallback: without a gfx950 device every entry point fails (HMPC_E_NO_DEVICE).
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "hmpc_builder_launch.h"
#include "hmpc_handle.h"
#include "hmpc_predict.h"
#include "hmpc_record.h"
#include "hmpc_select.h"

constexpr int MAX_VARS_ANY = 240;
constexpr int DBG_FLOATS_MAX = hmpc::dbg_layout(240, 2).TOTAL > hmpc::dbg_layout(180, 3).TOTAL ? hmpc::dbg_layout(240, 2).TOTAL
                                                                                              : hmpc::dbg_layout(180, 3).TOTAL;

// RAII for the two timing events of hmpc_time_solve
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() {
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
  }
};

extern "C" {

const char *hmpc_last_hip_error(void) { return hip_error_text().c_str(); }
const char *hmpc_version(void) { return "hector_mpc_hip 0.1 (gfx950)"; }

size_t hmpc_record_stride(int horizon) { return (size_t)hmpc::rec_stride(2, horizon); }
size_t hmpc_record_stride_ex(int horizon, int n_contacts) { return (size_t)hmpc::rec_stride(n_contacts == 3 ? 3 : 2, horizon); }

int hmpc_pack_record_ex(void *record, int horizon, int n_contacts, const double *p, const double *v, const double *q,
                        const double *w, const double *r, const double *joint_angles, double yaw, const double *weights,
                        const double *state_trajectory, const double *Alpha_K, const int *gait, const double *Rhand,
                        double f_max_hand) {
  if (n_contacts == 2)
    return hmpc_pack_record(record, horizon, p, v, q, w, r, joint_angles, yaw, weights, state_trajectory, Alpha_K, gait);
  if (n_contacts != 3) return HMPC_E_ARG;
  if (!record || !p || !v || !q || !w || !r || !joint_angles || !weights || !state_trajectory || !Alpha_K || !gait || !Rhand)
    return HMPC_E_ARG;
  if (horizon < 1 || horizon > 10) return HMPC_E_HORIZON;
  hmpc::pack_record<3>(record, horizon, hmpc::RecSource<double, int>{p, v, q, w, r, joint_angles, yaw, weights, state_trajectory, Alpha_K,
                                                                      gait, Rhand, f_max_hand});
  return HMPC_OK;
}

int hmpc_pack_record(void *record, int horizon, const double *p, const double *v, const double *q, const double *w,
                     const double *r, const double *joint_angles, double yaw, const double *weights,
                     const double *state_trajectory, const double *Alpha_K, const int *gait) {
  if (!record || !p || !v || !q || !w || !r || !joint_angles || !weights || !state_trajectory || !Alpha_K || !gait)
    return HMPC_E_ARG;
  if (horizon < 1 || horizon > HMPC_MAX_HORIZON) return HMPC_E_HORIZON;
  hmpc::pack_record<2>(record, horizon, hmpc::RecSource<double, int>{p, v, q, w, r, joint_angles, yaw, weights, state_trajectory, Alpha_K, gait});
  return HMPC_OK;
}

int hmpc_create(hmpc_handle **out, const struct problem_setup *setup, int max_batch, int device) {
  return hmpc_create_ex(out, setup, max_batch, device, 2);
}

int hmpc_contacts(const hmpc_handle *h) { return h ? h->nc : HMPC_E_ARG; }

int hmpc_create_ex(hmpc_handle **out, const struct problem_setup *setup, int max_batch, int device, int n_contacts) {
  if (!out || !setup || max_batch < 1 || (n_contacts != 2 && n_contacts != 3)) return HMPC_E_ARG;
  if (setup->horizon < 1 || setup->horizon > (n_contacts == 3 ? 10 : HMPC_MAX_HORIZON)) return HMPC_E_HORIZON;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) {
    hip_error_text() = "no HIP device visible (libhector_mpc_hip has no CPU fallback)";
    return HMPC_E_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  hmpc_handle *h = new (std::nothrow) hmpc_handle();
  if (!h) return HMPC_E_ARG;
  h->setup = *setup;
  h->max_batch = max_batch;
  h->device = device;
  h->nc = n_contacts;
  h->stride = (size_t)hmpc::rec_stride(n_contacts, setup->horizon);
  hmpc_default_params(&h->params);
  const size_t mb = (size_t)max_batch, nf = mb * 6 * n_contacts * setup->horizon;
  const bool ok = h->d_record_store.alloc(mb * h->stride) == hipSuccess && h->d_forces.ensure(nf) == hipSuccess &&
                  h->d_status.ensure(mb) == hipSuccess && alloc_filled_done(h->d_flagged, 1, 0) == hipSuccess &&
                  (n_contacts != 2 || alloc_filled_done(h->d_cls, mb, 0) == hipSuccess) &&
                  (max_batch <= DISPATCH_ORDER_MIN_BATCH || (h->d_order.alloc(mb) == hipSuccess && h->d_keys.alloc(mb) == hipSuccess));
  if (!ok) {
    hip_error_text() = "hipMalloc failed in hmpc_create";
    delete h;
    return HMPC_E_HIP;
  }
  h->d_records = h->d_record_store.get();
  *out = h;
  return HMPC_OK;
}

int hmpc_destroy(hmpc_handle *h) {
  if (!h) return HMPC_E_ARG;
  hipSetDevice(h->device);
  (void)settle(h);  // the stream rule: the handle's memory is freed next (an error here must not keep the handle alive)
  delete h;  // (every device buffer of the handle frees itself)
  return HMPC_OK;
}

// The handle now holds another batch: everything enqueued for the one before no longer counts.  max_stance = its widest reduced QP where
// the host knows it (else -1), cls_valid = whether the device already holds its size classes.
static void replace_batch(hmpc_handle *h, const unsigned char *records, int batch, int max_stance, int cls_valid) {
  h->d_records = records;
  h->batch = batch;
  h->results.on_batch();
  h->max_stance = max_stance;
  h->cls_valid = cls_valid;
}

// pitch = bytes between consecutive records of the batch in host memory (h->stride: a packed array)
static int upload_common(hmpc_handle *h, const void *host_records, int batch, bool async, hipStream_t stream, size_t pitch = 0) {
  if (!h || !host_records || batch < 0) return HMPC_E_ARG;
  if (batch > h->max_batch) return HMPC_E_BATCH;
  if (pitch == 0) pitch = h->stride;
  if (pitch < h->stride || pitch % 4 != 0) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  // the copy replaces the records a pending solve may have yet to read: behind the handle's stream, or once the handle has settled
  RC_TRY(async ? enter_stream(h, stream) : settle(h));
  if (pitch != h->stride) {
    if (batch > 0)
      HIP_TRY(hipMemcpy2DAsync(h->d_record_store.get(), h->stride, host_records, pitch, h->stride, (size_t)batch, hipMemcpyHostToDevice, stream));
  } else if (async)
    HIP_TRY(hipMemcpyAsync(h->d_record_store.get(), host_records, (size_t)batch * h->stride, hipMemcpyHostToDevice, stream));
  else
    HIP_TRY(hipMemcpy(h->d_record_store.get(), host_records, (size_t)batch * h->stride, hipMemcpyHostToDevice));
  // host-side scan of the gait tables: the widest reduced QP in the batch picks the kernel variant (LDS footprint)
  const int hz = h->setup.horizon;
  int mx = 0;
  const unsigned char *rec = (const unsigned char *)host_records;
  for (int b = 0; b < batch; ++b) {
    const int cnt = hmpc::rec_stance_count(rec + (size_t)b * pitch, h->nc, hz, h->setup.f_max);
    if (cnt > mx) mx = cnt;
  }
  replace_batch(h, h->d_record_store.get(), batch, 6 * mx, /*cls_valid=*/0);
  return HMPC_OK;
}

int hmpc_upload_records(hmpc_handle *h, const void *host_records, int batch) {
  return upload_common(h, host_records, batch, false, nullptr);
}

int hmpc_upload_records_async(hmpc_handle *h, const void *host_records, int batch, void *stream) {
  return upload_common(h, host_records, batch, true, (hipStream_t)stream);
}

int hmpc_upload_records_strided_async(hmpc_handle *h, const void *host_records, int batch, size_t pitch_bytes, void *stream) {
  return upload_common(h, host_records, batch, true, (hipStream_t)stream, pitch_bytes);
}

int hmpc_download_async(hmpc_handle *h, float *forces, uint32_t *status, void *stream) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  const size_t nf = (size_t)h->batch * 6 * h->nc * h->setup.horizon;
  if (forces && nf)
    HIP_TRY(hipMemcpyAsync(forces, h->d_forces.get(), nf * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (status && h->batch)
    HIP_TRY(hipMemcpyAsync(status, h->d_status.get(), (size_t)h->batch * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_set_device_records(hmpc_handle *h, const void *device_records, int batch) {
  if (!h || !device_records || batch < 0) return HMPC_E_ARG;
  if (batch > h->max_batch) return HMPC_E_BATCH;
  // (widest reduced QP unknown: hmpc_solve counts the size classes on the device, or hmpc_set_max_reduced_vars tells)
  replace_batch(h, (const unsigned char *)device_records, batch, /*max_stance=*/-1, /*cls_valid=*/0);
  return HMPC_OK;
}

int hmpc_set_max_reduced_vars(hmpc_handle *h, int n_reduced) {
  if (!h) return HMPC_E_ARG;
  h->max_stance = n_reduced;
  return HMPC_OK;
}

int hmpc_set_dispatch_order(hmpc_handle *h, int mode) {
  if (!h || (mode != 0 && mode != 1 && mode != 2)) return HMPC_E_ARG;
  if (mode != 0 && h->max_batch > DISPATCH_ORDER_MIN_BATCH && (!h->d_order.get() || !h->d_keys.get())) {
    HIP_TRY(hipSetDevice(h->device));
    if (!h->d_order.get()) HIP_TRY(h->d_order.alloc((size_t)h->max_batch));
    if (!h->d_keys.get()) HIP_TRY(h->d_keys.alloc((size_t)h->max_batch));
  }
  h->dispatch_order = mode;
  h->order_batch = 0;  // the next solve is ordered by the predictor (mode 1, 2) and leaves the iteration counts the one after it sorts by (mode 1)
  h->order_valid = false;
  return HMPC_OK;
}

int hmpc_set_max_iterations(hmpc_handle *h, int max_iter) {
  if (!h || max_iter < 0) return HMPC_E_ARG;
  h->iter_cap = max_iter;
  return HMPC_OK;
}

void hmpc_default_params(struct hmpc_params *p) {
  if (!p) return;
  p->mass = 9.0f;                                                   // SolverMPC.cpp:423
  p->inertia[0] = 0.5413f, p->inertia[1] = 0.5200f, p->inertia[2] = 0.0691f;  // RobotState.cpp:45
  p->mu = 2.0f, p->lt = 0.09f, p->lh = 0.06f;                       // SolverMPC.cpp:488-490
  p->gravity = 9.81f;                                               // SolverMPC.cpp:420
}

int hmpc_set_params(hmpc_handle *h, const struct hmpc_params *p) {
  if (!h) return HMPC_E_ARG;
  if (!p) {
    hmpc_default_params(&h->params);
    return HMPC_OK;
  }
  if (!params_ok(*p)) return HMPC_E_ARG;
  h->params = *p;
  return HMPC_OK;
}

int hmpc_set_instance_mu(hmpc_handle *h, const float *device_mu) {
  if (!h) return HMPC_E_ARG;
  h->d_mu_inst = device_mu;
  return HMPC_OK;
}

int hmpc_get_params(const hmpc_handle *h, struct hmpc_params *p) {
  if (!h || !p) return HMPC_E_ARG;
  *p = h->params;
  return HMPC_OK;
}

int hmpc_set_handover(hmpc_handle *h, int on) {
  if (!h) return HMPC_E_ARG;
  h->handover = on ? 1 : 0;
  return HMPC_OK;
}

int hmpc_set_auto_resolve(hmpc_handle *h, int on) {
  if (!h) return HMPC_E_ARG;
  h->auto_resolve = on ? 1 : 0;
  return HMPC_OK;
}

int hmpc_set_warm_start(hmpc_handle *h, int on) {
  if (!h) return HMPC_E_ARG;
  h->warm = on ? 1 : 0;
  return HMPC_OK;
}

int hmpc_set_tick_warm_start(hmpc_handle *h, int on, int horizon_shift) {
  if (!h || horizon_shift < 0) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  if (on && !h->d_wset.get()) HIP_TRY(alloc_filled_done(h->d_wset, (size_t)h->max_batch * 8 * h->nc * h->setup.horizon, 0));
  h->tick_warm = on ? 1 : 0;
  h->tick_shift = horizon_shift;
  return HMPC_OK;
}

int hmpc_reset_tick_warm_start(hmpc_handle *h) {
  if (!h) return HMPC_E_ARG;
  if (!h->d_wset.get()) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  // on the handle's stream, not the null stream: behind the solve that may still be writing the sets and ahead of the next one on that
  // stream, with no wait on the host (a solve on another stream settles the handle first, like any call that changes streams)
  HIP_TRY(hipMemsetAsync(h->d_wset.get(), 0, (size_t)h->max_batch * 8 * h->nc * h->setup.horizon, h->last_stream));
  return HMPC_OK;
}

int hmpc_set_device_outputs(hmpc_handle *h, float *device_forces, uint32_t *device_status) {
  if (!h) return HMPC_E_ARG;
  h->d_forces.set_caller(device_forces), h->d_status.set_caller(device_status);
  return HMPC_OK;
}

int hmpc_solve(hmpc_handle *h, void *stream) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  return enqueue_solve(h, (hipStream_t)stream, /*carry_wset=*/true);
}

int hmpc_solve_command_sweep(hmpc_handle *h, int group_size, void *stream) {
  if (!h || group_size < 1) return HMPC_E_ARG;
  if (h->nc != 2 || h->setup.horizon > 10) return HMPC_E_ARG;  // (the shapes the sweep kernels are built for)
  if (h->batch == 0) return HMPC_OK;
  if (h->batch % group_size != 0) return HMPC_E_ARG;
  if (group_size == 1) return hmpc_solve(h, stream);
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  return enqueue_command_sweep(h, (hipStream_t)stream, group_size);
}

int hmpc_resolve_failed(hmpc_handle *h, int *n_resolved) {
  if (!h) return HMPC_E_ARG;
  if (n_resolved) *n_resolved = 0;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return resolve_failed(h, n_resolved);
}

int hmpc_set_device_repair(hmpc_handle *h, int on) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  if (on && (!h->d_flag_list.get() || !h->d_flag_count.get())) {
    // both buffers or neither: they are committed to the handle only once both exist and are cleared
    DeviceBuffer<int> list;
    DeviceBuffer<unsigned int> count;
    if (alloc_filled_done(list, (size_t)(flag_list_cap(h->max_batch) + REG_LIST_CAP), 0) != hipSuccess || alloc_filled_done(count, 2, 0) != hipSuccess) {
      hip_error_text() = "hipMalloc failed in hmpc_set_device_repair";
      return HMPC_E_HIP;
    }
    h->d_flag_list = std::move(list), h->d_flag_count = std::move(count);
  }
  h->device_repair = (on == 2) ? 2 : (on ? 1 : 0);
  return HMPC_OK;
}

// the safe pass of hmpc_download / hmpc_download_f64: one 4-byte read of the device's flagged counter decides whether
// the status words need to be scanned at all (they almost never do: nominal inputs flag nothing)
static int resolve_if_flagged(hmpc_handle *h) {
  unsigned int now = 0;
  HIP_TRY(hipMemcpy(&now, h->d_flagged.get(), sizeof(now), hipMemcpyDeviceToHost));
  if (now == h->flagged_seen) return HMPC_OK;
  const int rc = hmpc_resolve_failed(h, nullptr);
  if (rc != HMPC_OK) return rc;
  HIP_TRY(hipMemcpy(&now, h->d_flagged.get(), sizeof(now), hipMemcpyDeviceToHost));  // the safe pass may have flagged again
  h->flagged_seen = now;
  return HMPC_OK;
}

int hmpc_download(hmpc_handle *h, float *forces, uint32_t *status) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  if (h->auto_resolve && h->batch) {
    int rc = resolve_if_flagged(h);
    if (rc != HMPC_OK) return rc;
  }
  const size_t nf = (size_t)h->batch * 6 * h->nc * h->setup.horizon;
  if (forces && nf) HIP_TRY(hipMemcpy(forces, h->d_forces.get(), nf * sizeof(float), hipMemcpyDeviceToHost));
  if (status && h->batch)
    HIP_TRY(hipMemcpy(status, h->d_status.get(), (size_t)h->batch * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_get_device_outputs(hmpc_handle *h, float **device_forces, uint32_t **device_status) {
  if (!h) return HMPC_E_ARG;
  if (device_forces) *device_forces = h->d_forces.get();
  if (device_status) *device_status = h->d_status.get();
  return HMPC_OK;
}

int hmpc_batch(const hmpc_handle *h) { return h ? h->batch : HMPC_E_ARG; }
int hmpc_horizon(const hmpc_handle *h) { return h ? h->setup.horizon : HMPC_E_ARG; }

int hmpc_time_solve(hmpc_handle *h, void *stream, int reps, float *ms_per_launch) {
  if (!h || reps < 1 || !ms_per_launch) return HMPC_E_ARG;
  *ms_per_launch = 0.f;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  EventPair ev;  // destroyed on every return path
  HIP_TRY(hipEventCreate(&ev.e0));
  HIP_TRY(hipEventCreate(&ev.e1));
  hipStream_t s = (hipStream_t)stream;
  RC_TRY(enter_stream(h, s));
  HIP_TRY(hipEventRecord(ev.e0, s));
  for (int i = 0; i < reps; ++i) {
    // a single timed launch is a genuine solve of the current batch (it consumes and leaves the tick-to-tick working sets);
    // repetitions of the same batch must not advance them again
    int rc = enqueue_solve(h, s, /*carry_wset=*/reps == 1);  // the same launches hmpc_solve enqueues (size classes, device repair)
    if (rc != HMPC_OK) return rc;
  }
  HIP_TRY(hipEventRecord(ev.e1, s));
  HIP_TRY(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_per_launch = ms / (float)reps;
  return HMPC_OK;
}

int hmpc_debug_assemble(hmpc_handle *h, int index, int *n, int *m, int *var_ind, float *H, float *g, float *Fc,
                        float *lb, float *ub, float *x0, float *Acd, float *Bcd) {
  if (!h || index < 0 || index >= h->batch) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const int vi = pick_variant(h);
  const Variant &v = variants()[vi];
  RC_TRY(enter_stream(h, nullptr));
  if (!h->d_dbg_f.get()) HIP_TRY(h->d_dbg_f.alloc((size_t)DBG_FLOATS_MAX));
  if (!h->d_dbg_i.get()) HIP_TRY(h->d_dbg_i.alloc(2 + MAX_VARS_ANY));
  HIP_TRY(hipMemset(h->d_dbg_i.get(), 0, sizeof(int) * (2 + MAX_VARS_ANY)));
  LaunchOpt ao;
  ao.assemble_only = true, ao.dbg_index = index;
  int rc = launch(h, 0, vi, ao);
  if (rc != HMPC_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<float> hf(v.dbg_floats);
  std::vector<int> hi(2 + MAX_VARS_ANY);
  HIP_TRY(hipMemcpy(hf.data(), h->d_dbg_f.get(), sizeof(float) * hf.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hi.data(), h->d_dbg_i.get(), sizeof(int) * hi.size(), hipMemcpyDeviceToHost));
  const int nn = hi[0], mm = hi[1], hz = h->setup.horizon;
  if (n) *n = nn;
  if (m) *m = mm;
  if (nn > v.nmax) return HMPC_OK;  // too large: only n, m are meaningful
  const int nc = v.nc;
  const hmpc::DbgOffsets o = hmpc::dbg_layout(v.nmax, nc);
  if (var_ind) memcpy(var_ind, hi.data() + 2, sizeof(int) * nn);
  if (H) memcpy(H, hf.data(), sizeof(float) * (size_t)nn * nn);
  if (g) memcpy(g, hf.data() + o.G, sizeof(float) * nn);
  if (Fc) memcpy(Fc, hf.data() + o.FC, sizeof(float) * 48 * nc * nc);
  if (lb) memcpy(lb, hf.data() + o.LB, sizeof(float) * 8 * nc * hz);
  if (ub) memcpy(ub, hf.data() + o.UB, sizeof(float) * 8 * nc * hz);
  if (x0) memcpy(x0, hf.data() + o.X0, sizeof(float) * 13);
  if (Acd) memcpy(Acd, hf.data() + o.ACD, sizeof(float) * 169);
  if (Bcd) memcpy(Bcd, hf.data() + o.BCD, sizeof(float) * 78 * nc);
  return HMPC_OK;
}

// Parity hook: stages S, W, Q of the kernel (inverse by sweeps, block start, dual active set, scatter) on QP data handed
// in from outside -- e.g. the reference's own H_red / g_red / fmat as its source left them -- instead of the kernel's own
// assembly.  The current batch's records still provide the gait tables (which leg-steps exist) and f_max.
int hmpc_debug_solve_external_qp(hmpc_handle *h, const float *H, const float *g, const float *Fc, int ld) {
  if (!h || !H || !g || !Fc || ld < 1) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  {
    // the kernel reads H[i*ld + j], g[i] for i, j < the instance's reduced-variable count: ld must cover the widest one
    // (known for host-uploaded records; otherwise whatever the variant that will be launched can hold)
    const int need = (h->max_stance >= 0) ? h->max_stance : variants()[pick_variant(h)].nmax;
    if (ld < need) return HMPC_E_ARG;
  }
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  const size_t nb = (size_t)h->batch, nfc = (size_t)8 * h->nc * 6 * h->nc;
  DeviceBuffer<float> ext;  // (freed on every return path)
  HIP_TRY(ext.alloc(nb * ((size_t)ld * ld + ld + nfc)));
  float *dH = ext.get(), *dg = dH + nb * ld * ld, *dF = dg + nb * ld;
  HIP_TRY(hipMemcpy(dH, H, sizeof(float) * nb * ld * ld, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dg, g, sizeof(float) * nb * ld, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dF, Fc, sizeof(float) * nb * nfc, hipMemcpyHostToDevice));
  h->d_ext_H = dH, h->d_ext_g = dg, h->d_ext_Fc = dF, h->ext_ld = ld;
  LaunchOpt xo;
  xo.carry_wset = false;
  const int rc = enqueue_fast(h, h->last_stream, pick_variant(h), /*classes=*/false, xo);
  const int src = settle(h);  // (ext is freed on return)
  h->d_ext_H = h->d_ext_g = h->d_ext_Fc = nullptr;
  h->ext_ld = 0;
  return rc != HMPC_OK ? rc : src;
}

int hmpc_debug_handover_slots(hmpc_handle *h, int *slots) {
  if (!h || !slots) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  if (!h->d_spill_slot.get()) {  // (no saving variant has run on this handle: nothing was ever handed over)
    for (int i = 0; i < h->batch; ++i) slots[i] = -1;
    return HMPC_OK;
  }
  HIP_TRY(hipMemcpy(slots, h->d_spill_slot.get(), (size_t)h->batch * sizeof(int), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_debug_phase_cycles(hmpc_handle *h, long long *cycles /*[batch][NPROF = 32]*/) {
#ifndef HMPC_PROFILE
  (void)h;
  (void)cycles;
  hip_error_text() = "library built without -DHMPC_PROFILE";
  return HMPC_E_ARG;
#else
  if (!h || !cycles) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nb = (size_t)h->max_batch * hmpc::NPROF * sizeof(long long);
  if (!h->d_prof.get()) HIP_TRY(h->d_prof.alloc((size_t)h->max_batch * hmpc::NPROF));
  HIP_TRY(hipMemset(h->d_prof.get(), 0, nb));
  // (with the device-side repair on, the whole chain: an instance's slot then holds the numbers of the LAST variant that ran it)
  int rc = h->device_repair ? enqueue_solve(h, h->last_stream, false) : launch(h, h->last_stream, pick_variant(h), LaunchOpt());
  if (rc != HMPC_OK) return rc;
  RC_TRY(settle(h));
  HIP_TRY(hipMemcpy(cycles, h->d_prof.get(), (size_t)h->batch * hmpc::NPROF * sizeof(long long), hipMemcpyDeviceToHost));
  h->d_prof.reset();
  return HMPC_OK;
#endif
}

// ---------------------------------------------------------------------------------------------------- rows f1-f3
int hmpc_build_records_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, double *device_wpd_out,
                              void *stream) {
  if (h && h->nc != 2) return HMPC_E_ARG;  // rows f1-f3 restate the reference's two-foot controller code
  if (!h || !device_ticks || batch < 0) return HMPC_E_ARG;
  if (batch > h->max_batch) return HMPC_E_BATCH;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));  // (the builder writes the record store and the size classes)
  HIP_TRY(hmpc::launch_build_records((const hmpc_tick_inputs *)device_ticks, batch, h->setup.horizon, dtMPC, h->d_record_store.get(),
                                     (int)h->stride, device_wpd_out, h->setup.f_max, h->d_cls.get(), (hipStream_t)stream));
  // (the builder left every instance's size class on the device: hmpc_solve routes by it)
  replace_batch(h, h->d_record_store.get(), batch, /*max_stance=*/-1, /*cls_valid=*/1);
  return HMPC_OK;
}

int hmpc_build_records(hmpc_handle *h, const struct hmpc_tick_inputs *host_ticks, int batch, double dtMPC, double *wpd_out) {
  if (!h || !host_ticks || batch < 0) return HMPC_E_ARG;
  if (batch > h->max_batch) return HMPC_E_BATCH;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));  // the shared scratch may hold a pending sweep's expanded ticks, the record store a pending solve's records
  const size_t nb = (size_t)(batch > 0 ? batch : 1);
  const size_t off_w = (sizeof(hmpc_tick_inputs) * nb + 255) & ~(size_t)255;
  void *sp = nullptr;
  int rc = scratch(h, off_w + sizeof(double) * 2 * nb, &sp);
  if (rc != HMPC_OK) return rc;
  hmpc_tick_inputs *d_t = (hmpc_tick_inputs *)sp;
  double *d_w = (double *)((char *)sp + off_w);
  HIP_TRY(hipMemcpy(d_t, host_ticks, sizeof(hmpc_tick_inputs) * (size_t)batch, hipMemcpyHostToDevice));
  rc = hmpc_build_records_device(h, d_t, batch, dtMPC, d_w, nullptr);
  if (rc != HMPC_OK) return rc;
  RC_TRY(settle(h));
  if (wpd_out && batch) HIP_TRY(hipMemcpy(wpd_out, d_w, sizeof(double) * 2 * (size_t)batch, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_body_wrench_device(hmpc_handle *h, const double *device_rBody, double *device_f_ff, void *stream) {
  if (h && h->nc != 2) return HMPC_E_ARG;  // rows f1-f3 restate the reference's two-foot controller code
  if (!h || !device_rBody || !device_f_ff) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_body_wrench(h->d_forces.get(), h->batch, h->setup.horizon, device_rBody, device_f_ff, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_body_wrench(hmpc_handle *h, const double *host_rBody, double *host_f_ff) {
  if (!h || !host_rBody || !host_f_ff) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t b = (size_t)h->batch;
  RC_TRY(settle(h));  // before the copies: the shared scratch may hold a pending sweep's expanded ticks
  void *sp = nullptr;
  int rc = scratch(h, sizeof(double) * (9 + 12) * b, &sp);
  if (rc != HMPC_OK) return rc;
  double *d_r = (double *)sp, *d_f = d_r + 9 * b;
  HIP_TRY(hipMemcpy(d_r, host_rBody, sizeof(double) * 9 * b, hipMemcpyHostToDevice));
  rc = hmpc_body_wrench_device(h, d_r, d_f, nullptr);
  if (rc != HMPC_OK) return rc;
  RC_TRY(settle(h));
  HIP_TRY(hipMemcpy(host_f_ff, d_f, sizeof(double) * 12 * b, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_leg_torques_device(hmpc_handle *h, const double *device_rBody, const double *device_leg_q, double *device_f_ff,
                            double *device_tau, void *stream) {
  if (h && h->nc != 2) return HMPC_E_ARG;  // rows f1-f3 restate the reference's two-foot controller code
  if (!h || !device_rBody || !device_leg_q || !device_tau) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_leg_torques(h->d_forces.get(), h->batch, h->setup.horizon, device_rBody, device_leg_q, device_f_ff, device_tau,
                                   /*ticks=*/nullptr, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_leg_torques(hmpc_handle *h, const double *host_rBody, const double *host_leg_q, double *host_f_ff, double *host_tau) {
  if (!h || !host_rBody || !host_leg_q || !host_tau) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nb = (size_t)h->batch;
  RC_TRY(settle(h));  // before the copies: the shared scratch may hold a pending sweep's expanded ticks
  void *sp = nullptr;
  int rc = scratch(h, sizeof(double) * (9 + 10 + 12 + 10) * nb, &sp);
  if (rc != HMPC_OK) return rc;
  double *d_r = (double *)sp, *d_q = d_r + 9 * nb, *d_f = d_q + 10 * nb, *d_t = d_f + 12 * nb;
  HIP_TRY(hipMemcpy(d_r, host_rBody, sizeof(double) * 9 * nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_q, host_leg_q, sizeof(double) * 10 * nb, hipMemcpyHostToDevice));
  rc = hmpc_leg_torques_device(h, d_r, d_q, d_f, d_t, nullptr);
  if (rc != HMPC_OK) return rc;
  RC_TRY(settle(h));
  if (host_f_ff) HIP_TRY(hipMemcpy(host_f_ff, d_f, sizeof(double) * 12 * nb, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(host_tau, d_t, sizeof(double) * 10 * nb, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// One MPC tick of a whole batch without leaving the device (rows f1+f2 -> a1..a16 -> f3 of SURVEY.md section 8):
// updateMPCIfNeeded's input construction + gait table (ConvexMPCLocomotion.cpp:283-406, GaitGenerator.cpp:85-103), the solve
// routed by size class (a walking tick runs on the 60-variable variant), then f_ff = -rBody [GRF; GRM] and tau = J_fm' f_ff
// (ConvexMPCLocomotion.cpp:419-440, common/LegController.cpp:57-61, 108-167) -- three or four launches on ONE stream, no
// host synchronisation, nothing but the tick structs in and the torques out.
int hmpc_tick_solve_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, double *device_wpd_out,
                           double *device_f_ff, double *device_tau, void *stream) {
  if (!h || !device_ticks || !device_tau || batch < 0) return HMPC_E_ARG;
  int rc = hmpc_build_records_device(h, device_ticks, batch, dtMPC, device_wpd_out, stream);
  if (rc != HMPC_OK) return rc;
  if (batch == 0) return HMPC_OK;
  rc = enqueue_solve(h, (hipStream_t)stream, /*carry_wset=*/true);
  if (rc != HMPC_OK) return rc;
  HIP_TRY(hmpc::launch_leg_torques(h->d_forces.get(), batch, h->setup.horizon, /*rBody=*/nullptr, /*leg_q=*/nullptr, device_f_ff, device_tau,
                                   (const hmpc_tick_inputs *)device_ticks, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_download_records(hmpc_handle *h, void *host_records) {
  if (!h || !host_records) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  if (h->batch) HIP_TRY(hipMemcpy(host_records, h->d_records, (size_t)h->batch * h->stride, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_enable_f64_output(hmpc_handle *h) {
  if (!h) return HMPC_E_ARG;
  if (h->d_x64.get()) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  // both buffers or neither
  DeviceBuffer<double> x, obj;
  HIP_TRY(x.alloc((size_t)h->max_batch * 6 * h->nc * h->setup.horizon));
  if (obj.alloc((size_t)h->max_batch) != hipSuccess) {
    hip_error_text() = "hipMalloc failed in hmpc_enable_f64_output";
    return HMPC_E_HIP;
  }
  h->d_x64 = std::move(x), h->d_obj64 = std::move(obj);
  return HMPC_OK;
}

int hmpc_download_f64(hmpc_handle *h, double *x, double *obj) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->d_x64.get()) {
    // the copy-out was not enabled before the solve: enable it and run the current batch once more -- without consuming
    // the tick-to-tick working sets a second time -- then give flagged instances the same safe pass hmpc_download gives
    int rc = hmpc_enable_f64_output(h);
    if (rc != HMPC_OK) return rc;
    rc = enqueue_solve(h, h->last_stream, /*carry_wset=*/false);
    if (rc != HMPC_OK) return rc;
  }
  RC_TRY(settle(h));
  if (h->auto_resolve) {
    const int rc = resolve_if_flagged(h);
    if (rc != HMPC_OK) return rc;
  }
  const size_t nb = (size_t)h->batch * 6 * h->nc * h->setup.horizon;
  if (x && nb) HIP_TRY(hipMemcpy(x, h->d_x64.get(), nb * sizeof(double), hipMemcpyDeviceToHost));
  if (obj && h->batch) HIP_TRY(hipMemcpy(obj, h->d_obj64.get(), (size_t)h->batch * sizeof(double), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Prediction: the model's own state trajectory and tracking cost under the forces of the last solve (hmpc_predict.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next prediction goes: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int prediction_buffers(hmpc_handle *h, float **states, double **cost) {
  HIP_TRY(h->d_pred_states.ensure((size_t)h->max_batch * h->setup.horizon * 13));
  HIP_TRY(h->d_pred_cost.ensure((size_t)h->max_batch * 2));
  *states = h->d_pred_states.get(), *cost = h->d_pred_cost.get();
  return HMPC_OK;
}

int hmpc_set_device_prediction(hmpc_handle *h, float *device_states, double *device_cost) {
  if (!h) return HMPC_E_ARG;
  h->d_pred_states.set_caller(device_states), h->d_pred_cost.set_caller(device_cost);
  h->results.retarget_prediction();
  return HMPC_OK;
}

int hmpc_get_device_prediction(hmpc_handle *h, float **device_states, double **device_cost) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  float *s = nullptr;
  double *c = nullptr;
  const int rc = prediction_buffers(h, &s, &c);
  if (rc != HMPC_OK) return rc;
  if (device_states) *device_states = s;
  if (device_cost) *device_cost = c;
  return HMPC_OK;
}

int hmpc_predict_states(hmpc_handle *h, void *stream) {
  if (!h || !h->results.has_solve()) return HMPC_E_ARG;  // no solve of the current batch: the force buffer holds another batch's forces, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  float *s = nullptr;
  double *c = nullptr;
  const int rc = prediction_buffers(h, &s, &c);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (no index list, no external QP data, relax 0: stage A as an ordinary solve runs it)
  set_problem_args(h, a);
  a.mu_inst = nullptr;  // (friction shapes the constraint block only; the model does not depend on it)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_predict(h->nc, a, s, c, (hipStream_t)stream));
  h->results.on_predict();
  return HMPC_OK;
}

int hmpc_download_prediction(hmpc_handle *h, float *states, double *cost) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_prediction()) return HMPC_E_ARG;  // nothing predicted from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  float *s = nullptr;
  double *c = nullptr;
  const int rc = prediction_buffers(h, &s, &c);
  if (rc != HMPC_OK) return rc;
  if (states) HIP_TRY(hipMemcpy(states, s, (size_t)h->batch * h->setup.horizon * 13 * sizeof(float), hipMemcpyDeviceToHost));
  if (cost) HIP_TRY(hipMemcpy(cost, c, (size_t)h->batch * 2 * sizeof(double), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Constraint margins: how far the forces of the last solve are from every limit the QP was solved under (hmpc_margins.hip).
// ------------------------------------------------------------------------------------------------------------------
struct MarginBuffers {
  double *slack, *summary;
  int32_t *where;
};

// where the next margins go: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int margin_buffers(hmpc_handle *h, MarginBuffers *b) {
  const size_t mb = (size_t)h->max_batch;
  HIP_TRY(h->d_mar_slack.ensure(mb * h->setup.horizon * h->nc * 10));
  HIP_TRY(h->d_mar_summary.ensure(mb * hmpc::MARGIN_CLASSES));
  HIP_TRY(h->d_mar_where.ensure(mb * hmpc::MARGIN_CLASSES));
  *b = {h->d_mar_slack.get(), h->d_mar_summary.get(), h->d_mar_where.get()};
  return HMPC_OK;
}

int hmpc_set_device_margins(hmpc_handle *h, double *device_slack, double *device_summary, int32_t *device_where) {
  if (!h) return HMPC_E_ARG;
  h->d_mar_slack.set_caller(device_slack), h->d_mar_summary.set_caller(device_summary), h->d_mar_where.set_caller(device_where);
  h->results.retarget_margins();
  return HMPC_OK;
}

int hmpc_get_device_margins(hmpc_handle *h, double **device_slack, double **device_summary, int32_t **device_where) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  MarginBuffers b;
  const int rc = margin_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_slack) *device_slack = b.slack;
  if (device_summary) *device_summary = b.summary;
  if (device_where) *device_where = b.where;
  return HMPC_OK;
}

int hmpc_constraint_margins(hmpc_handle *h, void *stream) {
  if (!h || !h->results.has_solve()) return HMPC_E_ARG;  // no solve of the current batch: the force buffer holds another batch's forces, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  MarginBuffers b;
  const int rc = margin_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (no index list, no external QP data, relax 0: stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: friction shapes the constraint block)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_margins(h->nc, a, b.slack, b.summary, b.where, (hipStream_t)stream));
  h->results.on_margins();
  return HMPC_OK;
}

int hmpc_download_margins(hmpc_handle *h, double *slack, double *summary, int32_t *where) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_margins()) return HMPC_E_ARG;  // nothing computed from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  MarginBuffers b;
  const int rc = margin_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch;
  if (slack) HIP_TRY(hipMemcpy(slack, b.slack, n * h->setup.horizon * h->nc * 10 * sizeof(double), hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, n * hmpc::MARGIN_CLASSES * sizeof(double), hipMemcpyDeviceToHost));
  if (where) HIP_TRY(hipMemcpy(where, b.where, n * hmpc::MARGIN_CLASSES * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_margin_penalty(hmpc_handle *h, const double floor[6], const double *device_penalty_in, double *device_penalty_out, void *stream) {
  if (!h || !floor || !device_penalty_out) return HMPC_E_ARG;
  if (!h->results.has_margins()) return HMPC_E_ARG;  // no margins of the last solve of this batch: the summary holds another solve's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  MarginBuffers b;
  const int rc = margin_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_margin_penalty(b.summary, floor, device_penalty_in, device_penalty_out, h->batch, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_set_sweep_margin_floor(hmpc_handle *h, const double floor[6]) {
  if (!h) return HMPC_E_ARG;
  h->sweep_floor_on = floor != nullptr;
  for (int k = 0; k < hmpc::MARGIN_CLASSES; ++k) h->sweep_floor[k] = floor ? floor[k] : 0.0;
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// KKT certificate: whether the forces of the last solve minimise the QP, and its multipliers (hmpc_certificate.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next certificate goes: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int certificate_buffers(hmpc_handle *h, hmpc::CertificateOut *b) {
  const size_t mb = (size_t)h->max_batch, ls = mb * h->setup.horizon * h->nc;
  HIP_TRY(h->d_cert_grad.ensure(ls * 6));
  HIP_TRY(h->d_cert_lambda.ensure(ls * 10));
  HIP_TRY(h->d_cert_resid.ensure(ls * 6));
  HIP_TRY(h->d_cert_summary.ensure(mb * hmpc::CERT_CLASSES));
  HIP_TRY(h->d_cert_where.ensure(mb * hmpc::CERT_WHERE));
  *b = {h->d_cert_grad.get(), h->d_cert_lambda.get(), h->d_cert_resid.get(), h->d_cert_summary.get(), h->d_cert_where.get()};
  return HMPC_OK;
}

int hmpc_set_device_certificate(hmpc_handle *h, double *device_grad, double *device_lambda, double *device_resid, double *device_summary,
                                int32_t *device_where) {
  if (!h) return HMPC_E_ARG;
  h->d_cert_grad.set_caller(device_grad), h->d_cert_lambda.set_caller(device_lambda), h->d_cert_resid.set_caller(device_resid);
  h->d_cert_summary.set_caller(device_summary), h->d_cert_where.set_caller(device_where);
  h->results.retarget_certificate();
  return HMPC_OK;
}

int hmpc_get_device_certificate(hmpc_handle *h, double **device_grad, double **device_lambda, double **device_resid, double **device_summary,
                                int32_t **device_where) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::CertificateOut b;
  const int rc = certificate_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_grad) *device_grad = b.grad;
  if (device_lambda) *device_lambda = b.lambda;
  if (device_resid) *device_resid = b.resid;
  if (device_summary) *device_summary = b.summary;
  if (device_where) *device_where = b.where;
  return HMPC_OK;
}

int hmpc_set_certificate_tolerance(hmpc_handle *h, double act_tol) {
  if (!h || !(act_tol > 0.0 && act_tol < 0.005)) return HMPC_E_ARG;  // (0.005: half the Mx window, above which both sides of row 4 would be active at once)
  h->cert_act_tol = act_tol;
  return HMPC_OK;
}

int hmpc_kkt_certificate(hmpc_handle *h, void *stream) {
  if (!h || !h->results.has_solve()) return HMPC_E_ARG;  // no solve of the current batch: the force buffer holds another batch's forces, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::CertificateOut b;
  const int rc = certificate_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (no index list, no external QP data, relax 0: stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: friction shapes the constraint block)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_certificate(h->nc, a, h->cert_act_tol, b, (hipStream_t)stream));
  h->results.on_certificate();
  return HMPC_OK;
}

int hmpc_download_certificate(hmpc_handle *h, double *grad, double *lambda, double *resid, double *summary, int32_t *where) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_certificate()) return HMPC_E_ARG;  // nothing computed from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::CertificateOut b;
  const int rc = certificate_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, ls = n * h->setup.horizon * h->nc;
  if (grad) HIP_TRY(hipMemcpy(grad, b.grad, ls * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (lambda) HIP_TRY(hipMemcpy(lambda, b.lambda, ls * 10 * sizeof(double), hipMemcpyDeviceToHost));
  if (resid) HIP_TRY(hipMemcpy(resid, b.resid, ls * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, n * hmpc::CERT_CLASSES * sizeof(double), hipMemcpyDeviceToHost));
  if (where) HIP_TRY(hipMemcpy(where, b.where, n * hmpc::CERT_WHERE * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_certificate_penalty(hmpc_handle *h, const double ceil[3], const double *device_penalty_in, double *device_penalty_out, void *stream) {
  if (!h || !ceil || !device_penalty_out) return HMPC_E_ARG;
  if (!h->results.has_certificate()) return HMPC_E_ARG;  // no certificate of the last solve of this batch: the summary holds another solve's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::CertificateOut b;
  const int rc = certificate_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_certificate_penalty(b.summary, ceil, device_penalty_in, device_penalty_out, h->batch, (hipStream_t)stream));
  return HMPC_OK;
}

int hmpc_set_sweep_certificate_ceiling(hmpc_handle *h, const double ceil[3]) {
  if (!h) return HMPC_E_ARG;
  h->sweep_ceil_on = ceil != nullptr;
  for (int k = 0; k < hmpc::CERT_CEILS; ++k) h->sweep_ceil[k] = ceil ? ceil[k] : 0.0;
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Feedback gains: du_0/dx_0 and du_0/dX_d of the QP the last solve solved, and the first-order wrench from them (hmpc_feedback.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next gains go: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int gain_buffers(hmpc_handle *h, hmpc::FeedbackOut *b) {
  const size_t mb = (size_t)h->max_batch, u = 6 * (size_t)h->nc;
  HIP_TRY(h->d_fb_gain.ensure(mb * u * 13));
  HIP_TRY(h->d_fb_ref.ensure(mb * h->setup.horizon * u * 12));
  HIP_TRY(h->d_fb_summary.ensure(mb * hmpc::FB_SUMMARY));
  HIP_TRY(h->d_fb_free.ensure(mb * h->setup.horizon));
  *b = {h->d_fb_gain.get(), h->d_fb_ref.get(), h->d_fb_summary.get(), h->d_fb_free.get()};
  return HMPC_OK;
}

struct FirstOrderBuffers {
  float *wrench;
  double *worst;
};

static int first_order_buffers(hmpc_handle *h, FirstOrderBuffers *b) {
  const size_t mb = (size_t)h->max_batch;
  HIP_TRY(h->d_fo_wrench.ensure(mb * 6 * h->nc));
  HIP_TRY(h->d_fo_worst.ensure(mb));
  *b = {h->d_fo_wrench.get(), h->d_fo_worst.get()};
  return HMPC_OK;
}

int hmpc_set_device_gains(hmpc_handle *h, double *device_gain, double *device_ref_gain, double *device_summary, int32_t *device_free_dims) {
  if (!h) return HMPC_E_ARG;
  h->d_fb_gain.set_caller(device_gain), h->d_fb_ref.set_caller(device_ref_gain), h->d_fb_summary.set_caller(device_summary);
  h->d_fb_free.set_caller(device_free_dims);
  h->results.retarget_gains();
  return HMPC_OK;
}

int hmpc_get_device_gains(hmpc_handle *h, double **device_gain, double **device_ref_gain, double **device_summary, int32_t **device_free_dims) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::FeedbackOut b;
  const int rc = gain_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_gain) *device_gain = b.gain;
  if (device_ref_gain) *device_ref_gain = b.ref_gain;
  if (device_summary) *device_summary = b.summary;
  if (device_free_dims) *device_free_dims = b.free_dims;
  return HMPC_OK;
}

int hmpc_feedback_gains(hmpc_handle *h, void *stream) {
  if (!h || !h->results.has_solve()) return HMPC_E_ARG;  // no solve of the current batch: the force buffer holds another batch's forces, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::FeedbackOut b;
  const int rc = gain_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (no index list, no external QP data, relax 0: stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: friction shapes the constraint block)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_feedback(h->nc, a, h->cert_act_tol, b, (hipStream_t)stream));
  h->results.on_gains();
  return HMPC_OK;
}

int hmpc_download_gains(hmpc_handle *h, double *gain, double *ref_gain, double *summary, int32_t *free_dims) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_gains()) return HMPC_E_ARG;  // nothing computed from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::FeedbackOut b;
  const int rc = gain_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, u = 6 * (size_t)h->nc;
  if (gain) HIP_TRY(hipMemcpy(gain, b.gain, n * u * 13 * sizeof(double), hipMemcpyDeviceToHost));
  if (ref_gain) HIP_TRY(hipMemcpy(ref_gain, b.ref_gain, n * h->setup.horizon * u * 12 * sizeof(double), hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, n * hmpc::FB_SUMMARY * sizeof(double), hipMemcpyDeviceToHost));
  if (free_dims) HIP_TRY(hipMemcpy(free_dims, b.free_dims, n * h->setup.horizon * sizeof(int32_t), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_set_device_first_order(hmpc_handle *h, float *device_wrench, double *device_worst_slack) {
  if (!h) return HMPC_E_ARG;
  h->d_fo_wrench.set_caller(device_wrench), h->d_fo_worst.set_caller(device_worst_slack);
  h->results.retarget_first_order();
  return HMPC_OK;
}

int hmpc_first_order_wrench(hmpc_handle *h, const void *device_records_new, void *stream) {
  if (!h || !device_records_new || !h->results.has_gains()) return HMPC_E_ARG;  // no gains of the last solve of this batch: the buffers hold another solve's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::FeedbackOut g;
  int rc = gain_buffers(h, &g);
  if (rc != HMPC_OK) return rc;
  FirstOrderBuffers b;
  rc = first_order_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));
  set_problem_args(h, a);
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_first_order(h->nc, a, (const unsigned char *)device_records_new, g, b.wrench, b.worst, (hipStream_t)stream));
  h->results.on_first_order();
  return HMPC_OK;
}

int hmpc_download_first_order(hmpc_handle *h, float *wrench, double *worst_slack) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_first_order()) return HMPC_E_ARG;  // nothing computed from the gains of the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  FirstOrderBuffers b;
  const int rc = first_order_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch;
  if (wrench) HIP_TRY(hipMemcpy(wrench, b.wrench, n * 6 * h->nc * sizeof(float), hipMemcpyDeviceToHost));
  if (worst_slack) HIP_TRY(hipMemcpy(worst_slack, b.worst, n * sizeof(double), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Adjoint: the gradients of a loss over the force trajectory in the state, the reference, the weights and Alpha_K (hmpc_adjoint.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next adjoint goes: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int adjoint_buffers(hmpc_handle *h, hmpc::AdjointOut *b) {
  const size_t mb = (size_t)h->max_batch, u = 6 * (size_t)h->nc, hz = (size_t)h->setup.horizon;
  HIP_TRY(h->d_adj_x0.ensure(mb * 13));
  HIP_TRY(h->d_adj_traj.ensure(mb * hz * 12));
  HIP_TRY(h->d_adj_weights.ensure(mb * 12));
  HIP_TRY(h->d_adj_alpha.ensure(mb * u));
  HIP_TRY(h->d_adj_dir.ensure(mb * hz * u));
  HIP_TRY(h->d_adj_summary.ensure(mb * hmpc::ADJ_SUMMARY));
  *b = {h->d_adj_x0.get(), h->d_adj_traj.get(), h->d_adj_weights.get(), h->d_adj_alpha.get(), h->d_adj_dir.get(), h->d_adj_summary.get()};
  return HMPC_OK;
}

int hmpc_set_device_adjoint(hmpc_handle *h, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                            double *device_grad_alpha, double *device_dir, double *device_summary) {
  if (!h) return HMPC_E_ARG;
  h->d_adj_x0.set_caller(device_grad_x0), h->d_adj_traj.set_caller(device_grad_traj), h->d_adj_weights.set_caller(device_grad_weights);
  h->d_adj_alpha.set_caller(device_grad_alpha), h->d_adj_dir.set_caller(device_dir), h->d_adj_summary.set_caller(device_summary);
  h->results.retarget_adjoint();
  return HMPC_OK;
}

int hmpc_get_device_adjoint(hmpc_handle *h, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                            double **device_grad_alpha, double **device_dir, double **device_summary) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::AdjointOut b;
  const int rc = adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_grad_x0) *device_grad_x0 = b.grad_x0;
  if (device_grad_traj) *device_grad_traj = b.grad_traj;
  if (device_grad_weights) *device_grad_weights = b.grad_weights;
  if (device_grad_alpha) *device_grad_alpha = b.grad_alpha;
  if (device_dir) *device_dir = b.dir;
  if (device_summary) *device_summary = b.summary;
  return HMPC_OK;
}

int hmpc_solve_adjoint(hmpc_handle *h, const double *device_seed, void *stream) {
  if (!h || !device_seed || !h->results.has_solve()) return HMPC_E_ARG;  // no solve of the current batch: the force buffer holds another batch's forces, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::AdjointOut b;
  const int rc = adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (no index list, no external QP data, relax 0: stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: friction shapes the constraint block)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_adjoint(h->nc, a, h->cert_act_tol, device_seed, b, (hipStream_t)stream));
  h->results.on_adjoint();
  return HMPC_OK;
}

// doubles per instance of the six arrays of an adjoint, in the order of AdjointOut
static void adjoint_row_sizes(const hmpc_handle *h, size_t n[6]) {
  const size_t u = 6 * (size_t)h->nc, hz = (size_t)h->setup.horizon;
  n[0] = 13, n[1] = hz * 12, n[2] = 12, n[3] = u, n[4] = hz * u, n[5] = hmpc::ADJ_SUMMARY;
}

// slice 0 of where the multi-seed adjoint is or goes next: per array the caller's buffer, else the handle's own (NULL before the first
// launch reserved it)
static hmpc::AdjointOut adjoint_multi_base(const hmpc_handle *h) {
  double *p[6];
  for (int k = 0; k < 6; ++k) p[k] = h->adjm_caller[k] ? h->adjm_caller[k] : h->d_adjm_own[k].get();
  return {p[0], p[1], p[2], p[3], p[4], p[5]};
}

// where the CURRENT adjoint is -- the parent of the model, limit and record gradients and what hmpc_download_adjoint returns: the buffers
// of hmpc_solve_adjoint, or the slice of the multi-seed adjoint that hmpc_select_adjoint_seed chose (pointer arithmetic alone)
static int current_adjoint(hmpc_handle *h, hmpc::AdjointOut *b) {
  const int s = h->results.selected_adjoint_seed();
  if (s < 0) return adjoint_buffers(h, b);
  size_t n[6];
  adjoint_row_sizes(h, n);
  const hmpc::AdjointOut m = adjoint_multi_base(h);
  const size_t at = (size_t)s * (size_t)h->batch;
  *b = {m.grad_x0 + at * n[0], m.grad_traj + at * n[1], m.grad_weights + at * n[2], m.grad_alpha + at * n[3], m.dir + at * n[4], m.summary + at * n[5]};
  return HMPC_OK;
}

int hmpc_set_device_adjoint_multi(hmpc_handle *h, int n_seeds, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                                  double *device_grad_alpha, double *device_dir, double *device_summary) {
  if (!h) return HMPC_E_ARG;
  double *p[6] = {device_grad_x0, device_grad_traj, device_grad_weights, device_grad_alpha, device_dir, device_summary};
  bool any = false;
  for (int k = 0; k < 6; ++k) any = any || p[k];
  if (any && (n_seeds < 1 || n_seeds > HMPC_ADJOINT_MAX_SEEDS)) return HMPC_E_ARG;
  for (int k = 0; k < 6; ++k) h->adjm_caller[k] = p[k];
  h->adjm_caller_seeds = any ? n_seeds : 0;
  h->results.retarget_adjoint_multi();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_multi(hmpc_handle *h, int *n_seeds, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                                  double **device_grad_alpha, double **device_dir, double **device_summary) {
  if (!h) return HMPC_E_ARG;
  const hmpc::AdjointOut b = adjoint_multi_base(h);
  if (n_seeds) *n_seeds = h->results.adjoint_multi_seeds_enqueued();
  if (device_grad_x0) *device_grad_x0 = b.grad_x0;
  if (device_grad_traj) *device_grad_traj = b.grad_traj;
  if (device_grad_weights) *device_grad_weights = b.grad_weights;
  if (device_grad_alpha) *device_grad_alpha = b.grad_alpha;
  if (device_dir) *device_dir = b.dir;
  if (device_summary) *device_summary = b.summary;
  return HMPC_OK;
}

int hmpc_solve_adjoint_multi(hmpc_handle *h, const double *device_seeds, int n_seeds, void *stream) {
  if (!h || !device_seeds || n_seeds < 1 || n_seeds > HMPC_ADJOINT_MAX_SEEDS || !h->results.has_solve() || h->d_ext_Fc) return HMPC_E_ARG;
  bool caller = false, own = false;
  for (int k = 0; k < 6; ++k) (h->adjm_caller[k] ? caller : own) = true;
  if (caller && n_seeds > h->adjm_caller_seeds) return HMPC_E_ARG;  // the caller's buffers hold fewer slices
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (own) {  // the handle's own: room for (n_seeds, max_batch); an older, smaller allocation may still be read on any stream
    size_t n[6];
    adjoint_row_sizes(h, n);
    const bool grows = n_seeds > h->adjm_own_seeds;
    if (grows) h->results.retarget_adjoint_multi();  // (what the old buffers hold goes with them)
    for (int k = 0; k < 6; ++k)
      if (!h->adjm_caller[k]) HIP_TRY(h->d_adjm_own[k].reserve((size_t)n_seeds * (size_t)h->max_batch * n[k] * sizeof(double), (hipStream_t)stream, true));
    if (grows) h->adjm_own_seeds = n_seeds;
  }
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (as hmpc_solve_adjoint)
  set_problem_args(h, a);
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_adjoint_multi(h->nc, a, h->cert_act_tol, device_seeds, n_seeds, adjoint_multi_base(h), (hipStream_t)stream));
  h->results.on_adjoint_multi(n_seeds);
  return HMPC_OK;
}

int hmpc_select_adjoint_seed(hmpc_handle *h, int s) {
  if (!h || !h->results.has_adjoint_multi() || s < 0 || s >= h->results.adjoint_multi_seeds_enqueued()) return HMPC_E_ARG;
  h->results.on_select_adjoint(s);
  return HMPC_OK;
}

int hmpc_download_adjoint_multi(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, double *grad_alpha, double *dir,
                                double *summary) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_adjoint_multi()) return HMPC_E_ARG;  // nothing computed from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  const hmpc::AdjointOut b = adjoint_multi_base(h);
  size_t n[6];
  adjoint_row_sizes(h, n);
  const size_t rows = (size_t)h->results.adjoint_multi_seeds_enqueued() * (size_t)h->batch, d = sizeof(double);
  if (grad_x0) HIP_TRY(hipMemcpy(grad_x0, b.grad_x0, rows * n[0] * d, hipMemcpyDeviceToHost));
  if (grad_traj) HIP_TRY(hipMemcpy(grad_traj, b.grad_traj, rows * n[1] * d, hipMemcpyDeviceToHost));
  if (grad_weights) HIP_TRY(hipMemcpy(grad_weights, b.grad_weights, rows * n[2] * d, hipMemcpyDeviceToHost));
  if (grad_alpha) HIP_TRY(hipMemcpy(grad_alpha, b.grad_alpha, rows * n[3] * d, hipMemcpyDeviceToHost));
  if (dir) HIP_TRY(hipMemcpy(dir, b.dir, rows * n[4] * d, hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, rows * n[5] * d, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

int hmpc_download_adjoint(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, double *grad_alpha, double *dir,
                          double *summary) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_adjoint()) return HMPC_E_ARG;  // nothing computed from the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::AdjointOut b;
  const int rc = current_adjoint(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, u = 6 * (size_t)h->nc, hz = (size_t)h->setup.horizon, d = sizeof(double);
  if (grad_x0) HIP_TRY(hipMemcpy(grad_x0, b.grad_x0, n * 13 * d, hipMemcpyDeviceToHost));
  if (grad_traj) HIP_TRY(hipMemcpy(grad_traj, b.grad_traj, n * hz * 12 * d, hipMemcpyDeviceToHost));
  if (grad_weights) HIP_TRY(hipMemcpy(grad_weights, b.grad_weights, n * 12 * d, hipMemcpyDeviceToHost));
  if (grad_alpha) HIP_TRY(hipMemcpy(grad_alpha, b.grad_alpha, n * u * d, hipMemcpyDeviceToHost));
  if (dir) HIP_TRY(hipMemcpy(dir, b.dir, n * hz * u * d, hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, n * hmpc::ADJ_SUMMARY * d, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Model gradients: the gradients of the adjoint's loss in Acd, Bcd, the foot positions, the mass and the body inertia
// (hmpc_model_adjoint.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next model gradients go: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int model_adjoint_buffers(hmpc_handle *h, hmpc::ModelAdjointOut *b) {
  const size_t mb = (size_t)h->max_batch, u = 6 * (size_t)h->nc;
  HIP_TRY(h->d_madj_A.ensure(mb * 169));
  HIP_TRY(h->d_madj_B.ensure(mb * 13 * u));
  HIP_TRY(h->d_madj_r.ensure(mb * 3 * (size_t)h->nc));
  HIP_TRY(h->d_madj_params.ensure(mb * hmpc::MADJ_PARAMS));
  HIP_TRY(h->d_madj_costate.ensure(mb * hmpc::MADJ_COSTATE));
  *b = {h->d_madj_A.get(), h->d_madj_B.get(), h->d_madj_r.get(), h->d_madj_params.get(), h->d_madj_costate.get()};
  return HMPC_OK;
}

int hmpc_set_device_adjoint_model(hmpc_handle *h, double *device_grad_A, double *device_grad_B, double *device_grad_r,
                                  double *device_grad_params, double *device_costate) {
  if (!h) return HMPC_E_ARG;
  h->d_madj_A.set_caller(device_grad_A), h->d_madj_B.set_caller(device_grad_B), h->d_madj_r.set_caller(device_grad_r);
  h->d_madj_params.set_caller(device_grad_params), h->d_madj_costate.set_caller(device_costate);
  h->results.retarget_model_adjoint();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_model(hmpc_handle *h, double **device_grad_A, double **device_grad_B, double **device_grad_r,
                                  double **device_grad_params, double **device_costate) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::ModelAdjointOut b;
  const int rc = model_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_grad_A) *device_grad_A = b.grad_A;
  if (device_grad_B) *device_grad_B = b.grad_B;
  if (device_grad_r) *device_grad_r = b.grad_r;
  if (device_grad_params) *device_grad_params = b.grad_params;
  if (device_costate) *device_costate = b.costate;
  return HMPC_OK;
}

int hmpc_adjoint_model(hmpc_handle *h, void *stream) {
  if (!h || !h->results.has_adjoint()) return HMPC_E_ARG;  // no adjoint of the last solve of the current batch: dir is another seed's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::AdjointOut adj;
  int rc = current_adjoint(h, &adj);  // (where that adjoint went -- a single launch or a selected slice: moving them would have made it stale)
  if (rc != HMPC_OK) return rc;
  hmpc::ModelAdjointOut b;
  rc = model_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: the assembly is the solve's)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_model_adjoint(h->nc, a, (double)h->params.mass, adj.dir, b, (hipStream_t)stream));
  h->results.on_model_adjoint();
  return HMPC_OK;
}

int hmpc_download_adjoint_model(hmpc_handle *h, double *grad_A, double *grad_B, double *grad_r, double *grad_params, double *costate) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_model_adjoint()) return HMPC_E_ARG;  // nothing computed from the last adjoint of the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::ModelAdjointOut b;
  const int rc = model_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, u = 6 * (size_t)h->nc, d = sizeof(double);
  if (grad_A) HIP_TRY(hipMemcpy(grad_A, b.grad_A, n * 169 * d, hipMemcpyDeviceToHost));
  if (grad_B) HIP_TRY(hipMemcpy(grad_B, b.grad_B, n * 13 * u * d, hipMemcpyDeviceToHost));
  if (grad_r) HIP_TRY(hipMemcpy(grad_r, b.grad_r, n * 3 * (size_t)h->nc * d, hipMemcpyDeviceToHost));
  if (grad_params) HIP_TRY(hipMemcpy(grad_params, b.grad_params, n * hmpc::MADJ_PARAMS * d, hipMemcpyDeviceToHost));
  if (costate) HIP_TRY(hipMemcpy(costate, b.costate, n * hmpc::MADJ_COSTATE * d, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Limit gradients: the gradients of the adjoint's loss in the constraint block, the bounds and, through the assembly's rows, mu, lt, lh
// and the Fz caps (hmpc_limit_adjoint.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next limit gradients go: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int limit_adjoint_buffers(hmpc_handle *h, hmpc::LimitAdjointOut *b) {
  const size_t mb = (size_t)h->max_batch, nc = (size_t)h->nc, u = 6 * nc, ls = 10 * nc * (size_t)h->setup.horizon;
  HIP_TRY(h->d_ladj_limits.ensure(mb * (3 + nc)));
  HIP_TRY(h->d_ladj_Fc.ensure(mb * 8 * nc * u));
  HIP_TRY(h->d_ladj_bound.ensure(mb * ls));
  HIP_TRY(h->d_ladj_lambda.ensure(mb * ls));
  HIP_TRY(h->d_ladj_nu.ensure(mb * ls));
  HIP_TRY(h->d_ladj_summary.ensure(mb * hmpc::LADJ_SUMMARY));
  *b = {h->d_ladj_limits.get(), h->d_ladj_Fc.get(), h->d_ladj_bound.get(), h->d_ladj_lambda.get(), h->d_ladj_nu.get(), h->d_ladj_summary.get()};
  return HMPC_OK;
}

int hmpc_set_device_adjoint_limits(hmpc_handle *h, double *device_grad_limits, double *device_grad_Fc, double *device_grad_bound,
                                   double *device_lambda, double *device_nu, double *device_summary) {
  if (!h) return HMPC_E_ARG;
  h->d_ladj_limits.set_caller(device_grad_limits), h->d_ladj_Fc.set_caller(device_grad_Fc), h->d_ladj_bound.set_caller(device_grad_bound);
  h->d_ladj_lambda.set_caller(device_lambda), h->d_ladj_nu.set_caller(device_nu), h->d_ladj_summary.set_caller(device_summary);
  h->results.retarget_limit_adjoint();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_limits(hmpc_handle *h, double **device_grad_limits, double **device_grad_Fc, double **device_grad_bound,
                                   double **device_lambda, double **device_nu, double **device_summary) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::LimitAdjointOut b;
  const int rc = limit_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_grad_limits) *device_grad_limits = b.grad_limits;
  if (device_grad_Fc) *device_grad_Fc = b.grad_Fc;
  if (device_grad_bound) *device_grad_bound = b.grad_bound;
  if (device_lambda) *device_lambda = b.lambda;
  if (device_nu) *device_nu = b.nu;
  if (device_summary) *device_summary = b.summary;
  return HMPC_OK;
}

int hmpc_adjoint_limits(hmpc_handle *h, const double *device_seed, void *stream) {
  if (!h || !device_seed || !h->results.has_adjoint()) return HMPC_E_ARG;  // no adjoint of the last solve of the current batch: dir is another seed's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::AdjointOut adj;
  int rc = current_adjoint(h, &adj);  // (where that adjoint went -- a single launch or a selected slice: moving them would have made it stale)
  if (rc != HMPC_OK) return rc;
  hmpc::LimitAdjointOut b;
  rc = limit_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: the assembly is the solve's)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_limit_adjoint(h->nc, a, h->cert_act_tol, adj.dir, device_seed, b, (hipStream_t)stream));
  h->results.on_limit_adjoint();
  return HMPC_OK;
}

int hmpc_download_adjoint_limits(hmpc_handle *h, double *grad_limits, double *grad_Fc, double *grad_bound, double *lambda, double *nu,
                                 double *summary) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_limit_adjoint()) return HMPC_E_ARG;  // nothing computed from the last adjoint of the last solve of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::LimitAdjointOut b;
  const int rc = limit_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, nc = (size_t)h->nc, u = 6 * nc, ls = 10 * nc * (size_t)h->setup.horizon, d = sizeof(double);
  if (grad_limits) HIP_TRY(hipMemcpy(grad_limits, b.grad_limits, n * (3 + nc) * d, hipMemcpyDeviceToHost));
  if (grad_Fc) HIP_TRY(hipMemcpy(grad_Fc, b.grad_Fc, n * 8 * nc * u * d, hipMemcpyDeviceToHost));
  if (grad_bound) HIP_TRY(hipMemcpy(grad_bound, b.grad_bound, n * ls * d, hipMemcpyDeviceToHost));
  if (lambda) HIP_TRY(hipMemcpy(lambda, b.lambda, n * ls * d, hipMemcpyDeviceToHost));
  if (nu) HIP_TRY(hipMemcpy(nu, b.nu, n * ls * d, hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, b.summary, n * hmpc::LADJ_SUMMARY * d, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Record gradients: the gradient of the adjoint's loss in every float of the packed record, the quaternion and the joint angles through
// stage A1 + A2 included (hmpc_pose_adjoint.hip).
// ------------------------------------------------------------------------------------------------------------------
// where the next record gradients go: the caller's buffers, else the handle's own (allocated here, for max_batch, on first need)
static int record_adjoint_buffers(hmpc_handle *h, hmpc::PoseAdjointOut *b) {
  const size_t mb = (size_t)h->max_batch, nc = (size_t)h->nc;
  HIP_TRY(h->d_padj_record.ensure(mb * ((size_t)hmpc::rec_fixed_floats(h->nc) + 12 * (size_t)h->setup.horizon)));
  HIP_TRY(h->d_padj_frames.ensure(mb * (1 + nc) * 9));
  HIP_TRY(h->d_padj_rpy.ensure(mb * 3));
  *b = {h->d_padj_record.get(), h->d_padj_frames.get(), h->d_padj_rpy.get()};
  return HMPC_OK;
}

int hmpc_set_device_adjoint_record(hmpc_handle *h, double *device_grad_record, double *device_grad_frames, double *device_grad_rpy) {
  if (!h) return HMPC_E_ARG;
  h->d_padj_record.set_caller(device_grad_record), h->d_padj_frames.set_caller(device_grad_frames), h->d_padj_rpy.set_caller(device_grad_rpy);
  h->results.retarget_record_adjoint();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_record(hmpc_handle *h, double **device_grad_record, double **device_grad_frames, double **device_grad_rpy) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::PoseAdjointOut b;
  const int rc = record_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (device_grad_record) *device_grad_record = b.grad_record;
  if (device_grad_frames) *device_grad_frames = b.grad_frames;
  if (device_grad_rpy) *device_grad_rpy = b.grad_rpy;
  return HMPC_OK;
}

int hmpc_adjoint_record(hmpc_handle *h, void *stream) {
  // the three inputs: an adjoint of the last solve of the current batch, and model and limit gradients behind it; the chain goes through
  // the handle's own assembly, which an external constraint block is not
  if (!h || !h->results.can_record_adjoint() || h->d_ext_Fc) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hmpc::AdjointOut adj;
  int rc = current_adjoint(h, &adj);  // (where the three went: moving them would have made them stale)
  if (rc != HMPC_OK) return rc;
  hmpc::ModelAdjointOut mo;
  rc = model_adjoint_buffers(h, &mo);
  if (rc != HMPC_OK) return rc;
  hmpc::LimitAdjointOut lo;
  rc = limit_adjoint_buffers(h, &lo);
  if (rc != HMPC_OK) return rc;
  hmpc::PoseAdjointOut b;
  rc = record_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: the assembly is the solve's)
  const hmpc::PoseAdjointIn in = {adj.grad_x0, adj.grad_traj, adj.grad_weights, adj.grad_alpha, mo.grad_A, mo.grad_B, mo.grad_r, lo.grad_limits, lo.grad_Fc};
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_pose_adjoint(h->nc, a, in, b, (hipStream_t)stream));
  h->results.on_record_adjoint();
  return HMPC_OK;
}

int hmpc_download_adjoint_record(hmpc_handle *h, double *grad_record, double *grad_frames, double *grad_rpy) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_record_adjoint()) return HMPC_E_ARG;  // nothing computed from the last adjoint, model and limit gradients of this batch
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  hmpc::PoseAdjointOut b;
  const int rc = record_adjoint_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t n = (size_t)h->batch, nc = (size_t)h->nc, d = sizeof(double);
  const size_t nrec = (size_t)hmpc::rec_fixed_floats(h->nc) + 12 * (size_t)h->setup.horizon;
  if (grad_record) HIP_TRY(hipMemcpy(grad_record, b.grad_record, n * nrec * d, hipMemcpyDeviceToHost));
  if (grad_frames) HIP_TRY(hipMemcpy(grad_frames, b.grad_frames, n * (1 + nc) * 9 * d, hipMemcpyDeviceToHost));
  if (grad_rpy) HIP_TRY(hipMemcpy(grad_rpy, b.grad_rpy, n * 3 * d, hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Chain of the multi-seed adjoint: the model, limit and record gradients of every seed behind one assembly (hmpc_adjoint_chain.hip).
// ------------------------------------------------------------------------------------------------------------------
constexpr int CHAIN_ARRAYS = 14, CHAIN_COMPACT = 6;
static_assert(sizeof(hmpc_adjoint_chain) == CHAIN_ARRAYS * sizeof(double *), "struct hmpc_adjoint_chain is fourteen pointers, in the order of the rows below");

// doubles per instance of the fourteen arrays of a chain, in the member order of struct hmpc_adjoint_chain
static void chain_row_sizes(const hmpc_handle *h, size_t n[CHAIN_ARRAYS]) {
  const size_t nc = (size_t)h->nc, u = 6 * nc, hz = (size_t)h->setup.horizon, ls = 10 * nc * hz;
  const size_t rows[CHAIN_ARRAYS] = {(size_t)hmpc::rec_fixed_floats(h->nc) + 12 * hz, (1 + nc) * 9, 3, hmpc::MADJ_PARAMS, 3 + nc, hmpc::LADJ_SUMMARY,
                                     169, 13 * u, 3 * nc, hmpc::MADJ_COSTATE, 8 * nc * u, ls, ls, ls};
  for (int k = 0; k < CHAIN_ARRAYS; ++k) n[k] = rows[k];
}

// slice 0 of where the chain is or goes next: per compact array the caller's buffer, else the handle's own (NULL before the first launch
// reserved it); per detail array the caller's buffer, else NULL (not written)
static void chain_base(const hmpc_handle *h, double *p[CHAIN_ARRAYS]) {
  for (int k = 0; k < CHAIN_ARRAYS; ++k) p[k] = h->chain_caller[k] ? h->chain_caller[k] : (k < CHAIN_COMPACT ? h->d_chain_own[k].get() : nullptr);
}

int hmpc_set_device_adjoint_chain_multi(hmpc_handle *h, int n_seeds, const struct hmpc_adjoint_chain *device_buffers) {
  if (!h) return HMPC_E_ARG;
  double *p[CHAIN_ARRAYS] = {};
  if (device_buffers) memcpy(p, device_buffers, sizeof(p));
  bool any = false;
  for (int k = 0; k < CHAIN_ARRAYS; ++k) any = any || p[k];
  if (any && (n_seeds < 1 || n_seeds > HMPC_ADJOINT_MAX_SEEDS)) return HMPC_E_ARG;
  for (int k = 0; k < CHAIN_ARRAYS; ++k) h->chain_caller[k] = p[k];
  h->chain_caller_seeds = any ? n_seeds : 0;
  h->results.retarget_adjoint_chain();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_chain_multi(hmpc_handle *h, int *n_seeds, struct hmpc_adjoint_chain *device_buffers) {
  if (!h) return HMPC_E_ARG;
  if (n_seeds) *n_seeds = h->results.has_adjoint_chain() ? h->results.adjoint_multi_seeds_enqueued() : 0;
  if (device_buffers) {
    double *p[CHAIN_ARRAYS];
    chain_base(h, p);
    memcpy(device_buffers, p, sizeof(p));
  }
  return HMPC_OK;
}

int hmpc_adjoint_chain_multi(hmpc_handle *h, const double *device_seeds, void *stream) {
  // the chain goes through the handle's own assembly, which an external constraint block is not
  if (!h || !device_seeds || !h->results.has_adjoint_multi() || h->d_ext_Fc) return HMPC_E_ARG;
  const int n_seeds = h->results.adjoint_multi_seeds_enqueued();
  bool caller = false, own = false;
  for (int k = 0; k < CHAIN_ARRAYS; ++k)
    if (h->chain_caller[k]) caller = true;
    else if (k < CHAIN_COMPACT) own = true;
  if (caller && n_seeds > h->chain_caller_seeds) return HMPC_E_ARG;  // the caller's buffers hold fewer slices
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  size_t n[CHAIN_ARRAYS];
  chain_row_sizes(h, n);
  if (own) {  // the handle's own: room for (n_seeds, max_batch); an older, smaller allocation may still be read on any stream
    const bool grows = n_seeds > h->chain_own_seeds;
    if (grows) h->results.retarget_adjoint_chain();  // (what the old buffers hold goes with them)
    for (int k = 0; k < CHAIN_COMPACT; ++k)
      if (!h->chain_caller[k]) HIP_TRY(h->d_chain_own[k].reserve((size_t)n_seeds * (size_t)h->max_batch * n[k] * sizeof(double), (hipStream_t)stream, true));
    if (grows) h->chain_own_seeds = n_seeds;
  }
  const hmpc::AdjointOut m = adjoint_multi_base(h);  // (where that adjoint went: moving it would have made it stale)
  const hmpc::AdjointChainIn in = {device_seeds, m.dir, m.grad_x0, m.grad_traj, m.grad_weights, m.grad_alpha};
  double *p[CHAIN_ARRAYS];
  chain_base(h, p);
  const hmpc::AdjointChainOut out = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13]};
  hmpc::KernelArgs a;
  memset(&a, 0, sizeof(a));  // (stage A as an ordinary solve runs it -- the handle's own assembly)
  set_problem_args(h, a);    // (mu_inst stays: the assembly is the solve's)
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_adjoint_chain(h->nc, a, h->cert_act_tol, (double)h->params.mass, in, n_seeds, out, (hipStream_t)stream));
  for (int k = 0; k < CHAIN_ARRAYS; ++k) h->chain_written[k] = p[k] != nullptr;
  h->results.on_adjoint_chain();
  return HMPC_OK;
}

int hmpc_download_adjoint_chain_multi(hmpc_handle *h, const struct hmpc_adjoint_chain *host_buffers) {
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  if (!h->results.has_adjoint_chain()) return HMPC_E_ARG;  // nothing computed from the multi-seed adjoint that stands
  double *dst[CHAIN_ARRAYS] = {};
  if (host_buffers) memcpy(dst, host_buffers, sizeof(dst));
  for (int k = 0; k < CHAIN_ARRAYS; ++k)
    if (dst[k] && !h->chain_written[k]) return HMPC_E_ARG;  // a detail array that was not written
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  double *src[CHAIN_ARRAYS];
  chain_base(h, src);
  size_t n[CHAIN_ARRAYS];
  chain_row_sizes(h, n);
  const size_t rows = (size_t)h->results.adjoint_multi_seeds_enqueued() * (size_t)h->batch;
  for (int k = 0; k < CHAIN_ARRAYS; ++k)
    if (dst[k]) HIP_TRY(hipMemcpy(dst[k], src[k], rows * n[k] * sizeof(double), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Selection: the best command of every sweep group, from the last solve's status and forces and the last prediction (hmpc_select.hip).
// ------------------------------------------------------------------------------------------------------------------
struct SelectionBuffers {
  int32_t *index;
  double *score;
  float *forces;
  uint32_t *status;
  float *states;
};

// where the next selection goes: the caller's buffers, else the handle's own (allocated here, for max_batch groups, on first need)
static int selection_buffers(hmpc_handle *h, SelectionBuffers *b) {
  const size_t mb = (size_t)h->max_batch, hz = (size_t)h->setup.horizon;
  HIP_TRY(h->d_sel_index.ensure(mb));
  HIP_TRY(h->d_sel_score.ensure(mb));
  HIP_TRY(h->d_sel_forces.ensure(mb * 6 * h->nc * hz));
  HIP_TRY(h->d_sel_status.ensure(mb));
  HIP_TRY(h->d_sel_states.ensure(mb * hz * 13));
  *b = {h->d_sel_index.get(), h->d_sel_score.get(), h->d_sel_forces.get(), h->d_sel_status.get(), h->d_sel_states.get()};
  return HMPC_OK;
}

int hmpc_set_device_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states) {
  if (!h) return HMPC_E_ARG;
  h->d_sel_index.set_caller(index), h->d_sel_score.set_caller(score), h->d_sel_forces.set_caller(forces);
  h->d_sel_status.set_caller(status), h->d_sel_states.set_caller(states);
  h->results.retarget_selection();
  return HMPC_OK;
}

int hmpc_get_device_selection(hmpc_handle *h, int32_t **index, double **score, float **forces, uint32_t **status, float **states,
                              int *n_groups) {
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  SelectionBuffers b;
  const int rc = selection_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  if (index) *index = b.index;
  if (score) *score = b.score;
  if (forces) *forces = b.forces;
  if (status) *status = b.status;
  if (states) *states = b.states;
  if (n_groups) *n_groups = h->results.selected_groups();
  return HMPC_OK;
}

int hmpc_sweep_select(hmpc_handle *h, int group_size, const double *device_penalty, void *stream) {
  if (!h || group_size < 1) return HMPC_E_ARG;
  if (h->batch % group_size != 0) return HMPC_E_ARG;
  if (!h->results.has_prediction()) return HMPC_E_ARG;  // no prediction from the last solve of this batch: the cost buffer holds another solve's, or none
  HIP_TRY(hipSetDevice(h->device));
  float *ps = nullptr;
  double *pc = nullptr;
  int rc = prediction_buffers(h, &ps, &pc);
  if (rc != HMPC_OK) return rc;
  SelectionBuffers b;
  rc = selection_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  hmpc::SelectArgs a;
  a.cost = pc, a.states = ps, a.status = h->d_status.get(), a.forces = h->d_forces.get(), a.penalty = device_penalty;
  a.groups = h->batch / group_size, a.group_size = group_size;
  a.force_words = 6 * h->nc * h->setup.horizon, a.state_words = 13 * h->setup.horizon;
  a.index = b.index, a.score = b.score, a.out_forces = b.forces, a.out_status = b.status, a.out_states = b.states;
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_select(a, (hipStream_t)stream));
  h->results.on_select(a.groups);
  return HMPC_OK;
}

int hmpc_download_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states) {
  if (!h || !h->results.has_selection()) return HMPC_E_ARG;  // nothing selected from the last prediction
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));
  SelectionBuffers b;
  const int rc = selection_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  const size_t g = (size_t)h->results.selected_groups(), hz = (size_t)h->setup.horizon;
  if (index) HIP_TRY(hipMemcpy(index, b.index, g * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (score) HIP_TRY(hipMemcpy(score, b.score, g * sizeof(double), hipMemcpyDeviceToHost));
  if (forces) HIP_TRY(hipMemcpy(forces, b.forces, g * 6 * h->nc * hz * sizeof(float), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, b.status, g * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (states) HIP_TRY(hipMemcpy(states, b.states, g * hz * 13 * sizeof(float), hipMemcpyDeviceToHost));
  return HMPC_OK;
}

// One planning tick without leaving the device: n_ticks robot states x group_size candidate commands -> records -> sweep solve ->
// prediction -> selection -> the joint torques of every state's best command.  Every stage is the entry point of its own name; new here
// are the expansion of ticks x commands (hmpc_select.hip) and the torque launch over the compact winner rows.
int hmpc_tick_sweep_device(hmpc_handle *h, const void *device_ticks, int n_ticks, const struct hmpc_command *device_commands,
                           int group_size, double dtMPC, const double *device_penalty, double *device_wpd_out, double *device_f_ff,
                           double *device_tau, void *stream) {
  if (!h || !device_ticks || !device_commands || !device_tau || n_ticks < 0 || group_size < 1) return HMPC_E_ARG;
  if (h->nc != 2 || h->setup.horizon > 10) return HMPC_E_ARG;  // (the sweep's limits)
  if ((long long)n_ticks * group_size > h->max_batch) return HMPC_E_BATCH;
  const int batch = n_ticks * group_size;
  if (batch == 0) return hmpc_build_records_device(h, device_ticks, 0, dtMPC, nullptr, stream);
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(enter_stream(h, (hipStream_t)stream));  // (the expansion writes the shared scratch)
  void *sp = nullptr;
  int rc = scratch(h, sizeof(hmpc_tick_inputs) * (size_t)batch, &sp);
  if (rc != HMPC_OK) return rc;
  HIP_TRY(hmpc::launch_expand_ticks((const hmpc_tick_inputs *)device_ticks, n_ticks, device_commands, group_size, (hmpc_tick_inputs *)sp,
                                    device_wpd_out, (hipStream_t)stream));
  rc = hmpc_build_records_device(h, sp, batch, dtMPC, nullptr, stream);
  if (rc == HMPC_OK) rc = hmpc_solve_command_sweep(h, group_size, stream);
  if (rc == HMPC_OK) rc = hmpc_predict_states(h, stream);
  if (rc == HMPC_OK && h->sweep_floor_on) {  // commands whose margins miss the floor are masked: margins, then the penalty into scratch of the handle
    HIP_TRY(h->d_sweep_penalty.reserve((size_t)h->max_batch * sizeof(double), (hipStream_t)stream, /*whole_device=*/true));
    rc = hmpc_constraint_margins(h, stream);
    if (rc == HMPC_OK) rc = hmpc_margin_penalty(h, h->sweep_floor, device_penalty, h->d_sweep_penalty.get(), stream);
    device_penalty = h->d_sweep_penalty.get();
  }
  if (rc == HMPC_OK && h->sweep_ceil_on) {  // ... and those whose certificate exceeds the ceiling: behind the margin penalty, through the same scratch (in place)
    HIP_TRY(h->d_sweep_penalty.reserve((size_t)h->max_batch * sizeof(double), (hipStream_t)stream, /*whole_device=*/true));
    rc = hmpc_kkt_certificate(h, stream);
    if (rc == HMPC_OK) rc = hmpc_certificate_penalty(h, h->sweep_ceil, device_penalty, h->d_sweep_penalty.get(), stream);
    device_penalty = h->d_sweep_penalty.get();
  }
  if (rc == HMPC_OK) rc = hmpc_sweep_select(h, group_size, device_penalty, stream);
  if (rc != HMPC_OK) return rc;
  SelectionBuffers b;
  rc = selection_buffers(h, &b);
  if (rc != HMPC_OK) return rc;
  HIP_TRY(hmpc::launch_leg_torques(b.forces, n_ticks, h->setup.horizon, /*rBody=*/nullptr, /*leg_q=*/nullptr, device_f_ff, device_tau,
                                   (const hmpc_tick_inputs *)device_ticks, (hipStream_t)stream));
  return HMPC_OK;
}

}  // extern "C"
