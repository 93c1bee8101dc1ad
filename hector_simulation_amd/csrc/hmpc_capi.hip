// hmpc_capi.hip -- the batched C ABI of include/hector_mpc.h over the gfx950 kernels: handles, batches, settings, solves, downloads, the
// debug hooks, the caller-side rows f1-f3 and the device-resident tick.  What a solve launches is hmpc_launch.hip's; the results derived
// from a solve (prediction ... the chain, and the planning tick over them) are hmpc_results.hip's; the reference's own process-global
// interface is hmpc_legacy.hip's.
// There is NO CPU fallback: without a gfx950 device every entry point fails (HMPC_E_NO_DEVICE).
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <utility>
#include <vector>

#include "hmpc_builder_launch.h"
#include "hmpc_front.h"
#include "hmpc_handle.h"
#include "hmpc_record.h"

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

int hmpc_debug_set_front_prologue(hmpc_handle *h, int on) {
  if (!h) return HMPC_E_ARG;
  h->front_prologue = on ? 1 : 0;  // (read at the head of the next fast pass: nothing enqueued depends on it)
  return HMPC_OK;
}

int hmpc_debug_front_scalars(hmpc_handle *h, void *out) {
  if (!h || !out || h->nc != 2) return HMPC_E_ARG;
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const int vi = fast_variant(/*long_h=*/h->setup.horizon > 10, /*size=*/1, /*sweep=*/false);  // (a variant that reads the blocks, whatever the batch's own is)
  const int was = h->front_prologue;
  h->front_prologue = 1;
  bool ready = false;
  const int rc = enqueue_front(h, h->last_stream, &vi, 1, &ready);
  h->front_prologue = was;
  if (rc != HMPC_OK) return rc;
  if (!ready) return HMPC_E_ARG;
  RC_TRY(settle(h));
  HIP_TRY(hipMemcpy(out, h->d_front.get(), (size_t)h->batch * sizeof(hmpc::FrontScalars), hipMemcpyDeviceToHost));
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
  int rc;
  if (h->device_repair) {
    rc = enqueue_solve(h, h->last_stream, false);
  } else {  // (one launch of the batch's variant behind the prologue a solve puts in front of it: the product path)
    const int vi = pick_variant(h);
    LaunchOpt po;
    rc = enqueue_front(h, h->last_stream, &vi, 1, &po.front_ready);
    if (rc == HMPC_OK) rc = launch(h, h->last_stream, vi, po);
  }
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

}  // extern "C"
