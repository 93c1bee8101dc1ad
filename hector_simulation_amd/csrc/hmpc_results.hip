// hmpc_results.hip -- the results derived from a solve, over the batched C ABI of include/hector_mpc.h: prediction, selection, margins,
// certificate, gains, first-order wrench, adjoint, multi-seed adjoint, model, limit and record gradients, the chain, and the planning tick
// that strings them together (hmpc_tick_sweep_device).  What every family's arrays are and how large is hmpc_results.h's table; where
// they go, what guards them and how they are copied is written once, in the functions at the head of this unit, and every extern "C"
// entry below gathers its arguments and calls them.  The kernels are their own units' (hmpc_predict.hip ... hmpc_adjoint_chain.hip).
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "hmpc_builder_launch.h"
#include "hmpc_handle.h"
#include "hmpc_predict.h"
#include "hmpc_select.h"

using hmpc::FAMILIES;
using hmpc::KernelArgs;

// the table's literals are the kernels' constants
static_assert(hmpc::MARGIN_ROWS[1].row(2, 1) == hmpc::MARGIN_CLASSES && hmpc::MARGIN_ROWS[2].row(2, 1) == hmpc::MARGIN_CLASSES, "margins: summary, where");
static_assert(hmpc::CERTIFICATE_ROWS[3].row(2, 1) == hmpc::CERT_CLASSES && hmpc::CERTIFICATE_ROWS[4].row(2, 1) == hmpc::CERT_WHERE, "certificate: summary, where");
static_assert(hmpc::GAIN_ROWS[2].row(2, 1) == hmpc::FB_SUMMARY && hmpc::ADJOINT_ROWS[5].row(2, 1) == hmpc::ADJ_SUMMARY, "gains, adjoint: summary");
static_assert(hmpc::MODEL_ROWS[3].row(2, 1) == hmpc::MADJ_PARAMS && hmpc::MODEL_ROWS[4].row(2, 1) == hmpc::MADJ_COSTATE, "model gradients: grad_params, costate");
static_assert(hmpc::LIMIT_ROWS[5].row(2, 1) == hmpc::LADJ_SUMMARY, "limit gradients: summary");
static_assert(sizeof(hmpc_adjoint_chain) == hmpc::CHAIN_ARRAYS * sizeof(double *), "struct hmpc_adjoint_chain is the pointers of CHAIN_ROWS, in their order");

// the families without an *Out struct of their kernel's: their arrays as the launchers take them
struct PredictionBuffers {
  float *states;
  double *cost;
};
struct MarginBuffers {
  double *slack, *summary;
  int32_t *where;
};
struct FirstOrderBuffers {
  float *wrench;
  double *worst;
};
struct SelectionBuffers {
  int32_t *index;
  double *score;
  float *forces;
  uint32_t *status;
  float *states;
};

// an all-pointer struct from the pointers of family F, in the table's order
template <int F, class Out>
static Out as(void *const p[]) {
  static_assert(sizeof(Out) == FAMILIES[F].n * sizeof(void *), "the struct is the pointers of the family's arrays, in the order of the table");
  Out o;
  memcpy(&o, p, sizeof(o));
  return o;
}

static int hip_failed(const char *what, const hmpc::ResultFamily &fam, const char *array, hipError_t e) {
  hip_error_text() = std::string(what) + " (" + fam.name + (array ? "." : "") + (array ? array : "") + "): " + hipGetErrorString(e);
  return HMPC_E_HIP;
}

// ---------------------------------------------------------------------------------------------------- the four generic functions
// ensure: where the next result of family f goes -- per array the caller's buffer, else the handle's own, allocated here for max_batch rows
// on first need.  (An own buffer never grows: a call may ensure before it enters its stream.)
static int ensure(hmpc_handle *h, int f, void *p[]) {
  const hmpc::ResultFamily &fam = FAMILIES[f];
  for (int k = 0; k < fam.n; ++k) {
    const hipError_t e = h->d_result[f][k].ensure(hmpc::array_bytes(fam, k, h->nc, h->setup.horizon, (size_t)h->max_batch));
    if (e != hipSuccess) return hip_failed("hipMalloc", fam, fam.arrays[k].name, e);
    p[k] = h->d_result[f][k].get();
  }
  return HMPC_OK;
}

// set: the caller's buffers for family F (NULL = the handle's own); whatever was computed went elsewhere
template <int F, class... T>
static int set_family(hmpc_handle *h, T *...caller) {
  static_assert(sizeof...(T) == FAMILIES[F].n, "one pointer per array of the family");
  if (!h) return HMPC_E_ARG;
  void *const p[] = {caller...};
  for (int k = 0; k < FAMILIES[F].n; ++k) h->d_result[F][k].set_caller((unsigned char *)p[k]);
  h->results.retarget(FAMILIES[F].node);
  return HMPC_OK;
}

// get: ensure, then where the arrays are, into every `out` that is not NULL
template <int F, class... T>
static int get_family(hmpc_handle *h, T **...out) {
  static_assert(sizeof...(T) == FAMILIES[F].n, "one pointer per array of the family");
  if (!h) return HMPC_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  void *p[hmpc::MAX_SINGLE_ARRAYS];
  RC_TRY(ensure(h, F, p));
  int k = 0;
  ((out ? (void)(*out = (T *)p[k]) : (void)0, ++k), ...);
  return HMPC_OK;
}

// slice 0 of where the multi-seed adjoint is or goes next: per array the caller's buffer, else the handle's own (NULL before the first
// launch reserved it)
static void adjoint_multi_base(const hmpc_handle *h, void *p[]) {
  for (int k = 0; k < hmpc::ADJOINT_ARRAYS; ++k) p[k] = h->adjm_caller[k] ? h->adjm_caller[k] : h->d_adjm_own[k].get();
}

// slice 0 of where the chain is or goes next: per compact array the caller's buffer, else the handle's own (NULL before the first launch
// reserved it); per detail array the caller's buffer, else NULL (not written)
static void chain_base(const hmpc_handle *h, void *p[]) {
  for (int k = 0; k < hmpc::CHAIN_ARRAYS; ++k) p[k] = h->chain_caller[k] ? h->chain_caller[k] : (k < hmpc::CHAIN_COMPACT ? h->d_chain_own[k].get() : nullptr);
}

// where the CURRENT adjoint is -- the parent of the model, limit and record gradients and what hmpc_download_adjoint returns: the buffers
// of hmpc_solve_adjoint (which allocated them), or the slice of the multi-seed adjoint that hmpc_select_adjoint_seed chose (pointer
// arithmetic alone)
static hmpc::AdjointOut current_adjoint(const hmpc_handle *h) {
  void *p[hmpc::ADJOINT_ARRAYS];
  const int s = h->results.selected_adjoint_seed();
  if (s < 0)
    for (int k = 0; k < hmpc::ADJOINT_ARRAYS; ++k) p[k] = h->d_result[hmpc::F_ADJOINT][k].get();
  else {
    adjoint_multi_base(h, p);
    for (int k = 0; k < hmpc::ADJOINT_ARRAYS; ++k)
      p[k] = (unsigned char *)p[k] + hmpc::array_bytes(FAMILIES[hmpc::F_ADJOINT], k, h->nc, h->setup.horizon, (size_t)s * (size_t)h->batch);
  }
  return as<hmpc::F_ADJOINT, hmpc::AdjointOut>(p);
}

// download: the guards in their order, the wait, then one copy per destination that is not NULL, of the rows that stand at the table's
// size.  (The selection has one row per group and no batch == 0 shortcut: it answers HMPC_E_ARG where nothing was selected.)
static int download(hmpc_handle *h, int f, void *const dst[]) {
  const hmpc::ResultFamily &fam = FAMILIES[f];
  if (!h) return HMPC_E_ARG;
  if (h->batch == 0 && f != hmpc::F_SELECTION) return HMPC_OK;
  if (f == hmpc::F_ADJOINT_CHAIN ? !h->results.has_adjoint_chain() : !h->results.has(fam.node)) return HMPC_E_ARG;  // nothing computed from what stands
  if (f == hmpc::F_ADJOINT_CHAIN)
    for (int k = 0; k < fam.n; ++k)
      if (dst[k] && !h->chain_written[k]) return HMPC_E_ARG;  // a detail array that was not written
  HIP_TRY(hipSetDevice(h->device));
  RC_TRY(settle(h));  // the stream rule: before any host copy
  void *src[hmpc::MAX_ARRAYS];
  size_t rows = (size_t)h->batch;
  if (f == hmpc::F_ADJOINT) {
    const hmpc::AdjointOut a = current_adjoint(h);
    memcpy(src, &a, sizeof(a));
  } else if (f == hmpc::F_ADJOINT_MULTI || f == hmpc::F_ADJOINT_CHAIN) {
    f == hmpc::F_ADJOINT_MULTI ? adjoint_multi_base(h, src) : chain_base(h, src);
    rows *= (size_t)h->results.adjoint_multi_seeds_enqueued();
  } else {
    RC_TRY(ensure(h, f, src));
    if (f == hmpc::F_SELECTION) rows = (size_t)h->results.selected_groups();
  }
  for (int k = 0; k < fam.n; ++k)
    if (dst[k]) {
      const hipError_t e = hipMemcpy(dst[k], src[k], hmpc::array_bytes(fam, k, h->nc, h->setup.horizon, rows), hipMemcpyDeviceToHost);
      if (e != hipSuccess) return hip_failed("hipMemcpy", fam, fam.arrays[k].name, e);
    }
  return HMPC_OK;
}
template <int F, class... T>
static int download_family(hmpc_handle *h, T *...dst) {
  static_assert(sizeof...(T) == FAMILIES[F].n, "one pointer per array of the family");
  void *const p[] = {dst...};
  return download(h, F, p);
}

// What stage A of a derived kernel reads: no index list, no external QP data, relax 0 -- the handle's own assembly, as an ordinary solve
// runs it.  (mu_inst stays: friction shapes the constraint block.)
static KernelArgs problem_args(const hmpc_handle *h) {
  KernelArgs a;
  memset(&a, 0, sizeof(a));
  set_problem_args(h, a);
  return a;
}

// The launch of family f behind `parent`, in the order every such entry keeps: the guards (ok = the entry's own arguments), batch == 0,
// the device, ensure, the kernel's arguments, enter_stream (the stream rule: before the launch), launch(a, p) -- the family's kernel on
// the arrays p -- and the family's node.
template <class Launch>
static int enqueue_family(hmpc_handle *h, int f, ResultNode parent, bool ok, void *stream, Launch launch) {
  if (!h || !ok || !h->results.has(parent)) return HMPC_E_ARG;  // nothing of the current batch's last solve to compute it from
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  void *p[hmpc::MAX_SINGLE_ARRAYS];
  RC_TRY(ensure(h, f, p));
  KernelArgs a = problem_args(h);
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  const hipError_t e = launch(a, p);
  if (e != hipSuccess) return hip_failed("launch", FAMILIES[f], nullptr, e);
  h->results.set(FAMILIES[f].node);
  return HMPC_OK;
}

// The handle's own buffers of a per-seed family (its first n_own arrays, where the caller gave none): room for (n_seeds, max_batch).  An
// older, smaller allocation may still be read on any stream, so growing waits for the whole device; what the old buffers hold goes with them.
static int reserve_seed_slices(hmpc_handle *h, int f, DeviceBuffer<double> own[], double *const caller[], int n_own, int n_seeds, int *own_seeds, void *stream) {
  const bool grows = n_seeds > *own_seeds;
  if (grows) f == hmpc::F_ADJOINT_MULTI ? h->results.retarget_adjoint_multi() : h->results.retarget_adjoint_chain();
  for (int k = 0; k < n_own; ++k)
    if (!caller[k]) {
      const size_t bytes = hmpc::array_bytes(FAMILIES[f], k, h->nc, h->setup.horizon, (size_t)n_seeds * (size_t)h->max_batch);
      const hipError_t e = own[k].reserve(bytes, (hipStream_t)stream, /*whole_device=*/true);
      if (e != hipSuccess) return hip_failed("reserve", FAMILIES[f], FAMILIES[f].arrays[k].name, e);
    }
  if (grows) *own_seeds = n_seeds;
  return HMPC_OK;
}

// the caller's buffers of a per-seed family: all NULL = the handle's own, else room for n_seeds slices
static int set_seed_slices(double *caller[], int *caller_seeds, int n, int n_seeds, double *const p[]) {
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || p[k];
  if (any && (n_seeds < 1 || n_seeds > HMPC_ADJOINT_MAX_SEEDS)) return HMPC_E_ARG;
  for (int k = 0; k < n; ++k) caller[k] = p[k];
  *caller_seeds = any ? n_seeds : 0;
  return HMPC_OK;
}

// out[i] from the summary of family f (margins or certificate) by `rule`: no kernel arguments, no node of its own
template <class Rule>
static int enqueue_penalty(hmpc_handle *h, int f, bool ok, void *stream, Rule rule) {
  if (!h || !ok) return HMPC_E_ARG;
  if (!h->results.has(FAMILIES[f].node)) return HMPC_E_ARG;  // the summary holds another solve's, or none
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  void *p[hmpc::MAX_SINGLE_ARRAYS];
  RC_TRY(ensure(h, f, p));
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  const hipError_t e = rule(p);
  if (e != hipSuccess) return hip_failed("penalty launch", FAMILIES[f], nullptr, e);
  return HMPC_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------------- prediction (hmpc_predict.hip)
int hmpc_set_device_prediction(hmpc_handle *h, float *device_states, double *device_cost) {
  return set_family<hmpc::F_PREDICTION>(h, device_states, device_cost);
}

int hmpc_get_device_prediction(hmpc_handle *h, float **device_states, double **device_cost) {
  return get_family<hmpc::F_PREDICTION>(h, device_states, device_cost);
}

int hmpc_predict_states(hmpc_handle *h, void *stream) {
  return enqueue_family(h, hmpc::F_PREDICTION, ResultNode::SOLVE, true, stream, [&](KernelArgs &a, void *const p[]) {
    a.mu_inst = nullptr;  // (friction shapes the constraint block only; the model does not depend on it)
    const PredictionBuffers b = as<hmpc::F_PREDICTION, PredictionBuffers>(p);
    return hmpc::launch_predict(h->nc, a, b.states, b.cost, (hipStream_t)stream);
  });
}

int hmpc_download_prediction(hmpc_handle *h, float *states, double *cost) { return download_family<hmpc::F_PREDICTION>(h, states, cost); }

// ---------------------------------------------------------------------------------------------------- constraint margins (hmpc_margins.hip)
int hmpc_set_device_margins(hmpc_handle *h, double *device_slack, double *device_summary, int32_t *device_where) {
  return set_family<hmpc::F_MARGINS>(h, device_slack, device_summary, device_where);
}

int hmpc_get_device_margins(hmpc_handle *h, double **device_slack, double **device_summary, int32_t **device_where) {
  return get_family<hmpc::F_MARGINS>(h, device_slack, device_summary, device_where);
}

int hmpc_constraint_margins(hmpc_handle *h, void *stream) {
  return enqueue_family(h, hmpc::F_MARGINS, ResultNode::SOLVE, true, stream, [&](KernelArgs &a, void *const p[]) {
    const MarginBuffers b = as<hmpc::F_MARGINS, MarginBuffers>(p);
    return hmpc::launch_margins(h->nc, a, b.slack, b.summary, b.where, (hipStream_t)stream);
  });
}

int hmpc_download_margins(hmpc_handle *h, double *slack, double *summary, int32_t *where) {
  return download_family<hmpc::F_MARGINS>(h, slack, summary, where);
}

int hmpc_margin_penalty(hmpc_handle *h, const double floor[6], const double *device_penalty_in, double *device_penalty_out, void *stream) {
  return enqueue_penalty(h, hmpc::F_MARGINS, floor && device_penalty_out, stream, [&](void *const p[]) {
    return hmpc::launch_margin_penalty(as<hmpc::F_MARGINS, MarginBuffers>(p).summary, floor, device_penalty_in, device_penalty_out, h->batch, (hipStream_t)stream);
  });
}

int hmpc_set_sweep_margin_floor(hmpc_handle *h, const double floor[6]) {
  if (!h) return HMPC_E_ARG;
  h->sweep_floor_on = floor != nullptr;
  for (int k = 0; k < hmpc::MARGIN_CLASSES; ++k) h->sweep_floor[k] = floor ? floor[k] : 0.0;
  return HMPC_OK;
}

// ---------------------------------------------------------------------------------------------------- KKT certificate (hmpc_certificate.hip)
int hmpc_set_device_certificate(hmpc_handle *h, double *device_grad, double *device_lambda, double *device_resid, double *device_summary,
                                int32_t *device_where) {
  return set_family<hmpc::F_CERTIFICATE>(h, device_grad, device_lambda, device_resid, device_summary, device_where);
}

int hmpc_get_device_certificate(hmpc_handle *h, double **device_grad, double **device_lambda, double **device_resid, double **device_summary,
                                int32_t **device_where) {
  return get_family<hmpc::F_CERTIFICATE>(h, device_grad, device_lambda, device_resid, device_summary, device_where);
}

int hmpc_set_certificate_tolerance(hmpc_handle *h, double act_tol) {
  if (!h || !(act_tol > 0.0 && act_tol < 0.005)) return HMPC_E_ARG;  // (0.005: half the Mx window, above which both sides of row 4 would be active at once)
  h->cert_act_tol = act_tol;
  return HMPC_OK;
}

int hmpc_kkt_certificate(hmpc_handle *h, void *stream) {
  return enqueue_family(h, hmpc::F_CERTIFICATE, ResultNode::SOLVE, true, stream, [&](KernelArgs &a, void *const p[]) {
    return hmpc::launch_certificate(h->nc, a, h->cert_act_tol, as<hmpc::F_CERTIFICATE, hmpc::CertificateOut>(p), (hipStream_t)stream);
  });
}

int hmpc_download_certificate(hmpc_handle *h, double *grad, double *lambda, double *resid, double *summary, int32_t *where) {
  return download_family<hmpc::F_CERTIFICATE>(h, grad, lambda, resid, summary, where);
}

int hmpc_certificate_penalty(hmpc_handle *h, const double ceil[3], const double *device_penalty_in, double *device_penalty_out, void *stream) {
  return enqueue_penalty(h, hmpc::F_CERTIFICATE, ceil && device_penalty_out, stream, [&](void *const p[]) {
    return hmpc::launch_certificate_penalty(as<hmpc::F_CERTIFICATE, hmpc::CertificateOut>(p).summary, ceil, device_penalty_in, device_penalty_out, h->batch,
                                            (hipStream_t)stream);
  });
}

int hmpc_set_sweep_certificate_ceiling(hmpc_handle *h, const double ceil[3]) {
  if (!h) return HMPC_E_ARG;
  h->sweep_ceil_on = ceil != nullptr;
  for (int k = 0; k < hmpc::CERT_CEILS; ++k) h->sweep_ceil[k] = ceil ? ceil[k] : 0.0;
  return HMPC_OK;
}

// ---------------------------------------------------------------------------------------------------- feedback gains, first-order wrench (hmpc_feedback.hip)
int hmpc_set_device_gains(hmpc_handle *h, double *device_gain, double *device_ref_gain, double *device_summary, int32_t *device_free_dims) {
  return set_family<hmpc::F_GAINS>(h, device_gain, device_ref_gain, device_summary, device_free_dims);
}

int hmpc_get_device_gains(hmpc_handle *h, double **device_gain, double **device_ref_gain, double **device_summary, int32_t **device_free_dims) {
  return get_family<hmpc::F_GAINS>(h, device_gain, device_ref_gain, device_summary, device_free_dims);
}

int hmpc_feedback_gains(hmpc_handle *h, void *stream) {
  return enqueue_family(h, hmpc::F_GAINS, ResultNode::SOLVE, true, stream, [&](KernelArgs &a, void *const p[]) {
    return hmpc::launch_feedback(h->nc, a, h->cert_act_tol, as<hmpc::F_GAINS, hmpc::FeedbackOut>(p), (hipStream_t)stream);
  });
}

int hmpc_download_gains(hmpc_handle *h, double *gain, double *ref_gain, double *summary, int32_t *free_dims) {
  return download_family<hmpc::F_GAINS>(h, gain, ref_gain, summary, free_dims);
}

int hmpc_set_device_first_order(hmpc_handle *h, float *device_wrench, double *device_worst_slack) {
  return set_family<hmpc::F_FIRST_ORDER>(h, device_wrench, device_worst_slack);
}

int hmpc_first_order_wrench(hmpc_handle *h, const void *device_records_new, void *stream) {
  return enqueue_family(h, hmpc::F_FIRST_ORDER, ResultNode::GAINS, device_records_new != nullptr, stream, [&](KernelArgs &a, void *const p[]) {
    void *g[hmpc::MAX_SINGLE_ARRAYS];  // (where those gains went: moving them would have made them stale)
    for (int k = 0; k < FAMILIES[hmpc::F_GAINS].n; ++k) g[k] = h->d_result[hmpc::F_GAINS][k].get();
    const FirstOrderBuffers b = as<hmpc::F_FIRST_ORDER, FirstOrderBuffers>(p);
    return hmpc::launch_first_order(h->nc, a, (const unsigned char *)device_records_new, as<hmpc::F_GAINS, hmpc::FeedbackOut>(g), b.wrench, b.worst,
                                    (hipStream_t)stream);
  });
}

int hmpc_download_first_order(hmpc_handle *h, float *wrench, double *worst_slack) {
  return download_family<hmpc::F_FIRST_ORDER>(h, wrench, worst_slack);
}

// ---------------------------------------------------------------------------------------------------- adjoint (hmpc_adjoint.hip)
int hmpc_set_device_adjoint(hmpc_handle *h, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                            double *device_grad_alpha, double *device_dir, double *device_summary) {
  return set_family<hmpc::F_ADJOINT>(h, device_grad_x0, device_grad_traj, device_grad_weights, device_grad_alpha, device_dir, device_summary);
}

int hmpc_get_device_adjoint(hmpc_handle *h, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                            double **device_grad_alpha, double **device_dir, double **device_summary) {
  return get_family<hmpc::F_ADJOINT>(h, device_grad_x0, device_grad_traj, device_grad_weights, device_grad_alpha, device_dir, device_summary);
}

int hmpc_solve_adjoint(hmpc_handle *h, const double *device_seed, void *stream) {
  return enqueue_family(h, hmpc::F_ADJOINT, ResultNode::SOLVE, device_seed != nullptr, stream, [&](KernelArgs &a, void *const p[]) {
    return hmpc::launch_adjoint(h->nc, a, h->cert_act_tol, device_seed, as<hmpc::F_ADJOINT, hmpc::AdjointOut>(p), (hipStream_t)stream);
  });
}

int hmpc_download_adjoint(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, double *grad_alpha, double *dir,
                          double *summary) {
  return download_family<hmpc::F_ADJOINT>(h, grad_x0, grad_traj, grad_weights, grad_alpha, dir, summary);
}

// ---------------------------------------------------------------------------------------------------- multi-seed adjoint (hmpc_adjoint_multi.hip)
int hmpc_set_device_adjoint_multi(hmpc_handle *h, int n_seeds, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                                  double *device_grad_alpha, double *device_dir, double *device_summary) {
  if (!h) return HMPC_E_ARG;
  double *const p[hmpc::ADJOINT_ARRAYS] = {device_grad_x0, device_grad_traj, device_grad_weights, device_grad_alpha, device_dir, device_summary};
  RC_TRY(set_seed_slices(h->adjm_caller, &h->adjm_caller_seeds, hmpc::ADJOINT_ARRAYS, n_seeds, p));
  h->results.retarget_adjoint_multi();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_multi(hmpc_handle *h, int *n_seeds, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                                  double **device_grad_alpha, double **device_dir, double **device_summary) {
  if (!h) return HMPC_E_ARG;
  void *p[hmpc::ADJOINT_ARRAYS];
  adjoint_multi_base(h, p);
  if (n_seeds) *n_seeds = h->results.adjoint_multi_seeds_enqueued();
  double **const out[hmpc::ADJOINT_ARRAYS] = {device_grad_x0, device_grad_traj, device_grad_weights, device_grad_alpha, device_dir, device_summary};
  for (int k = 0; k < hmpc::ADJOINT_ARRAYS; ++k)
    if (out[k]) *out[k] = (double *)p[k];
  return HMPC_OK;
}

int hmpc_solve_adjoint_multi(hmpc_handle *h, const double *device_seeds, int n_seeds, void *stream) {
  if (!h || !device_seeds || n_seeds < 1 || n_seeds > HMPC_ADJOINT_MAX_SEEDS || !h->results.has_solve() || h->d_ext_Fc) return HMPC_E_ARG;
  bool caller = false, own = false;
  for (int k = 0; k < hmpc::ADJOINT_ARRAYS; ++k) (h->adjm_caller[k] ? caller : own) = true;
  if (caller && n_seeds > h->adjm_caller_seeds) return HMPC_E_ARG;  // the caller's buffers hold fewer slices
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (own) RC_TRY(reserve_seed_slices(h, hmpc::F_ADJOINT_MULTI, h->d_adjm_own, h->adjm_caller, hmpc::ADJOINT_ARRAYS, n_seeds, &h->adjm_own_seeds, stream));
  const KernelArgs a = problem_args(h);
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  void *p[hmpc::ADJOINT_ARRAYS];
  adjoint_multi_base(h, p);
  HIP_TRY(hmpc::launch_adjoint_multi(h->nc, a, h->cert_act_tol, device_seeds, n_seeds, as<hmpc::F_ADJOINT_MULTI, hmpc::AdjointOut>(p), (hipStream_t)stream));
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
  return download_family<hmpc::F_ADJOINT_MULTI>(h, grad_x0, grad_traj, grad_weights, grad_alpha, dir, summary);
}

// ---------------------------------------------------------------------------------------------------- model gradients (hmpc_model_adjoint.hip)
int hmpc_set_device_adjoint_model(hmpc_handle *h, double *device_grad_A, double *device_grad_B, double *device_grad_r,
                                  double *device_grad_params, double *device_costate) {
  return set_family<hmpc::F_MODEL_ADJOINT>(h, device_grad_A, device_grad_B, device_grad_r, device_grad_params, device_costate);
}

int hmpc_get_device_adjoint_model(hmpc_handle *h, double **device_grad_A, double **device_grad_B, double **device_grad_r,
                                  double **device_grad_params, double **device_costate) {
  return get_family<hmpc::F_MODEL_ADJOINT>(h, device_grad_A, device_grad_B, device_grad_r, device_grad_params, device_costate);
}

int hmpc_adjoint_model(hmpc_handle *h, void *stream) {
  return enqueue_family(h, hmpc::F_MODEL_ADJOINT, ResultNode::ADJOINT, true, stream, [&](KernelArgs &a, void *const p[]) {
    // (dir: where that adjoint went -- a single launch or a selected slice: moving them would have made it stale)
    return hmpc::launch_model_adjoint(h->nc, a, (double)h->params.mass, current_adjoint(h).dir, as<hmpc::F_MODEL_ADJOINT, hmpc::ModelAdjointOut>(p),
                                      (hipStream_t)stream);
  });
}

int hmpc_download_adjoint_model(hmpc_handle *h, double *grad_A, double *grad_B, double *grad_r, double *grad_params, double *costate) {
  return download_family<hmpc::F_MODEL_ADJOINT>(h, grad_A, grad_B, grad_r, grad_params, costate);
}

// ---------------------------------------------------------------------------------------------------- limit gradients (hmpc_limit_adjoint.hip)
int hmpc_set_device_adjoint_limits(hmpc_handle *h, double *device_grad_limits, double *device_grad_Fc, double *device_grad_bound,
                                   double *device_lambda, double *device_nu, double *device_summary) {
  return set_family<hmpc::F_LIMIT_ADJOINT>(h, device_grad_limits, device_grad_Fc, device_grad_bound, device_lambda, device_nu, device_summary);
}

int hmpc_get_device_adjoint_limits(hmpc_handle *h, double **device_grad_limits, double **device_grad_Fc, double **device_grad_bound,
                                   double **device_lambda, double **device_nu, double **device_summary) {
  return get_family<hmpc::F_LIMIT_ADJOINT>(h, device_grad_limits, device_grad_Fc, device_grad_bound, device_lambda, device_nu, device_summary);
}

int hmpc_adjoint_limits(hmpc_handle *h, const double *device_seed, void *stream) {
  return enqueue_family(h, hmpc::F_LIMIT_ADJOINT, ResultNode::ADJOINT, device_seed != nullptr, stream, [&](KernelArgs &a, void *const p[]) {
    return hmpc::launch_limit_adjoint(h->nc, a, h->cert_act_tol, current_adjoint(h).dir, device_seed, as<hmpc::F_LIMIT_ADJOINT, hmpc::LimitAdjointOut>(p),
                                      (hipStream_t)stream);
  });
}

int hmpc_download_adjoint_limits(hmpc_handle *h, double *grad_limits, double *grad_Fc, double *grad_bound, double *lambda, double *nu,
                                 double *summary) {
  return download_family<hmpc::F_LIMIT_ADJOINT>(h, grad_limits, grad_Fc, grad_bound, lambda, nu, summary);
}

// ---------------------------------------------------------------------------------------------------- record gradients (hmpc_pose_adjoint.hip)
int hmpc_set_device_adjoint_record(hmpc_handle *h, double *device_grad_record, double *device_grad_frames, double *device_grad_rpy) {
  return set_family<hmpc::F_RECORD_ADJOINT>(h, device_grad_record, device_grad_frames, device_grad_rpy);
}

int hmpc_get_device_adjoint_record(hmpc_handle *h, double **device_grad_record, double **device_grad_frames, double **device_grad_rpy) {
  return get_family<hmpc::F_RECORD_ADJOINT>(h, device_grad_record, device_grad_frames, device_grad_rpy);
}

int hmpc_adjoint_record(hmpc_handle *h, void *stream) {
  // the three inputs: an adjoint of the last solve of the current batch, and model and limit gradients behind it; the chain goes through
  // the handle's own assembly, which an external constraint block is not
  const bool ok = h && h->results.can_record_adjoint() && !h->d_ext_Fc;
  return enqueue_family(h, hmpc::F_RECORD_ADJOINT, ResultNode::ADJOINT, ok, stream, [&](KernelArgs &a, void *const p[]) {
    const hmpc::AdjointOut adj = current_adjoint(h);  // (where the three went: moving them would have made them stale)
    const OutputBuffer<unsigned char> *mo = h->d_result[hmpc::F_MODEL_ADJOINT], *lo = h->d_result[hmpc::F_LIMIT_ADJOINT];
    const hmpc::PoseAdjointIn in = {adj.grad_x0, adj.grad_traj, adj.grad_weights, adj.grad_alpha, (const double *)mo[0].get(), (const double *)mo[1].get(),
                                    (const double *)mo[2].get(), (const double *)lo[0].get(), (const double *)lo[1].get()};
    return hmpc::launch_pose_adjoint(h->nc, a, in, as<hmpc::F_RECORD_ADJOINT, hmpc::PoseAdjointOut>(p), (hipStream_t)stream);
  });
}

int hmpc_download_adjoint_record(hmpc_handle *h, double *grad_record, double *grad_frames, double *grad_rpy) {
  return download_family<hmpc::F_RECORD_ADJOINT>(h, grad_record, grad_frames, grad_rpy);
}

// ---------------------------------------------------------------------------------------------------- chain of the multi-seed adjoint (hmpc_adjoint_chain.hip)
int hmpc_set_device_adjoint_chain_multi(hmpc_handle *h, int n_seeds, const struct hmpc_adjoint_chain *device_buffers) {
  if (!h) return HMPC_E_ARG;
  double *p[hmpc::CHAIN_ARRAYS] = {};
  if (device_buffers) memcpy(p, device_buffers, sizeof(p));
  RC_TRY(set_seed_slices(h->chain_caller, &h->chain_caller_seeds, hmpc::CHAIN_ARRAYS, n_seeds, p));
  h->results.retarget_adjoint_chain();
  return HMPC_OK;
}

int hmpc_get_device_adjoint_chain_multi(hmpc_handle *h, int *n_seeds, struct hmpc_adjoint_chain *device_buffers) {
  if (!h) return HMPC_E_ARG;
  if (n_seeds) *n_seeds = h->results.has_adjoint_chain() ? h->results.adjoint_multi_seeds_enqueued() : 0;
  if (device_buffers) {
    void *p[hmpc::CHAIN_ARRAYS];
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
  for (int k = 0; k < hmpc::CHAIN_ARRAYS; ++k)
    if (h->chain_caller[k]) caller = true;
    else if (k < hmpc::CHAIN_COMPACT) own = true;
  if (caller && n_seeds > h->chain_caller_seeds) return HMPC_E_ARG;  // the caller's buffers hold fewer slices
  if (h->batch == 0) return HMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (own) RC_TRY(reserve_seed_slices(h, hmpc::F_ADJOINT_CHAIN, h->d_chain_own, h->chain_caller, hmpc::CHAIN_COMPACT, n_seeds, &h->chain_own_seeds, stream));
  void *m[hmpc::ADJOINT_ARRAYS], *p[hmpc::CHAIN_ARRAYS];
  adjoint_multi_base(h, m);  // (where that adjoint went: moving it would have made it stale)
  const hmpc::AdjointOut adj = as<hmpc::F_ADJOINT_MULTI, hmpc::AdjointOut>(m);
  const hmpc::AdjointChainIn in = {device_seeds, adj.dir, adj.grad_x0, adj.grad_traj, adj.grad_weights, adj.grad_alpha};
  chain_base(h, p);
  const KernelArgs a = problem_args(h);
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_adjoint_chain(h->nc, a, h->cert_act_tol, (double)h->params.mass, in, n_seeds, as<hmpc::F_ADJOINT_CHAIN, hmpc::AdjointChainOut>(p),
                                     (hipStream_t)stream));
  for (int k = 0; k < hmpc::CHAIN_ARRAYS; ++k) h->chain_written[k] = p[k] != nullptr;
  h->results.on_adjoint_chain();
  return HMPC_OK;
}

int hmpc_download_adjoint_chain_multi(hmpc_handle *h, const struct hmpc_adjoint_chain *host_buffers) {
  void *dst[hmpc::CHAIN_ARRAYS] = {};
  if (host_buffers) memcpy(dst, host_buffers, sizeof(dst));
  return download(h, hmpc::F_ADJOINT_CHAIN, dst);
}

// ---------------------------------------------------------------------------------------------------- selection (hmpc_select.hip)
// The best command of every sweep group, from the last solve's status and forces and the last prediction: one row per group, the handle's
// own buffers allocated for max_batch groups.
int hmpc_set_device_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states) {
  return set_family<hmpc::F_SELECTION>(h, index, score, forces, status, states);
}

int hmpc_get_device_selection(hmpc_handle *h, int32_t **index, double **score, float **forces, uint32_t **status, float **states,
                              int *n_groups) {
  RC_TRY(get_family<hmpc::F_SELECTION>(h, index, score, forces, status, states));
  if (n_groups) *n_groups = h->results.selected_groups();
  return HMPC_OK;
}

int hmpc_sweep_select(hmpc_handle *h, int group_size, const double *device_penalty, void *stream) {
  if (!h || group_size < 1) return HMPC_E_ARG;
  if (h->batch % group_size != 0) return HMPC_E_ARG;
  if (!h->results.has_prediction()) return HMPC_E_ARG;  // no prediction from the last solve of this batch: the cost buffer holds another solve's, or none
  HIP_TRY(hipSetDevice(h->device));
  void *pp[hmpc::MAX_SINGLE_ARRAYS], *ps[hmpc::MAX_SINGLE_ARRAYS];
  RC_TRY(ensure(h, hmpc::F_PREDICTION, pp));
  RC_TRY(ensure(h, hmpc::F_SELECTION, ps));
  const PredictionBuffers pred = as<hmpc::F_PREDICTION, PredictionBuffers>(pp);
  const SelectionBuffers b = as<hmpc::F_SELECTION, SelectionBuffers>(ps);
  hmpc::SelectArgs a;
  a.cost = pred.cost, a.states = pred.states, a.status = h->d_status.get(), a.forces = h->d_forces.get(), a.penalty = device_penalty;
  a.groups = h->batch / group_size, a.group_size = group_size;
  a.force_words = (int)hmpc::SELECTION_ROWS[2].row(h->nc, h->setup.horizon), a.state_words = (int)hmpc::SELECTION_ROWS[4].row(h->nc, h->setup.horizon);
  a.index = b.index, a.score = b.score, a.out_forces = b.forces, a.out_status = b.status, a.out_states = b.states;
  RC_TRY(enter_stream(h, (hipStream_t)stream));
  HIP_TRY(hmpc::launch_select(a, (hipStream_t)stream));
  h->results.on_select(a.groups);
  return HMPC_OK;
}

int hmpc_download_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states) {
  return download_family<hmpc::F_SELECTION>(h, index, score, forces, status, states);
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
  void *ps[hmpc::MAX_SINGLE_ARRAYS];
  RC_TRY(ensure(h, hmpc::F_SELECTION, ps));
  HIP_TRY(hmpc::launch_leg_torques(as<hmpc::F_SELECTION, SelectionBuffers>(ps).forces, n_ticks, h->setup.horizon, /*rBody=*/nullptr, /*leg_q=*/nullptr,
                                   device_f_ff, device_tau, (const hmpc_tick_inputs *)device_ticks, (hipStream_t)stream));
  return HMPC_OK;
}

}  // extern "C"
