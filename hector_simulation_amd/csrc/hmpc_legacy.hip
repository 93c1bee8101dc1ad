// hmpc_legacy.hip -- the reference's own interface (convexMPC_interface.cpp:42-118, SolverMPC.cpp:94-97, 371-738) over the batched C ABI
// of include/hector_mpc.h: process-global, single-threaded, blocking.  A maintainer drops the library in place of those translation units.
// There is NO CPU fallback: without a gfx950 device the entry points print the error and leave the previous solution in place.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/hector_mpc.h"
#include "hmpc_plan.h"
#include "hmpc_record.h"

extern "C" {

static problem_setup g_setup = {0.f, 0.f, 0.f, 0};
static problem_setup g_handle_setup = {0.f, 0.f, 0.f, 0};  // what g_handle was created with
static update_data_t g_update;
static hmpc_handle *g_handle = nullptr;
static double *g_q_soln = nullptr;  // 12*horizon doubles, solver-owned (SolverMPC.cpp:52, :94-97)
static int g_q_len = 0;
static int g_has_solved = 0;
static uint32_t g_last_status = 0;
static int g_setup_error = 0;
static hmpc_params g_legacy_params = {9.0f, {0.5413f, 0.5200f, 0.0691f}, 2.0f, 0.09f, 0.06f, 9.81f};  // hmpc_legacy_set_params
static float g_pred[13 * HMPC_MAX_HORIZON];  // hmpc_legacy_predicted_state: the last solve's predicted states, fetched on first use
static int g_pred_valid = 0;
static double g_slack[10 * 2 * HMPC_MAX_HORIZON];  // hmpc_legacy_constraint_slack: the last solve's slacks, fetched on first use
static int g_slack_valid = 0;
static double g_lambda[10 * 2 * HMPC_MAX_HORIZON], g_cert_summary[4];  // hmpc_legacy_multiplier, hmpc_legacy_stationarity: the last solve's certificate, fetched on first use
static int g_cert_valid = 0;
static double g_gain[12 * 13];  // hmpc_legacy_feedback_gain: K_0 of the last solve, fetched on first use
static int g_gain_valid = 0;
static int g_legacy_iter_cap = 0;  // hmpc_legacy_set_max_iterations: explicit opt-in (update_solver_settings is inert, as in the reference)
// one tick = one pinned staging buffer [record | 12h forces | status word] and one contiguous device output block, so that
// a blocking tick costs one asynchronous H2D copy, one launch, one asynchronous D2H copy and a single synchronisation
static unsigned char *g_pin = nullptr;
static float *g_dev_out = nullptr;
static size_t g_pin_rec_bytes = 0;

static void free_tick_buffers(void) {
  if (g_pin) hipHostFree(g_pin);
  if (g_dev_out) hipFree(g_dev_out);
  g_pin = nullptr, g_dev_out = nullptr, g_pin_rec_bytes = 0;
}

void setup_problem(double dt, int horizon, double mu, double f_max) {
  g_setup.horizon = horizon;
  g_setup.f_max = (float)f_max;
  g_setup.mu = (float)mu;
  g_setup.dt = (float)dt;
  g_setup_error = 0;
  if (horizon < 1 || horizon > HMPC_MAX_HORIZON) {
    // the reference throws std::runtime_error("horizon is too long!") from c2qp for horizon > 19; we never throw across C
    fprintf(stderr, "[hector_mpc_hip] setup_problem: horizon %d outside [1,%d]\n", horizon, HMPC_MAX_HORIZON);
    g_setup_error = HMPC_E_HORIZON;
    return;
  }
  // the reference frees and re-mallocs every buffer on every call (resize_qp_mats); we only rebuild when the
  // problem shape or scalars change, the observable behaviour (q_soln valid until the next setup) is the same.
  if (g_handle && (g_handle_setup.horizon != horizon || g_handle_setup.dt != g_setup.dt || g_handle_setup.f_max != g_setup.f_max)) {
    hmpc_destroy(g_handle);
    g_handle = nullptr;
    free_tick_buffers();
  }
  if (!g_handle) {
    // the reference has no notion of a device: HMPC_DEVICE (default 0) picks the GPU of the process-global solver
    const char *env = getenv("HMPC_DEVICE");
    const int dev = (env && *env) ? atoi(env) : 0;
    int rc = hmpc_create(&g_handle, &g_setup, 1, dev);
    g_handle_setup = g_setup;
    if (rc != HMPC_OK) {
      fprintf(stderr, "[hector_mpc_hip] setup_problem failed (%d): %s\n", rc, hmpc_last_hip_error());
      g_handle = nullptr;
      g_setup_error = rc;
      return;
    }
    g_pin_rec_bytes = ((size_t)hmpc::rec_stride(2, horizon) + 63) & ~(size_t)63;
    const size_t out_bytes = sizeof(float) * 12 * horizon + sizeof(uint32_t);
    if (hipHostMalloc((void **)&g_pin, g_pin_rec_bytes + out_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&g_dev_out, out_bytes) != hipSuccess ||
        hmpc_set_device_outputs(g_handle, g_dev_out, (uint32_t *)(g_dev_out + 12 * horizon)) != HMPC_OK) {
      fprintf(stderr, "[hector_mpc_hip] setup_problem: could not allocate the tick buffers\n");
      free_tick_buffers();
      hmpc_destroy(g_handle);
      g_handle = nullptr;
      g_setup_error = HMPC_E_HIP;
      return;
    }
  }
  if (g_q_len != 12 * horizon) {
    free(g_q_soln);
    g_q_soln = (double *)calloc((size_t)12 * horizon, sizeof(double));
    g_q_len = 12 * horizon;
  }
}

static void solve_global(void) {
  if (!g_handle || g_setup_error) {
    fprintf(stderr, "[hector_mpc_hip] solve requested without a valid setup_problem (error %d)\n", g_setup_error);
    return;
  }
  const int hz = g_setup.horizon;
  unsigned char *rec = g_pin;
  const update_data_t &u = g_update;
  hmpc::pack_record<2>(rec, hz, hmpc::RecSource<float, unsigned char>{u.p, u.v, u.q, u.w, u.r, u.joint_angles, u.yaw, u.weights, u.traj, u.Alpha_K, u.gait});
  const float *forces = (const float *)(g_pin + g_pin_rec_bytes);
  const uint32_t *pst = (const uint32_t *)(forces + 12 * hz);
  const size_t out_bytes = sizeof(float) * 12 * hz + sizeof(uint32_t);
  uint32_t st = 0;
  hmpc_set_max_iterations(g_handle, g_legacy_iter_cap);
  hmpc_set_params(g_handle, &g_legacy_params);
  int rc = hmpc_upload_records_async(g_handle, rec, 1, nullptr);  // pinned source: a true asynchronous copy
  if (rc == HMPC_OK) rc = hmpc_solve(g_handle, nullptr);
  if (rc == HMPC_OK && (hipMemcpyAsync(g_pin + g_pin_rec_bytes, g_dev_out, out_bytes, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
                        hipStreamSynchronize(nullptr) != hipSuccess))
    rc = HMPC_E_HIP;
  if (rc == HMPC_OK) {
    st = *pst;
    if (flagged(st, g_legacy_iter_cap)) {  // (the cap the handle was given above)
      // flagged by the fast variant: the safe pass (full-size working set, then relaxed bounds), as hmpc_download gives it
      rc = hmpc_resolve_failed(g_handle, nullptr);
      if (rc == HMPC_OK && hipMemcpy(g_pin + g_pin_rec_bytes, g_dev_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        rc = HMPC_E_HIP;
      st = *pst;
    }
  }
  if (rc != HMPC_OK) {
    fprintf(stderr, "[hector_mpc_hip] solve failed (%d): %s\n", rc, hmpc_last_hip_error());
    return;
  }
  g_last_status = st;
  // SolverMPC.cpp:714-715: the reference prints this line and scatters whatever qpOASES left in q_red all the same; so do
  // we (the forces of a flagged instance are the last iterate; hmpc_last_status() tells the caller, which the reference
  // cannot).  HMPC_S_OK_RELAXED is a solved instance.
  const uint32_t code = HMPC_STATUS_CODE(st);
  if (code != HMPC_S_OK && code != HMPC_S_OK_RELAXED) printf("failed to solve!\n");
  for (int i = 0; i < 12 * hz; ++i) g_q_soln[i] = (double)forces[i];
  g_has_solved = 1;
  g_pred_valid = 0;
  g_slack_valid = 0;
  g_cert_valid = 0;
  g_gain_valid = 0;
}

void update_problem_data(double *p, double *v, double *q, double *w, double *r, double *joint_angles, double yaw,
                         double *weights, double *state_trajectory, double *Alpha_K, int *gait) {
  const int hz = g_setup.horizon;
  if (hz < 1 || hz > HMPC_MAX_HORIZON) return;
  for (int i = 0; i < 3; ++i) g_update.p[i] = (float)p[i], g_update.v[i] = (float)v[i], g_update.w[i] = (float)w[i];
  for (int i = 0; i < 4; ++i) g_update.q[i] = (float)q[i];
  for (int i = 0; i < 6; ++i) g_update.r[i] = (float)r[i];
  for (int i = 0; i < 10; ++i) g_update.joint_angles[i] = (float)joint_angles[i];
  g_update.yaw = (float)yaw;
  for (int i = 0; i < 12; ++i) g_update.weights[i] = (float)weights[i], g_update.Alpha_K[i] = (float)Alpha_K[i];
  for (int i = 0; i < 12 * hz; ++i) g_update.traj[i] = (float)state_trajectory[i];
  for (int i = 0; i < 2 * hz; ++i) g_update.gait[i] = (unsigned char)gait[i];
  solve_global();
}

double get_solution(int index) {
  if (!g_has_solved) return 0.0;  // convexMPC_interface.cpp:107
  if (index < 0 || index >= g_q_len) return 0.0;
  return g_q_soln[index];
}

double hmpc_legacy_predicted_state(int step, int component) {
  if (!g_has_solved || !g_handle) return 0.0;  // as get_solution: 0 before the first solve and for out-of-range arguments
  if (step < 0 || step >= g_setup.horizon || component < 0 || component >= 13) return 0.0;
  if (!g_pred_valid) {  // once per solve, on first use: one launch and one small copy
    int rc = hmpc_predict_states(g_handle, nullptr);
    if (rc == HMPC_OK) rc = hmpc_download_prediction(g_handle, g_pred, nullptr);
    if (rc != HMPC_OK) {
      fprintf(stderr, "[hector_mpc_hip] prediction failed (%d): %s\n", rc, hmpc_last_hip_error());
      return 0.0;
    }
    g_pred_valid = 1;
  }
  return (double)g_pred[13 * step + component];
}

double hmpc_legacy_constraint_slack(int step, int contact, int j) {
  if (!g_has_solved || !g_handle) return 0.0;  // as get_solution: 0 before the first solve and for out-of-range arguments
  if (step < 0 || step >= g_setup.horizon || contact < 0 || contact >= 2 || j < 0 || j >= 10) return 0.0;
  if (!g_slack_valid) {  // once per solve, on first use: one launch and one small copy
    int rc = hmpc_constraint_margins(g_handle, nullptr);
    if (rc == HMPC_OK) rc = hmpc_download_margins(g_handle, g_slack, nullptr, nullptr);
    if (rc != HMPC_OK) {
      fprintf(stderr, "[hector_mpc_hip] constraint margins failed (%d): %s\n", rc, hmpc_last_hip_error());
      return 0.0;
    }
    g_slack_valid = 1;
  }
  return g_slack[10 * (2 * step + contact) + j];
}

// once per solve, on first use: one launch and two small copies
static bool legacy_certificate(void) {
  if (g_cert_valid) return true;
  int rc = hmpc_kkt_certificate(g_handle, nullptr);
  if (rc == HMPC_OK) rc = hmpc_download_certificate(g_handle, nullptr, g_lambda, nullptr, g_cert_summary, nullptr);
  if (rc != HMPC_OK) {
    fprintf(stderr, "[hector_mpc_hip] KKT certificate failed (%d): %s\n", rc, hmpc_last_hip_error());
    return false;
  }
  g_cert_valid = 1;
  return true;
}

double hmpc_legacy_multiplier(int step, int contact, int j) {
  if (!g_has_solved || !g_handle) return 0.0;  // as get_solution: 0 before the first solve and for out-of-range arguments
  if (step < 0 || step >= g_setup.horizon || contact < 0 || contact >= 2 || j < 0 || j >= 10) return 0.0;
  return legacy_certificate() ? g_lambda[10 * (2 * step + contact) + j] : 0.0;
}

double hmpc_legacy_stationarity(void) {
  if (!g_has_solved || !g_handle) return 0.0;
  return legacy_certificate() ? g_cert_summary[0] : 0.0;
}

double hmpc_legacy_feedback_gain(int component, int state) {
  if (!g_has_solved || !g_handle) return 0.0;  // as get_solution: 0 before the first solve and for out-of-range arguments
  if (component < 0 || component >= 12 || state < 0 || state >= 13) return 0.0;
  if (!g_gain_valid) {  // once per solve, on first use: one launch and one small copy
    int rc = hmpc_feedback_gains(g_handle, nullptr);
    if (rc == HMPC_OK) rc = hmpc_download_gains(g_handle, g_gain, nullptr, nullptr, nullptr);
    if (rc != HMPC_OK) {
      fprintf(stderr, "[hector_mpc_hip] feedback gains failed (%d): %s\n", rc, hmpc_last_hip_error());
      return 0.0;
    }
    g_gain_valid = 1;
  }
  return g_gain[13 * component + state];
}

void update_solver_settings(int max_iter, double rho, double sigma, double solver_alpha, double terminate,
                            double use_jcqp) {
  // Stored exactly as the reference stores them (convexMPC_interface.cpp:112-118) -- and, as in the reference, read by
  // NOTHING: its qpOASES path runs with a fixed nWSR (SolverMPC.cpp:706) whatever max_iter says, so a caller that passes a
  // small JCQP/ADMM-style max_iter (the knobs belong to a solver the reference does not ship) gets full solves there and
  // must get them here.  The opt-in with a meaning for this solver is hmpc_legacy_set_max_iterations / hmpc_set_max_iterations.
  g_update.max_iterations = max_iter;
  g_update.rho = rho;
  g_update.sigma = sigma;
  g_update.solver_alpha = solver_alpha;
  g_update.terminate = terminate;
  (void)use_jcqp;
}

int hmpc_legacy_set_params(const struct hmpc_params *p) {
  hmpc_params d;
  hmpc_default_params(&d);
  if (p && !params_ok(*p)) return HMPC_E_ARG;
  g_legacy_params = p ? *p : d;
  return HMPC_OK;
}

int hmpc_legacy_set_max_iterations(int max_iter) {
  if (max_iter < 0) return HMPC_E_ARG;
  g_legacy_iter_cap = max_iter;
  return HMPC_OK;
}

void hmpc_solve_mpc(struct update_data_t *update, struct problem_setup *setup) {
  if (!update || !setup) return;
  if (!g_handle || g_setup.horizon != setup->horizon || g_setup.dt != setup->dt || g_setup.f_max != setup->f_max)
    setup_problem((double)setup->dt, setup->horizon, (double)setup->mu, (double)setup->f_max);
  if (update != &g_update) g_update = *update;
  solve_global();
}
void solveDenseMPC(struct update_data_t *update, struct problem_setup *setup) { hmpc_solve_mpc(update, setup); }
double *hmpc_get_q_soln(void) { return g_q_soln; }
uint32_t hmpc_last_status(void) { return g_last_status; }

}  // extern "C"

// C++-linkage symbols with the reference's exact names (SolverMPC.h:56, :63), for callers that include its header
void solve_mpc(update_data_t *update, problem_setup *setup) { hmpc_solve_mpc(update, setup); }
double *get_q_soln() { return hmpc_get_q_soln(); }
