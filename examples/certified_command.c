/* Which command should the robot execute -- among those whose answer really is the minimiser?  The sweep of safe_command.c with a ceiling
 * on the KKT certificate: per planning tick a command sweep and the prediction, then ONE more launch that certifies every candidate's
 * forces (hmpc_kkt_certificate: the gradient of the QP objective from the prediction model, multipliers >= 0 on the active limits from a
 * small non-negative least-squares problem per stance leg-step, the stationarity residual they leave -- nothing of it shared with the
 * solver), ONE tiny launch turns "residual above the ceiling" into a +inf penalty (hmpc_certificate_penalty) and the selection
 * (hmpc_sweep_select) skips the masked candidates.  (hmpc_tick_sweep_device does the same inside one call once
 * hmpc_set_sweep_certificate_ceiling is set.)
 * Tick 0 takes the solver's answers as they are: nothing is masked.  In tick 1 one candidate's slot of the force buffer is spoiled by 1 N
 * after the solve (what stale state would do without touching the status word): the certificate masks exactly that one.
 * Printed per tick: how many commands the ceiling masked, and the winners; checked against the host route.
 * The penalty and the forces live in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/certified_command.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o certified_command */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "hector_mpc.h"

enum { H = 10, STATES = 3, COMMANDS = 8, N = STATES * COMMANDS, TICKS = 2, SPOILED = 1 * COMMANDS + 3 };

static void pack(unsigned char *rec, double vx_body, double vx_cmd, double tilt) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {vx_body, 0, 0}, w[3] = {0, 0, 0};
  double q[4] = {cos(tilt / 2), 0, sin(tilt / 2), 0}; /* pitched by `tilt` */
  double r[6] = {0.02, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0};
  int gait[2 * H];
  for (int i = 0; i < H; ++i) {
    traj[12 * i + 3] = i * 0.04 * vx_cmd, traj[12 * i + 5] = 0.55, traj[12 * i + 9] = vx_cmd;
    gait[2 * i] = gait[2 * i + 1] = 1; /* double support */
  }
  hmpc_pack_record(rec, H, p, v, q, w, r, ja, 0.0, Q, traj, A, gait);
}

typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);

int main(void) {
  struct problem_setup ps = {0.04f, 0.25f, 500.f, H};
  hmpc_handle *h = NULL;
  int rc = hmpc_create(&h, &ps, N, 0);
  if (rc != HMPC_OK) {
    fprintf(stderr, "hmpc_create failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 2;
  }
  malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
  free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
  memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
  double *d_penalty = NULL;
  float *d_forces = NULL;
  uint32_t *d_status = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_penalty, N * sizeof(double)) != 0 ||
      dev_malloc((void **)&d_forces, (size_t)N * 12 * H * sizeof(float)) != 0 || dev_malloc((void **)&d_status, N * sizeof(uint32_t)) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  hmpc_set_device_outputs(h, d_forces, d_status); /* the force buffer is ours: tick 1 spoils one slot of it */
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  const double v_body[STATES] = {-0.2, 0.0, 0.3}, v_cmd[COMMANDS] = {-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8};
  const double ceiling[3] = {1e-2, NAN, 1e-5}; /* stationarity (N m-ish units of the gradient), no test of complementarity, primal violation */
  double cost[N * 2], summary[N * 4], score[STATES];
  int32_t best[STATES];
  uint32_t st[STATES];
  int bad = 0;
  bad += hmpc_certificate_penalty(h, ceiling, NULL, d_penalty, NULL) != HMPC_E_ARG; /* no certificate yet: refused, nothing enqueued */

  for (int tick = 0; tick < TICKS; ++tick) {
    for (int s = 0; s < STATES; ++s)
      for (int c = 0; c < COMMANDS; ++c) pack(recs + (size_t)(s * COMMANDS + c) * stride, v_body[s] + 0.05 * tick, v_cmd[c], 0.02 * s);
    rc = hmpc_upload_records(h, recs, N);
    if (rc == HMPC_OK) rc = hmpc_solve_command_sweep(h, COMMANDS, NULL);
    if (rc == HMPC_OK && tick == 1) { /* 1 N moved between the feet's first Fz of one candidate: feasible, not optimal, status word untouched */
      float two[6];
      float *slot = d_forces + (size_t)SPOILED * 12 * H; /* (a blocking copy on the null stream waits for the solve enqueued there) */
      bad += dev_memcpy(two, slot, sizeof(two), 2 /* device to host */) != 0;
      two[2] += 1.0f, two[5] -= 1.0f;
      bad += dev_memcpy(slot, two, sizeof(two), 1 /* host to device */) != 0;
    }
    if (rc == HMPC_OK) rc = hmpc_predict_states(h, NULL);
    if (rc == HMPC_OK) rc = hmpc_kkt_certificate(h, NULL);
    if (rc == HMPC_OK) rc = hmpc_certificate_penalty(h, ceiling, NULL, d_penalty, NULL);
    if (rc == HMPC_OK) rc = hmpc_sweep_select(h, COMMANDS, d_penalty, NULL);
    if (rc == HMPC_OK) rc = hmpc_download_selection(h, best, score, NULL, st, NULL);
    if (rc == HMPC_OK) rc = hmpc_download_certificate(h, NULL, NULL, NULL, summary, NULL);
    if (rc == HMPC_OK) rc = hmpc_download_prediction(h, NULL, cost); /* (only for the check below) */
    if (rc != HMPC_OK) {
      fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
      return 1;
    }
    int masked = 0;
    double worst_kept = 0.0;
    for (int i = 0; i < N; ++i) {
      const int out = !(summary[4 * i] <= ceiling[0]) || !(summary[4 * i + 2] <= ceiling[2]);
      masked += out;
      if (!out && summary[4 * i] > worst_kept) worst_kept = summary[4 * i];
    }
    printf("tick %d: the ceiling masked %d of %d commands (largest stationarity residual kept %.2e", tick, masked, N, worst_kept);
    if (tick == 1) printf(", of the spoiled candidate %.2e", summary[4 * SPOILED]);
    printf(")\n");
    bad += masked != (tick == 1 ? 1 : 0);
    if (tick == 1) bad += summary[4 * SPOILED] <= ceiling[0];
    for (int s = 0; s < STATES; ++s) {
      int host_best = -1; /* the host route: argmin over the certified candidates, lowest index first */
      for (int c = 0; c < COMMANDS; ++c) {
        const int i = s * COMMANDS + c;
        if (!(summary[4 * i] <= ceiling[0]) || !(summary[4 * i + 2] <= ceiling[2])) continue;
        if (host_best < 0 || cost[2 * i] + cost[2 * i + 1] < cost[2 * (s * COMMANDS + host_best)] + cost[2 * (s * COMMANDS + host_best) + 1]) host_best = c;
      }
      bad += best[s] != host_best || best[s] < 0 || HMPC_STATUS_CODE(st[s]) != HMPC_S_OK;
      bad += s * COMMANDS + best[s] == SPOILED && tick == 1;
      printf("  state %d (body at %+.2f m/s): command %d, vx %+.2f m/s (score %.4f, stationarity residual %.2e)\n", s, v_body[s] + 0.05 * tick,
             best[s], best[s] < 0 ? 0.0 : v_cmd[best[s]], score[s], best[s] < 0 ? 0.0 : summary[4 * (s * COMMANDS + best[s])]);
    }
  }
  printf("certified command of %d states x %d commands over %d ticks: %d problems\n", STATES, COMMANDS, TICKS, bad);
  dev_free(d_penalty), dev_free(d_forces), dev_free(d_status);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
