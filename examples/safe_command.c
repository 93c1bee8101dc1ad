/* Which command should the robot execute -- without getting close to slipping?  The sweep of best_command.c with a floor on the friction
 * headroom: after the command sweep and the prediction, ONE more launch computes how far every candidate's forces are from the limits the
 * QP was solved under (hmpc_constraint_margins: friction pyramid, Mx, line contact, Fz floor and cap, and per instance the smallest
 * friction slack as a fraction of the normal force), ONE tiny launch turns "headroom below the floor" into a +inf penalty
 * (hmpc_margin_penalty) and the selection (hmpc_sweep_select) skips the masked candidates: cheapest among the safe ones, no force row
 * ever leaves the device.  (hmpc_tick_sweep_device does the same inside one call once hmpc_set_sweep_margin_floor is set.)
 * Printed per state: the unmasked and the masked winner with their headroom; checked against the host route (download every cost and
 * summary, argmin over the candidates that meet the floor).
 * The penalty lives in device memory; a plain C program takes the allocator from the HIP runtime the library brought into the process.
 *   gcc -std=c11 -Iinclude examples/safe_command.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o safe_command */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "hector_mpc.h"

enum { H = 10, STATES = 3, COMMANDS = 8, N = STATES * COMMANDS };

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

int main(void) {
  struct problem_setup ps = {0.04f, 0.25f, 500.f, H};
  struct hmpc_params prm;
  hmpc_handle *h = NULL;
  int rc = hmpc_create(&h, &ps, N, 0);
  if (rc != HMPC_OK) {
    fprintf(stderr, "hmpc_create failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 2;
  }
  malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
  free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
  double *d_penalty = NULL;
  if (!dev_malloc || !dev_free || dev_malloc((void **)&d_penalty, N * sizeof(double)) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  hmpc_default_params(&prm);
  prm.mu = 0.5f; /* a surface on which the tangential forces of a fast command matter */
  hmpc_set_params(h, &prm);
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  const double v_body[STATES] = {-0.2, 0.0, 0.3}, v_cmd[COMMANDS] = {-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8};
  double cost[N * 2], summary[N * 6], score[STATES];
  int32_t plain[STATES], safe[STATES];
  uint32_t st[STATES];
  int bad = 0;

  for (int s = 0; s < STATES; ++s)
    for (int c = 0; c < COMMANDS; ++c) pack(recs + (size_t)(s * COMMANDS + c) * stride, v_body[s], v_cmd[c], 0.02 * s);
  rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve_command_sweep(h, COMMANDS, NULL);
  const double no_floor[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
  const int early = hmpc_margin_penalty(h, no_floor, NULL, d_penalty, NULL); /* no margins yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_predict_states(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_constraint_margins(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_sweep_select(h, COMMANDS, NULL, NULL); /* the unmasked winners */
  if (rc == HMPC_OK) rc = hmpc_download_selection(h, plain, NULL, NULL, NULL, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_margins(h, NULL, summary, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_prediction(h, NULL, cost); /* (only for the check below) */
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  bad += early != HMPC_E_ARG;
  /* the floor: just above the smallest headroom among the unmasked winners, so that at least that state has to choose again */
  double limit[6] = {NAN, NAN, NAN, NAN, NAN, NAN}, least = INFINITY;
  for (int s = 0; s < STATES; ++s) {
    if (plain[s] < 0) return 1;
    const double head = summary[6 * (s * COMMANDS + plain[s]) + 5];
    if (head < least) least = head;
  }
  limit[5] = nextafter(least, INFINITY);
  rc = hmpc_margin_penalty(h, limit, NULL, d_penalty, NULL);
  if (rc == HMPC_OK) rc = hmpc_sweep_select(h, COMMANDS, d_penalty, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_selection(h, safe, score, NULL, st, NULL);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  int changed = 0;
  for (int s = 0; s < STATES; ++s) {
    int host_best = -1; /* the host route: argmin over the candidates whose headroom meets the floor, lowest index first */
    for (int c = 0; c < COMMANDS; ++c) {
      const int i = s * COMMANDS + c;
      if (!(summary[6 * i + 5] >= limit[5])) continue;
      if (host_best < 0 || cost[2 * i] + cost[2 * i + 1] < cost[2 * (s * COMMANDS + host_best)] + cost[2 * (s * COMMANDS + host_best) + 1]) host_best = c;
    }
    bad += safe[s] != host_best;
    changed += safe[s] != plain[s];
    printf("state %d (body at %+.2f m/s): unmasked winner %d, vx %+.2f m/s (headroom %.3f) -> ", s, v_body[s], plain[s], v_cmd[plain[s]],
           summary[6 * (s * COMMANDS + plain[s]) + 5]);
    if (safe[s] < 0) {
      printf("no command meets the floor %.3f\n", limit[5]);
      bad += st[s] != HMPC_SELECT_NONE;
    } else {
      printf("masked winner %d, vx %+.2f m/s (headroom %.3f, score %.4f)\n", safe[s], v_cmd[safe[s]],
             summary[6 * (s * COMMANDS + safe[s]) + 5], score[s]);
      bad += HMPC_STATUS_CODE(st[s]) != HMPC_S_OK || !(summary[6 * (s * COMMANDS + safe[s]) + 5] >= limit[5]);
    }
  }
  bad += changed < 1;
  printf("safe command of %d states x %d commands: %d problems\n", STATES, COMMANDS, bad);
  dev_free(d_penalty);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
