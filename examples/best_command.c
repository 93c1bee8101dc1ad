/* Which command should the robot execute?  A planner's inner loop on the device: a few robot states x a few candidate forward velocities
 * are solved as one command sweep (hmpc_solve_command_sweep: H assembled and inverted once per state), ONE more launch scores every
 * candidate with the model's own prediction (hmpc_predict_states) and ONE more picks, per state, the candidate of smallest
 * tracking + force cost (hmpc_sweep_select) -- the command the body can follow most cheaply -- and leaves its forces, status word and
 * predicted states in compact rows: nothing but one row per state has to come back.  (A planner with a term of its own -- the distance
 * of a candidate from the operator's command, an obstacle mask as NaN -- hands it in as device_penalty[batch]; a plain C program has no
 * device allocator, so this one passes NULL.)
 * Printed per state: the chosen command and the forward velocity the model predicts under it at the last horizon step; checked against
 * the host route the selection replaces (download every cost, argmin per state).
 *   gcc -std=c11 -Iinclude examples/best_command.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o best_command */
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

int main(void) {
  struct problem_setup ps = {0.04f, 0.25f, 500.f, H};
  hmpc_handle *h = NULL;
  int rc = hmpc_create(&h, &ps, N, 0);
  if (rc != HMPC_OK) {
    fprintf(stderr, "hmpc_create failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 2;
  }
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  const double v_body[STATES] = {-0.2, 0.0, 0.3}, v_cmd[COMMANDS] = {-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8};
  double cost[N * 2], score[STATES];
  int32_t index[STATES];
  uint32_t st[STATES];
  float states[STATES * H * 13];
  int bad = 0;

  /* records of one group (one state) differ in the reference trajectory only */
  for (int s = 0; s < STATES; ++s)
    for (int c = 0; c < COMMANDS; ++c) pack(recs + (size_t)(s * COMMANDS + c) * stride, v_body[s], v_cmd[c], 0.02 * s);
  rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve_command_sweep(h, COMMANDS, NULL);
  const int early = hmpc_sweep_select(h, COMMANDS, NULL, NULL); /* nothing predicted yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_predict_states(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_sweep_select(h, COMMANDS, NULL, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_selection(h, index, score, NULL, st, states);
  if (rc == HMPC_OK) rc = hmpc_download_prediction(h, NULL, cost); /* (only for the check below) */
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  bad += early != HMPC_E_ARG;
  for (int s = 0; s < STATES; ++s) {
    const int k = index[s];
    if (k < 0 || k >= COMMANDS) {
      printf("state %d (body at %+.2f m/s): no eligible command\n", s, v_body[s]);
      ++bad;
      continue;
    }
    const float *last = states + ((size_t)s * H + (H - 1)) * 13; /* x_H of the winner: rpy, position, angular velocity, velocity, g */
    bad += HMPC_STATUS_CODE(st[s]) != HMPC_S_OK || !(score[s] < INFINITY) || last[12] != 9.81f;
    int host_best = 0; /* the host route: argmin over the downloaded costs, lowest index first */
    for (int c = 1; c < COMMANDS; ++c) {
      const double *a = cost + 2 * (s * COMMANDS + c), *b = cost + 2 * (s * COMMANDS + host_best);
      if (a[0] + a[1] < b[0] + b[1]) host_best = c;
    }
    bad += k != host_best || score[s] != cost[2 * (s * COMMANDS + k)] + cost[2 * (s * COMMANDS + k) + 1];
    printf("state %d (body at %+.2f m/s): chosen command %d, vx %+.2f m/s (score %.4f) -> predicted vx at step %d %+.4f m/s\n", s, v_body[s], k,
           v_cmd[k], score[s], H, (double)last[9]);
  }
  printf("best command of %d states x %d commands: %d problems\n", STATES, COMMANDS, bad);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
