/* What would each command do to the body?  One command sweep -- a few robot states x a few commanded forward velocities, H assembled
 * and inverted once per state (hmpc_solve_command_sweep) -- then ONE more launch (hmpc_predict_states) returns the state trajectory the
 * MPC's own model predicts under every instance's optimal forces, and the tracking cost that optimum achieves: no host-side copy of
 * the reference's model (RobotState::set, ct_ss_mats, c2qp) needed.  Printed per state: commanded against predicted forward velocity at
 * the last horizon step, for each command.
 *   gcc -std=c11 -Iinclude examples/predicted_trajectory.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o predicted_trajectory */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "hector_mpc.h"

enum { H = 10, STATES = 3, COMMANDS = 4, N = STATES * COMMANDS };

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
  float *forces = (float *)malloc(sizeof(float) * N * 12 * H), *states = (float *)malloc(sizeof(float) * N * H * 13);
  double *cost = (double *)malloc(sizeof(double) * N * 2);
  uint32_t *st = (uint32_t *)malloc(sizeof(uint32_t) * N);
  const double v_body[STATES] = {-0.2, 0.0, 0.3}, v_cmd[COMMANDS] = {-0.4, 0.0, 0.3, 0.6};
  int bad = 0;

  /* records of one group (one state) differ in the reference trajectory only */
  for (int s = 0; s < STATES; ++s)
    for (int c = 0; c < COMMANDS; ++c) pack(recs + (size_t)(s * COMMANDS + c) * stride, v_body[s], v_cmd[c], 0.02 * s);
  rc = hmpc_upload_records(h, recs, N);
  const int early = hmpc_predict_states(h, NULL); /* nothing solved yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_solve_command_sweep(h, COMMANDS, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, forces, st); /* (runs the safe pass for anything flagged -- before predicting) */
  if (rc == HMPC_OK) rc = hmpc_predict_states(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_prediction(h, states, cost);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  bad += early != HMPC_E_ARG;
  for (int s = 0; s < STATES; ++s) {
    printf("state %d (body at %+.2f m/s):\n", s, v_body[s]);
    for (int c = 0; c < COMMANDS; ++c) {
      const int k = s * COMMANDS + c;
      const float *last = states + ((size_t)k * H + (H - 1)) * 13; /* x_H: rpy, position, angular velocity, velocity, g */
      bad += HMPC_STATUS_CODE(st[k]) != HMPC_S_OK;
      /* the model pulls the velocity from where the body is towards the command (it may overshoot to catch up with the commanded position) */
      const double gap0 = fabs(v_cmd[c] - v_body[s]), gap = fabs(v_cmd[c] - (double)last[9]);
      bad += (gap0 > 0.1 && !(gap < gap0)) || last[12] != 9.81f;
      printf("  commanded vx %+.2f m/s -> predicted vx at step %d %+.4f m/s, height %.4f m; cost: tracking %.4f + force %.4f\n", v_cmd[c], H,
             (double)last[9], (double)last[5], cost[2 * k], cost[2 * k + 1]);
    }
  }
  printf("prediction of %d states x %d commands: %d problems\n", STATES, COMMANDS, bad);
  hmpc_destroy(h);
  free(recs), free(forces), free(states), free(cost), free(st);
  return bad == 0 ? 0 : 1;
}
