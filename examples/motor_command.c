/* Ticks in, complete motor commands out.  16 walking robots, each commanded its own forward speed (0, 0.02, ... 0.30 m/s), for one gait
 * cycle of ticks (10 horizon steps x 8 ticks): per tick the solve with its stance torques (hmpc_tick_solve_device), the swing update
 * (hmpc_swing_legs_device: swing sub-phase, touchdown point, Bezier foot trajectory, inverse kinematics -- the reference's
 * SwingLegController.cpp) reading those torques, and the plant step, all on the device; the tick structs and the swing state never leave
 * it.  What a caller sends to the motors is struct hmpc_motor_cmd: tau, q, dq, Kp, Kd per joint -- a torque for a leg in stance (gains 0),
 * a joint-angle target with gains for a leg in swing.  (hmpc_tick_command_device is the first two calls in one; hmpc_set_rollout_swing puts
 * the swing update into hmpc_rollout_device.  This example keeps them apart to read the update's intermediate values every tick.)
 * Printed: the swing phase, the height of the Bezier target and qDes of the left leg of the robot commanded 0.2 m/s.
 *   gcc -std=c11 -Iinclude examples/motor_command.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o motor_command */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 16, TICKS_PER_STEP = 8, TICKS = H * TICKS_PER_STEP, SHOWN = 10 };

typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);
enum { HOST_TO_DEVICE = 1, DEVICE_TO_HOST = 2 }; /* hipMemcpyKind */

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
  void *d_ticks = NULL, *d_state = NULL, *d_cmd = NULL;
  double *d_tau = NULL, *d_wpd = NULL, *d_detail = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc(&d_ticks, N * sizeof(struct hmpc_tick_inputs)) != 0 ||
      dev_malloc(&d_state, N * sizeof(struct hmpc_swing_state)) != 0 || dev_malloc(&d_cmd, N * sizeof(struct hmpc_motor_cmd)) != 0 ||
      dev_malloc((void **)&d_tau, N * 10 * sizeof(double)) != 0 || dev_malloc((void **)&d_wpd, N * 2 * sizeof(double)) != 0 ||
      dev_malloc((void **)&d_detail, N * 2 * 16 * sizeof(double)) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  /* upright at 0.55 m, feet under the hips, walking: the left leg stands for the first five horizon steps, the right one for the last five */
  static struct hmpc_tick_inputs ticks[N];
  const double pi = 3.14159265359, knee[5] = {0, 0, -0.3 * pi, 0.6 * pi, -0.3 * pi};
  memset(ticks, 0, sizeof(ticks));
  for (int i = 0; i < N; ++i) {
    struct hmpc_tick_inputs *t = &ticks[i];
    t->position[2] = 0.55;
    t->orientation[0] = 1.0;
    t->rBody[0] = t->rBody[4] = t->rBody[8] = 1.0;
    for (int k = 0; k < 10; ++k) t->leg_q[k] = knee[k % 5];
    t->flags = HMPC_TICK_LEG_Q_MOTOR; /* raw motor angles */
    t->pFoot[1] = 0.06, t->pFoot[4] = -0.06;
    t->gait_offsets[1] = 5;
    t->gait_durations[0] = t->gait_durations[1] = 5;
    t->v_des_robot[0] = 0.02 * i;
  }
  rc = dev_memcpy(d_ticks, ticks, sizeof(ticks), HOST_TO_DEVICE) ? HMPC_E_HIP : HMPC_OK;

  struct hmpc_plant plant;
  hmpc_default_plant(&plant);
  plant.flags = HMPC_PLANT_GYRO | HMPC_PLANT_PLACE_FEET;
  struct hmpc_swing swing;
  hmpc_default_swing(&swing);
  swing.ticks_per_step = TICKS_PER_STEP;
  if (rc == HMPC_OK) rc = hmpc_swing_state_init_device(h, (struct hmpc_swing_state *)d_state, N, NULL);

  static double detail[N][2][16];
  static struct hmpc_motor_cmd cmd[N];
  int bad = 0, swing_ticks = 0;
  double top = 0.0;
  for (int k = 0; k < TICKS && rc == HMPC_OK; ++k) {
    swing.subtick = k % TICKS_PER_STEP;
    plant.advance_gait = (k + 1) % TICKS_PER_STEP == 0;
    rc = hmpc_tick_solve_device(h, d_ticks, N, 0.04, d_wpd, NULL, d_tau, NULL);
    if (rc == HMPC_OK)
      rc = hmpc_swing_legs_device(h, d_ticks, N, &swing, (struct hmpc_swing_state *)d_state, d_tau, (struct hmpc_motor_cmd *)d_cmd, d_detail, NULL);
    if (rc == HMPC_OK) rc = hmpc_plant_step_device(h, d_ticks, N, &plant, NULL, 0, NULL, d_wpd, NULL, NULL);
    /* (a plain copy on the null stream waits for the launches above: they were enqueued on it) */
    if (rc == HMPC_OK && (dev_memcpy(detail, d_detail, sizeof(detail), DEVICE_TO_HOST) != 0 || dev_memcpy(cmd, d_cmd, sizeof(cmd), DEVICE_TO_HOST) != 0))
      rc = HMPC_E_HIP;
    if (rc != HMPC_OK) break;
    const double phase = detail[SHOWN][0][0], height = detail[SHOWN][0][6];
    const struct hmpc_motor_cmd *c = &cmd[SHOWN];
    swing_ticks += phase > 0;
    if (height > top) top = height;
    for (int i = 0; i < N; ++i)
      for (int leg = 0; leg < 2; ++leg) {
        const int in_swing = detail[i][leg][0] > 0;
        for (int j = 0; j < 5; ++j) {
          bad += !isfinite(cmd[i].q[5 * leg + j]) || !isfinite(cmd[i].tau[5 * leg + j]);
          bad += cmd[i].Kp[5 * leg + j] != (in_swing ? swing.kp[j] : 0.0) || cmd[i].Kd[5 * leg + j] != (in_swing ? swing.kd[j] : 0.0);
        }
      }
    if (k % 4 == 0)
      printf("tick %2d: left leg swing phase %.3f, target height %.3f m, qDes %+.3f %+.3f %+.3f %+.3f %+.3f, Kp %g\n", k, phase, height, c->q[0],
             c->q[1], c->q[2], c->q[3], c->q[4], c->Kp[0]);
  }
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  /* the left leg swings for the second half of the cycle -- the reference's sub-phase runs over (0, 1]: the tick at exactly 0 is "not in
   * swing" and the first tick of the cycle is the swing's last, at sub-phase 1 -- and its target passes the apex, 0.15 m, at sub-phase 0.5 */
  bad += swing_ticks != TICKS / 2;
  bad += top != swing.height;
  printf("the left leg swings on %d of %d ticks; highest target %.3f m\n", swing_ticks, TICKS, top);
  printf("motor command example: %d problems\n", bad);
  dev_free(d_ticks), dev_free(d_state), dev_free(d_cmd), dev_free(d_tau), dev_free(d_wpd), dev_free(d_detail);
  hmpc_destroy(h);
  return bad == 0 ? 0 : 1;
}
