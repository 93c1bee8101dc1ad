/* Which command keeps a pushed robot closest to where it should be over the next 0.2 s?  16 standing robots, each pushed sideways at the
 * centre of mass by a force of its own (0, 10, ... 150 N) for the whole window; eight candidate commands per robot -- sideways velocities
 * from -0.3 to +0.4 m/s --, each rolled out in closed loop for 40 MPC ticks: ONE call of hmpc_rollout_sweep_device expands 16 states x 8
 * commands into 128 instances, runs solve + plant step per tick, scores every instance's log (tracking + effort, a fallen instance masked)
 * and picks the cheapest candidate per robot, all on one stream; only 16 winners come back.  The push is the plant's
 * (hmpc_plant.device_ext_wrench, per expanded instance): the MPC does not know about it.
 * Printed per robot: the winning command, its score, and the joint torques to apply now (the winner's tick 0).
 *   gcc -std=c11 -Iinclude examples/rollout_sweep.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o rollout_sweep */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 16, K = 8, TICKS = 40, TICKS_PER_STEP = 8 };

typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);
typedef int (*sync_fn)(void);
enum { HOST_TO_DEVICE = 1, DEVICE_TO_HOST = 2 }; /* hipMemcpyKind */

int main(void) {
  struct problem_setup ps = {0.04f, 0.25f, 500.f, H};
  hmpc_handle *h = NULL;
  int rc = hmpc_create(&h, &ps, N * K, 0);
  if (rc != HMPC_OK) {
    fprintf(stderr, "hmpc_create failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 2;
  }
  malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
  free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
  memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
  sync_fn dev_sync = (sync_fn)dlsym(RTLD_DEFAULT, "hipDeviceSynchronize");
  /* one device allocation: ticks, commands, pushes, then the five arrays of the choice */
  static struct hmpc_tick_inputs ticks[N], ticks_after[N];
  static struct hmpc_command commands[N][K];
  static double push[N * K][6];
  const size_t o_cmd = sizeof(ticks), o_push = o_cmd + sizeof(commands), o_index = o_push + sizeof(push), o_score = o_index + N * sizeof(double),
               o_wrench = o_score + N * sizeof(double), o_tau = o_wrench + N * 12 * sizeof(float), o_summary = o_tau + N * 10 * sizeof(double),
               total = o_summary + N * 4 * sizeof(int32_t);
  char *d = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || !dev_sync || dev_malloc((void **)&d, total) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  /* the nominal standing tick: upright at 0.55 m, feet under the hips, both legs in stance for the whole horizon */
  const double pi = 3.14159265359, knee[5] = {0, 0, -0.3 * pi, 0.6 * pi, -0.3 * pi};
  const double vy[K] = {0.0, -0.1, 0.1, -0.2, 0.2, -0.3, 0.3, 0.4};
  memset(ticks, 0, sizeof(ticks));
  memset(commands, 0, sizeof(commands));
  memset(push, 0, sizeof(push));
  for (int i = 0; i < N; ++i) {
    struct hmpc_tick_inputs *t = &ticks[i];
    t->position[2] = 0.55;
    t->orientation[0] = 1.0;
    t->rBody[0] = t->rBody[4] = t->rBody[8] = 1.0;
    for (int k = 0; k < 10; ++k) t->leg_q[k] = knee[k % 5];
    t->pFoot[1] = 0.06, t->pFoot[4] = -0.06;
    t->gait_durations[0] = t->gait_durations[1] = H;
    for (int k = 0; k < K; ++k) {
      commands[i][k].v_des_robot[1] = vy[k];
      push[i * K + k][1] = 10.0 * i; /* N, world y: the same push for every candidate of robot i */
    }
  }
  rc = dev_memcpy(d, ticks, sizeof(ticks), HOST_TO_DEVICE) || dev_memcpy(d + o_cmd, commands, sizeof(commands), HOST_TO_DEVICE) ||
               dev_memcpy(d + o_push, push, sizeof(push), HOST_TO_DEVICE)
           ? HMPC_E_HIP
           : HMPC_OK;

  struct hmpc_plant plant;
  hmpc_default_plant(&plant);
  plant.flags = HMPC_PLANT_GYRO;
  plant.device_ext_wrench = (const double *)(d + o_push);
  struct hmpc_rollout_cost cost;
  hmpc_default_rollout_cost(&cost);
  struct hmpc_rollout_choice choice = {(int32_t *)(d + o_index), (double *)(d + o_score), (float *)(d + o_wrench), (double *)(d + o_tau),
                                       (int32_t *)(d + o_summary)};
  if (rc == HMPC_OK)
    rc = hmpc_rollout_sweep_device(h, d, N, (const struct hmpc_command *)(d + o_cmd), K, TICKS, 0.04, TICKS_PER_STEP, 0, &plant, &cost, NULL,
                                   &choice, NULL);
  static int32_t index[N], summary[N][4], all_summary[N * K][4];
  static double score[N], tau[N][10];
  if (rc == HMPC_OK) rc = hmpc_download_rollout(h, NULL, NULL, NULL, NULL, &all_summary[0][0]); /* (waits for the stream) */
  if (rc == HMPC_OK && (dev_sync() || dev_memcpy(index, d + o_index, sizeof(index), DEVICE_TO_HOST) ||
                        dev_memcpy(score, d + o_score, sizeof(score), DEVICE_TO_HOST) || dev_memcpy(tau, d + o_tau, sizeof(tau), DEVICE_TO_HOST) ||
                        dev_memcpy(summary, d + o_summary, sizeof(summary), DEVICE_TO_HOST) ||
                        dev_memcpy(ticks_after, d, sizeof(ticks_after), DEVICE_TO_HOST)))
    rc = HMPC_E_HIP;
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  int bad = 0, fallen = 0;
  for (int i = 0; i < N * K; ++i) fallen += all_summary[i][1] >= 0;
  for (int i = 0; i < N; ++i) {
    if (index[i] < 0) {
      printf("robot %2d, push %5.1f N: every candidate fell\n", i, 10.0 * i);
      bad += !(isinf(score[i]) && summary[i][1] == -1);
      for (int k = 0; k < K; ++k) bad += all_summary[i * K + k][1] < 0; /* ... then every one of them did */
      continue;
    }
    printf("robot %2d, push %5.1f N: best command vy = %+.1f m/s (candidate %d), score %.4f, hip torques now %+.2f %+.2f N m\n", i, 10.0 * i,
           vy[index[i]], index[i], score[i], tau[i][0], tau[i][5]);
    bad += index[i] >= K || !isfinite(score[i]);
    bad += summary[i][1] >= 0;                              /* a winner has not fallen */
    bad += memcmp(summary[i], all_summary[i * K + index[i]], sizeof(summary[i])) != 0; /* and its summary row is its own */
  }
  bad += memcmp(ticks, ticks_after, sizeof(ticks)) != 0; /* the robot states are not modified: the rollouts ran on the handle's copies */
  bad += index[0] < 0;                                   /* the robot nobody pushed has a winner */
  printf("%d of %d rollouts fell\n", fallen, N * K);
  printf("rollout sweep example: %d problems\n", bad);
  dev_free(d);
  hmpc_destroy(h);
  return bad == 0 ? 0 : 1;
}
