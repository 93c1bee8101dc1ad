/* How hard a sideways push does the standing controller survive?  64 standing robots, each pushed sideways at the centre of mass by a force
 * of its own (0, 10, 20, ... 630 N) for 10 MPC ticks (50 ms), then left alone for 60 more ticks: two calls of hmpc_rollout_device -- per
 * tick the solve and one launch of the plant step, on one stream, the tick structs never leaving the device -- instead of 70 host round
 * trips and a host-side copy of the plant.  The push is the plant's (hmpc_plant.device_ext_wrench): the MPC does not know about it.
 * Printed: the sideways velocity the push left behind, and how many robots hold their height and have not tipped over at the end.
 * The tick structs live in device memory; a plain C program takes allocator and copies from the HIP runtime the library brought into
 * the process.
 *   gcc -std=c11 -Iinclude examples/rollout.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o rollout */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 64, PUSH_TICKS = 10, FREE_TICKS = 60, TICKS_PER_STEP = 8 };

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
  void *d_ticks = NULL;
  double *d_push = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc(&d_ticks, N * sizeof(struct hmpc_tick_inputs)) != 0 ||
      dev_malloc((void **)&d_push, N * 6 * sizeof(double)) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  /* the nominal standing tick: upright at 0.55 m, feet under the hips, zero commands, both legs in stance for the whole horizon */
  static struct hmpc_tick_inputs ticks[N];
  static double push[N][6];
  const double pi = 3.14159265359, knee[5] = {0, 0, -0.3 * pi, 0.6 * pi, -0.3 * pi};
  memset(ticks, 0, sizeof(ticks));
  memset(push, 0, sizeof(push));
  for (int i = 0; i < N; ++i) {
    struct hmpc_tick_inputs *t = &ticks[i];
    t->position[2] = 0.55;
    t->orientation[0] = 1.0;
    t->rBody[0] = t->rBody[4] = t->rBody[8] = 1.0;
    for (int k = 0; k < 10; ++k) t->leg_q[k] = knee[k % 5];
    t->pFoot[1] = 0.06, t->pFoot[4] = -0.06;
    t->gait_durations[0] = t->gait_durations[1] = H;
    push[i][1] = 10.0 * i; /* N, world y */
  }
  rc = dev_memcpy(d_ticks, ticks, sizeof(ticks), HOST_TO_DEVICE) || dev_memcpy(d_push, push, sizeof(push), HOST_TO_DEVICE) ? HMPC_E_HIP : HMPC_OK;

  struct hmpc_plant plant;
  hmpc_default_plant(&plant);
  plant.flags = HMPC_PLANT_GYRO;
  static double state[N][PUSH_TICKS][12];
  static int32_t summary[N][4], summary_push[N][4];
  if (rc == HMPC_OK) rc = hmpc_set_tick_warm_start(h, 1, 0);
  plant.device_ext_wrench = d_push; /* pushed ... */
  if (rc == HMPC_OK) rc = hmpc_rollout_device(h, d_ticks, N, PUSH_TICKS, 0.04, TICKS_PER_STEP, 0, &plant, NULL, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_rollout(h, &state[0][0][0], NULL, NULL, NULL, &summary_push[0][0]);
  plant.device_ext_wrench = NULL; /* ... and left alone */
  if (rc == HMPC_OK) rc = hmpc_rollout_device(h, d_ticks, N, FREE_TICKS, 0.04, TICKS_PER_STEP, PUSH_TICKS, &plant, NULL, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_rollout(h, NULL, NULL, NULL, NULL, &summary[0][0]);
  if (rc == HMPC_OK && dev_memcpy(ticks, d_ticks, sizeof(ticks), DEVICE_TO_HOST) != 0) rc = HMPC_E_HIP;
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  int hold = 0, fallen = 0, bad = 0, strongest = -1;
  for (int i = 0; i < N; ++i) {
    const struct hmpc_tick_inputs *t = &ticks[i];
    const int down = (t->flags & HMPC_TICK_FALLEN) != 0, holds = !down && fabs(t->position[2] - 0.55) < 0.04;
    hold += holds, fallen += down;
    if (holds) strongest = i;
    bad += summary_push[i][0] + summary[i][0] != PUSH_TICKS + FREE_TICKS && !down; /* every tick of a robot that stands was stepped */
    bad += down != (summary_push[i][1] >= 0 || summary[i][1] >= 0);
    if (i % 8 == 0 || i == N - 1)
      printf("push %5.1f N: vy after the push %+.3f m/s; after %d ticks: height %.3f m, roll %+.3f rad, %s\n", push[i][1], state[i][PUSH_TICKS - 1][10],
             PUSH_TICKS + FREE_TICKS, t->position[2], t->rpy[0], down ? "fallen" : (holds ? "holds" : "off its height"));
  }
  bad += !(fabs(ticks[0].position[2] - 0.55) < 0.04) || (ticks[0].flags & HMPC_TICK_FALLEN); /* the robot nobody pushed stands */
  bad += !(state[N - 1][PUSH_TICKS - 1][10] > state[1][PUSH_TICKS - 1][10]);                 /* a harder push leaves more velocity */
  printf("%d of %d robots hold their height (%d fallen); the hardest push survived: %.1f N\n", hold, N, fallen, strongest >= 0 ? push[strongest][1] : 0.0);
  printf("rollout example: %d problems\n", bad);
  dev_free(d_ticks), dev_free(d_push);
  hmpc_destroy(h);
  return bad == 0 ? 0 : 1;
}
