/* What should the robot push with between two MPC ticks?  The reference applies the forces of the last solve until the next one; feedback
 * MPC applies u_0 + K (x - x_0) at sensor rate.  One launch behind a solve (hmpc_feedback_gains) gives K_0 = du_0/dx_0 and du_0/dX_d of
 * the QP that was solved, with its linearisation and its active limits frozen -- a Riccati recursion over the prediction model, nothing of
 * the solver in it; one small launch (hmpc_first_order_wrench) applies them to records that hold the same robots a moment later.
 * Here: a standing batch is solved, every robot's velocity is nudged by 1 mm/s, and the first-order wrench is printed beside step 0 of a
 * re-solve of the nudged records.  Identical records must return step 0 of the force buffer bit for bit.
 * The records live in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/feedback_gain.c -Lhector_simulation_amd -lhector_mpc_hip -lm -Wl,-rpath,$PWD/hector_simulation_amd -o feedback_gain */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 4 };

static void pack(unsigned char *rec, double vx_body, double vz_body, double tilt) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {vx_body, 0, vz_body}, w[3] = {0, 0, 0};
  double q[4] = {cos(tilt / 2), 0, sin(tilt / 2), 0}; /* pitched by `tilt` */
  double r[6] = {0.02, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0};
  int gait[2 * H];
  for (int i = 0; i < H; ++i) {
    traj[12 * i + 5] = 0.55;
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
  const size_t stride = hmpc_record_stride(H);
  unsigned char *d_new = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_new, N * stride) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  unsigned char *recs = (unsigned char *)calloc(N, stride), *nudged = (unsigned char *)calloc(N, stride);
  const double v_body[N] = {-0.2, 0.0, 0.1, 0.3}, nudge = 1e-3; /* 1 mm/s */
  for (int i = 0; i < N; ++i) {
    pack(recs + i * stride, v_body[i], 0.0, 0.02 * i);
    pack(nudged + i * stride, v_body[i] + nudge, -nudge, 0.02 * i);
  }
  static float forces[N * 12 * H], resolved[N * 12 * H], same[N * 12], wrench[N * 12];
  static double gain[N * 12 * 13], summary[N * 2], worst[N];
  static int32_t free_dims[N * H];
  uint32_t st[N];
  int bad = 0;
  bad += hmpc_feedback_gains(h, NULL) != HMPC_E_ARG; /* no solve yet: refused, nothing enqueued */
  rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, forces, st);
  bad += hmpc_first_order_wrench(h, d_new, NULL) != HMPC_E_ARG; /* no gains yet: refused */
  if (rc == HMPC_OK) rc = hmpc_feedback_gains(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_gains(h, gain, NULL, summary, free_dims);
  /* the same records: step 0 of the force buffer, bit for bit */
  if (rc == HMPC_OK) rc = dev_memcpy(d_new, recs, N * stride, 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_first_order_wrench(h, d_new, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_first_order(h, same, NULL);
  /* the nudged records: to first order ... */
  if (rc == HMPC_OK) rc = dev_memcpy(d_new, nudged, N * stride, 1) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_first_order_wrench(h, d_new, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_first_order(h, wrench, worst);
  /* ... and by a re-solve */
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, nudged, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, resolved, st);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  bad += hmpc_download_gains(h, gain, NULL, NULL, NULL) != HMPC_E_ARG; /* a newer solve: the gains are stale */
  for (int i = 0; i < N; ++i) {
    bad += memcmp(same + 12 * i, forces + (size_t)12 * H * i, 12 * sizeof(float)) != 0;
    double err = 0.0, moved = 0.0;
    for (int c = 0; c < 12; ++c) {
      const double e = fabs((double)wrench[12 * i + c] - (double)resolved[(size_t)12 * H * i + c]);
      const double m = fabs((double)resolved[(size_t)12 * H * i + c] - (double)forces[(size_t)12 * H * i + c]);
      err = e > err ? e : err, moved = m > moved ? m : moved;
    }
    printf("robot %d (body at %+.2f m/s): free directions at step 0: %d, max |K_0| %.1f N per unit state, smallest pivot ratio %.3f\n", i, v_body[i],
           free_dims[H * i], summary[2 * i + 1], summary[2 * i]);
    printf("  Fz left / right: solved %.3f / %.3f N, first order %.3f / %.3f N, re-solved %.3f / %.3f N\n", forces[(size_t)12 * H * i + 2],
           forces[(size_t)12 * H * i + 5], wrench[12 * i + 2], wrench[12 * i + 5], resolved[(size_t)12 * H * i + 2], resolved[(size_t)12 * H * i + 5]);
    printf("  the re-solve moved the wrench by %.4f N, the first-order update misses it by %.4f N; least step-0 slack %.2e\n", moved, err, worst[i]);
    bad += !(err <= 0.05 + 0.5 * moved) || !(summary[2 * i + 1] > 1.0) || !(summary[2 * i] > 0.0) || HMPC_STATUS_CODE(st[i]) != HMPC_S_OK;
  }
  printf("feedback gains of %d standing robots, nudged by 1 mm/s: %d problems\n", N, bad);
  dev_free(d_new);
  hmpc_destroy(h);
  free(recs), free(nudged);
  return bad == 0 ? 0 : 1;
}
