/* How does a loss over the forces change when the reference trajectory, the weights or Alpha_K are tuned?  One launch behind a solve
 * (hmpc_solve_adjoint) turns a seed dL/du over the whole force trajectory into dL/dx0, dL/dX_d, dL/dweights and dL/dAlpha_K of the QP that
 * was solved, with its linearisation and its active limits frozen -- instead of 12 + 12 h + 6 NC extra solves by finite differences.
 * Here: a standing batch is solved, the loss is "step-0 vertical force of the left foot" (the seed is 1 on that entry), and grad_traj is
 * printed; then the reference height of step 3 is raised by 5 mm, the batch is re-solved, and the predicted change of the loss is printed
 * beside the actual one.
 * The seed lives in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/loss_gradient.c -Lhector_simulation_amd -lhector_mpc_hip -lm -ldl -Wl,-rpath,$PWD/hector_simulation_amd -o loss_gradient
 * (-ldl: dlsym, for a C library that still keeps it apart) */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 4, U = 12, STEP = 3, ENTRY = 5 /* the reference height */, FZ_LEFT = 2 };

static void pack(unsigned char *rec, double vx_body, double tilt, double dz_ref) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {vx_body, 0, 0}, w[3] = {0, 0, 0};
  double q[4] = {cos(tilt / 2), 0, sin(tilt / 2), 0}; /* pitched by `tilt` */
  double r[6] = {0.02, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0};
  int gait[2 * H];
  for (int i = 0; i < H; ++i) {
    traj[12 * i + ENTRY] = 0.55 + (i == STEP ? dz_ref : 0.0);
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
  double *d_seed = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_seed, sizeof(double) * N * H * U) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride), *moved = (unsigned char *)calloc(N, stride);
  const double v_body[N] = {-0.2, 0.0, 0.1, 0.3}, dz = 5e-3;
  static float before[N * U * H], after[N * U * H];
  for (int i = 0; i < N; ++i) {
    pack(recs + i * stride, v_body[i], 0.02 * i, 0.0);
    pack(moved + i * stride, v_body[i], 0.02 * i, dz);
  }
  /* dz as the records hold it: the difference of the two binary32 entries */
  float z0, z1;
  memcpy(&z0, recs + 4 * (54 + 12 * STEP + ENTRY), 4), memcpy(&z1, moved + 4 * (54 + 12 * STEP + ENTRY), 4);
  const double dz32 = (double)z1 - (double)z0;
  static double seed[N * H * U], grad_x0[N * 13], grad_traj[N * H * 12], grad_w[N * 12], grad_a[N * U], summary[N * 2];
  for (int i = 0; i < N; ++i) seed[(size_t)i * H * U + FZ_LEFT] = 1.0; /* L = u_0[Fz of the left foot] */
  uint32_t st[N], st2[N];
  int bad = 0;
  bad += hmpc_solve_adjoint(h, d_seed, NULL) != HMPC_E_ARG; /* no solve yet: refused, nothing enqueued */
  rc = dev_memcpy(d_seed, seed, sizeof(seed), 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, before, st);
  bad += hmpc_solve_adjoint(h, NULL, NULL) != HMPC_E_ARG; /* a NULL seed: refused */
  if (rc == HMPC_OK) rc = hmpc_solve_adjoint(h, d_seed, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_adjoint(h, grad_x0, grad_traj, grad_w, grad_a, NULL, summary);
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, moved, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, after, st2);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  bad += hmpc_download_adjoint(h, grad_x0, NULL, NULL, NULL, NULL, NULL) != HMPC_E_ARG; /* a newer solve: the adjoint is stale */
  for (int i = 0; i < N; ++i) {
    const double *g = grad_traj + (size_t)i * H * 12;
    printf("robot %d (body at %+.2f m/s): dFz_left/d(reference height), N per m, steps 1 .. %d:", i, v_body[i], H);
    for (int j = 0; j < H; ++j) printf(" %.1f", g[12 * j + ENTRY]);
    const double predicted = g[12 * STEP + ENTRY] * dz32;
    const double actual = (double)after[(size_t)i * U * H + FZ_LEFT] - (double)before[(size_t)i * U * H + FZ_LEFT];
    printf("\n  Fz left %.3f N; reference height of step %d raised by %.1f mm: predicted %+.4f N, re-solved %+.4f N;  dFz/dvz %.2f N s/m, "
           "dFz/dw_z %.4f, dFz/dAlpha_K[Fz left] %.1f\n", before[(size_t)i * U * H + FZ_LEFT], STEP + 1, 1e3 * dz32, predicted, actual, grad_x0[13 * i + 11],
           grad_w[12 * i + 5], grad_a[U * i + FZ_LEFT]);
    bad += !(fabs(predicted - actual) <= 0.01 + 0.25 * fabs(actual)) || !(fabs(predicted) > 0.0) || !(summary[2 * i] > 0.0) ||
           HMPC_STATUS_CODE(st[i]) != HMPC_S_OK || HMPC_STATUS_CODE(st2[i]) != HMPC_S_OK;
  }
  printf("loss gradients of %d standing robots, reference height moved by 5 mm: %d problems\n", N, bad);
  dev_free(d_seed);
  hmpc_destroy(h);
  free(recs), free(moved);
  return bad == 0 ? 0 : 1;
}
