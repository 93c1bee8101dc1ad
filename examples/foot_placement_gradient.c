/* Where should the foot go, and what does a payload do to the forces?  One launch behind hmpc_solve_adjoint (hmpc_adjoint_model) turns
 * the adjoint's direction into the gradients of the same loss in the foot positions r, the mass and the body inertia of the QP that was
 * solved, its active limits frozen -- instead of 3 NC + 4 extra solves by finite differences, which are noisy because r, the mass and
 * the inertia change H itself.
 * Here: a standing batch is solved, the loss is "step-0 vertical force of the left foot" (the seed is 1 on that entry), and grad_r and
 * grad_params are printed; then the left foot is moved forward by 1 mm and the batch re-solved, and the mass is raised by 1 % and the
 * batch re-solved, and the predicted changes of the loss are printed beside the actual ones.
 * The seed lives in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/foot_placement_gradient.c -Lhector_simulation_amd -lhector_mpc_hip -lm -ldl -Wl,-rpath,$PWD/hector_simulation_amd -o foot_placement_gradient
 * (-ldl: dlsym, for a C library that still keeps it apart) */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 4, NC = 2, U = 12, FZ_LEFT = 2 };

static void pack(unsigned char *rec, double vx_body, double tilt, double dx_left) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {vx_body, 0, 0}, w[3] = {0, 0, 0};
  double q[4] = {cos(tilt / 2), 0, sin(tilt / 2), 0}; /* pitched by `tilt` */
  double r[6] = {0.02 + dx_left, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0}; /* r[axis][contact] */
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
  double *d_seed = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_seed, sizeof(double) * N * H * U) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride), *moved = (unsigned char *)calloc(N, stride);
  const double v_body[N] = {-0.2, 0.0, 0.1, 0.3}, dx = 1e-3;
  static float before[N * U * H], foot[N * U * H], heavy[N * U * H];
  for (int i = 0; i < N; ++i) {
    pack(recs + i * stride, v_body[i], 0.02 * i, 0.0);
    pack(moved + i * stride, v_body[i], 0.02 * i, dx);
  }
  /* the moves as the solver sees them: differences of binary32 values */
  const double dx32 = (double)(float)(0.02 + dx) - (double)(float)0.02;
  struct hmpc_params par;
  hmpc_default_params(&par);
  const double mass0 = (double)par.mass;
  par.mass = (float)(1.01 * mass0);
  const double dm32 = (double)par.mass - mass0;
  static double seed[N * H * U], grad_A[N * 169], grad_B[N * 13 * U], grad_r[N * 3 * NC], grad_p[N * 4], costate[N * 26], grad_x0[N * 13];
  for (int i = 0; i < N; ++i) seed[(size_t)i * H * U + FZ_LEFT] = 1.0; /* L = u_0[Fz of the left foot] */
  uint32_t st[N], st2[N], st3[N];
  int bad = 0;
  rc = dev_memcpy(d_seed, seed, sizeof(seed), 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, before, st);
  bad += hmpc_adjoint_model(h, NULL) != HMPC_E_ARG; /* no adjoint yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_solve_adjoint(h, d_seed, NULL);
  if (rc == HMPC_OK) rc = hmpc_adjoint_model(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_adjoint(h, grad_x0, NULL, NULL, NULL, NULL, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_adjoint_model(h, grad_A, grad_B, grad_r, grad_p, costate);
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, moved, N); /* the left foot 1 mm further forward */
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, foot, st2);
  bad += hmpc_download_adjoint_model(h, NULL, NULL, grad_r, NULL, NULL) != HMPC_E_ARG; /* a newer solve: the gradients are stale */
  if (rc == HMPC_OK) rc = hmpc_set_params(h, &par); /* the first batch again, 1 % heavier */
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, heavy, st3);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  for (int i = 0; i < N; ++i) {
    const double *gr = grad_r + (size_t)i * 3 * NC, *gp = grad_p + 4 * i;
    const double f0 = (double)before[(size_t)i * U * H + FZ_LEFT];
    const double pred_r = gr[0 * NC + 0] * dx32, act_r = (double)foot[(size_t)i * U * H + FZ_LEFT] - f0;
    const double pred_m = gp[0] * dm32, act_m = (double)heavy[(size_t)i * U * H + FZ_LEFT] - f0;
    printf("robot %d (body at %+.2f m/s): Fz left %.3f N; dFz/dr, N per m: left (%.2f %.2f %.2f) right (%.2f %.2f %.2f); dFz/dmass %.4f N/kg, "
           "dFz/dinertia (%.3f %.3f %.3f); dFz/dgravity %.4f\n", i, v_body[i], f0, gr[0], gr[2], gr[4], gr[1], gr[3], gr[5], gp[0], gp[1], gp[2], gp[3],
           grad_x0[13 * i + 12]);
    printf("  left foot moved forward by %.3f mm: predicted %+.5f N, re-solved %+.5f N;  mass raised by %.4f kg: predicted %+.5f N, re-solved %+.5f N\n",
           1e3 * dx32, pred_r, act_r, dm32, pred_m, act_m);
    bad += !(fabs(pred_r - act_r) <= 0.01 + 0.25 * fabs(act_r)) || !(fabs(pred_m - act_m) <= 0.01 + 0.25 * fabs(act_m)) || !(fabs(pred_m) > 0.0) ||
           HMPC_STATUS_CODE(st[i]) != HMPC_S_OK || HMPC_STATUS_CODE(st2[i]) != HMPC_S_OK || HMPC_STATUS_CODE(st3[i]) != HMPC_S_OK;
  }
  printf("foot and payload gradients of %d standing robots, a foot moved by 1 mm and the mass raised by 1 %%: %d problems\n", N, bad);
  dev_free(d_seed);
  hmpc_destroy(h);
  free(recs), free(moved);
  return bad == 0 ? 0 : 1;
}
