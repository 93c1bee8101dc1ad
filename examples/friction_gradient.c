/* How much lateral force does a little more friction buy?  One launch behind hmpc_solve_adjoint (hmpc_adjoint_limits) turns the adjoint's
 * direction into the gradients of the same loss in what enters the QP through its limits -- the friction parameter mu, the foot lengths
 * lt and lh, the Fz caps -- with the active limits frozen: it forms the multipliers of the solved QP and of the adjoint problem on the
 * active rows, which the caller cannot get from the other outputs.  By finite differences that is 3 + NC more solves, each at a kink
 * whenever a limit is weakly active.
 * Here: a standing batch pushed sideways is solved on slippery ground (mu = 0.3), the loss is the sum of the step-0 lateral forces of
 * both feet (the seed is 1 on those two entries), and grad_mu is printed beside a re-solve at mu (1 + 1e-3) and mu (1 - 1e-3).
 * The seed lives in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/friction_gradient.c -Lhector_simulation_amd -lhector_mpc_hip -lm -ldl -Wl,-rpath,$PWD/hector_simulation_amd -o friction_gradient
 * (-ldl: dlsym, for a C library that still keeps it apart) */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

enum { H = 10, N = 4, NC = 2, U = 12, FY_LEFT = 1, FY_RIGHT = 4 };

static void pack(unsigned char *rec, double vy_body) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {0, vy_body, 0}, w[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0};
  double r[6] = {0.02, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0}; /* r[axis][contact] */
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

static double lateral(const float *forces, int i) { return (double)forces[(size_t)i * U * H + FY_LEFT] + (double)forces[(size_t)i * U * H + FY_RIGHT]; }

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
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  const double v_body[N] = {-0.6, 0.2, 0.5, 0.9};
  static float at[N * U * H], up[N * U * H], down[N * U * H];
  for (int i = 0; i < N; ++i) pack(recs + i * stride, v_body[i]);
  struct hmpc_params par, par_up, par_down;
  hmpc_default_params(&par);
  par.mu = 0.3f;
  par_up = par_down = par;
  par_up.mu = (float)(0.3 * (1.0 + 1e-3)), par_down.mu = (float)(0.3 * (1.0 - 1e-3));
  const double dmu32 = (double)par_up.mu - (double)par_down.mu; /* the move as the solver sees it: a difference of binary32 values */
  static double seed[N * H * U], grad_limits[N * (3 + NC)], summary[N * 3];
  for (int i = 0; i < N; ++i) seed[(size_t)i * H * U + FY_LEFT] = seed[(size_t)i * H * U + FY_RIGHT] = 1.0; /* L = Fy left + Fy right at step 0 */
  uint32_t st[N], st2[N], st3[N];
  int bad = 0;
  rc = dev_memcpy(d_seed, seed, sizeof(seed), 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_set_params(h, &par);
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, at, st);
  bad += hmpc_adjoint_limits(h, d_seed, NULL) != HMPC_E_ARG; /* no adjoint yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_solve_adjoint(h, d_seed, NULL);
  bad += hmpc_adjoint_limits(h, NULL, NULL) != HMPC_E_ARG; /* the seed is passed again */
  if (rc == HMPC_OK) rc = hmpc_adjoint_limits(h, d_seed, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_adjoint_limits(h, grad_limits, NULL, NULL, NULL, NULL, summary);
  if (rc == HMPC_OK) rc = hmpc_set_params(h, &par_up); /* the same batch on slightly rougher ground */
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, up, st2);
  bad += hmpc_download_adjoint_limits(h, grad_limits, NULL, NULL, NULL, NULL, NULL) != HMPC_E_ARG; /* a newer solve: the gradients are stale */
  if (rc == HMPC_OK) rc = hmpc_set_params(h, &par_down); /* and on slightly smoother ground */
  if (rc == HMPC_OK) rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, down, st3);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  int moved = 0;
  for (int i = 0; i < N; ++i) {
    const double *g = grad_limits + (size_t)i * (3 + NC);
    const double pred = g[0] * dmu32, act = lateral(up, i) - lateral(down, i);
    printf("robot %d (pushed at %+.2f m/s): lateral force %+.3f N; dL/dmu %+.4f N, dL/dlt %+.4f, dL/dlh %+.4f N/m, dL/dcap (%+.5f %+.5f); seed check %.1e\n", i,
           v_body[i], lateral(at, i), g[0], g[1], g[2], g[3], g[4], summary[3 * i + 1]);
    printf("  mu moved by %.6f: predicted %+.6f N, re-solved %+.6f N\n", dmu32, pred, act);
    moved += fabs(g[0]) > 0.0;
    bad += !(fabs(pred - act) <= 0.002 + 0.25 * fabs(act)) || !(summary[3 * i + 1] <= 1e-9) || HMPC_STATUS_CODE(st[i]) != HMPC_S_OK ||
           HMPC_STATUS_CODE(st2[i]) != HMPC_S_OK || HMPC_STATUS_CODE(st3[i]) != HMPC_S_OK;
  }
  bad += moved == 0; /* a batch without an active friction row would show nothing */
  printf("friction gradients of %d pushed standing robots beside re-solves at mu (1 +- 1e-3): %d problems\n", N, bad);
  dev_free(d_seed);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
