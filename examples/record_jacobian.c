/* The full Jacobian of the step-0 wrench in every float of the record, by TWO calls.  hmpc_solve_adjoint_multi runs the matrix backward
 * pass once for the twelve unit seeds e_c at step 0; hmpc_adjoint_chain_multi then runs, for every seed of it, the chain model gradients
 * -> limit gradients -> record gradients behind ONE record load, assembly, forward chain, active set and lambda: row c of d u_0 / d record
 * is slice c of its grad_record, bit for bit what examples/wrench_jacobian.c forms row by row with a selection and three launches each.
 * Here: four standing robots are solved, the twelve rows are formed, and the column "left foot's x position" is printed; its entry for
 * the vertical force of the left foot -- the number examples/wrench_jacobian.c prints -- is compared with re-solves that have the foot
 * moved by +-1 mm.
 * The seeds live in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/record_jacobian.c -Lhector_simulation_amd -lhector_mpc_hip -lm -ldl -Wl,-rpath,$PWD/hector_simulation_amd -o record_jacobian
 * (-ldl: dlsym, for a C library that still keeps it apart) */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

/* NREC: the floats of a two-contact record (54 fixed, 12 per step); RX_LEFT: where r[x][left foot] lies in it */
enum { H = 10, N = 4, NC = 2, U = 12, FZ_LEFT = 2, NREC = 54 + 12 * H, RX_LEFT = 13 };
#define STEP 1e-3
/* 2 x the largest error measured on an MI355X (profiles/r24/README.md), relative to max(1, max |force|) */
#define BOUND 2.6e-6

static const double V_BODY[N] = {-0.2, 0.0, 0.1, 0.3};

static float pack(unsigned char *rec, double vx_body, double tilt, double dx_left) {
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
  return (float)r[0];
}

typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);

/* the batch with the left foot moved by dx, solved; what the record holds of the foot's x (binary32) */
static int solve_moved(hmpc_handle *h, unsigned char *recs, size_t stride, double dx, float *forces, uint32_t *st, float *rx32) {
  for (int i = 0; i < N; ++i) rx32[i] = pack(recs + i * stride, V_BODY[i], 0.02 * i, dx);
  int rc = hmpc_upload_records(h, recs, N);
  if (rc == HMPC_OK) rc = hmpc_solve(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download(h, forces, st);
  return rc;
}

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
  double *d_seeds = NULL;
  const size_t slice = (size_t)N * H * U; /* doubles of one seed: [batch][h][U] */
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_seeds, sizeof(double) * U * slice) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  static float at[N * U * H], plus[N * U * H], minus[N * U * H], rx0[N], rxp[N], rxm[N];
  static double seeds[U * N * H * U], jac[U][N * NREC], params[U][N * 4], summary[U][N * 3];
  uint32_t st[N], stp[N], stm[N];
  for (int c = 0; c < U; ++c) /* seed c: e_c at step 0, for every robot */
    for (int i = 0; i < N; ++i) seeds[c * slice + (size_t)i * H * U + c] = 1.0;
  int bad = 0;
  rc = dev_memcpy(d_seeds, seeds, sizeof(seeds), 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  if (rc == HMPC_OK) rc = hmpc_set_certificate_tolerance(h, 1.5e-4); /* what the tolerance's rule gives for forces below 60 N */
  if (rc == HMPC_OK) rc = solve_moved(h, recs, stride, STEP, plus, stp, rxp);
  if (rc == HMPC_OK) rc = solve_moved(h, recs, stride, -STEP, minus, stm, rxm);
  bad += hmpc_adjoint_chain_multi(h, d_seeds, NULL) != HMPC_E_ARG; /* no multi-seed adjoint yet: refused */
  if (rc == HMPC_OK) rc = solve_moved(h, recs, stride, 0.0, at, st, rx0);
  if (rc == HMPC_OK) rc = hmpc_solve_adjoint_multi(h, d_seeds, U, NULL); /* call one: the matrix backward pass once for twelve seeds */
  bad += hmpc_adjoint_chain_multi(h, NULL, NULL) != HMPC_E_ARG;
  if (rc == HMPC_OK) rc = hmpc_adjoint_chain_multi(h, d_seeds, NULL); /* call two: model -> limits -> record of all twelve, the seeds passed again */
  const struct hmpc_adjoint_chain host = {.grad_record = &jac[0][0], .grad_params = &params[0][0], .limit_summary = &summary[0][0]};
  if (rc == HMPC_OK) rc = hmpc_download_adjoint_chain_multi(h, &host); /* [seed][robot][...]: row c of the Jacobian is slice c */
  const struct hmpc_adjoint_chain detail = {.grad_A = &jac[0][0]};
  bad += hmpc_download_adjoint_chain_multi(h, &detail) != HMPC_E_ARG; /* no buffer was given for grad_A: it was not written */
  bad += hmpc_select_adjoint_seed(h, 0) != HMPC_OK; /* the selection keeps working beside the chain ... */
  if (rc == HMPC_OK) rc = hmpc_download_adjoint_chain_multi(h, &host); /* ... and does not touch it */
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  static const char *NAME[U] = {"Fx left", "Fy left", "Fz left", "Fx right", "Fy right", "Fz right", "Mx left", "My left", "Mz left", "Mx right", "My right", "Mz right"};
  for (int i = 0; i < N; ++i) {
    double scale = 1.0;
    for (int t = 0; t < U * H; ++t) scale = fmax(scale, fabs((double)at[(size_t)i * U * H + t]));
    const double step = ((double)rxp[i] - (double)rxm[i]) / 2; /* the move as the solver sees it: a difference of binary32 values */
    printf("robot %d (body at %+.2f m/s): d u_0 / d (x of the left foot), N per m (N m per m), beside central differences of re-solves:\n", i, V_BODY[i]);
    for (int c = 0; c < U; ++c) {
      const double g = jac[c][(size_t)i * NREC + RX_LEFT];
      const double fd = ((double)plus[(size_t)i * U * H + c] - (double)minus[(size_t)i * U * H + c]) / (2 * step);
      printf("  %-8s %+10.4f  %+10.4f\n", NAME[c], g, fd);
    }
    const double pred = jac[FZ_LEFT][(size_t)i * NREC + RX_LEFT] * 2 * step;
    const double act = (double)plus[(size_t)i * U * H + FZ_LEFT] - (double)minus[(size_t)i * U * H + FZ_LEFT];
    const double err = fabs(pred - act) / scale;
    printf("  Fz left, the foot moved by +-%.3f mm: predicted %+.6f N, re-solved %+.6f N (error %.1e of the force scale, bound %.1e)\n", 1e3 * step, pred, act,
           err, BOUND);
    for (int c = 0; c < U; ++c) bad += !(summary[c][(size_t)i * 3 + 1] < 1e-6); /* the seeds passed again were the adjoint's */
    bad += !(err <= BOUND) || !(fabs(pred) > 0.0) || (double)rx0[i] != (double)(float)0.02 || HMPC_STATUS_CODE(st[i]) != HMPC_S_OK ||
           HMPC_STATUS_CODE(stp[i]) != HMPC_S_OK || HMPC_STATUS_CODE(stm[i]) != HMPC_S_OK;
  }
  printf("step-0 record Jacobian of %d standing robots from two calls, a foot moved by +-1 mm: %d problems\n", N, bad);
  dev_free(d_seeds);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
