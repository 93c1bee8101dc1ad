/* How does the left foot's load change when the body tilts, or when the feet turn?  One launch behind hmpc_solve_adjoint,
 * hmpc_adjoint_model and hmpc_adjoint_limits (hmpc_adjoint_record) chains their outputs through the assembly -- the quaternion -> Euler
 * angle map, Rb^-1(yaw, pitch), I_w^-1 = (R I_b R')^-1, the foot rotations, the rows of the constraint block -- and returns the gradient
 * of the same loss in every float of the packed record, the quaternion and the joint angles included: the total derivative in the
 * attitude, where grad_x0[0:3] alone is the partial one with the linearisation frozen.  By finite differences that is 4 + 10 more
 * solves, each of which moves H and every constraint row.
 * Here: a standing batch that is pitching (so that the feet's moment limits are active), the loss is the step-0 vertical force of the
 * left foot (the seed is 1 on that entry), and dL/dq and dL/d(joint angles) are printed beside re-solves with the body rolled by
 * +-1e-3 rad and with both hip-yaw joints turned by +-1e-3 rad.
 * The seed lives in device memory; a plain C program takes the allocator from the HIP runtime the library brought in.
 *   gcc -std=c11 -Iinclude examples/pose_gradient.c -Lhector_simulation_amd -lhector_mpc_hip -lm -ldl -Wl,-rpath,$PWD/hector_simulation_amd -o pose_gradient
 * (-ldl: dlsym, for a C library that still keeps it apart) */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hector_mpc.h"

/* NREC: the floats of a two-contact record (54 fixed, 12 per step); Q_AT, JA_AT: where its quaternion and joint angles start */
enum { H = 10, N = 4, NC = 2, U = 12, FZ_LEFT = 2, NREC = 54 + 12 * H, Q_AT = 6, JA_AT = 19 };
#define TILT 1e-3
/* the bounds of tests/pose_adjoint_mirror.py (2 x the error measured against the reference's qpOASES), relative to max(1, max |force|) */
#define BOUND_Q 1.524e-4
#define BOUND_JA 8.66e-7

static void pack(unsigned char *rec, double pitch_rate, double roll, double hip_yaw, float *q32, float *ja32) {
  double Q[12] = {100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1};
  double A[12] = {1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2};
  double p[3] = {0, 0, 0.55}, v[3] = {0, 0, 0}, w[3] = {0, pitch_rate, 0}, q[4] = {cos(roll / 2), sin(roll / 2), 0, 0};
  double r[6] = {0.02, -0.02, 0.06, -0.06, -0.55, -0.55}, ja[10] = {0}, traj[12 * H] = {0}; /* r[axis][contact] */
  int gait[2 * H];
  ja[0] = ja[5] = hip_yaw;
  for (int i = 0; i < H; ++i) {
    traj[12 * i + 5] = 0.55;
    gait[2 * i] = gait[2 * i + 1] = 1; /* double support */
  }
  for (int k = 0; k < 4; ++k) q32[k] = (float)q[k];
  for (int k = 0; k < 10; ++k) ja32[k] = (float)ja[k];
  hmpc_pack_record(rec, H, p, v, q, w, r, ja, 0.0, Q, traj, A, gait);
}

typedef int (*malloc_fn)(void **, size_t);
typedef int (*free_fn)(void *);
typedef int (*memcpy_fn)(void *, const void *, size_t, int);

static const double PITCH_RATE[N] = {-1.5, 0.8, 1.5, 2.5};

/* the batch with the body rolled and the hip-yaw joints turned, solved; what the record holds of q and the joint angles (binary32) */
static int solve_moved(hmpc_handle *h, unsigned char *recs, size_t stride, double roll, double hip_yaw, float *forces, uint32_t *st, float *q32, float *ja32) {
  for (int i = 0; i < N; ++i) pack(recs + i * stride, PITCH_RATE[i], roll, hip_yaw, q32 + 4 * i, ja32 + 10 * i);
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
  double *d_seed = NULL;
  if (!dev_malloc || !dev_free || !dev_memcpy || dev_malloc((void **)&d_seed, sizeof(double) * N * H * U) != 0) {
    fprintf(stderr, "no device allocator\n");
    return 2;
  }
  const size_t stride = hmpc_record_stride(H);
  unsigned char *recs = (unsigned char *)calloc(N, stride);
  static float at[N * U * H], up[N * U * H], down[N * U * H];
  static float q0[4 * N], qa[4 * N], qb[4 * N], j0[10 * N], ja[10 * N], jb[10 * N];
  static double seed[N * H * U], grad_record[N * NREC], grad_rpy[N * 3];
  for (int i = 0; i < N; ++i) seed[(size_t)i * H * U + FZ_LEFT] = 1.0; /* L = Fz of the left foot at step 0 */
  uint32_t st[N], st2[N], st3[N];
  int bad = 0;
  rc = dev_memcpy(d_seed, seed, sizeof(seed), 1 /* host to device */) == 0 ? HMPC_OK : HMPC_E_HIP;
  /* Which rows count as active.  The default tolerance, 1e-3, is derived for forces at the 500 N cap (8 x 500 N x 2^-24 x |row|_1); the
   * forces of this batch stay below 60 N, for which the same rule gives 1.2e-4.  It matters here because the Mx window is only 0.01 wide:
   * at step 8 robot 0's Mx sits 5.5e-4 inside it, the default would freeze that row as active, and the frozen-set gradient in the hip
   * yaw would be 0.26 % off the re-solve. */
  if (rc == HMPC_OK) rc = hmpc_set_certificate_tolerance(h, 1.5e-4);
  if (rc == HMPC_OK) rc = solve_moved(h, recs, stride, 0.0, 0.0, at, st, q0, j0);
  if (rc == HMPC_OK) rc = hmpc_solve_adjoint(h, d_seed, NULL);
  if (rc == HMPC_OK) rc = hmpc_adjoint_model(h, NULL);
  bad += hmpc_adjoint_record(h, NULL) != HMPC_E_ARG; /* no limit gradients yet: refused, nothing enqueued */
  if (rc == HMPC_OK) rc = hmpc_adjoint_limits(h, d_seed, NULL);
  if (rc == HMPC_OK) rc = hmpc_adjoint_record(h, NULL);
  if (rc == HMPC_OK) rc = hmpc_download_adjoint_record(h, grad_record, NULL, grad_rpy);
  if (rc != HMPC_OK) {
    fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
    return 1;
  }
  double fmax = 1.0; /* the scale of the bounds: max(1, max |force|) over the batch */
  for (size_t k = 0; k < (size_t)N * U * H; ++k) fmax = fabs((double)at[k]) > fmax ? fabs((double)at[k]) : fmax;
  int moved_q = 0, moved_ja = 0;
  for (int pass = 0; pass < 2; ++pass) { /* 0: the body rolled; 1: the hip-yaw joints turned */
    rc = solve_moved(h, recs, stride, pass == 0 ? TILT : 0.0, pass == 0 ? 0.0 : TILT, up, st2, qa, ja);
    if (pass == 0) bad += hmpc_download_adjoint_record(h, grad_record, NULL, NULL) != HMPC_E_ARG; /* a newer solve: the gradients are stale */
    if (rc == HMPC_OK) rc = solve_moved(h, recs, stride, pass == 0 ? -TILT : 0.0, pass == 0 ? 0.0 : -TILT, down, st3, qb, jb);
    if (rc != HMPC_OK) {
      fprintf(stderr, "failed (%d): %s\n", rc, hmpc_last_hip_error());
      return 1;
    }
    for (int i = 0; i < N; ++i) {
      const double *g = grad_record + (size_t)i * NREC;
      double pred = 0.0; /* the move as the solver sees it: differences of binary32 values */
      if (pass == 0)
        for (int k = 0; k < 4; ++k) pred += g[Q_AT + k] * ((double)qa[4 * i + k] - (double)qb[4 * i + k]);
      else
        for (int k = 0; k < 10; ++k) pred += g[JA_AT + k] * ((double)ja[10 * i + k] - (double)jb[10 * i + k]);
      const double act = (double)up[(size_t)i * U * H + FZ_LEFT] - (double)down[(size_t)i * U * H + FZ_LEFT];
      const double err = fabs(pred - act) / fmax;
      if (pass == 0) {
        printf("robot %d (pitching at %+.1f rad/s): Fz left %+.3f N; dL/dq (%+.3f %+.3f %+.3f %+.3f) N, dL/drpy (%+.3f %+.3f %+.3f) N/rad\n",
               i, PITCH_RATE[i], (double)at[(size_t)i * U * H + FZ_LEFT], g[Q_AT], g[Q_AT + 1], g[Q_AT + 2], g[Q_AT + 3], grad_rpy[3 * i], grad_rpy[3 * i + 1],
               grad_rpy[3 * i + 2]);
        printf("  rolled by +-%.0e rad: predicted %+.6f N, re-solved %+.6f N (error %.1e of the force scale, bound %.1e)\n", TILT, pred, act, err, BOUND_Q);
        moved_q += fabs(pred) > 0.0;
      } else {
        printf("robot %d: dL/d(joint angles) left (%+.4f %+.4f %+.4f x3), right (%+.4f %+.4f %+.4f x3) N/rad\n", i, g[JA_AT], g[JA_AT + 1], g[JA_AT + 2],
               g[JA_AT + 5], g[JA_AT + 6], g[JA_AT + 7]);
        printf("  hip yaw turned by +-%.0e rad: predicted %+.6f N, re-solved %+.6f N (error %.1e of the force scale, bound %.1e)\n", TILT, pred, act, err, BOUND_JA);
        moved_ja += fabs(pred) > 0.0;
      }
      bad += !(err <= (pass == 0 ? BOUND_Q : BOUND_JA)) || g[JA_AT + 2] != g[JA_AT + 3] || g[JA_AT + 2] != g[JA_AT + 4] || HMPC_STATUS_CODE(st[i]) != HMPC_S_OK ||
             HMPC_STATUS_CODE(st2[i]) != HMPC_S_OK || HMPC_STATUS_CODE(st3[i]) != HMPC_S_OK;
    }
  }
  bad += moved_q == 0 || moved_ja == 0; /* a batch without an active moment row would show nothing of the joint angles */
  printf("pose gradients of %d pitching standing robots beside re-solves under a %.0e rad tilt: %d problems\n", N, TILT, bad);
  dev_free(d_seed);
  hmpc_destroy(h);
  free(recs);
  return bad == 0 ? 0 : 1;
}
