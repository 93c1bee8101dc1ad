// hmpc_model_adjoint.h -- the model gradients of the solve (hmpc_adjoint_model): from the direction `dir` that
// hmpc_solve_adjoint left, the gradients of the loss in the prediction model itself -- G_A = dL/dAcd, G_B = dL/dBcd -- and, chained
// through stage A2's B, in the foot positions r, the mass and the body inertia; everything BEHIND the assembly, as device functions
// over plain LDS arrays.  The kernels that assemble (hmpc_model_adjoint.hip) call model_adjoint_of_instance with what the solve kernel's
// own stage function left in LDS; tests/src/model_adjoint_on_host.cpp compiles this header for the CPU (one thread per lane) against a
// plain loop.
//
// With the active set frozen, dL/dtheta = dir' d(Hu + g)/dtheta.  For a theta that enters through A = Acd and B = Bcd only this is two
// costate chains and a sum of outer products: no Riccati pass, no H, nothing of the solver, and -- the constraint block not depending
// on r, mass or inertia -- no multipliers.
//
// Definition (fixed in include/hector_mpc.h; tests/model_adjoint_mirror.py restates it in numpy).  All binary64, every chain ascending
// from +0 by explicit fused multiply-adds; q2 = (w + w, 0); u_i the force buffer's step i, du_i = dir's.
//   Forward, x_0 = x0, dx_0 = 0, i = 0 .. h-1:
//     x_{i+1}[s]  = chain_k A[s][k] x_i[k] continued by chain_c B[s][c] u_i[c]         (as hmpc_predict_states and the adjoint have it)
//     dx_{i+1}[s] = chain_k A[s][k] dx_i[k] continued by chain_c B[s][c] du_i[c]       (the adjoint's chain, over the stored dir)
//   Backward, c_{h+1} = d_{h+1} = 0, j = h .. 1:
//     c_j[s] = fma(q2[s], x_j[s] - traj[12 (j-1) + s], chain_k A[k][s] c_{j+1}[k])     (s < 12; the chain alone for s = 12)
//     d_j[s] = fma(q2[s], dx_j[s],                     chain_k A[k][s] d_{j+1}[k])     (likewise)
//   Accumulation, one chain over i = 0 .. h-1 per entry, the c term first:
//     G_A[a][b] = chain_i ( c_{i+1}[a] dx_i[b] , d_{i+1}[a] x_i[b] )
//     G_B[a][c] = chain_i ( c_{i+1}[a] du_i[c] , d_{i+1}[a] u_i[c] )
//   Chain rules, with Mb[a][m] = B[6+a][3 NC + m] (the assembled dt Iinv), rc[k] the record's r[k NC + c] and cm_c = {0, -rc2, rc1; rc2,
//   0, -rc0; -rc1, rc0, 0} as stage A2 writes it (binary32, widened), R the binary32 quat_to_R of the record's quaternion, widened:
//     T_c[m][b]   = chain_a Mb[a][m] G_B[6+a][3c+b]                                    (a < 3)
//     grad_r[c]   = (T_c[2][1] - T_c[1][2], T_c[0][2] - T_c[2][0], T_c[1][0] - T_c[0][1])
//     grad_mass   = 0 - ((+0 + G_B[9][0] + G_B[10][1] + G_B[11][2] + G_B[9][3] + ...  c ascending, a ascending) * B[9][0]) / mass
//     Gam[a][m]   = over c ascending: acc + G_B[6+a][3 NC + 3c + m], then chain_b G_B[6+a][3c+b] cm_c[m][b]   (b < 3; zeros included)
//     w_k[a]      = chain_m Mb[a][m] R[m][k];  t_k[a] = chain_m Gam[a][m] w_k[m];  grad_inertia[k] = 0 - (chain_a w_k[a] t_k[a]) / dt
//   costate = (c_1, d_1).  Gravity needs nothing new: it is x0[12], whose gradient is the adjoint's grad_x0[12].
// Every loop's trip count is fixed by (h, NC): nothing iterates on data, so NaN input ends like any other.
// Mapping: forward pass x on lanes 64 .. 76, dx on lanes 0 .. 12, one barrier per step; backward pass c on lanes 0 .. 12, d on lanes
// 13 .. 25, one barrier per step; accumulation one entry per lane and round (at most four rounds of NT = 128), no barrier inside; chain
// rules on lanes 0 .. NC-1 (r), 64 (mass), 65 .. 67 (inertia).  No atomics, no inline assembly, no matrix cores.
#pragma once
#include <hip/hip_runtime.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT

namespace hmpc {
constexpr int MADJ_NT = DERIVED_NT;     // lanes of the workgroup
constexpr int MADJ_PARAMS = 4;   // grad_params: mass, inertia 0 .. 2
constexpr int MADJ_COSTATE = 26; // costate: c_1[13], d_1[13]

// what model_adjoint_of_instance keeps of its inputs (LDS, or any memory all lanes see); filled by its first phase
template <int NC, int HMAX>
struct ModelAdjointKeep {
  static constexpr int U = 6 * NC;
  double A[169], B[13 * U], q2[13];
  double du[HMAX * U];  // dir
  float traj[12 * HMAX], x0[16], r[3 * NC], R[9];
};

// the passes' arrays; may overlay the binary32 inputs of model_adjoint_of_instance but u, which are not read again once the first phase
// has ended.  c and d hold rows 1 .. h+1 at 13 (j - 1).
template <int NC, int HMAX>
struct ModelAdjointWork {
  static constexpr int U = 6 * NC;
  double x[(HMAX + 1) * 13], dx[(HMAX + 1) * 13], c[(HMAX + 1) * 13], d[(HMAX + 1) * 13];
  double GA[169], GB[13 * U];
  double gr[3 * NC], gp[MADJ_PARAMS];
};

// The model gradients of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): x0[13], Acd[13][13],
// Bcd[13][6 NC], W[12], traj[12 h], r[3 NC] in the record's order [axis][contact], R[9] (quat_to_R of the record's quaternion), u[h][6 NC];
// dir[h][6 NC] (any memory); dt, mass.  Out: gA[13][13], gB[13][6 NC], gr[3][NC], gp[4], costate[2][13] (any may be null).  Every lane of
// the workgroup calls it.
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void model_adjoint_of_instance(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj,
                                                          const float *r, const float *R, const float *u, const double *dir, const int h,
                                                          const double dt, const double mass, ModelAdjointKeep<NC, HMAX> &Kp,
                                                          ModelAdjointWork<NC, HMAX> &Wk, double *gA, double *gB, double *gr, double *gp,
                                                          double *costate) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  static_assert(169 + 13 * U <= 4 * NT, "at most four entries of G_A, G_B per lane");
  // ---- first phase: what the passes read of the inputs, widened
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < 13) Kp.x0[tid] = x0[tid];
  if (tid >= 32 && tid < 32 + 3 * NC) Kp.r[tid - 32] = r[tid - 32];
  if (tid >= 64 && tid < 64 + 9) Kp.R[tid - 64] = R[tid - 64];
  for (int t = tid; t < 12 * h; t += NT) Kp.traj[t] = traj[t];
  for (int t = tid; t < U * h; t += NT) Kp.du[t] = dir[t];
  __syncthreads();  // the binary32 inputs but u are not read below: Wk may take their place
  const double *A = Kp.A, *B = Kp.B;
  // ---- forward pass
  if (tid < 13) Wk.dx[tid] = 0.0, Wk.x[tid] = (double)Kp.x0[tid];
  if (tid < 26) (tid < 13 ? Wk.c : Wk.d)[13 * h + tid % 13] = 0.0;  // c_{h+1} = d_{h+1} = 0
  __syncthreads();
  for (int i = 0; i < h; ++i) {
    if (tid < 13) {  // dx_{i+1} = A dx_i + B du_i
      const double *dxi = Wk.dx + 13 * i, *du = Kp.du + U * i;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[tid * 13 + k], dxi[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma(B[tid * U + c], du[c], acc);
      Wk.dx[13 * (i + 1) + tid] = acc;
    } else if (tid >= 64 && tid < 64 + 13) {  // x_{i+1}, as hmpc_predict_states has it
      const int s = tid - 64;
      const double *xi = Wk.x + 13 * i;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[s * 13 + k], xi[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma(B[s * U + c], (double)u[U * i + c], acc);
      Wk.x[13 * (i + 1) + s] = acc;
    }
    __syncthreads();
  }
  // ---- backward pass: c on lanes 0 .. 12, d on lanes 13 .. 25
  for (int j = h; j >= 1; --j) {
    if (tid < 26) {
      const int s = tid % 13;
      const bool isc = tid < 13;
      double *v = isc ? Wk.c : Wk.d;
      const double *nx = v + 13 * j;  // row j+1
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[k * 13 + s], nx[k], acc);
      if (s < 12) {
        const double e = isc ? Wk.x[13 * j + s] - (double)Kp.traj[12 * (j - 1) + s] : Wk.dx[13 * j + s];
        acc = __builtin_fma(Kp.q2[s], e, acc);
      }
      v[13 * (j - 1) + s] = acc;
    }
    __syncthreads();
  }
  // ---- accumulation: one entry per lane and round, one chain over the steps
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    const int t = tid + NT * round;
    if (t < 169 + 13 * U) {
      const bool isA = t < 169;
      const int a = isA ? t / 13 : (t - 169) / U, b = isA ? t % 13 : (t - 169) % U;
      double acc = 0.0;
      for (int i = 0; i < h; ++i) {
        const double ci = Wk.c[13 * i + a], di = Wk.d[13 * i + a];  // c_{i+1}, d_{i+1}
        const double f0 = isA ? Wk.dx[13 * i + b] : Kp.du[U * i + b];
        const double f1 = isA ? Wk.x[13 * i + b] : (double)u[U * i + b];
        acc = __builtin_fma(ci, f0, acc);
        acc = __builtin_fma(di, f1, acc);
      }
      (isA ? Wk.GA : Wk.GB)[isA ? t : t - 169] = acc;
    }
  }
  __syncthreads();
  // ---- chain rules
  const double *GB = Wk.GB;
  const double *Mb = B + 6 * U + 3 * NC;  // Mb[a][m] = Mb[a * U + m]
  if (tid < NC) {  // grad_r of contact tid
    const int c = tid;
    double T[9];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) acc = __builtin_fma(Mb[a * U + m], GB[(6 + a) * U + 3 * c + b], acc);
        T[3 * m + b] = acc;
      }
    Wk.gr[0 * NC + c] = T[7] - T[5];
    Wk.gr[1 * NC + c] = T[2] - T[6];
    Wk.gr[2 * NC + c] = T[3] - T[1];
  } else if (tid == 64) {  // grad_mass
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int a = 0; a < 3; ++a) acc = acc + GB[(9 + a) * U + 3 * c + a];
    Wk.gp[0] = 0.0 - (acc * B[9 * U]) / mass;
  } else if (tid >= 65 && tid < 68) {  // grad_inertia[k]
    const int k = tid - 65;
    double Gam[9], w[3], tk[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float r0 = Kp.r[0 * NC + c], r1 = Kp.r[1 * NC + c], r2 = Kp.r[2 * NC + c];
          const float cm[9] = {0.0f, -r2, r1, r2, 0.0f, -r0, -r1, r0, 0.0f};
          acc = acc + GB[(6 + a) * U + 3 * NC + 3 * c + m];
#pragma unroll
          for (int b = 0; b < 3; ++b) acc = __builtin_fma(GB[(6 + a) * U + 3 * c + b], (double)cm[3 * m + b], acc);
        }
        Gam[3 * a + m] = acc;
      }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) acc = __builtin_fma(Mb[a * U + m], (double)Kp.R[3 * m + k], acc);
      w[a] = acc;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) acc = __builtin_fma(Gam[3 * a + m], w[m], acc);
      tk[a] = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) acc = __builtin_fma(w[a], tk[a], acc);
    Wk.gp[1 + k] = 0.0 - acc / dt;
  }
  __syncthreads();
  // ---- outputs, coalesced from LDS
  if (gA)
    for (int t = tid; t < 169; t += NT) gA[t] = Wk.GA[t];
  if (gB)
    for (int t = tid; t < 13 * U; t += NT) gB[t] = Wk.GB[t];
  if (gr && tid < 3 * NC) gr[tid] = Wk.gr[tid];
  if (gp && tid >= 32 && tid < 32 + MADJ_PARAMS) gp[tid - 32] = Wk.gp[tid - 32];
  if (costate && tid >= 64 && tid < 64 + MADJ_COSTATE) costate[tid - 64] = (tid - 64 < 13) ? Wk.c[tid - 64] : Wk.d[tid - 64 - 13];
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct ModelAdjointOut {
  double *grad_A, *grad_B, *grad_r, *grad_params, *costate;  // [batch][13][13], [batch][13][6 nc], [batch][3][nc], [batch][4], [batch][2][13]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, the robot
// constants, mu_inst) and `forces`; it reads dir[batch][h][6 nc] (what hmpc_solve_adjoint wrote), writes `out` and nothing else.  Shapes:
// derived_shape (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_model_adjoint(int nc, const KernelArgs &args, double mass, const double *dir, const ModelAdjointOut &out, hipStream_t stream);
}  // namespace hmpc
#endif
