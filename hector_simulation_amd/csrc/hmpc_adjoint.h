// hmpc_adjoint.h -- the adjoint of the solve (hmpc_solve_adjoint): the gradients of a scalar loss L(u) over the whole
// force trajectory in the state, the reference trajectory, the weights and Alpha_K, from the seed l = dL/du; everything BEHIND the assembly,
// as device functions over plain LDS arrays.  The kernels that assemble (hmpc_adjoint.hip) call adjoint_of_instance with what the solve
// kernel's own stage function left in LDS; tests/src/adjoint_on_host.cpp compiles this header for the CPU (one thread per lane) against a
// plain loop.
//
// With the active set of the solved QP frozen the MPC is an equality-constrained LQ problem, and l' du*/dtheta = dir' d(Hu + g)/dtheta with
// dir = -Z (Z'HZ)^-1 Z' l the minimiser of the same LQ problem under the linear force cost l: the matrices of the gains' Riccati recursion
// (hmpc_feedback.h) and one vector recursion next to them.
//
// Definition (fixed in include/hector_mpc.h; tests/adjoint_mirror.py restates it in numpy).  Slacks, stance rule, active set, Z_i and the
// matrix backward pass (PA, PB, W, G, the Cholesky factor, X, S_i, K_i, M_i, P_i; M_0 as well) are hmpc_feedback.h's, the same code.  Per
// step i = h-1 .. 0, with p = p_{i+1} (p_h = 0), l_i the seed of step i, all binary64, every chain ascending from +0:
//   v[c]   = l_i[c] + chain_k B[k][c] p[k]                                        (k < 13)
//   y[a]   = chain_k Z_i[k][a] v[k]              over the six rows of column a's contact; then L y' = y, L' y'' = y' with the chains of X
//   k_i[c] = 0 - chain_b Z_i[c][b] y''[b]        over the columns of c's contact; exactly 0 when r_i = 0
//   p_i[s] = chain_k M_i[k][s] p[k] (k < 13) continued by chain_c K_i[c][s] l_i[c] (c < U)
// Forward, dx_0 = 0, x_0 = x0:  du_i[c] = (chain_s K_i[c][s] dx_i[s]) + k_i[c];  dx_{i+1}[s] = chain_k A[s][k] dx_i[k] continued by
//   chain_c B[s][c] du_i[c];  x_{i+1} as hmpc_predict_states has it (the same two chains over x_i and u_i).
// Outputs: grad_x0 = p_0;  grad_traj[j-1][s] = 0 - q2[s] dx_j[s];  grad_weights[s] = chain_j (e + e) dx_j[s], e = x_j[s] - traj[12 (j-1) + s],
//   j = 1 .. h;  grad_alpha[c] = chain_i (u_i[c] + u_i[c]) du_i[c];  dir = du;  summary[0] = the gains' pivot minimum, summary[1] = max |dir|
//   (NaN counting as +inf).
// Every loop's trip count is fixed by (h, NC) and the number of held vectors: nothing iterates on data.
// Mapping: as the gains' (one output entry per lane and pass, a barrier between dependent products).  The vector recursion rides in the
// matrix passes' spare lanes: v beside PA / PB, y beside W / X, the triangular solves of y on lane 13 beside the thirteen columns of X,
// k_i beside S, p_i beside P_i -- no barrier of its own.  K_i and k_i of every step stay in LDS (they take the place of the gains' M_1 ..
// M_{h-1} and Psi; du_i overwrites k_i); the forward pass' arrays overlay the backward pass' matrices.  No atomics, no inline assembly.
//
// The matrix step is the gains' own: riccati_gain_step / riccati_cost_step of hmpc_feedback.h, compiled here with the vector recursion
// switched on (the gains' kernels are the same machine code as before the step was factored out: profiles/r20/README.md).
#pragma once
#include "hmpc_feedback.h"

namespace hmpc {
constexpr int ADJ_SUMMARY = 2;

// what adjoint_of_instance keeps from its first phase beside FeedbackKeep (LDS, or any memory all lanes see)
template <int NC, int HMAX>
struct AdjointKeep {
  double ell[6 * NC * HMAX];  // the seed
  float traj[12 * HMAX], x0[16];
};

// scratch of the backward and the forward pass; may overlay the binary32 inputs of adjoint_of_instance, which are not read again once the
// first phase has ended
template <int NC, int HMAX>
struct AdjointWork {
  static constexpr int U = 6 * NC;
  double K[HMAX * U * 13];  // K_0 .. K_{h-1}
  double k[HMAX * U];       // k_i, then du_i
  union {
    struct {
      double P[169], PA[169], M[169], PB[13 * U];
      double W[U * U], WZ[U * U], G[U * U], Ld[U], piv[U];
      double X[U * 13], S[U * 13], y[U], v[U], p[2][16];
    } b;  // the backward pass
    struct {
      double x[(HMAX + 1) * 13], dx[(HMAX + 1) * 13], red[FB_NT], pivmin;
    } f;  // the forward pass
  } o;
};

// The adjoint of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): x0[13], Acd[13][13], Bcd[13][6 NC],
// W[12], traj[12 h], alpha[6 NC], Fc[8 NC][6 NC], u[h][6 NC], gait[NC h] bytes, cap[NC]; seed[h][6 NC] (any memory).  Out: gx0[13], gtraj[h][12],
// gw[12], galpha[6 NC], dir[h][6 NC], summary[2].  Every lane of the workgroup calls it.  Wk may overlay the binary32 inputs but u.
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void adjoint_of_instance(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj,
                                                    const float *alpha, const float *Fc, const float *u, const unsigned char *gait,
                                                    const float *cap, const double *seed, const int h, const double act_tol,
                                                    FeedbackKeep<NC, HMAX> &Kp, AdjointKeep<NC, HMAX> &Ak, AdjointWork<NC, HMAX> &Wk,
                                                    double *gx0, double *gtraj, double *gw, double *galpha, double *dir, double *summary_out) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  // ---- first phase: what the passes need of the inputs, in binary64; slacks; free directions (as feedback_of_instance)
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < U) Kp.r2[tid] = (double)alpha[tid] + (double)alpha[tid];
  if (tid < 13) Ak.x0[tid] = x0[tid];
  for (int t = tid; t < 12 * h; t += NT) Ak.traj[t] = traj[t];
  for (int t = tid; t < U * h; t += NT) Ak.ell[t] = seed[t];
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, Kp.slack, Kp.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  for (int ls = tid; ls < NC * h; ls += NT)
    Kp.held[ls] = stance(cap[ls % NC], gait[ls]) ? (unsigned char)free_directions<NC>(Fc, ls % NC, Kp.slack + 10 * ls, act_tol, Kp.Z + 36 * ls)
                                                 : (unsigned char)6;
  __syncthreads();  // the binary32 inputs but u are not read below
  // ---- backward pass
  auto &Bk = Wk.o.b;
  double pivmin = 1.0;  // (lane 64's is the one that counts)
  for (int t = tid; t < 169; t += NT) Bk.P[t] = (t % 14 == 0) ? Kp.q2[t / 13] : 0.0;
  if (tid < 13) Bk.p[0][tid] = 0.0;
  __syncthreads();
  int cur = 0;
  for (int i = h - 1; i >= 0; --i) {  // the gains' matrix step (hmpc_feedback.h) with the vector recursion in its spare lanes
    double *Ki = Wk.K + 13 * U * i;
    const RiccatiVec vec{Ak.ell + U * i, Bk.p[cur], Bk.p[cur ^ 1], Wk.k + U * i};
    riccati_gain_step<NC, HMAX, NT, true>(Kp, Bk, i, Ki, pivmin, vec);
    __syncthreads();
    riccati_cost_step<NC, HMAX, NT, true>(Kp, Bk, Ki, Bk.M, i > 0, vec);  // (M_0 as well; P_0 is not formed)
    cur ^= 1;
  }
  if (gx0 && tid < 13) gx0[tid] = Bk.p[cur][tid];
  __syncthreads();  // the backward pass' matrices are dead: the forward pass' arrays take their place
  // ---- forward pass
  const double *A = Kp.A, *B = Kp.B;
  auto &Fw = Wk.o.f;
  if (tid < 13) Fw.dx[tid] = 0.0, Fw.x[tid] = (double)Ak.x0[tid];
  if (tid == 64) Fw.pivmin = pivmin;
  __syncthreads();
  for (int i = 0; i < h; ++i) {
    const double *dxi = Fw.dx + 13 * i, *xi = Fw.x + 13 * i;
    double *du = Wk.k + U * i;
    if (tid < U) {  // du_i = K_i dx_i + k_i
      const double *Kr = Wk.K + 13 * U * i + 13 * tid;
      double acc = 0.0;
#pragma unroll
      for (int s = 0; s < 13; ++s) acc = __builtin_fma(Kr[s], dxi[s], acc);
      du[tid] = acc + du[tid];
    } else if (tid >= 64 && tid < 64 + 13) {  // x_{i+1}, as hmpc_predict_states has it
      const int s = tid - 64;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[s * 13 + k], xi[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma(B[s * U + c], (double)u[U * i + c], acc);
      Fw.x[13 * (i + 1) + s] = acc;
    }
    __syncthreads();
    if (tid < 13) {  // dx_{i+1} = A dx_i + B du_i
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[tid * 13 + k], dxi[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma(B[tid * U + c], du[c], acc);
      Fw.dx[13 * (i + 1) + tid] = acc;
    }
    __syncthreads();
  }
  // ---- outputs
  double dmax = 0.0;
  for (int t = tid; t < U * h; t += NT) {
    const double dv = Wk.k[t], a = __builtin_fabs(dv), v = (a == a) ? a : margins_inf();
    if (dir) dir[t] = dv;
    dmax = (v > dmax) ? v : dmax;
  }
  Fw.red[tid] = dmax;
  if (gtraj)
    for (int t = tid; t < 12 * h; t += NT) gtraj[t] = 0.0 - Kp.q2[t % 12] * Fw.dx[13 * (t / 12 + 1) + t % 12];
  if (tid < 12) {
    double acc = 0.0;
    for (int j = 1; j <= h; ++j) {
      const double e = Fw.x[13 * j + tid] - (double)Ak.traj[12 * (j - 1) + tid];
      acc = __builtin_fma(e + e, Fw.dx[13 * j + tid], acc);
    }
    if (gw) gw[tid] = acc;
  } else if (tid >= 64 && tid < 64 + U) {
    const int c = tid - 64;
    double acc = 0.0;
    for (int i = 0; i < h; ++i) {
      const double uv = (double)u[U * i + c];
      acc = __builtin_fma(uv + uv, Wk.k[U * i + c], acc);
    }
    if (galpha) galpha[c] = acc;
  }
  __syncthreads();
  if (tid == 0 && summary_out) {
    double best = 0.0;
    for (int t = 0; t < NT; ++t) best = (Fw.red[t] > best) ? Fw.red[t] : best;
    summary_out[0] = Fw.pivmin, summary_out[1] = best;
  }
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct AdjointOut {
  double *grad_x0, *grad_traj, *grad_weights, *grad_alpha, *dir, *summary;  // [batch][13], [batch][h][12], [batch][12], [batch][6 nc], [batch][h][6 nc], [batch][2]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants, mu_inst) and `forces`; it reads seed[batch][h][6 nc], writes `out` and nothing else.  Shapes: derived_shape
// (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_adjoint(int nc, const KernelArgs &args, double act_tol, const double *seed, const AdjointOut &out, hipStream_t stream);
}  // namespace hmpc
#endif
