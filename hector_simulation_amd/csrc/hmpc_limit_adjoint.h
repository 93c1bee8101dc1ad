// hmpc_limit_adjoint.h -- the limit gradients of the solve (hmpc_adjoint_limits): from the direction `dir` that
// hmpc_solve_adjoint left and the seed it was made from, the gradients of the loss in what enters the QP through the constraint block --
// G_Fc = dL/dFc, dL/dbeta of the ten one-sided limits and, chained through the assembly's rows, dL/dmu, dL/dlt, dL/dlh and dL/dcap;
// everything BEHIND the assembly, as device functions over plain LDS arrays.  The kernels that assemble (hmpc_limit_adjoint.hip) call
// limit_adjoint_of_instance with what the solve kernel's own stage function left in LDS; tests/src/limit_adjoint_on_host.cpp compiles this
// header for the CPU (one thread per lane) against a plain loop.
//
// With the admitted active normals frozen the QP is min f(u) s.t. n_j'.v + beta_j' = s_j' (held) on every stance leg-step, stationarity
// reads grad f = sum lambda_j' n_j', and the adjoint problem's own stationarity rho = l + H dir = sum nu_j' n_j'.  Then
//   dL/dtheta = (what hmpc_solve_adjoint / hmpc_adjoint_model return) - sum lambda_j' (dn_j'/dtheta . dir) - sum nu_j' (dn_j'/dtheta . v + dbeta_j'/dtheta)
// so the gradient in a constraint row is two small triangular solves per leg-step against the adjoint's own orthonormal vectors.
//
// Definition (fixed in include/hector_mpc.h; tests/limit_adjoint_mirror.py restates it in numpy).  All binary64, every chain ascending
// from +0 by explicit fused multiply-adds; q2 = (w + w, 0), a2 = alpha + alpha; u_i the force buffer's step i, du_i = dir's, l_i the seed's.
//   x_j, dx_j, c_j, d_j                                as hmpc_model_adjoint.h has them, chain for chain
//   grad_i[k] = fma(a2[k], u_i[k],  chain_a B[a][k] c_{i+1}[a]);  hd_i[k] = fma(a2[k], du_i[k], chain_a B[a][k] d_{i+1}[a]);  rho = l + hd
//   slacks, stance rule: margins_of_instance (hmpc_margins.h); admitted rows j_0 < .. < j_{m-1} and q_0 .. q_{m-1}: admitted_normals
//   (hmpc_feedback.h), the decisions of free_directions
//   stance leg-step (i, c), n_b = sigma_{j_b} Fc[8 c + src(j_b)][cols(c)]:  T[a][b] = chain_k q_a[k] n_b[k] (a <= b),  y_a = chain_k q_a[k] rhs[k],
//     x_a = (y_a - chain_{b > a} T[a][b] x_b) / T[a][a] for a = m-1 .. 0;  rhs = grad_i[cols(c)] gives lambda_{j_a} = x_a, rhs = rho_i[cols(c)]
//     gives nu;  e[k] = rhs[k] - chain_{b < m} n_b[k] x_b.  Rows not admitted and swing leg-steps: exact zeros, no residual.
//   G[8 c + r][col_k] = one chain over i ascending and, inside a step, over the row's j' ascending (rows 4 and 7 serve two):
//     fma(0 - sigma_j' lambda_j', du_i[col_k], .), then fma(0 - sigma_j' nu_j', (double)u_i[col_k], .);  zeros outside cols(c)
//   grad_bound[i][c][j'] = 0 - nu_j'
//   grad_mu = over c ascending, from +0: + G[8c+1][3c] - G[8c][3c] + G[8c+3][3c+1] - G[8c+2][3c+1]
//   grad_lt = (chain_c chain_{k<3} G[8c+5][3c+k] (double)Fc[8c+5][3c+k]) / lt;  grad_lh the same over row 6 and lh (IEEE for a zero divisor)
//   grad_cap[c] = chain_i grad_bound[i][c][9] (double)(float)gait[NC i + c]
//   summary = max |e| of lambda, max |e| of nu over the stance leg-steps, max |G| (NaN counting as +inf; 0 with no candidate)
// Every loop's trip count is fixed by (h, NC) and the number of admitted normals (<= 6): nothing iterates on data.
// Mapping: the passes on the model adjoint's lanes (dx on 0 .. 12, x on 64 .. 76; c on 0 .. 12, d on 13 .. 25; one barrier per step);
// grad and rho one entry per lane and round; the NC h multiplier problems one per lane, each on the 36 doubles of its own slot of Q, the
// two solutions in registers; G one lane per non-zero entry (48 NC); the chain rules on lanes 0 .. 2 (mu, lt, lh) and 64 .. 64 + NC - 1
// (caps), the three maxima on lanes 32 .. 34.  No atomics, no inline assembly, no matrix cores.
#pragma once
#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_feedback.h"

namespace hmpc {
constexpr int LADJ_NT = DERIVED_NT;    // lanes of the workgroup
constexpr int LADJ_SUMMARY = 3;
constexpr int LADJ_SWING = 7;   // `held` of a swing leg-step (a stance leg-step admits 0 .. 6)

// what limit_adjoint_of_instance keeps of its inputs (LDS, or any memory all lanes see); filled by its first phase
template <int NC, int HMAX>
struct LimitAdjointKeep {
  static constexpr int U = 6 * NC;
  double A[169], B[13 * U], q2[13], a2[U];
  double du[HMAX * U], ell[HMAX * U];  // dir, the seed
  double slack[10 * NC * HMAX];
  double Q[36 * NC * HMAX];  // per leg-step: the admitted normals' orthonormal vectors
  MarginMin wave_min[LADJ_NT / 64][MARGIN_CLASSES];
  unsigned rows[NC * HMAX];  // per leg-step: nibble b = j_b
  float traj[12 * HMAX], x0[16], Fc[8 * NC * U];
  unsigned char held[NC * HMAX], gait[NC * HMAX];
};

// the passes' arrays and the staged outputs; may overlay the binary32 inputs of limit_adjoint_of_instance but u, which are not read again
// once the first phase has ended.  c and d hold rows 1 .. h+1 at 13 (j - 1).
template <int NC, int HMAX>
struct LimitAdjointWork {
  static constexpr int U = 6 * NC;
  double x[(HMAX + 1) * 13], dx[(HMAX + 1) * 13], c[(HMAX + 1) * 13], d[(HMAX + 1) * 13];
  double grad[HMAX * U], rho[HMAX * U];
  double lam[10 * NC * HMAX], nu[10 * NC * HMAX];
  double G[8 * NC * U], lim[3 + NC];
  double red[LADJ_SUMMARY][LADJ_NT], summary[LADJ_SUMMARY];
};

__device__ __forceinline__ double ladj_mag(const double v) {  // |v|, NaN counting as +inf
  const double a = __builtin_fabs(v);
  return (a == a) ? a : margins_inf();
}

// The limit gradients of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): x0[13], Acd[13][13],
// Bcd[13][6 NC], W[12], traj[12 h], alpha[6 NC], Fc[8 NC][6 NC], u[h][6 NC], gait[NC h] bytes, cap[NC]; dir[h][6 NC], seed[h][6 NC] (any
// memory); act_tol, lt, lh.  Out: glim[3 + NC], gFc[8 NC][6 NC], gbound[h][NC][10], lam_out, nu_out [h][NC][10], summary_out[3] (any may
// be null).  Every lane of the workgroup calls it.  Wk may overlay the binary32 inputs but u.
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void limit_adjoint_of_instance(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj,
                                                          const float *alpha, const float *Fc, const float *u, const unsigned char *gait,
                                                          const float *cap, const double *dir, const double *seed, const int h,
                                                          const double act_tol, const double lt, const double lh,
                                                          LimitAdjointKeep<NC, HMAX> &Kp, LimitAdjointWork<NC, HMAX> &Wk, double *glim,
                                                          double *gFc, double *gbound, double *lam_out, double *nu_out, double *summary_out) {
  constexpr int U = 6 * NC, C8 = 8 * NC;
  const int tid = threadIdx.x;
  static_assert(NT == LADJ_NT && 48 * NC <= 2 * NT && NC * HMAX <= NT && NC <= 3, "lane budget");
  // ---- first phase: what the passes read of the inputs, widened; slacks; admitted normals (as adjoint_of_instance)
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < U) Kp.a2[tid] = (double)alpha[tid] + (double)alpha[tid];
  if (tid < 13) Kp.x0[tid] = x0[tid];
  for (int t = tid; t < NC * h; t += NT) Kp.gait[t] = gait[t];
  for (int t = tid; t < C8 * U; t += NT) Kp.Fc[t] = Fc[t];
  for (int t = tid; t < 12 * h; t += NT) Kp.traj[t] = traj[t];
  for (int t = tid; t < U * h; t += NT) Kp.du[t] = dir[t], Kp.ell[t] = seed[t];
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, Kp.slack, Kp.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  for (int ls = tid; ls < NC * h; ls += NT) {
    unsigned list = 0;
    const bool st = stance(cap[ls % NC], gait[ls]);
    const int m = st ? admitted_normals<NC>(Fc, ls % NC, Kp.slack + 10 * ls, act_tol, Kp.Q + 36 * ls, list) : LADJ_SWING;
    Kp.held[ls] = (unsigned char)m, Kp.rows[ls] = list;
  }
  __syncthreads();  // the binary32 inputs but u are not read below: Wk may take their place
  const double *A = Kp.A, *B = Kp.B;
  // ---- forward pass (hmpc_model_adjoint.h, chain for chain)
  if (tid < 13) Wk.dx[tid] = 0.0, Wk.x[tid] = (double)Kp.x0[tid];
  if (tid < 26) (tid < 13 ? Wk.c : Wk.d)[13 * h + tid % 13] = 0.0;  // c_{h+1} = d_{h+1} = 0
  for (int t = tid; t < 10 * NC * h; t += NT) Wk.lam[t] = 0.0, Wk.nu[t] = 0.0;
  for (int t = tid; t < C8 * U; t += NT) Wk.G[t] = 0.0;
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
  // ---- gradient and residual: one entry per lane and round
  for (int t = tid; t < 2 * U * h; t += NT) {
    const bool isr = t >= U * h;
    const int e = isr ? t - U * h : t, i = e / U, k = e % U;
    const double *co = (isr ? Wk.d : Wk.c) + 13 * i;  // c_{i+1}, d_{i+1}
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 13; ++a) acc = __builtin_fma(B[a * U + k], co[a], acc);
    if (isr) Wk.rho[e] = Kp.ell[e] + __builtin_fma(Kp.a2[k], Kp.du[e], acc);
    else Wk.grad[e] = __builtin_fma(Kp.a2[k], (double)u[e], acc);
  }
  __syncthreads();
  // ---- multipliers: leg-step ls on lane ls
  {
    double worst_l = 0.0, worst_n = 0.0;
    const int ls = tid;
    const int m = (ls < NC * h) ? (int)Kp.held[ls] : LADJ_SWING;
    if (m <= 6) {
      const int c = ls % NC, i = ls / NC;
      const unsigned list = Kp.rows[ls];
      const double *q = Kp.Q + 36 * ls;
      const float *rw = Kp.Fc + 8 * c * U;
      auto N = [&](const int j, const int k) -> double { return cert_sign(j) * (double)rw[cert_src(j) * U + fb_col<NC>(c, k)]; };
      double rl[6], rn[6], xl[6], xn[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) rl[k] = Wk.grad[U * i + fb_col<NC>(c, k)], rn[k] = Wk.rho[U * i + fb_col<NC>(c, k)];
#pragma unroll
      for (int a = 5; a >= 0; --a) {
        xl[a] = 0.0, xn[a] = 0.0;
        if (a < m) {
          const double *qa = q + 6 * a;
          const int ja = (int)((list >> (4 * a)) & 15u);
          double taa = 0.0, yl = 0.0, yn = 0.0, sl = 0.0, sn = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            taa = __builtin_fma(qa[k], N(ja, k), taa);
            yl = __builtin_fma(qa[k], rl[k], yl);
            yn = __builtin_fma(qa[k], rn[k], yn);
          }
#pragma unroll
          for (int b = a + 1; b < 6; ++b)
            if (b < m) {
              const int jb = (int)((list >> (4 * b)) & 15u);
              double tab = 0.0;
#pragma unroll
              for (int k = 0; k < 6; ++k) tab = __builtin_fma(qa[k], N(jb, k), tab);
              sl = __builtin_fma(tab, xl[b], sl);
              sn = __builtin_fma(tab, xn[b], sn);
            }
          xl[a] = (yl - sl) / taa, xn[a] = (yn - sn) / taa;
        }
      }
      double el[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, en[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int b = 0; b < 6; ++b)
        if (b < m) {
          const int jb = (int)((list >> (4 * b)) & 15u);
          Wk.lam[10 * ls + jb] = xl[b], Wk.nu[10 * ls + jb] = xn[b];
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            const double n = N(jb, k);
            el[k] = __builtin_fma(n, xl[b], el[k]);
            en[k] = __builtin_fma(n, xn[b], en[k]);
          }
        }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double vl = ladj_mag(rl[k] - el[k]), vn = ladj_mag(rn[k] - en[k]);
        worst_l = (vl > worst_l) ? vl : worst_l;
        worst_n = (vn > worst_n) ? vn : worst_n;
      }
    }
    Wk.red[0][tid] = worst_l, Wk.red[1][tid] = worst_n;
  }
  __syncthreads();
  // ---- row gradients: one lane per non-zero entry of the block; the bound gradients leave beside them
  if (gbound)
    for (int t = tid; t < 10 * NC * h; t += NT) gbound[t] = 0.0 - Wk.nu[t];
  {
    double worst_g = 0.0;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int t = tid + NT * round;
      if (t < 48 * NC) {
        const int c = t / 48, r = (t / 6) % 8, col = fb_col<NC>(c, t % 6);
        const int j0 = (r < 5) ? r : (r + 1);  // rows 4 and 7 serve j0 and j0 + 1
        const bool two = (r == 4) || (r == 7);
        const double s0 = cert_sign(j0), s1 = cert_sign(j0 + 1);
        double acc = 0.0;
        for (int i = 0; i < h; ++i) {
          const double *lm = Wk.lam + 10 * (NC * i + c), *nm = Wk.nu + 10 * (NC * i + c);
          const double dv = Kp.du[U * i + col], uv = (double)u[U * i + col];
          acc = __builtin_fma(0.0 - s0 * lm[j0], dv, acc);
          acc = __builtin_fma(0.0 - s0 * nm[j0], uv, acc);
          if (two) {
            acc = __builtin_fma(0.0 - s1 * lm[j0 + 1], dv, acc);
            acc = __builtin_fma(0.0 - s1 * nm[j0 + 1], uv, acc);
          }
        }
        Wk.G[(8 * c + r) * U + col] = acc;
        const double v = ladj_mag(acc);
        worst_g = (v > worst_g) ? v : worst_g;
      }
    }
    Wk.red[2][tid] = worst_g;
  }
  __syncthreads();
  // ---- chain rules and maxima, on single lanes
  if (tid == 0) {  // mu
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double *g = Wk.G + 8 * c * U;
      acc = acc + g[1 * U + 3 * c];
      acc = acc - g[0 * U + 3 * c];
      acc = acc + g[3 * U + 3 * c + 1];
      acc = acc - g[2 * U + 3 * c + 1];
    }
    Wk.lim[0] = acc;
  } else if (tid == 1 || tid == 2) {  // lt (row 5), lh (row 6)
    const int r = 4 + tid;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc = __builtin_fma(Wk.G[(8 * c + r) * U + 3 * c + k], (double)Kp.Fc[(8 * c + r) * U + 3 * c + k], acc);
    Wk.lim[tid] = acc / ((tid == 1) ? lt : lh);
  } else if (tid >= 32 && tid < 32 + LADJ_SUMMARY) {
    const double *red = Wk.red[tid - 32];
    double best = 0.0;
    for (int t = 0; t < NT; ++t) best = (red[t] > best) ? red[t] : best;
    Wk.summary[tid - 32] = best;
  } else if (tid >= 64 && tid < 64 + NC) {  // caps
    const int c = tid - 64;
    double acc = 0.0;
    for (int i = 0; i < h; ++i) acc = __builtin_fma(0.0 - Wk.nu[10 * (NC * i + c) + 9], (double)(float)Kp.gait[NC * i + c], acc);
    Wk.lim[3 + c] = acc;
  }
  __syncthreads();
  // ---- outputs, coalesced from LDS
  if (gFc)
    for (int t = tid; t < C8 * U; t += NT) gFc[t] = Wk.G[t];
  if (lam_out)
    for (int t = tid; t < 10 * NC * h; t += NT) lam_out[t] = Wk.lam[t];
  if (nu_out)
    for (int t = tid; t < 10 * NC * h; t += NT) nu_out[t] = Wk.nu[t];
  if (glim && tid < 3 + NC) glim[tid] = Wk.lim[tid];
  if (summary_out && tid >= 64 && tid < 64 + LADJ_SUMMARY) summary_out[tid - 64] = Wk.summary[tid - 64];
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct LimitAdjointOut {
  double *grad_limits, *grad_Fc, *grad_bound, *lambda, *nu, *summary;  // [batch][3 + nc], [batch][8 nc][6 nc], 3 x [batch][h][nc][10], [batch][3]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants, mu_inst) and `forces`; it reads dir[batch][h][6 nc] (what hmpc_solve_adjoint wrote) and seed[batch][h][6 nc], writes
// `out` and nothing else.  Shapes: derived_shape (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_limit_adjoint(int nc, const KernelArgs &args, double act_tol, const double *dir, const double *seed, const LimitAdjointOut &out,
                                hipStream_t stream);
}  // namespace hmpc
#endif
