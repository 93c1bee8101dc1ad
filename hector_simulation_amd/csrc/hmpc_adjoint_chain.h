// hmpc_adjoint_chain.h -- the model, limit and record gradients of the solve under several seeds (hmpc_adjoint_chain_multi, DESIGN.md
// section 4.21): for every seed of the multi-seed adjoint that stands, the chain hmpc_adjoint_model -> hmpc_adjoint_limits ->
// hmpc_adjoint_record in ONE launch per tile of seeds; everything BEHIND the assembly, as device functions over plain LDS arrays.  The
// kernel that assembles (hmpc_adjoint_chain.hip) calls adjoint_chain_of_instance with what the solve kernel's own stage function left in
// LDS; tests/src/adjoint_chain_on_host.cpp compiles this header for the CPU (one thread per lane) against the three single-seed headers.
//
// Definition: none of its own.  Slice s of every output is, bit for bit, what model_adjoint_of_instance (hmpc_model_adjoint.h), then
// limit_adjoint_of_instance (hmpc_limit_adjoint.h), then pose_adjoint_of_instance (hmpc_pose_adjoint.h) write under slice s of the
// multi-seed adjoint and seed s alone: every chain of theirs is restated here term for term, in their order, from +0, by explicit
// fused multiply-adds.  What does not depend on the seed is formed ONCE per instance and tile: the widened A, B, q2, a2, the forward
// chain x_j, the tracking costate c_j, grad_i, the slacks, the active set, the admitted normals (Q, rows, held), lambda and its residual,
// the foot frames Rf_c and the quaternion rows J.  What does is formed for a SUB-TILE of SUB seeds at a time, the seeds' 13-lane chains
// side by side: dx_j and d_j on lanes 13 q + s (one barrier per step for all of them), nu one lane per (seed, leg-step) with rho_i formed
// in its registers, the outer-product sums one lane per (seed, entry), the chain rules one lane per (seed, chain).  Sub-tiles loop inside
// the workgroup over the shared part.
// Kept where: see DESIGN.md section 4.21.  dir of a seed is staged in LDS (read by four phases); the seed itself is read from HBM once,
// where rho needs it; G_A, G_B and the full grad_Fc never stand in LDS: an entry leaves for HBM from the lane that owns it when a detail
// buffer asks for it, and only what a chain rule reads (G_A[0:3, 6:9], G_B rows 6 .. 11, the 48 NC entries of G inside cols(c)) is kept.
// With no detail buffer for grad_A (grad_B) the other entries are not formed at all.
// Every loop's trip count is fixed by (h, NC, the seeds of the tile) and the number of admitted normals: nothing iterates on data, so
// NaN in one seed ends like any other and reaches no other seed.  No atomics, no inline assembly, no matrix cores.
#pragma once
#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_limit_adjoint.h"
#include "hmpc_model_adjoint.h"
#include "hmpc_pose_adjoint.h"

namespace hmpc {
constexpr int CADJ_NT = DERIVED_NT;  // lanes of the workgroup

// what adjoint_chain_of_instance keeps of its inputs and forms once for all seeds (LDS, or any memory all lanes see); the part that
// must not overlay the binary32 inputs: filled by the first phase, which reads them
template <int NC, int HMAX>
struct ChainKeep {
  static constexpr int U = 6 * NC;
  double A[169], B[13 * U], q2[13], a2[U];
  union {
    double slack[10 * NC * HMAX];  // read by the first phase alone (the active set, the admitted normals) ...
    double lam[10 * NC * HMAX];    // ... lambda takes its place behind it
  };
  double Q[36 * NC * HMAX];  // per leg-step: the admitted normals' orthonormal vectors
  double Rf[NC][9], ang[NC][6];  // the foot frames; s0, c0, s1, c1, sb, cb of the contact's leg
  double J[3][4], tq[4];         // the Euler Jacobian's rows; the doubled quaternion
  double ypsc[4], Ab[9], Mb[9];
  MarginMin wave_min[CADJ_NT / 64][MARGIN_CLASSES];
  unsigned rows[NC * HMAX];  // per leg-step: nibble b = j_b
  float traj[12 * HMAX], x0[16], Fc[8 * NC * U], r[3 * NC], R[9];
  unsigned char held[NC * HMAX], gait[NC * HMAX];
};

// what one seed of a sub-tile keeps
template <int NC, int HMAX>
struct ChainSeed {
  static constexpr int U = 6 * NC;
  double du[HMAX * U];                               // dir
  double dx[(HMAX + 1) * 13], d[(HMAX + 1) * 13];    // d holds rows 1 .. h+1 at 13 (j - 1)
  double nu[10 * NC * HMAX], wn[NC * HMAX];          // nu; max |e| of nu per leg-step
  double G[48 * NC];                                 // grad_Fc inside cols(c): [c][row][k], col = fb_col(c, k)
  double GB[6 * U], GA[9];                           // grad_B rows 6 .. 11, grad_A[0:3, 6:9]
  double gx[3], gr[3 * NC], gp[MADJ_PARAMS], lim[3 + NC], summary[LADJ_SUMMARY];
  double P[NC + 1][9], GRf[NC][9], E[4], rpy[3], ja[10], gq[4], frames0[9];
};

// the seed-independent passes and the sub-tile's seeds; may overlay the binary32 inputs of adjoint_chain_of_instance but u, which are not
// read again once the first phase has ended.  c holds rows 1 .. h+1 at 13 (j - 1).
template <int NC, int HMAX, int SUB>
struct ChainWork {
  static constexpr int U = 6 * NC;
  double x[(HMAX + 1) * 13], c[(HMAX + 1) * 13];
  double grad[HMAX * U], wl[NC * HMAX];
  double worst_l;
  ChainSeed<NC, HMAX> sd[SUB];
};

// where the instance's rows of slice 0 are, and how far the next slice lies (doubles): seed-major over the batch.  Inputs: the seeds and
// what the multi-seed adjoint wrote.  Outputs: compact (never null), then detail (any may be null: not written).
struct ChainIo {
  const double *seed, *dir, *gx0, *gtraj, *gw, *gal;
  double *grec, *gframes, *grpy, *gparams, *glim, *summary;
  double *gA, *gB, *gr, *costate, *gFc, *gbound, *lam, *nu;
  size_t batch;  // rows of a slice: the stride of array X is batch * (doubles per instance of X)
};

// The chain of one instance under seeds 0 .. ns-1 of `io`, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): x0[13],
// Acd[13][13], Bcd[13][6 NC], W[12], traj[12 h], alpha[6 NC], Fc[8 NC][6 NC], u[h][6 NC], gait[NC h] bytes, cap[NC], rec = the record's
// floats, sc[10][2], sc234[2][2], ypsc[4], R[9] (quat_to_R of the record's quaternion); act_tol, dt, mass, lt, lh, Ib[3] widened.  Every
// lane of the workgroup calls it.  Wk may overlay the binary32 inputs but u.
template <int NC, int HMAX, int NT, int SUB>
__device__ __forceinline__ void adjoint_chain_of_instance(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj,
                                                          const float *alpha, const float *Fc, const float *u, const unsigned char *gait,
                                                          const float *cap, const float *rec, const float *sc, const float *sc234,
                                                          const float *ypsc, const float *R, const ChainIo &io, const int ns, const int h,
                                                          const double act_tol, const double dt, const double mass, const double lt,
                                                          const double lh, const double Ib0, const double Ib1, const double Ib2,
                                                          ChainKeep<NC, HMAX> &Kp, ChainWork<NC, HMAX, SUB> &Wk) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, C8 = 8 * NC, NREC = RL::NF;
  const int tid = threadIdx.x;
  static_assert(NT == CADJ_NT && NC * HMAX <= NT && NC <= 3 && SUB >= 1, "lane budget");
  const size_t nb = io.batch, hz = (size_t)h;
  // ---- first phase: what the passes read of the inputs, widened; slacks; admitted normals; the pose chain's tables
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < U) Kp.a2[tid] = (double)alpha[tid] + (double)alpha[tid];
  if (tid < 13) Kp.x0[tid] = x0[tid];
  if (tid >= 32 && tid < 32 + 3 * NC) Kp.r[tid - 32] = rec[RL::R + tid - 32];
  if (tid >= 64 && tid < 64 + 9) {
    const int k = tid - 64;
    Kp.R[k] = R[k];
    Kp.Ab[k] = (double)Acd[(k / 3) * 13 + 6 + k % 3];
    Kp.Mb[k] = (double)Bcd[(6 + k / 3) * U + 3 * NC + k % 3];
  }
  if (tid >= 96 && tid < 96 + 4) Kp.ypsc[tid - 96] = (double)ypsc[tid - 96];
  for (int t = tid; t < NC * h; t += NT) Kp.gait[t] = gait[t];
  for (int t = tid; t < C8 * U; t += NT) Kp.Fc[t] = Fc[t];
  for (int t = tid; t < 12 * h; t += NT) Kp.traj[t] = traj[t];
  if (tid >= 100 && tid < 100 + NC) {  // the foot frame of contact c, as pose_adjoint_of_instance forms it
    const int c = tid - 100;
    const int b = (c < 2) ? 5 * c : 0;
    const double s0 = (double)sc[2 * b], c0 = (double)sc[2 * b + 1], s1 = (double)sc[2 * b + 2], c1 = (double)sc[2 * b + 3];
    const double sb = (double)sc234[2 * (c & 1)], cb = (double)sc234[2 * (c & 1) + 1];
    double *Rf = Kp.Rf[c], *an = Kp.ang[c];
    an[0] = s0, an[1] = c0, an[2] = s1, an[3] = c1, an[4] = sb, an[5] = cb;
    {
      const double t = s0 * s1, v = c0 * s1;
      Rf[0] = __builtin_fma(c0, cb, 0.0 - t * sb), Rf[1] = 0.0 - s0 * c1, Rf[2] = __builtin_fma(c0, sb, t * cb);
      Rf[3] = __builtin_fma(s0, cb, v * sb), Rf[4] = c0 * c1, Rf[5] = __builtin_fma(s0, sb, 0.0 - v * cb);
      Rf[6] = 0.0 - c1 * sb, Rf[7] = s1, Rf[8] = c1 * cb;
    }
    if (NC == 3 && c == 2) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rf[k] = (double)rec[RL::RH + k];
    }
  } else if (tid == 104) {  // the Euler Jacobian's rows, as pose_adjoint_of_instance forms them
    const float qw = rec[RL::Q], qx = rec[RL::Q + 1], qy = rec[RL::Q + 2], qz = rec[RL::Q + 3];
    const double tw = (double)qw + (double)qw, tx = (double)qx + (double)qx, ty = (double)qy + (double)qy, tz = (double)qz + (double)qz;
    Kp.tq[0] = tw, Kp.tq[1] = tx, Kp.tq[2] = ty, Kp.tq[3] = tz;
    {  // numerators and denominators as stage A1 forms them
      const float n0 = 2.0f * (qw * qx + qy * qz);
      const double d0 = 1.0 - (double)(2.0f * (qx * qx + qy * qy));
      const double dn[4] = {tx, tw, tz, ty}, dd[4] = {0.0, 0.0 - (tx + tx), 0.0 - (ty + ty), 0.0};
      padj_atan2_row((double)n0, d0, dn, dd, Kp.J[0]);
    }
    {
      const float t = qw * qy - qx * qz;
      const double asd = 2.0 * (double)t;
      const bool clamped = !(asd < 0.99999);
      const double cosp = __builtin_sqrt(__builtin_fma(0.0 - asd, asd, 1.0));
      const double das[4] = {ty, 0.0 - tz, tw, 0.0 - tx};
#pragma unroll
      for (int k = 0; k < 4; ++k) Kp.J[1][k] = clamped ? 0.0 : das[k] / cosp;
    }
    {
      const float n2 = 2.0f * (qw * qz + qx * qy);
      const double d2 = 1.0 - (double)(2.0f * (qy * qy + qz * qz));
      const double dn[4] = {tz, ty, tx, tw}, dd[4] = {0.0, 0.0, 0.0 - (ty + ty), 0.0 - (tz + tz)};
      padj_atan2_row((double)n2, d2, dn, dd, Kp.J[2]);
    }
  }
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, Kp.slack, Kp.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  for (int ls = tid; ls < NC * h; ls += NT) {
    unsigned list = 0;
    const bool st = stance(cap[ls % NC], gait[ls]);
    const int m = st ? admitted_normals<NC>(Fc, ls % NC, Kp.slack + 10 * ls, act_tol, Kp.Q + 36 * ls, list) : LADJ_SWING;
    Kp.held[ls] = (unsigned char)m, Kp.rows[ls] = list;
  }
  __syncthreads();  // the binary32 inputs but u are not read below: Wk may take their place
  const double *A = Kp.A, *B = Kp.B;
  // ---- the ends of the chains that are formed once for all seeds; the chains themselves ride the barriers of the first sub-tile
  if (tid < 13) Wk.x[tid] = (double)Kp.x0[tid], Wk.c[13 * h + tid] = 0.0;  // c_{h+1} = 0
  for (int t = tid; t < 10 * NC * h; t += NT) Kp.lam[t] = 0.0;
  // the triangular solve of one leg-step against its admitted normals: x, and max |rhs - sum n_b x_b| (limit_adjoint_of_instance's chains)
  auto multiplier = [&](const int ls, const double *rhs, double *xs) -> double {
    const int m = (int)Kp.held[ls], c = ls % NC;
    const unsigned list = Kp.rows[ls];
    const double *q = Kp.Q + 36 * ls;
    const float *rw = Kp.Fc + 8 * c * U;
    auto N = [&](const int j, const int k) -> double { return cert_sign(j) * (double)rw[cert_src(j) * U + fb_col<NC>(c, k)]; };
#pragma unroll
    for (int a = 5; a >= 0; --a) {
      xs[a] = 0.0;
      if (a < m) {
        const double *qa = q + 6 * a;
        const int ja = (int)((list >> (4 * a)) & 15u);
        double taa = 0.0, y = 0.0, sm = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          taa = __builtin_fma(qa[k], N(ja, k), taa);
          y = __builtin_fma(qa[k], rhs[k], y);
        }
#pragma unroll
        for (int b = a + 1; b < 6; ++b)
          if (b < m) {
            const int jb = (int)((list >> (4 * b)) & 15u);
            double tab = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) tab = __builtin_fma(qa[k], N(jb, k), tab);
            sm = __builtin_fma(tab, xs[b], sm);
          }
        xs[a] = (y - sm) / taa;
      }
    }
    double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 6; ++b)
      if (b < m) {
        const int jb = (int)((list >> (4 * b)) & 15u);
#pragma unroll
        for (int k = 0; k < 6; ++k) e[k] = __builtin_fma(N(jb, k), xs[b], e[k]);
      }
    double worst = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double v = ladj_mag(rhs[k] - e[k]);
      worst = (v > worst) ? v : worst;
    }
    return worst;
  };
  const bool fullA = io.gA != nullptr, fullB = io.gB != nullptr;
  const int nA = fullA ? 169 : 9, nB = fullB ? 13 * U : 6 * U;
  const size_t nrec = (size_t)NREC + 12 * hz, nls = (size_t)10 * NC * hz;
  // ============ the seeds, a sub-tile at a time
  for (int q0 = 0; q0 < ns; q0 += SUB) {
    const int nq = (ns - q0 < SUB) ? ns - q0 : SUB;
    // ---- dir of every seed, staged; the chains' ends
    for (int q = 0; q < nq; ++q) {
      ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      const size_t s = (size_t)(q0 + q);
      const double *dir = io.dir + s * nb * hz * U;
      for (int t = tid; t < U * h; t += NT) Sd.du[t] = dir[t];
      for (int t = tid; t < 10 * NC * h; t += NT) Sd.nu[t] = 0.0;
      if (tid < 13) Sd.dx[tid] = 0.0, Sd.d[13 * h + tid] = 0.0;  // dx_0 = 0, d_{h+1} = 0
      if (tid >= 32 && tid < 35) Sd.gx[tid - 32] = io.gx0[s * nb * 13 + tid - 32];
    }
    __syncthreads();
    // ---- forward pass: dx of seed q on lanes 13 q .. 13 q + 12, one barrier per step for all seeds
    for (int i = 0; i < h; ++i) {
      for (int t = tid; t < 13 * nq; t += NT) {
        ChainSeed<NC, HMAX> &Sd = Wk.sd[t / 13];
        const int s = t % 13;
        const double *dxi = Sd.dx + 13 * i, *du = Sd.du + U * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[s * 13 + k], dxi[k], acc);
#pragma unroll
        for (int c = 0; c < U; ++c) acc = __builtin_fma(B[s * U + c], du[c], acc);
        Sd.dx[13 * (i + 1) + s] = acc;
      }
      if (q0 == 0 && tid >= NT - 13) {  // once for all seeds, beside the first sub-tile: x_{i+1}, as hmpc_predict_states has it
        const int s = tid - (NT - 13);
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
    // ---- backward pass: d likewise
    for (int j = h; j >= 1; --j) {
      for (int t = tid; t < 13 * nq; t += NT) {
        ChainSeed<NC, HMAX> &Sd = Wk.sd[t / 13];
        const int s = t % 13;
        const double *nx = Sd.d + 13 * j;  // row j+1
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[k * 13 + s], nx[k], acc);
        if (s < 12) acc = __builtin_fma(Kp.q2[s], Sd.dx[13 * j + s], acc);
        Sd.d[13 * (j - 1) + s] = acc;
      }
      if (q0 == 0 && tid >= NT - 13) {  // once for all seeds: c_j (x stands whole: the forward pass has ended)
        const int s = tid - (NT - 13);
        const double *nx = Wk.c + 13 * j;  // row j+1
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[k * 13 + s], nx[k], acc);
        if (s < 12) acc = __builtin_fma(Kp.q2[s], Wk.x[13 * j + s] - (double)Kp.traj[12 * (j - 1) + s], acc);
        Wk.c[13 * (j - 1) + s] = acc;
      }
      __syncthreads();
    }
    if (q0 == 0) {
      // ---- once for all seeds: grad_i, one entry per lane and round
      for (int e = tid; e < U * h; e += NT) {
        const int i = e / U, k = e % U;
        const double *co = Wk.c + 13 * i;  // c_{i+1}
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 13; ++a) acc = __builtin_fma(B[a * U + k], co[a], acc);
        Wk.grad[e] = __builtin_fma(Kp.a2[k], (double)u[e], acc);
      }
      __syncthreads();
      // ---- once for all seeds: lambda, leg-step ls on lane ls
      if (tid < NC * h) {
        const int ls = tid;
        double worst = 0.0;
        if ((int)Kp.held[ls] <= 6) {
          const int c = ls % NC, i = ls / NC;
          double rl[6], xl[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) rl[k] = Wk.grad[U * i + fb_col<NC>(c, k)];
          worst = multiplier(ls, rl, xl);
          const unsigned list = Kp.rows[ls];
#pragma unroll
          for (int b = 0; b < 6; ++b)
            if (b < (int)Kp.held[ls]) Kp.lam[10 * ls + (int)((list >> (4 * b)) & 15u)] = xl[b];
        }
        Wk.wl[ls] = worst;
      }
      __syncthreads();
      if (tid == 0) {  // (read behind the barriers below)
        double best = 0.0;
        for (int t = 0; t < NC * h; ++t) best = (Wk.wl[t] > best) ? Wk.wl[t] : best;
        Wk.worst_l = best;
      }
    }
    // ---- nu: one lane per (seed, leg-step); hd and rho of its six columns in registers
    for (int t = tid; t < NC * h * nq; t += NT) {
      const int q = t / (NC * h), ls = t % (NC * h);
      ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      double worst = 0.0;
      if ((int)Kp.held[ls] <= 6) {
        const int c = ls % NC, i = ls / NC;
        const double *ell = io.seed + (size_t)(q0 + q) * nb * hz * U, *co = Sd.d + 13 * i;  // d_{i+1}
        double rn[6], xn[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int col = fb_col<NC>(c, k), e = U * i + col;
          double acc = 0.0;
#pragma unroll
          for (int a = 0; a < 13; ++a) acc = __builtin_fma(B[a * U + col], co[a], acc);
          rn[k] = ell[e] + __builtin_fma(Kp.a2[col], Sd.du[e], acc);
        }
        worst = multiplier(ls, rn, xn);
        const unsigned list = Kp.rows[ls];
#pragma unroll
        for (int b = 0; b < 6; ++b)
          if (b < (int)Kp.held[ls]) Sd.nu[10 * ls + (int)((list >> (4 * b)) & 15u)] = xn[b];
      }
      Sd.wn[ls] = worst;
    }
    __syncthreads();
    // ---- the sums over the steps: one lane per (seed, entry) of G, G_A, G_B; no barrier inside
    for (int t = tid; t < 48 * NC * nq; t += NT) {  // limit_adjoint_of_instance's row gradients
      const int q = t / (48 * NC), e = t % (48 * NC);
      ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      const int c = e / 48, r = (e / 6) % 8, col = fb_col<NC>(c, e % 6);
      const int j0 = (r < 5) ? r : (r + 1);  // rows 4 and 7 serve j0 and j0 + 1
      const bool two = (r == 4) || (r == 7);
      const double s0 = cert_sign(j0), s1 = cert_sign(j0 + 1);
      double acc = 0.0;
      for (int i = 0; i < h; ++i) {
        const double *lm = Kp.lam + 10 * (NC * i + c), *nm = Sd.nu + 10 * (NC * i + c);
        const double dv = Sd.du[U * i + col], uv = (double)u[U * i + col];
        acc = __builtin_fma(0.0 - s0 * lm[j0], dv, acc);
        acc = __builtin_fma(0.0 - s0 * nm[j0], uv, acc);
        if (two) {
          acc = __builtin_fma(0.0 - s1 * lm[j0 + 1], dv, acc);
          acc = __builtin_fma(0.0 - s1 * nm[j0 + 1], uv, acc);
        }
      }
      Sd.G[e] = acc;
    }
    for (int t = tid; t < (nA + nB) * nq; t += NT) {  // model_adjoint_of_instance's accumulation
      const int q = t / (nA + nB), e = t % (nA + nB);
      ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      const bool isA = e < nA;
      int a, b;
      if (isA) a = fullA ? e / 13 : e / 3, b = fullA ? e % 13 : 6 + e % 3;
      else a = (fullB ? 0 : 6) + (e - nA) / U, b = (e - nA) % U;
      double acc = 0.0;
      for (int i = 0; i < h; ++i) {
        const double ci = Wk.c[13 * i + a], di = Sd.d[13 * i + a];  // c_{i+1}, d_{i+1}
        const double f0 = isA ? Sd.dx[13 * i + b] : Sd.du[U * i + b];
        const double f1 = isA ? Wk.x[13 * i + b] : (double)u[U * i + b];
        acc = __builtin_fma(ci, f0, acc);
        acc = __builtin_fma(di, f1, acc);
      }
      const size_t s = (size_t)(q0 + q);
      if (isA) {
        if (fullA) io.gA[s * nb * 169 + a * 13 + b] = acc;
        if (a < 3 && b >= 6 && b < 9) Sd.GA[3 * a + b - 6] = acc;
      } else {
        if (fullB) io.gB[s * nb * 13 * U + a * U + b] = acc;
        if (a >= 6 && a < 12) Sd.GB[(a - 6) * U + b] = acc;
      }
    }
    __syncthreads();
    // ---- the chain rules: one lane per (seed, chain).  Chains of a seed: grad_r (NC), mass, inertia (3), mu, lt, lh, caps (NC), the two
    //      maxima, the contacts' frames and joint angles (NC), the inertia's and the Euler chain of the record gradients
    constexpr int K_R = 0, K_MASS = NC, K_IN = NC + 1, K_MU = NC + 4, K_LT = NC + 5, K_CAP = NC + 7, K_MAXN = 2 * NC + 7, K_MAXG = 2 * NC + 8,
                  K_CT = 2 * NC + 9, K_PIN = 3 * NC + 9, K_EU = 3 * NC + 10, CHAINS = 3 * NC + 11;
    for (int t = tid; t < CHAINS * nq; t += NT) {
      const int q = t % nq, kind = t / nq;  // (a wave's lanes share as few kinds as can be)
      ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      const double *GB = Sd.GB;                       // rows 6 .. 11: GB[(a - 6) * U + b]
      const double *Mb = B + 6 * U + 3 * NC;          // Mb[a][m] = Mb[a * U + m]
      auto GF = [&](const int c, const int r, const int k) -> double { return Sd.G[48 * c + 6 * r + k]; };  // G[8 c + r][fb_col(c, k)]
      if (kind >= K_R && kind < K_R + NC) {  // grad_r of contact c
        const int c = kind - K_R;
        double T[9];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc = __builtin_fma(Mb[a * U + m], GB[a * U + 3 * c + b], acc);
            T[3 * m + b] = acc;
          }
        Sd.gr[0 * NC + c] = T[7] - T[5];
        Sd.gr[1 * NC + c] = T[2] - T[6];
        Sd.gr[2 * NC + c] = T[3] - T[1];
      } else if (kind == K_MASS) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int a = 0; a < 3; ++a) acc = acc + GB[(3 + a) * U + 3 * c + a];
        Sd.gp[0] = 0.0 - (acc * B[9 * U]) / mass;
      } else if (kind >= K_IN && kind < K_IN + 3) {  // grad_inertia[k]
        const int k = kind - K_IN;
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
              acc = acc + GB[a * U + 3 * NC + 3 * c + m];
#pragma unroll
              for (int b = 0; b < 3; ++b) acc = __builtin_fma(GB[a * U + 3 * c + b], (double)cm[3 * m + b], acc);
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
        Sd.gp[1 + k] = 0.0 - acc / dt;
      } else if (kind == K_MU) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          acc = acc + GF(c, 1, 0);
          acc = acc - GF(c, 0, 0);
          acc = acc + GF(c, 3, 1);
          acc = acc - GF(c, 2, 1);
        }
        Sd.lim[0] = acc;
      } else if (kind == K_LT || kind == K_LT + 1) {  // lt (row 5), lh (row 6)
        const int r = 5 + kind - K_LT;
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int k = 0; k < 3; ++k) acc = __builtin_fma(GF(c, r, k), (double)Kp.Fc[(8 * c + r) * U + 3 * c + k], acc);
        Sd.lim[1 + kind - K_LT] = acc / ((kind == K_LT) ? lt : lh);
      } else if (kind >= K_CAP && kind < K_CAP + NC) {
        const int c = kind - K_CAP;
        double acc = 0.0;
        for (int i = 0; i < h; ++i) acc = __builtin_fma(0.0 - Sd.nu[10 * (NC * i + c) + 9], (double)(float)Kp.gait[NC * i + c], acc);
        Sd.lim[3 + c] = acc;
      } else if (kind == K_MAXN) {
        double best = 0.0;
        for (int ls = 0; ls < NC * h; ++ls) best = (Sd.wn[ls] > best) ? Sd.wn[ls] : best;
        Sd.summary[0] = Wk.worst_l, Sd.summary[1] = best;
      } else if (kind == K_MAXG) {
        double best = 0.0;
        for (int e = 0; e < 48 * NC; ++e) {
          const double v = ladj_mag(Sd.G[e]);
          best = (v > best) ? v : best;
        }
        Sd.summary[2] = best;
      } else if (kind >= K_CT && kind < K_CT + NC) {  // contact c: the rows of the constraint block -> the body rotation, the foot frame, the joint angles
        const int c = kind - K_CT;
        const double *Rf = Kp.Rf[c], *an = Kp.ang[c];
        const double s0 = an[0], c0 = an[1], s1 = an[2], c1 = an[3], sb = an[4], cb = an[5];
        const double sg = (c == 1) ? 1.0 : -1.0;
        double Gg[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          Gg[3 * j + 0] = GF(c, 4, 3 + j);
          Gg[3 * j + 1] = GF(c, 5, 3 + j) + sg * GF(c, 6, 3 + j);
          Gg[3 * j + 2] = __builtin_fma(0.0 - lt, GF(c, 5, j), (0.0 - lh) * GF(c, 6, j));
        }
        double GRf[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc = __builtin_fma((double)Kp.R[3 * j + a], Gg[3 * j + m], acc);
            GRf[3 * a + m] = acc;
          }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) acc = __builtin_fma(Gg[3 * i + m], Rf[3 * j + m], acc);
            Sd.P[c][3 * i + j] = acc;
          }
#pragma unroll
        for (int k = 0; k < 9; ++k) Sd.GRf[c][k] = GRf[k];
        if (!(NC == 3 && c == 2)) {
          double a0 = 0.0, a1 = 0.0, ab = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) a0 = __builtin_fma(GRf[k], 0.0 - Rf[3 + k], a0);
#pragma unroll
          for (int k = 0; k < 3; ++k) a0 = __builtin_fma(GRf[3 + k], Rf[k], a0);
          const double e[3] = {c1 * sb, 0.0 - s1, 0.0 - c1 * cb}, f[3] = {s1 * sb, c1, 0.0 - s1 * cb};
#pragma unroll
          for (int k = 0; k < 3; ++k) a1 = __builtin_fma(GRf[k], (0.0 - s0) * e[k], a1);
#pragma unroll
          for (int k = 0; k < 3; ++k) a1 = __builtin_fma(GRf[3 + k], c0 * e[k], a1);
#pragma unroll
          for (int k = 0; k < 3; ++k) a1 = __builtin_fma(GRf[6 + k], f[k], a1);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            ab = __builtin_fma(GRf[3 * i], 0.0 - Rf[3 * i + 2], ab);
            ab = __builtin_fma(GRf[3 * i + 2], Rf[3 * i], ab);
          }
          double *ja = Sd.ja + 5 * c;
          ja[0] = a0, ja[1] = a1, ja[2] = ab, ja[3] = ab, ja[4] = ab;
        }
      } else if (kind == K_PIN) {  // the inertia: Bcd rows 6 .. 8 -> I_w^-1 -> the body rotation
        double Gam[9], GI[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const float r0 = Kp.r[0 * NC + c], r1 = Kp.r[1 * NC + c], r2 = Kp.r[2 * NC + c];
              const float cm[9] = {0.0f, -r2, r1, r2, 0.0f, -r0, -r1, r0, 0.0f};
              acc = acc + GB[a * U + 3 * NC + 3 * c + m];
#pragma unroll
              for (int b = 0; b < 3; ++b) acc = __builtin_fma(GB[a * U + 3 * c + b], (double)cm[3 * m + b], acc);
            }
            Gam[3 * a + m] = acc;
          }
        padj_inverse_adjoint(Kp.Mb, Gam, dt, GI);
        const double Ib[3] = {Ib0, Ib1, Ib2};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc = __builtin_fma(GI[3 * i + j] + GI[3 * j + i], (double)Kp.R[3 * j + k], acc);
            Sd.P[NC][3 * i + k] = acc * Ib[k];
          }
      } else if (kind == K_EU) {  // the Euler chain: Acd[0:3, 6:9] -> Rb -> yaw, pitch; the Euler angles -> the quaternion
        double GRb[9];
        padj_inverse_adjoint(Kp.Ab, Sd.GA, dt, GRb);
        const double cy = Kp.ypsc[0], sy = Kp.ypsc[1], cp = Kp.ypsc[2], sp = Kp.ypsc[3];
        double gy = 0.0, gp = 0.0;
        gy = __builtin_fma(GRb[0], 0.0 - sy * cp, gy);
        gy = __builtin_fma(GRb[1], 0.0 - cy, gy);
        gy = __builtin_fma(GRb[3], cy * cp, gy);
        gy = __builtin_fma(GRb[4], 0.0 - sy, gy);
        gp = __builtin_fma(GRb[0], 0.0 - cy * sp, gp);
        gp = __builtin_fma(GRb[3], 0.0 - sy * sp, gp);
        gp = __builtin_fma(GRb[6], 0.0 - cp, gp);
        const double g0 = Sd.gx[0], g1 = Sd.gx[1] + gp, g2 = Sd.gx[2] + gy;
        Sd.rpy[0] = g0, Sd.rpy[1] = g1, Sd.rpy[2] = g2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          double acc = 0.0;
          acc = __builtin_fma(Kp.J[0][k], g0, acc);
          acc = __builtin_fma(Kp.J[1][k], g1, acc);
          acc = __builtin_fma(Kp.J[2][k], g2, acc);
          Sd.E[k] = acc;
        }
      }
    }
    __syncthreads();
    // ---- the body rotation -> the quaternion: component k on lane 13 q + k; G_R for grad_frames, entry e on lane 13 q + 4 + e
    for (int t = tid; t < 13 * nq; t += NT) {
      ChainSeed<NC, HMAX> &Sd = Wk.sd[t / 13];
      const int k = t % 13;
      if (k < 4) {
        double d[9];
        padj_dR(k, Kp.tq[0], Kp.tq[1], Kp.tq[2], Kp.tq[3], d);
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          double g = 0.0;
#pragma unroll
          for (int p = 0; p <= NC; ++p) g = g + Sd.P[p][e];
          acc = __builtin_fma(g, d[e], acc);
        }
        Sd.gq[k] = acc + Sd.E[k];
      } else {
        const int e = k - 4;
        double g = 0.0;
#pragma unroll
        for (int p = 0; p <= NC; ++p) g = g + Sd.P[p][e];
        Sd.frames0[e] = g;
      }
    }
    __syncthreads();
    // ---- outputs: every entry from the lane that owns it, consecutive lanes on consecutive addresses
    for (int q = 0; q < nq; ++q) {
      const ChainSeed<NC, HMAX> &Sd = Wk.sd[q];
      const size_t s = (size_t)(q0 + q);
      {  // grad_record: the copies straight from the adjoint's slices into place
        double *grec = io.grec + s * nb * nrec;
        const double *gx0 = io.gx0 + s * nb * 13, *gtraj = io.gtraj + s * nb * hz * 12, *gw = io.gw + s * nb * 12, *gal = io.gal + s * nb * U;
        for (int t = tid; t < NREC + 12 * h; t += NT) {
          double v;
          if (t >= NREC) v = gtraj[t - NREC];
          else if (t < RL::V) v = gx0[3 + t - RL::P];
          else if (t < RL::Q) v = gx0[9 + t - RL::V];
          else if (t < RL::W) v = Sd.gq[t - RL::Q];
          else if (t < RL::R) v = gx0[6 + t - RL::W];
          else if (t < RL::JA) v = Sd.gr[t - RL::R];
          else if (t < RL::YAW) v = Sd.ja[t - RL::JA];
          else if (t < RL::WT) v = 0.0;
          else if (t < RL::AL) v = gw[t - RL::WT];
          else if (t < RL::RH) v = gal[t - RL::AL];
          else if (t < RL::FMH) v = Sd.GRf[NC - 1][t - RL::RH];  // (NC = 3 only: NF = RH for two contacts)
          else v = Sd.lim[3 + NC - 1];
          grec[t] = v;
        }
      }
      if (tid < 9 * (1 + NC)) io.gframes[s * nb * 9 * (1 + NC) + tid] = (tid < 9) ? Sd.frames0[tid] : Sd.GRf[(tid - 9) / 9][(tid - 9) % 9];
      if (tid >= 64 && tid < 67) io.grpy[s * nb * 3 + tid - 64] = Sd.rpy[tid - 64];
      if (tid >= 68 && tid < 68 + MADJ_PARAMS) io.gparams[s * nb * MADJ_PARAMS + tid - 68] = Sd.gp[tid - 68];
      if (tid >= 72 && tid < 72 + 3 + NC) io.glim[s * nb * (3 + NC) + tid - 72] = Sd.lim[tid - 72];
      if (tid >= 80 && tid < 80 + LADJ_SUMMARY) io.summary[s * nb * LADJ_SUMMARY + tid - 80] = Sd.summary[tid - 80];
      if (io.gr && tid >= 84 && tid < 84 + 3 * NC) io.gr[s * nb * 3 * NC + tid - 84] = Sd.gr[tid - 84];
      if (io.costate && tid >= 96 && tid < 96 + MADJ_COSTATE)
        io.costate[s * nb * MADJ_COSTATE + tid - 96] = (tid - 96 < 13) ? Wk.c[tid - 96] : Sd.d[tid - 96 - 13];
      if (io.gFc) {  // zeros outside cols(c)
        double *g = io.gFc + s * nb * C8 * U;
        for (int t = tid; t < C8 * U; t += NT) {
          const int row = t / U, col = t % U, c = row / 8;
          const int k = (col >= 3 * c && col < 3 * c + 3) ? col - 3 * c : ((col >= 3 * NC + 3 * c && col < 3 * NC + 3 * c + 3) ? col - 3 * NC - 3 * c + 3 : -1);
          g[t] = (k >= 0) ? Sd.G[48 * c + 6 * (row % 8) + k] : 0.0;
        }
      }
      if (io.gbound)
        for (int t = tid; t < 10 * NC * h; t += NT) io.gbound[s * nb * nls + t] = 0.0 - Sd.nu[t];
      if (io.lam)
        for (int t = tid; t < 10 * NC * h; t += NT) io.lam[s * nb * nls + t] = Kp.lam[t];
      if (io.nu)
        for (int t = tid; t < 10 * NC * h; t += NT) io.nu[s * nb * nls + t] = Sd.nu[t];
    }
    __syncthreads();  // the next sub-tile overwrites what these stores read
  }
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct AdjointChainIn {  // slice 0 of the seeds and of what hmpc_solve_adjoint_multi wrote
  const double *seeds, *dir, *grad_x0, *grad_traj, *grad_weights, *grad_alpha;
};
struct AdjointChainOut {  // slice 0, seed-major over args.batch; the detail members may be null
  double *grad_record, *grad_frames, *grad_rpy, *grad_params, *grad_limits, *limit_summary;
  double *grad_A, *grad_B, *grad_r, *costate, *grad_Fc, *grad_bound, *lambda, *nu;
};
// One launch per tile of 6 nc seeds over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch,
// horizon, dt, f_max, the robot constants, mu_inst) and `forces`; it reads `in`, writes `out` and nothing else.  Shapes: derived_shape
// (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_adjoint_chain(int nc, const KernelArgs &args, double act_tol, double mass, const AdjointChainIn &in, int n_seeds,
                                const AdjointChainOut &out, hipStream_t stream);
}  // namespace hmpc
#endif
