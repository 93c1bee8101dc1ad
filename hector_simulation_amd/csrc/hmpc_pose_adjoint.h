// hmpc_pose_adjoint.h -- the pose gradients of the solve (hmpc_adjoint_record): from what hmpc_solve_adjoint,
// hmpc_adjoint_model and hmpc_adjoint_limits last wrote, the gradient of the loss in EVERY float of the packed record -- the quaternion
// and the joint angles through stage A1 + A2 of the assembly (Euler angles, Rb^-1, I_w^-1, the foot rotations, the rows of the constraint
// block), everything else a copy into place; everything BEHIND the assembly, as device functions over plain LDS arrays.  The kernels
// that assemble (hmpc_pose_adjoint.hip) call pose_adjoint_of_instance with what the solve kernel's own stage function left in LDS;
// tests/src/pose_adjoint_on_host.cpp compiles this header for the CPU (one thread per lane) against a plain loop.
//
// Definition (fixed in include/hector_mpc.h; tests/pose_adjoint_mirror.py restates it in numpy).  All binary64, every chain ascending
// from +0 by explicit fused multiply-adds; the assembly's FORMULA is differentiated, not its binary32 rounding; the stage's tabulated
// binary32 values enter widened: (s_k, c_k) = sc[k], (s_b, c_b) = sc234[leg], (cy, sy, cp, sp) = ypsc, R = quat_to_R of the record's
// quaternion, Ab = Acd[0:3, 6:9], Mb = Bcd[6:9, 3 NC .. 3 NC + 2].  G_F = grad_Fc, cf = 3c, cmo = 3 NC + 3c, sigma_c = +1 for c = 1, else -1.
//   Rf_c (c < 2; 0 = 5c)  t = s0 s1, v = c0 s1:  {fma(c0, cb, 0 - t sb), 0 - s0 c1, fma(c0, sb, t cb);  fma(s0, cb, v sb), c0 c1, fma(s0, sb, 0 - v cb);
//                         0 - c1 sb, s1, c1 cb}  = Rz(a0) Rx(a1) Ry(a2 + a3 + a4), what the stage's expanded products equal;  Rf_2 = Rhand
//   Gg_c[j][0] = G_F[8c+4][cmo+j];  Gg_c[j][1] = G_F[8c+5][cmo+j] + sigma_c G_F[8c+6][cmo+j];  Gg_c[j][2] = fma(0 - lt, G_F[8c+5][cf+j], (0 - lh) G_F[8c+6][cf+j])
//   G_Rf[c][a][m] = chain_j R[j][a] Gg_c[j][m];   P_c[i][j] = chain_m Gg_c[i][m] Rf_c[j][m]
//   grad_ja[5c]     = chain_k ( G_Rf[0][k] (0 - Rf[1][k]) ), then chain_k G_Rf[1][k] Rf[0][k]
//   grad_ja[5c + 1] = e = (c1 sb, 0 - s1, 0 - c1 cb), f = (s1 sb, c1, 0 - s1 cb):  chain_k G_Rf[0][k] ((0 - s0) e[k]), then G_Rf[1][k] (c0 e[k]), then G_Rf[2][k] f[k]
//   grad_ja[5c + 2 .. 4] = chain_i ( G_Rf[i][0] (0 - Rf[i][2]), G_Rf[i][2] Rf[i][0] )                    (one number, written three times)
//   Gam as hmpc_model_adjoint.h;  X[m][n] = chain_a Mb[a][m] Gam[a][n];  Y[m][k] = chain_n X[m][n] Mb[k][n];  G_Iw = 0 - Y / dt;
//   P_NC[i][k] = (chain_j (G_Iw[i][j] + G_Iw[j][i]) R[j][k]) Ib[k]
//   G_R[i][j] = +0 + P_0[i][j] + .. + P_NC[i][j]
//   X'[m][n] = chain_a Ab[a][m] grad_A[a][6+n];  Y'[m][k] = chain_n X'[m][n] Ab[k][n];  G_Rb = 0 - Y' / dt
//   G_yaw   = chain ( G_Rb[0][0] (0 - sy cp), G_Rb[0][1] (0 - cy), G_Rb[1][0] (cy cp), G_Rb[1][1] (0 - sy) )
//   G_pitch = chain ( G_Rb[0][0] (0 - cy sp), G_Rb[1][0] (0 - sy sp), G_Rb[2][0] (0 - cp) )
//   grad_rpy = (grad_x0[0], grad_x0[1] + G_pitch, grad_x0[2] + G_yaw)
//   J (3 x 4, columns qw qx qy qz), from the stage's own n0, d0, t, n2, d2 (binary32 products as the stage forms them, widened):
//     roll  row: fma(d0, dn0[k], 0 - n0 dd0[k]) / fma(n0, n0, d0 d0),  dn0 = (2qx, 2qw, 2qz, 2qy), dd0 = (0, -4qx, -4qy, 0)
//     pitch row: asd = 2 t;  exactly 0 where !(asd < 0.99999);  else das[k] / sqrt(fma(0 - asd, asd, 1)),  das = (2qy, -2qz, 2qw, -2qx)
//     yaw   row: as roll over n2, d2,  dn2 = (2qz, 2qy, 2qx, 2qw), dd2 = (0, 0, -4qy, -4qz)
//   E[k] = chain ( J[0][k] grad_rpy[0], J[1][k] grad_rpy[1], J[2][k] grad_rpy[2] )
//   grad_q[k] = (chain_{ij row-major} G_R[i][j] dR[i][j]/dq_k) + E[k],  dR/dq of quat_to_R's polynomial, zero entries included
//   grad_record: q <- grad_q, ja <- grad_ja, Rhand <- G_Rf[2], p, w, v <- grad_x0[3:6], [6:9], [9:12], r <- grad_r, weights <- grad_weights,
//     Alpha_K <- grad_alpha, traj <- grad_traj, f_max_hand <- grad_limits[3 + 2], yaw <- +0
//   grad_frames = (G_R, G_Rf[0 .. NC-1]);  grad_rpy as above
// Every loop's trip count is fixed by NC: nothing iterates on data, so NaN input ends like any other.
// Mapping: the upstream buffers arrive in LDS in coalesced bursts (the copies straight into the staged record); the contacts on lanes
// 0 .. NC-1 of wave 0 (one instruction stream for all of them), the inertia chain on lane 64 and the Euler chain on lane 65 of wave 1; one
// barrier; G_q on lanes 0 .. 3, G_R for grad_frames on lanes 4 .. 12; a barrier; coalesced stores.  No atomics, no inline assembly, no
// matrix cores.
#pragma once
#include <hip/hip_runtime.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_record.h"

namespace hmpc {
constexpr int PADJ_NT = DERIVED_NT;  // lanes of the workgroup

// the staged upstream gradients, the partial results and the staged outputs (LDS, or any memory all lanes see)
template <int NC, int HMAX>
struct PoseAdjointWork {
  static constexpr int U = 6 * NC, NREC = RecLayout<NC>::NF + 12 * HMAX;
  double GF[8 * NC * U];   // grad_Fc
  double GB[3 * U];        // grad_B rows 6 .. 8
  double GA[9];            // grad_A[0:3, 6:9]
  double gx[3];            // grad_x0[0:3]
  double P[NC + 1][9];     // the contributions to G_R: one per contact, then the inertia's
  double GRf[NC][9];
  double E[4];             // J' grad_rpy
  double rpy[3];
  double frames0[9];       // G_R
  double out[NREC];        // grad_record
};

// body of the chain X = A' G, Y = X A', result 0 - Y / dt: the adjoint of a 3 x 3 inverse scaled by dt (A = dt M^-1 assembled)
__device__ __forceinline__ void padj_inverse_adjoint(const double *A, const double *G, const double dt, double *out) {
  double X[9];
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) acc = __builtin_fma(A[3 * a + m], G[3 * a + n], acc);
      X[3 * m + n] = acc;
    }
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int n = 0; n < 3; ++n) acc = __builtin_fma(X[3 * m + n], A[3 * k + n], acc);
      out[3 * m + k] = 0.0 - acc / dt;
    }
}

// dR[i][j]/dq_k of quat_to_R's polynomial, row-major, from the doubled quaternion (tw, tx, ty, tz)
__device__ __forceinline__ void padj_dR(const int k, const double tw, const double tx, const double ty, const double tz, double *d) {
  if (k == 0) d[0] = 0.0, d[1] = 0.0 - tz, d[2] = ty, d[3] = tz, d[4] = 0.0, d[5] = 0.0 - tx, d[6] = 0.0 - ty, d[7] = tx, d[8] = 0.0;
  else if (k == 1) d[0] = 0.0, d[1] = ty, d[2] = tz, d[3] = ty, d[4] = 0.0 - (tx + tx), d[5] = 0.0 - tw, d[6] = tz, d[7] = tw, d[8] = 0.0 - (tx + tx);
  else if (k == 2) d[0] = 0.0 - (ty + ty), d[1] = tx, d[2] = tw, d[3] = tx, d[4] = 0.0, d[5] = tz, d[6] = 0.0 - tw, d[7] = tz, d[8] = 0.0 - (ty + ty);
  else d[0] = 0.0 - (tz + tz), d[1] = 0.0 - tw, d[2] = tx, d[3] = tw, d[4] = 0.0 - (tz + tz), d[5] = ty, d[6] = tx, d[7] = ty, d[8] = 0.0;
}

// a row of the Euler Jacobian of atan2(n, d): fma(d, dn[k], 0 - n dd[k]) / fma(n, n, d d)
__device__ __forceinline__ void padj_atan2_row(const double n, const double d, const double *dn, const double *dd, double *row) {
  const double den = __builtin_fma(n, n, d * d);
#pragma unroll
  for (int k = 0; k < 4; ++k) row[k] = __builtin_fma(d, dn[k], 0.0 - n * dd[k]) / den;
}

// The pose gradients of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): rec = the record's floats,
// sc[10][2], sc234[2][2], ypsc[4] (cy, sy, cp, sp), R[9] (quat_to_R of the record's quaternion), Acd[13][13], Bcd[13][6 NC]; the upstream
// buffers of the instance (any memory): gx0[13], gtraj[12 h], gw[12], gal[6 NC], gA[13][13], gB[13][6 NC], gr[3 NC], glim[3 + NC],
// gFc[8 NC][6 NC]; dt, lt, lh, Ib[3] widened.  Out: grec[NF + 12 h], gframes[1 + NC][9], grpy[3] (any may be null).  Every lane of the
// workgroup calls it.
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void pose_adjoint_of_instance(const float *rec, const float *sc, const float *sc234, const float *ypsc, const float *R,
                                                         const float *Acd, const float *Bcd, const double *gx0, const double *gtraj,
                                                         const double *gw, const double *gal, const double *gA, const double *gB,
                                                         const double *gr, const double *glim, const double *gFc, const int h, const double dt,
                                                         const double lt, const double lh, const double Ib0, const double Ib1, const double Ib2,
                                                         PoseAdjointWork<NC, HMAX> &Wk, double *grec, double *gframes, double *grpy) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, C8 = 8 * NC;
  const int tid = threadIdx.x;
  static_assert(NT == PADJ_NT && NC <= 3 && 96 + 6 * NC <= NT, "lane budget");
  // ---- the upstream gradients, staged; the copies go straight into place
  for (int t = tid; t < C8 * U; t += NT) Wk.GF[t] = gFc[t];
  for (int t = tid; t < 3 * U; t += NT) Wk.GB[t] = gB[6 * U + t];
  for (int t = tid; t < 12 * h; t += NT) Wk.out[RL::NF + t] = gtraj[t];
  if (tid < 9) Wk.GA[tid] = gA[(tid / 3) * 13 + 6 + tid % 3];
  else if (tid < 12) Wk.gx[tid - 9] = gx0[tid - 9];
  else if (tid < 21) {  // p, w, v <- grad_x0[3:6], [6:9], [9:12]
    const int s = tid - 12;
    Wk.out[(s < 3 ? RL::P : (s < 6 ? RL::W - 3 : RL::V - 6)) + s] = gx0[3 + s];
  } else if (tid == 21) Wk.out[RL::YAW] = 0.0;
  else if (tid == 22 && NC == 3) Wk.out[RL::FMH] = glim[3 + 2];
  else if (tid >= 32 && tid < 32 + 3 * NC) Wk.out[RL::R + tid - 32] = gr[tid - 32];
  else if (tid >= 64 && tid < 64 + 12) Wk.out[RL::WT + tid - 64] = gw[tid - 64];
  else if (tid >= 96 && tid < 96 + U) Wk.out[RL::AL + tid - 96] = gal[tid - 96];
  __syncthreads();
  // ---- the chains, one lane each
  if (tid < NC) {  // contact tid: the rows of the constraint block -> the body rotation, the foot frame, the joint angles
    const int c = tid, cf = 3 * c, cmo = 3 * NC + 3 * c;
    const int b = (c < 2) ? 5 * c : 0;
    const double s0 = (double)sc[2 * b], c0 = (double)sc[2 * b + 1], s1 = (double)sc[2 * b + 2], c1 = (double)sc[2 * b + 3];
    const double sb = (double)sc234[2 * (c & 1)], cb = (double)sc234[2 * (c & 1) + 1];
    double Rf[9];
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
    const double sg = (c == 1) ? 1.0 : -1.0;
    const double *G4 = Wk.GF + (8 * c + 4) * U, *G5 = Wk.GF + (8 * c + 5) * U, *G6 = Wk.GF + (8 * c + 6) * U;
    double Gg[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Gg[3 * j + 0] = G4[cmo + j];
      Gg[3 * j + 1] = G5[cmo + j] + sg * G6[cmo + j];
      Gg[3 * j + 2] = __builtin_fma(0.0 - lt, G5[cf + j], (0.0 - lh) * G6[cf + j]);
    }
    double GRf[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc = __builtin_fma((double)R[3 * j + a], Gg[3 * j + m], acc);
        GRf[3 * a + m] = acc;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) acc = __builtin_fma(Gg[3 * i + m], Rf[3 * j + m], acc);
        Wk.P[c][3 * i + j] = acc;
      }
#pragma unroll
    for (int k = 0; k < 9; ++k) Wk.GRf[c][k] = GRf[k];
    if (NC == 3 && c == 2) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Wk.out[RL::RH + k] = GRf[k];
    } else {
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
      double *ja = Wk.out + RL::JA + 5 * c;
      ja[0] = a0, ja[1] = a1, ja[2] = ab, ja[3] = ab, ja[4] = ab;
    }
  } else if (tid == 64) {  // the inertia: Bcd rows 6 .. 8 -> I_w^-1 -> the body rotation
    double Gam[9], Mb[9], GI[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        Mb[3 * a + m] = (double)Bcd[(6 + a) * U + 3 * NC + m];
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float r0 = rec[RL::R + 0 * NC + c], r1 = rec[RL::R + 1 * NC + c], r2 = rec[RL::R + 2 * NC + c];
          const float cm[9] = {0.0f, -r2, r1, r2, 0.0f, -r0, -r1, r0, 0.0f};
          acc = acc + Wk.GB[a * U + 3 * NC + 3 * c + m];
#pragma unroll
          for (int b = 0; b < 3; ++b) acc = __builtin_fma(Wk.GB[a * U + 3 * c + b], (double)cm[3 * m + b], acc);
        }
        Gam[3 * a + m] = acc;
      }
    padj_inverse_adjoint(Mb, Gam, dt, GI);
    const double Ib[3] = {Ib0, Ib1, Ib2};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc = __builtin_fma(GI[3 * i + j] + GI[3 * j + i], (double)R[3 * j + k], acc);
        Wk.P[NC][3 * i + k] = acc * Ib[k];
      }
  } else if (tid == 65) {  // the Euler chain: Acd[0:3, 6:9] -> Rb -> yaw, pitch; the Euler angles -> the quaternion
    double Ab[9], GRb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ab[k] = (double)Acd[(k / 3) * 13 + 6 + k % 3];
    padj_inverse_adjoint(Ab, Wk.GA, dt, GRb);
    const double cy = (double)ypsc[0], sy = (double)ypsc[1], cp = (double)ypsc[2], sp = (double)ypsc[3];
    double gy = 0.0, gp = 0.0;
    gy = __builtin_fma(GRb[0], 0.0 - sy * cp, gy);
    gy = __builtin_fma(GRb[1], 0.0 - cy, gy);
    gy = __builtin_fma(GRb[3], cy * cp, gy);
    gy = __builtin_fma(GRb[4], 0.0 - sy, gy);
    gp = __builtin_fma(GRb[0], 0.0 - cy * sp, gp);
    gp = __builtin_fma(GRb[3], 0.0 - sy * sp, gp);
    gp = __builtin_fma(GRb[6], 0.0 - cp, gp);
    const double g0 = Wk.gx[0], g1 = Wk.gx[1] + gp, g2 = Wk.gx[2] + gy;
    Wk.rpy[0] = g0, Wk.rpy[1] = g1, Wk.rpy[2] = g2;
    const float qw = rec[RL::Q], qx = rec[RL::Q + 1], qy = rec[RL::Q + 2], qz = rec[RL::Q + 3];
    const double tw = (double)qw + (double)qw, tx = (double)qx + (double)qx, ty = (double)qy + (double)qy, tz = (double)qz + (double)qz;
    double Jr[4], Jp[4], Jy[4];
    {  // numerators and denominators as stage A1 forms them
      const float n0 = 2.0f * (qw * qx + qy * qz);
      const double d0 = 1.0 - (double)(2.0f * (qx * qx + qy * qy));
      const double dn[4] = {tx, tw, tz, ty}, dd[4] = {0.0, 0.0 - (tx + tx), 0.0 - (ty + ty), 0.0};
      padj_atan2_row((double)n0, d0, dn, dd, Jr);
    }
    {
      const float t = qw * qy - qx * qz;
      const double asd = 2.0 * (double)t;
      const bool clamped = !(asd < 0.99999);
      const double cosp = __builtin_sqrt(__builtin_fma(0.0 - asd, asd, 1.0));
      const double das[4] = {ty, 0.0 - tz, tw, 0.0 - tx};
#pragma unroll
      for (int k = 0; k < 4; ++k) Jp[k] = clamped ? 0.0 : das[k] / cosp;
    }
    {
      const float n2 = 2.0f * (qw * qz + qx * qy);
      const double d2 = 1.0 - (double)(2.0f * (qy * qy + qz * qz));
      const double dn[4] = {tz, ty, tx, tw}, dd[4] = {0.0, 0.0, 0.0 - (ty + ty), 0.0 - (tz + tz)};
      padj_atan2_row((double)n2, d2, dn, dd, Jy);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double acc = 0.0;
      acc = __builtin_fma(Jr[k], g0, acc);
      acc = __builtin_fma(Jp[k], g1, acc);
      acc = __builtin_fma(Jy[k], g2, acc);
      Wk.E[k] = acc;
    }
  }
  __syncthreads();
  // ---- the body rotation -> the quaternion: component k on lane k; G_R for grad_frames, entry e on lane 4 + e
  if (tid < 4) {
    const float qw = rec[RL::Q], qx = rec[RL::Q + 1], qy = rec[RL::Q + 2], qz = rec[RL::Q + 3];
    const double tw = (double)qw + (double)qw, tx = (double)qx + (double)qx, ty = (double)qy + (double)qy, tz = (double)qz + (double)qz;
    double d[9];
    padj_dR(tid, tw, tx, ty, tz, d);
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      double g = 0.0;
#pragma unroll
      for (int p = 0; p <= NC; ++p) g = g + Wk.P[p][e];
      acc = __builtin_fma(g, d[e], acc);
    }
    Wk.out[RL::Q + tid] = acc + Wk.E[tid];
  } else if (tid < 13) {
    const int e = tid - 4;
    double g = 0.0;
#pragma unroll
    for (int p = 0; p <= NC; ++p) g = g + Wk.P[p][e];
    Wk.frames0[e] = g;
  }
  __syncthreads();
  // ---- outputs, coalesced from LDS
  if (grec)
    for (int t = tid; t < RL::NF + 12 * h; t += NT) grec[t] = Wk.out[t];
  if (gframes && tid < 9 * (1 + NC)) gframes[tid] = (tid < 9) ? Wk.frames0[tid] : Wk.GRf[(tid - 9) / 9][(tid - 9) % 9];
  if (grpy && tid >= 64 && tid < 67) grpy[tid - 64] = Wk.rpy[tid - 64];
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct PoseAdjointIn {  // what hmpc_solve_adjoint, hmpc_adjoint_model and hmpc_adjoint_limits last wrote, as it stands
  const double *grad_x0, *grad_traj, *grad_weights, *grad_alpha, *grad_A, *grad_B, *grad_r, *grad_limits, *grad_Fc;
};
struct PoseAdjointOut {
  double *grad_record, *grad_frames, *grad_rpy;  // [batch][NF + 12 h], [batch][1 + nc][9], [batch][3]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, the robot
// constants, mu_inst); it reads `in`, writes `out` and nothing else.  Shapes: derived_shape (hmpc_derived_shape.h); anything else:
// hipErrorInvalidValue, nothing launched.
hipError_t launch_pose_adjoint(int nc, const KernelArgs &args, const PoseAdjointIn &in, const PoseAdjointOut &out, hipStream_t stream);
}  // namespace hmpc
#endif
