// hmpc_front.h -- the scalar front of the assembly (stages A1 and A2), defined once and called from two places.
//
// What an instance's QP needs before the first chain runs -- joint and Euler trigonometry, the body algebra (dt Rbi, dt Iinv, dt Iinv [r]x),
// the foot rotations' rows of the constraint block, the stance prefix counts -- depends on nothing but the record and the handle's
// constants, and it is short serial chains in binary64: a lane each.  The functions below are those lane bodies.  They take and return
// values (pointers to the caller's arrays), never Smem members:
//   * stage_a_scalars (hmpc_kernel.h) calls them from the lanes it always ran them on and stores where it always stored: the in-kernel
//     path of every variant, of the eleven derived kernels, of the safe and continuation passes;
//   * front_scalars_kernel (hmpc_front.hip) calls them for a whole batch, sixteen lanes per instance, ahead of the fast two-contact solve
//     kernels, which then only scatter the results (struct FrontScalars) into their LDS.
// The same operation sequence per value under the same flags (-ffp-contract=off, explicit dfma / ffma) makes the two paths bit-identical
// by construction (HMPC-A1).  Compiles under hipcc and, for tests/test_front_on_host.py, as plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if !defined(__HIPCC__)
#include <math.h>
#endif

#include "hmpc_math.h"
#include "hmpc_record.h"

namespace hmpc {

// body rotation from the quaternion (RobotState.cpp:17-30; Eigen toRotationMatrix closed form) and its transpose
__device__ inline void quat_to_R(const float *q, float *R, float *Rt) {
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
  float twx = tx * qw, twy = ty * qw, twz = tz * qw;
  float txx = tx * qx, txy = ty * qx, txz = tz * qx;
  float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1.0f - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0f - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0f - (txx + tyy);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) Rt[k * 3 + i] = R[i * 3 + k];
}

// ---- A1: trigonometry (SolverMPC.cpp:374-393, 333-342, 74-85)
// joint angle i of the record with the reference's offsets, reduced to (-2 pi, 2 pi)
__device__ __forceinline__ float front_joint(const float *in_ja, const int i) {
  const double PI = 3.14159265359, PI2 = 2 * PI;
  float a = in_ja[i];
  const int k = i % 5;
  if (k == 2 || k == 4) a = (float)((double)a + 0.3 * PI);
  if (k == 3) a = (float)((double)a - 0.6 * PI);
  const double ad = (double)a;
  return (float)((__builtin_fabs(ad) < PI2) ? ad : fmod(ad, PI2));  // fmod(x,y) == x exactly when |x| < y
}
// the angle whose sine and cosine role t wants: t < 10 the joint angles, t = 10, 11 q2+q3+q4 of each leg
__device__ __forceinline__ float front_trig_angle(const float *in_ja, const int t) {
  const int b = 5 * (t - 10);
  return (t < 10) ? front_joint(in_ja, t) : (front_joint(in_ja, b + 2) + front_joint(in_ja, b + 3)) + front_joint(in_ja, b + 4);
}
// Euler angle WHICH (0 roll, 1 pitch, 2 yaw) of the quaternion = det_atan2(y, x) of these arguments (pitch: det_asin's own)
template <int WHICH>
__device__ __forceinline__ void front_euler_args(const float *in_q, double &y, double &x) {
  const float qw = in_q[0], qx = in_q[1], qy = in_q[2], qz = in_q[3];
  if constexpr (WHICH == 0) {
    float n0 = 2.0f * (qw * qx + qy * qz);
    double d0 = 1.0 - (double)(2.0f * (qx * qx + qy * qy));
    y = (double)n0, x = d0;
  } else if constexpr (WHICH == 1) {
    float t = qw * qy - qx * qz;
    double asd = 2.0 * (double)t;
    if (!(asd < 0.99999)) asd = 0.99999;
    float as = (float)asd;
    const double v = (double)as;
    y = v, x = __builtin_sqrt((1.0 - v) * (1.0 + v));
  } else {
    float n2 = 2.0f * (qw * qz + qx * qy);
    double d2 = 1.0 - (double)(2.0f * (qy * qy + qz * qz));
    y = (double)n2, x = d2;
  }
}
template <int WHICH>
__device__ __forceinline__ float front_euler_angle(const float *in_q) {
  double y, x;
  front_euler_args<WHICH>(in_q, y, x);
  return (float)det_atan2(y, x);
}
// a leg-step survives iff its Fz bound cap * gait is not ~0 (stance(), SolverMPC.cpp:589-637): per step the leg-steps and variables
// before it and its stance bits; nv, nl = the totals.  fz_cap(c) = the Fz cap of contact c
template <int NC, class CAP>
__device__ __forceinline__ void front_prefix(const unsigned char *gait, const int h, CAP fz_cap, unsigned char *pre_nl, unsigned char *pre_nv,
                                             unsigned char *pre_st, int &nv_out, int &nl_out) {
  int nv = 0, nl = 0;
  for (int i = 0; i < h; ++i) {
    int bits = 0, nst = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool st = stance(fz_cap(c), gait[NC * i + c]);
      bits |= st ? (1 << c) : 0;
      nst += (int)st;
    }
    pre_nl[i] = (unsigned char)(nl > 255 ? 255 : nl);
    pre_nv[i] = (unsigned char)(nv > 255 ? 255 : nv);
    pre_st[i] = (unsigned char)bits;
    nv += 6 * nst;
    nl += nst;
  }
  nv_out = nv, nl_out = nl;
}

// ---- A2: scalar algebra (RobotState.cpp:17-47, SolverMPC.cpp:65-89, 302-331, 420-433, 488-548)
// the body: the non-structural entries of the forward-Euler model (SolverMPC.cpp:312-331, 145-146) -- Acd's rows 0-2, columns 6-8
// (0 + dt Rbi), Bcd's rows 6-8: dt Iinv [r_leg]x per leg and dt Iinv.  ypsc = cos / sin of yaw, then of pitch
template <int NC>
__device__ __forceinline__ void front_body(const float *in_q, const float *ypsc, const float *in_r, const float *Ib3, const float dt,
                                           float *Rbi_dt, float *Iinv_dt, float (*blk_dt)[9]) {
  float R[9], Rt[9];
  quat_to_R(in_q, R, Rt);
  float Rbi[9];
  {
    const float cy = ypsc[0], sy = ypsc[1], cp = ypsc[2], sp = ypsc[3];
    float Rb[9] = {cy * cp, -sy, 0.0f, sy * cp, cy, 0.0f, -sp, 0.0f, 1.0f};
    inverse3(Rb, Rbi);
  }
  const float Ib[3] = {Ib3[0], Ib3[1], Ib3[2]};  // 0.5413, 0.5200, 0.0691 (RobotState.cpp:45)
  float RI[9], Iw[9], Iinv[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) RI[i * 3 + k] = R[i * 3 + k] * Ib[k];
  chain_mm<3, 3, 3>(RI, Rt, Iw);
  inverse3(Iw, Iinv);
#pragma unroll
  for (int k = 0; k < 9; ++k) Rbi_dt[k] = 0.0f + dt * Rbi[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) Iinv_dt[k] = dt * Iinv[k];
#pragma unroll
  for (int leg = 0; leg < NC; ++leg) {
    const float r0 = in_r[0 * NC + leg], r1 = in_r[1 * NC + leg], r2 = in_r[2 * NC + leg];
    float cm[9] = {0.0f, -r2, r1, r2, 0.0f, -r0, -r1, r0, 0.0f};
    float blk[9];
    chain_mm<3, 3, 3>(Iinv, cm, blk);
#pragma unroll
    for (int k = 0; k < 9; ++k) blk_dt[leg][k] = dt * blk[k];
  }
}
// one contact: foot rotation Rz(q0)Rx(q1)Ry(q2)Ry(q3)Ry(q4) (SolverMPC.cpp:426-433; the hand's frame `rh`, an input of the extension
// record, where NC == 3 and leg == 2) and the four vectors its 8 rows of the constraint block are made of (SolverMPC.cpp:488-548):
// t0, t1 = the frame's x and y axes in the body frame, flt, flh = its z axis scaled by the toe / heel lever arms.  sc[k] = (sin, cos)
// of joint angle k, sc234[leg] of q2+q3+q4
template <int NC>
__device__ __forceinline__ void front_foot(const float *in_q, const float (*sc)[2], const float (*sc234)[2], const int leg, const float lt,
                                           const float lh, const float *rh, float *t0, float *t1, float *flt, float *flh) {
  float R[9], Rt[9];
  quat_to_R(in_q, R, Rt);
  const int b = (leg < 2) ? 5 * leg : 0;
  const float s0 = sc[b][0], c0 = sc[b][1], s1 = sc[b + 1][0], c1 = sc[b + 1][1];
  const float s2 = sc[b + 2][0], c2 = sc[b + 2][1], s3 = sc[b + 3][0], c3 = sc[b + 3][1];
  const float s4 = sc[b + 4][0], c4 = sc[b + 4][1];
  const float s234 = sc234[leg & 1][0], c234 = sc234[leg & 1][1];
  // every operation in the type C++ gives it at SolverMPC.cpp:428-433: the "1.0" / "-1.0" literals promote the
  // product they start, and whatever that product is combined with, to binary64; one narrowing per entry
  const float a = c0 * s2 + (c2 * s0) * s1;
  const double bb = (double)(c0 * c2) - (((double)s0 * (double)s1) * (double)s2);
  const float d = c2 * s0 + (c0 * s1) * s2;
  const double e = (double)(s0 * s2) - (((double)c0 * (double)c2) * (double)s1);
  const double X = (double)(c3 * a) + (double)s3 * bb;
  const double Y = ((double)s3 * (double)a) - (double)c3 * bb;
  const double P = (double)(c3 * d) - ((double)s3) * e;
  const double Q = (double)(s3 * d) + (double)c3 * e;
  float Rf[9];
  Rf[0] = (float)((-(double)s4) * X - (double)c4 * Y);
  Rf[1] = -(c1 * s0);
  Rf[2] = (float)((double)c4 * X - (double)s4 * Y);
  Rf[3] = (float)((double)c4 * P - (double)s4 * Q);
  Rf[4] = c0 * c1;
  Rf[5] = (float)((double)c4 * Q + (double)s4 * P);
  Rf[6] = -(s234 * c1);
  Rf[7] = s1;
  Rf[8] = c234 * c1;
  if (NC == 3 && leg == 2) {  // the hand's contact frame is an input of the extension record
#pragma unroll
    for (int k = 0; k < 9; ++k) Rf[k] = rh[k];
  }
  float col0[3], col1[3], vlt[3], vlh[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    col0[k] = Rf[k * 3 + 0];
    col1[k] = Rf[k * 3 + 1];
    vlt[k] = -lt * Rf[k * 3 + 2];
    vlh[k] = -lh * Rf[k * 3 + 2];
  }
  chain_mm<1, 3, 3>(col0, Rt, t0);
  chain_mm<1, 3, 3>(col1, Rt, t1);
  chain_mm<1, 3, 3>(vlt, Rt, flt);
  chain_mm<1, 3, 3>(vlh, Rt, flh);
}

// ---- what front_scalars_kernel leaves for the fast two-contact solve kernels: one fixed-size block per instance, an array of structs
// so that a workgroup's read is one coalesced burst like the record's.  Only what is not structure: everything copied from the record,
// the handle's constants, the zeros and identities and the index tables stay with the solve kernel.
constexpr int FRONT_STEPS = 20;  // horizon steps a block has room for (the family's longest horizon)
struct FrontScalars {
  float rpy[3];         // x0[0..2]
  float Rbi_dt[9];      // Acd rows 0-2, columns 6-8: 0 + dt Rbi
  float Iinv_dt[9];     // Bcd rows 6-8, the moment columns of either leg
  float blk_dt[2][9];   // Bcd rows 6-8, the force columns of leg: dt Iinv [r_leg]x
  float foot[2][12];    // per leg t0, t1, flt, flh (front_foot)
  float pad0;
  unsigned char pre_nl[FRONT_STEPS], pre_nv[FRONT_STEPS], pre_st[FRONT_STEPS];  // front_prefix; zero beyond the horizon
  unsigned short n, nls;  // reduced variables, stance leg-steps
};
constexpr int FRONT_WORDS = (int)(sizeof(FrontScalars) / 4);
static_assert(sizeof(FrontScalars) == 320 && sizeof(FrontScalars) % 16 == 0, "one block = 80 words, a multiple of 16 B");

// ---- how a solve kernel rebuilds its arrays from a block (front_scatter, hmpc_kernel.h): an entry is its structural constant or its
// value from the block, decided by its own index.  Two contacts: 12 variables per horizon step, a 16 x 12 constraint block.  Written
// without a branch -- ONE read of the block per entry at an index that is always inside it, then a select --, so that the reads of all
// the arrays a lane fills are in flight together.
constexpr int FW_RPY = 0, FW_RBI = 3, FW_IINV = 12, FW_BLK = 21, FW_FOOT = 39;  // float offsets of the block's members
static_assert(offsetof(FrontScalars, Rbi_dt) == 4 * FW_RBI && offsetof(FrontScalars, Iinv_dt) == 4 * FW_IINV &&
                  offsetof(FrontScalars, blk_dt) == 4 * FW_BLK && offsetof(FrontScalars, foot) == 4 * FW_FOOT, "struct FrontScalars");
// entry t of Acd = I + dt A_ct, 13 x 13 (SolverMPC.cpp:312-331)
__device__ __forceinline__ float front_acd_entry(const FrontScalars &F, const int t, const float dt) {
  const float *Fw = reinterpret_cast<const float *>(&F);
  const int i = t / 13, j = t - 13 * i;
  const bool use = i < 3 && j >= 6 && j < 9;
  const float ld = Fw[use ? FW_RBI + 3 * i + j - 6 : 0];
  const float c = (i == j) ? 1.0f  // fl(delta + dt*0) = delta
                           : (i >= 3 && i < 6 && j == i + 6) ? 0.0f + dt * 1.0f : (i == 11 && j == 12) ? 0.0f + dt * -1.0f : 0.0f;
  return use ? ld : c;
}
// entry t of Bcd = dt B_ct, 13 x 12; inv_mass = fl(1 / mass) (9.0 in the reference, SolverMPC.cpp:423)
__device__ __forceinline__ float front_bcd_entry(const FrontScalars &F, const int t, const float dt, const float inv_mass) {
  const float *Fw = reinterpret_cast<const float *>(&F);
  const int i = t / 12, j = t - 12 * i;
  const bool use = i >= 6 && i < 9;
  const int k = 3 * (i - 6) + j % 3;
  const float ld = Fw[use ? ((j < 6) ? FW_BLK + 9 * (j / 3) + k : FW_IINV + k) : 0];
  const float c = (i >= 9 && i < 12 && j < 6 && j % 3 == i - 9) ? dt * inv_mass : 0.0f;  // fl(dt*0) = 0
  return use ? ld : c;
}
// entry (r, c) of the 16 x 12 constraint block (SolverMPC.cpp:488-548): rows 8 leg .. 8 leg + 7 are the leg's -- 0-3 friction
// (-+mu on x, y; 1 on z), 4 t0 on the moment, 5 flt on the force and t1 on the moment, 6 flh and -+t1, 7 the Fz row
__device__ __forceinline__ float front_fc_entry(const FrontScalars &F, const int r, const int c, const float mu) {
  const float *Fw = reinterpret_cast<const float *>(&F);
  const int leg = r >> 3, rr = r & 7;
  const int kf = c - 3 * leg, km = c - (6 + 3 * leg);  // 0..2: the column is this leg's force / moment component
  const bool isf = kf >= 0 && kf < 3, ism = km >= 0 && km < 3;
  // where in the leg's (t0, t1, flt, flh) the entry comes from; -1: a constant
  const int src = (rr == 4) ? (ism ? km : -1) : (rr == 5) ? (isf ? 6 + kf : (ism ? 3 + km : -1)) : (rr == 6) ? (isf ? 9 + kf : (ism ? 3 + km : -1)) : -1;
  const float ld = Fw[FW_FOOT + 12 * leg + (src < 0 ? 0 : src)];
  const float con = (rr < 4) ? ((isf && kf == 2) ? 1.0f : ((isf && kf == (rr >> 1)) ? ((rr & 1) ? mu : -mu) : 0.0f))
                             : ((rr == 7 && isf && kf == 2) ? 2.0f : 0.0f);
  const float v = (rr == 6 && ism && leg != 1) ? -ld : ld;
  return (src >= 0) ? v : con;
}
// entry t of x0 (13): rpy, then position, angular and linear velocity from the record rf, then the gravity state (SolverMPC.cpp:420)
__device__ __forceinline__ float front_x0_entry(const FrontScalars &F, const float *rf, const int t, const float gravity) {
  using RL = RecLayout<2>;
  const float a = F.rpy[t < 3 ? t : 0];
  const float b = rf[(t < 6) ? RL::P + t - 3 : (t < 9) ? RL::W + t - 6 : (t < 12) ? RL::V + t - 9 : 0];
  return (t < 3) ? a : (t < 12) ? b : gravity;
}

// what the prologue reads of the handle (set_problem_args fills the same fields of KernelArgs from the same members)
struct FrontArgs {
  const unsigned char *records;
  int stride, batch, horizon;
  float dt, f_max, Ib[3], lt, lh;
};
// mapping of front_scalars_kernel: FRONT_LANES lanes per instance -- the roles of stage A1 --, FRONT_IPW instances per workgroup
constexpr int FRONT_LANES = 16, FRONT_NT = 256, FRONT_IPW = FRONT_NT / FRONT_LANES;

#pragma GCC visibility push(hidden)
// out[a.batch] from a.records, on `stream` (hmpc_front.hip); a batch of 0 launches nothing
hipError_t launch_front_scalars(const FrontArgs &a, FrontScalars *out, hipStream_t stream);
#pragma GCC visibility pop

}  // namespace hmpc
