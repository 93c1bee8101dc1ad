// hmpc_swing.h -- the swing half of a tick's motor command, batched on the device: (tick structs, swing state, the
// tick's torques) -> one complete command per joint (q, dq, Kp, Kd, tau) and the swing state of the next update.  It is the reference's
// swingLegController::updateSwingLeg() (common/SwingLegController.cpp): foot position from the joint angles, swing sub-phase and timer,
// touchdown point, Bezier foot trajectory, body-frame target, the approximate 5-DoF inverse kinematics, gains.
// THE ARITHMETIC IS A CONTRACT: binary64, correctly rounded IEEE operations only, no contraction (hmpc_swing.hip is built with
// -ffp-contract=off, HMPC-A1 of DESIGN.md section 3), in the operation order the comment of include/hector_mpc.h above struct hmpc_swing
// writes out -- the numbering below is that comment's.  tests/swing_mirror.py restates the comment in numpy; what passes through
// trigonometry (det_sincos / det_atan2 / det_asin here, libm there) agrees within a measured tolerance, everything else bit for bit.
// Mapping: thread g -> instance g / 2, leg g % 2, as leg_torque_kernel; 256 threads per workgroup, nothing synchronised.  A thread reads
// ~0.3 KB of its tick struct and its leg's entries of the state: plain loads and stores, no LDS, no atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"
#include "hmpc_math.h"

namespace hmpc {

constexpr int SWING_NT = 256;
constexpr int SWING_DETAIL = 16;  // doubles per (instance, leg) of the detail buffer

// what a launch of the swing update reads besides the tick structs (by value: the host's hmpc_swing, the handle's horizon, the buffers)
struct SwingArgs {
  hmpc_swing cfg;
  int batch, horizon;
  hmpc_swing_state *state;  // [batch]
  const double *tau;        // [batch][10] or nullptr = zeros
  hmpc_motor_cmd *cmd;      // row i * cmd_stride + cmd_row, or nullptr = not written (a rollout without a command log)
  int cmd_stride, cmd_row;
  double *detail;           // [batch][2][SWING_DETAIL] or nullptr
};

__device__ __forceinline__ double swing_clamp1(double v) {
  const double t = (1.0 < v) ? 1.0 : v;
  return (-1.0 < t) ? t : -1.0;
}
__device__ __forceinline__ double swing_acos(double v) { return det_atan2(__builtin_sqrt((1.0 - v) * (1.0 + v)), v); }
__device__ __forceinline__ double swing_bez(double y0, double yf, double x) { return y0 + (x * x * x + 3 * (x * x * (1 - x))) * (yf - y0); }
__device__ __forceinline__ double swing_dbez(double y0, double yf, double x) { return (6 * x * (1 - x)) * (yf - y0); }

// step 2: data[leg].p of LegController.cpp:190-193 at the offset joint angles q[5]
__device__ inline void swing_leg_p(const double *q, double side, double *p) {
  double s0, c0, s1, c1, s2, c2, s3, c3, s4, c4;
  det_sincos(q[0], s0, c0);
  det_sincos(q[1], s1, c1);
  det_sincos(q[2], s2, c2);
  det_sincos(q[3], s3, c3);
  det_sincos(q[4], s4, c4);
  const double A = c0 * c2 - s0 * s1 * s2, B = c0 * s2 + c2 * s0 * s1, C = c2 * s0 + c0 * s1 * s2, D = s0 * s2 - c0 * c2 * s1;
  p[0] = -(3 * c0) / 200 - (9 * s4 * (c3 * A - s3 * B)) / 250 - (11 * c0 * s2) / 50 - (side * s0) / 50 - (11 * c3 * B) / 50 -
         (11 * s3 * A) / 50 - (9 * c4 * (c3 * B + s3 * A)) / 250 - (23 * c1 * side * s0) / 1000 - (11 * c2 * s0 * s1) / 50;
  p[1] = (c0 * side) / 50 - (9 * s4 * (c3 * C - s3 * D)) / 250 - (3 * s0) / 200 - (11 * s0 * s2) / 50 - (11 * c3 * D) / 50 -
         (11 * s3 * C) / 50 - (9 * c4 * (c3 * D + s3 * C)) / 250 + (23 * c0 * c1 * side) / 1000 + (11 * c0 * c2 * s1) / 50;
  p[2] = (23 * side * s1) / 1000 - (11 * c1 * c2) / 50 - (9 * c4 * (c1 * c2 * c3 - c1 * s2 * s3)) / 250 +
         (9 * s4 * (c1 * c2 * s3 + c1 * c3 * s2)) / 250 - (11 * c1 * c2 * c3) / 50 + (11 * c1 * s2 * s3) / 50 - 3.0 / 50.0;
}

// step 3: Gait::getSwingSubPhase() of leg j after setIterations(ticks_per_step, gait_iteration * ticks_per_step + subtick)
__device__ inline double swing_sub_phase(const hmpc_tick_inputs &tk, const hmpc_swing &c, int h, int j) {
  const int cur = tk.gait_iteration * c.ticks_per_step + c.subtick, per = c.ticks_per_step * h;
  const double phase = (double)(cur % per) / (double)per;
  const double offP = (double)tk.gait_offsets[j] / (double)h, durP = (double)tk.gait_durations[j] / (double)h;
  double so = offP + durP;
  if (so > 1) so = so - 1.;
  const double sd = 1. - durP;
  double pr = phase - so;
  if (pr < 0) pr = pr + 1.;
  return (pr > sd) ? 0. : (sd == 0 ? 0. : pr / sd);
}

// step 7: computeIK; f-independent inputs: q2, q3 = the leg's offset joint angles 2 and 3
__device__ inline void swing_ik(const double *pFoot_b, const hmpc_swing &c, int j, double q2, double q3, double *ik) {
  const double PI = 3.141592653589793;
  const double sideK = (j == 0) ? -1.0 : 1.0;
  const double hr[3] = {c.hip_roll[0] - c.ik_hip_x, 0.0, c.hip_yaw[0][2] + c.hip_roll[2] * 2};
  double f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) f[k] = pFoot_b[k] - hr[k];
  const double d3 = __builtin_sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]), dyz = __builtin_sqrt(f[1] * f[1] + f[2] * f[2]);
  const double dh = c.ik_horizontal, L = c.ik_link;
  const double m = dyz * dyz - dh * dh;
  const double dv = __builtin_sqrt((0.00001 < m) ? m : 0.00001), dxz = __builtin_sqrt(d3 * d3 - dh * dh);
  const double a1 = swing_clamp1(dxz / (2.0 * L)), a2 = swing_clamp1(dv / dxz);
  double div = __builtin_fabs(f[0]);
  if (div == 0.0) div = 1e-6;
  ik[0] = 0.0;
  ik[1] = det_asin(swing_clamp1(f[1] / dyz)) + det_asin(swing_clamp1(dh * sideK / dyz));
  ik[2] = swing_acos(a1) - swing_acos(a2) * f[0] / div;
  ik[3] = 2.0 * det_asin(swing_clamp1(dxz / 2.0 / L)) - PI;
  ik[4] = -q3 - q2;
  ik[2] = ik[2] - 0.3 * PI;
  ik[3] = ik[3] + 0.6 * PI;
  ik[4] = ik[4] - 0.3 * PI;
}

// One leg of one instance: `c.updates` updates of its state, then the command's five joints.  out[0..4] q, [5..9] Kp, [10..14] Kd; det = the
// detail row (SWING_DETAIL doubles) or nullptr.
__device__ inline void swing_leg_update(const hmpc_tick_inputs &tk, const hmpc_swing &c, int h, int j, hmpc_swing_state &st, double *out,
                                        double *det) {
  double q[5], R[9], pos[3], v[3];
#pragma unroll
  for (int k = 0; k < 5; ++k) q[k] = tk.leg_q[5 * j + k];
  if (tk.flags & HMPC_TICK_LEG_Q_MOTOR) q[2] = q[2] + 0.3 * 3.14159, q[3] = q[3] - 0.6 * 3.14159, q[4] = q[4] + 0.3 * 3.14159;  // 1
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = tk.rBody[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = tk.position[k], v[k] = tk.vWorld[k];
  const double *hy = c.hip_yaw[j];
  double p[3], u[3], pFoot_w[3];
  swing_leg_p(q, (j == 0) ? 1.0 : -1.0, p);  // 2
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = hy[k] + p[k];
#pragma unroll
  for (int k = 0; k < 2; ++k) pFoot_w[k] = pos[k] + (R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2]);
  pFoot_w[2] = 0.0;
  const double swing = swing_sub_phase(tk, c, h, j);  // 3
  int first = st.first_swing[j];
  double timer = st.swing_time[j], p0[3], pf[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p0[k] = st.p0[j][k], pf[k] = st.pf[j][k];
  const double cx = tk.v_des_robot[0], cy = tk.v_des_robot[1], stance = (double)tk.gait_durations[0];
  double vdw[2], rh[3];
#pragma unroll
  for (int a = 0; a < 2; ++a) vdw[a] = R[a] * cx + R[3 + a] * cy + R[6 + a] * 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) rh[k] = R[k] * hy[0] + R[3 + k] * hy[1] + R[6 + k] * hy[2];
  for (int upd = 0; upd < c.updates; ++upd) {
    if (first) {  // 4
      timer = c.dtMPC * (double)(h - tk.gait_durations[0]);
    } else {
      timer = timer - c.dt_update;
      if (timer <= 0) first = 1;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {  // 5
      const double Pf = (pos[a] + rh[a]) + v[a] * timer;
      double rel = c.place_gain_v * v[a] * 0.5 * stance * c.dtMPC + c.place_gain_err * (v[a] - vdw[a]);
      rel = (double)fminf(fmaxf((float)rel, (float)-c.place_max), (float)c.place_max);
      pf[a] = Pf + rel;
    }
    pf[2] = 0.0;
    if (swing > 0 && first) {  // 6a
      first = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) p0[k] = pFoot_w[k];
    }
  }
  st.first_swing[j] = first;
  st.swing_time[j] = timer;
#pragma unroll
  for (int k = 0; k < 3; ++k) st.p0[j][k] = p0[k], st.pf[j][k] = pf[k];
  double pDes[3] = {0.0, 0.0, 0.0}, vDes[3] = {0.0, 0.0, 0.0}, pFoot_b[3] = {0.0, 0.0, 0.0}, vFoot_b[3] = {0.0, 0.0, 0.0};
  if (swing > 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) pDes[k] = swing_bez(p0[k], pf[k], swing), vDes[k] = swing_dbez(p0[k], pf[k], swing);  // 6b
    const double top = p0[2] + c.height;
    if (swing < 0.5) {
      const double x = swing * 2;
      pDes[2] = swing_bez(p0[2], top, x), vDes[2] = swing_dbez(p0[2], top, x);
    } else {
      const double x = swing * 2 - 1;
      pDes[2] = swing_bez(top, pf[2], x), vDes[2] = swing_dbez(top, pf[2], x);
    }
    double d[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = pDes[k] - pos[k], e[k] = vDes[k] * 0.0 - v[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pFoot_b[k] = (R[3 * k] * d[0] + R[3 * k + 1] * d[1] + R[3 * k + 2] * d[2]) + c.hip_width_offset[j][k];
      vFoot_b[k] = R[3 * k] * e[0] + R[3 * k + 1] * e[1] + R[3 * k + 2] * e[2];
    }
    double ik[5];
    swing_ik(pFoot_b, c, j, q[2], q[3], ik);  // 7
#pragma unroll
    for (int k = 0; k < 5; ++k) st.q_des[5 * j + k] = ik[k], out[k] = ik[k], out[5 + k] = c.kp[k], out[10 + k] = c.kd[k];  // 8
  } else {
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = st.q_des[5 * j + k], out[5 + k] = 0.0, out[10 + k] = 0.0;
  }
  if (det) {
    det[0] = swing;
#pragma unroll
    for (int k = 0; k < 3; ++k) det[1 + k] = pFoot_w[k], det[4 + k] = pDes[k], det[7 + k] = vDes[k], det[10 + k] = pFoot_b[k], det[13 + k] = vFoot_b[k];
  }
}

__global__ __launch_bounds__(SWING_NT) void swing_legs_kernel(const hmpc_tick_inputs *ticks, SwingArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * a.batch) return;
  const int i = g >> 1, j = g & 1;
  double out[15];
  swing_leg_update(ticks[i], a.cfg, a.horizon, j, a.state[i], out, a.detail ? a.detail + (size_t)g * SWING_DETAIL : nullptr);
  if (a.cmd) {
    hmpc_motor_cmd &cm = a.cmd[(size_t)i * a.cmd_stride + a.cmd_row];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      cm.q[5 * j + k] = out[k], cm.dq[5 * j + k] = 0.0, cm.Kp[5 * j + k] = out[5 + k], cm.Kd[5 * j + k] = out[10 + k];
      cm.tau[5 * j + k] = a.tau ? a.tau[(size_t)10 * i + 5 * j + k] : 0.0;
    }
  }
}

// the reference's initial state: all-zero bytes, firstSwing = {true, true}
__global__ __launch_bounds__(SWING_NT) void swing_state_init_kernel(hmpc_swing_state *state, int batch) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * batch) return;
  const int i = g >> 1, j = g & 1;
  hmpc_swing_state &st = state[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) st.p0[j][k] = 0.0, st.pf[j][k] = 0.0;
  st.swing_time[j] = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) st.q_des[5 * j + k] = 0.0;
  st.first_swing[j] = 1;
}

}  // namespace hmpc
