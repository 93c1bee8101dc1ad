// hmpc_plant.h -- the plant side of a closed loop, batched on the device: (tick structs, step-0 forces) -> the tick
// structs of the next tick, in place.  The plant is the single rigid body the MPC predicts with (SolverMPC.cpp:312-331), integrated
// semi-implicitly with a quaternion attitude; swing feet are placed by the reference's heuristic (ConvexMPCLocomotion.cpp:148-164), stance
// feet and leg_q are never written (the plant has no legs).
// THE ARITHMETIC IS A CONTRACT: binary64, correctly rounded IEEE operations only, no contraction (hmpc_plant.hip is built with
// -ffp-contract=off, HMPC-A1 of DESIGN.md section 3), in the operation order the comment of include/hector_mpc.h above struct hmpc_plant
// writes out, step by step -- the numbering below is that comment's.  tests/rollout_mirror.py restates the comment in numpy and is compared
// with this kernel bit for bit (rpy excepted: det_atan2 / det_asin against libm).
// Mapping: one thread per instance, 256 threads per workgroup, nothing synchronised.  A thread reads the ~0.4 KB of its tick struct that
// change and 12 floats, and writes back the fields that changed: plain loads and stores, no LDS, no atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"
#include "hmpc_math.h"

namespace hmpc {

constexpr int PLANT_NT = 256;

// what a launch of the plant step reads besides the tick structs (by value: the host's hmpc_plant, the handle's horizon, the buffers)
struct PlantArgs {
  hmpc_plant plant;
  int batch, horizon;
  const float *forces;
  int force_stride;
  const uint32_t *status;
  const double *wpd;   // [batch][2] or nullptr
  int32_t *summary;    // [batch][4] or nullptr
  // the rollout's log (hmpc_rollout_log; every pointer may be nullptr): row (instance, tick) of n_ticks
  hmpc_rollout_log log;
  const double *tau;   // [batch][10], what the tick's torque launch wrote (read only when log.tau is set)
  int tick, n_ticks;
};

__device__ __forceinline__ void plant_cross(const double *x, const double *y, double *out) {
  out[0] = x[1] * y[2] - x[2] * y[1];
  out[1] = x[2] * y[0] - x[0] * y[2];
  out[2] = x[0] * y[1] - x[1] * y[0];
}

// step 12: rBody = transpose of the polynomial of orientation_tools.h:182-200
__device__ __forceinline__ void plant_rbody(const double *q, double *R) {
  const double e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3];
  R[0] = 1 - 2 * (e2 * e2 + e3 * e3), R[3] = 2 * (e1 * e2 - e0 * e3), R[6] = 2 * (e1 * e3 + e0 * e2);
  R[1] = 2 * (e1 * e2 + e0 * e3), R[4] = 1 - 2 * (e1 * e1 + e3 * e3), R[7] = 2 * (e2 * e3 - e0 * e1);
  R[2] = 2 * (e1 * e3 - e0 * e2), R[5] = 2 * (e2 * e3 + e0 * e1), R[8] = 1 - 2 * (e1 * e1 + e2 * e2);
}

// One instance, one tick.  Returns whether the tick struct was stepped (false: it had fallen before).
__device__ inline bool plant_step_instance(hmpc_tick_inputs &tk, const hmpc_plant &pl, int horizon, double m, const double *ext,
                                           const float *u0f, const double *wpd_base, bool &fell_now) {
  fell_now = false;
  const int flags_in = tk.flags;
  if (flags_in & HMPC_TICK_FALLEN) return false;
  double u0[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) u0[k] = (double)u0f[k];
  const double *FL = u0, *FR = u0 + 3, *ML = u0 + 6, *MR = u0 + 9;
  double p[3], v[3], w[3], q[4], R[9], foot[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = tk.position[k], v[k] = tk.vWorld[k], w[k] = tk.omegaWorld[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = tk.orientation[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = tk.rBody[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) foot[k] = tk.pFoot[k];
  const double cx = tk.v_des_robot[0], cy = tk.v_des_robot[1];
  double vdw0[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) vdw0[a] = (R[a] * cx + R[3 + a] * cy) + R[6 + a] * 0.0;
  const double *I = pl.inertia;
  const double d = pl.dt_tick / (double)pl.substeps, hd = 0.5 * d;
  for (int s = 0; s < pl.substeps; ++s) {
    double rL[3], rR[3], cL[3], cR[3], tau[3], F[3], tb[3], ab[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rL[k] = foot[k] - p[k], rR[k] = foot[3 + k] - p[k];  // 1
    plant_cross(rL, FL, cL);
    plant_cross(rR, FR, cR);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tau[k] = ((cL[k] + ML[k]) + (cR[k] + MR[k])) + ext[3 + k];  // 2
      F[k] = (FL[k] + FR[k]) + ext[k];                            // 3
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) tb[k] = (R[3 * k] * tau[0] + R[3 * k + 1] * tau[1]) + R[3 * k + 2] * tau[2];  // 4
    if (pl.flags & HMPC_PLANT_GYRO) {                                                                         // 5
      double wb[3], Iw[3], gy[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        wb[k] = (R[3 * k] * w[0] + R[3 * k + 1] * w[1]) + R[3 * k + 2] * w[2];
        Iw[k] = I[k] * wb[k];
      }
      plant_cross(wb, Iw, gy);
#pragma unroll
      for (int k = 0; k < 3; ++k) tb[k] = tb[k] - gy[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) ab[k] = tb[k] / I[k];  // 6
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double alpha = (R[k] * ab[0] + R[3 + k] * ab[1]) + R[6 + k] * ab[2];
      const double a = F[k] / m + (k == 2 ? -pl.gravity : 0.0);  // 7
      w[k] = w[k] + d * alpha;                                   // 8
      v[k] = v[k] + d * a;                                       // 9
      p[k] = p[k] + d * v[k];                                    // 10
    }
    double e[4];  // 11
    e[0] = -((w[0] * q[1] + w[1] * q[2]) + w[2] * q[3]);
    e[1] = (w[0] * q[0] + w[1] * q[3]) - w[2] * q[2];
    e[2] = (w[1] * q[0] + w[2] * q[1]) - w[0] * q[3];
    e[3] = (w[2] * q[0] + w[0] * q[2]) - w[1] * q[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] + hd * e[k];
    const double n = __builtin_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
    plant_rbody(q, R);  // 12
  }
  // once per tick
#pragma unroll
  for (int k = 0; k < 3; ++k) tk.position[k] = p[k], tk.vWorld[k] = v[k], tk.omegaWorld[k] = w[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) tk.orientation[k] = q[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) tk.rBody[k] = R[k];
  tk.rpy[0] = det_atan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]));
  double sp = 2 * (q[0] * q[2] - q[1] * q[3]);
  if (!(sp < 0.99999)) sp = 0.99999;
  if (sp < -0.99999) sp = -0.99999;  // (two-sided, unlike the solve kernel's quat_to_rpy: rounding takes |sp| past 1 at pitch -90 degrees too)
  tk.rpy[1] = det_asin(sp);
  tk.rpy[2] = det_atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3]));
#pragma unroll
  for (int a = 0; a < 2; ++a) tk.world_position_desired[a] = wpd_base[a] + pl.dt_tick * vdw0[a];
  int gi = tk.gait_iteration;
  if (pl.advance_gait) {
    gi = (gi + 1) % horizon;
    tk.gait_iteration = gi;
  }
  if (pl.flags & HMPC_PLANT_PLACE_FEET) {
    double vdw[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) vdw[a] = (R[a] * cx + R[3 + a] * cy) + R[6 + a] * 0.0;
    const double stance_steps = (double)tk.gait_durations[0];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int progress = gi % horizon - tk.gait_offsets[j];
      if (progress < 0) progress += horizon;
      if (progress < tk.gait_durations[j]) continue;  // in stance: the foot stays where it is, bit for bit
      double Pf[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double rh = (R[k] * pl.hip[j][0] + R[3 + k] * pl.hip[j][1]) + R[6 + k] * pl.hip[j][2];
        Pf[k] = (p[k] + rh) + v[k] * 0.0;
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        double rel = ((v[a] * 0.5) * stance_steps) * pl.dtMPC + 0.02 * (v[a] - vdw[a]);
        rel = (double)fminf(fmaxf((float)rel, (float)-0.4), (float)0.4);
        tk.pFoot[3 * j + a] = Pf[a] + rel;
      }
      tk.pFoot[3 * j + 2] = 0.0;
    }
  }
  if (R[8] < pl.fall_cos) {
    tk.flags = flags_in | HMPC_TICK_FALLEN;
    fell_now = true;
  }
  return true;
}

__global__ __launch_bounds__(PLANT_NT) void plant_step_kernel(hmpc_tick_inputs *ticks, PlantArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.batch) return;
  const float *u0f = a.forces + (size_t)i * a.force_stride;
  const uint32_t st = a.status[i];
  hmpc_tick_inputs &tk = ticks[i];
  double ext[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) ext[k] = a.plant.device_ext_wrench ? a.plant.device_ext_wrench[(size_t)6 * i + k] : 0.0;
  const double m = a.plant.device_mass ? a.plant.device_mass[i] : a.plant.mass;
  double base[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) base[k] = a.wpd ? a.wpd[(size_t)2 * i + k] : tk.world_position_desired[k];
  bool fell_now;
  const bool stepped = plant_step_instance(tk, a.plant, a.horizon, m, ext, u0f, base, fell_now);
  if (stepped && a.summary) {
    int32_t *row = a.summary + (size_t)4 * i;
    const int32_t done = row[0];
    if (fell_now && row[1] < 0) row[1] = done;
    row[0] = done + 1;
    const uint32_t code = HMPC_STATUS_CODE(st);
    if (code != HMPC_S_OK && code != HMPC_S_OK_RELAXED) row[2] = row[2] + 1;
    const int32_t it = (int32_t)HMPC_STATUS_ITERS(st);
    if (it > row[3]) row[3] = it;
  }
  // the rollout's log, row (i, tick): written for a fallen instance too (its frozen state, what the solve made of it)
  const size_t rowi = (size_t)i * a.n_ticks + a.tick;
  if (a.log.state) {
    double *s = a.log.state + rowi * 12;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = tk.rpy[k], s[3 + k] = tk.position[k], s[6 + k] = tk.omegaWorld[k], s[9 + k] = tk.vWorld[k];
  }
  if (a.log.wrench) {
#pragma unroll
    for (int k = 0; k < 12; ++k) a.log.wrench[rowi * 12 + k] = u0f[k];
  }
  if (a.log.status) a.log.status[rowi] = st;
  if (a.log.tau) {
#pragma unroll
    for (int k = 0; k < 10; ++k) a.log.tau[rowi * 10 + k] = a.tau[(size_t)10 * i + k];
  }
}

// {0, -1, 0, 0} in every row (the start of a rollout)
__global__ __launch_bounds__(PLANT_NT) void plant_summary_init_kernel(int32_t *summary, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  summary[4 * (size_t)i + 0] = 0, summary[4 * (size_t)i + 1] = -1, summary[4 * (size_t)i + 2] = 0, summary[4 * (size_t)i + 3] = 0;
}

}  // namespace hmpc
