// tests/test_swing_kernel_on_host.py: csrc/hmpc_swing.h -- the swing update of the motor command -- compiled for the CPU against
// tests/src/hip_lane_shim (one thread per lane) and
//   (no arguments)  run against a plain loop written from the comment above struct hmpc_swing in include/hector_mpc.h, in the reference's own
//                   shape (every one of the `updates` updates runs ALL of updateSwingLeg(), trajectory and IK included, as run() calls it):
//                   batches 1, 24 and 257 (a partial last workgroup at two threads per instance), both leg_q flag settings, updates 1 and 2,
//                   with and without the torques and the detail buffer; fresh state and state in mid swing.  Everything is compared as bit
//                   patterns.
//   (in out)        run on the inputs of a file the test wrote, outputs written to a file the test compares with tests/swing_mirror.py.
//   (ik in out)     the header's computeIK alone on body-frame foot positions of a file (the ankle identity of the geometry test).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "hmpc_swing.h"

using hmpc::SwingArgs;

static void run_kernel(const std::vector<hmpc_tick_inputs> &ticks, SwingArgs a) {
  hipLaunchKernelGGL(hmpc::swing_legs_kernel, dim3((2 * a.batch + hmpc::SWING_NT - 1) / hmpc::SWING_NT), dim3(hmpc::SWING_NT), 0, nullptr, ticks.data(), a);
}

// ---- the plain loop
static double clamp1(double v) { return std::max(-1.0, std::min(v, 1.0)); }
static double asin_(double v) { return hmpc::det_asin(v); }
static double acos_(double v) { return hmpc::det_atan2(std::sqrt((1 - v) * (1 + v)), v); }
static double bez(double y0, double yf, double x) { return y0 + (x * x * x + 3 * (x * x * (1 - x))) * (yf - y0); }
static double dbez(double y0, double yf, double x) { return (6 * x * (1 - x)) * (yf - y0); }

struct LegOut { double swing, pFoot_w[3], pDes[3], vDes[3], pFoot_b[3], vFoot_b[3], kp[5], kd[5]; };

static void plain_update(const hmpc_tick_inputs &tk, const hmpc_swing &c, int h, int j, hmpc_swing_state &st, LegOut &o) {
  const double PI = M_PI, PI3 = 3.14159;
  const double *R = tk.rBody, *pos = tk.position, *v = tk.vWorld;
  double q0 = tk.leg_q[5 * j], q1 = tk.leg_q[5 * j + 1], q2 = tk.leg_q[5 * j + 2], q3 = tk.leg_q[5 * j + 3], q4 = tk.leg_q[5 * j + 4];
  if (tk.flags & HMPC_TICK_LEG_Q_MOTOR) q2 = q2 + 0.3 * PI3, q3 = q3 - 0.6 * PI3, q4 = q4 + 0.3 * PI3;
  double s0, c0, s1, c1, s2, c2, s3, c3, s4, c4;
  hmpc::det_sincos(q0, s0, c0), hmpc::det_sincos(q1, s1, c1), hmpc::det_sincos(q2, s2, c2), hmpc::det_sincos(q3, s3, c3), hmpc::det_sincos(q4, s4, c4);
  const double side = j == 0 ? 1.0 : -1.0;
  const double A = c0 * c2 - s0 * s1 * s2, B = c0 * s2 + c2 * s0 * s1, C = c2 * s0 + c0 * s1 * s2, D = s0 * s2 - c0 * c2 * s1;
  double p[3];
  p[0] = -(3 * c0) / 200 - (9 * s4 * (c3 * A - s3 * B)) / 250 - (11 * c0 * s2) / 50 - (side * s0) / 50 - (11 * c3 * B) / 50 - (11 * s3 * A) / 50 -
         (9 * c4 * (c3 * B + s3 * A)) / 250 - (23 * c1 * side * s0) / 1000 - (11 * c2 * s0 * s1) / 50;
  p[1] = (c0 * side) / 50 - (9 * s4 * (c3 * C - s3 * D)) / 250 - (3 * s0) / 200 - (11 * s0 * s2) / 50 - (11 * c3 * D) / 50 - (11 * s3 * C) / 50 -
         (9 * c4 * (c3 * D + s3 * C)) / 250 + (23 * c0 * c1 * side) / 1000 + (11 * c0 * c2 * s1) / 50;
  p[2] = (23 * side * s1) / 1000 - (11 * c1 * c2) / 50 - (9 * c4 * (c1 * c2 * c3 - c1 * s2 * s3)) / 250 + (9 * s4 * (c1 * c2 * s3 + c1 * c3 * s2)) / 250 -
         (11 * c1 * c2 * c3) / 50 + (11 * c1 * s2 * s3) / 50 - 3.0 / 50.0;
  const double *hy = c.hip_yaw[j];
  const double u[3] = {hy[0] + p[0], hy[1] + p[1], hy[2] + p[2]};
  for (int k = 0; k < 2; ++k) o.pFoot_w[k] = pos[k] + (R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2]);
  o.pFoot_w[2] = 0.0;
  // Gait::setIterations + getSwingSubPhase
  const int cur = tk.gait_iteration * c.ticks_per_step + c.subtick, per = c.ticks_per_step * h;
  const double phase = (double)(cur % per) / (double)per, offP = (double)tk.gait_offsets[j] / (double)h, durP = (double)tk.gait_durations[j] / (double)h;
  double so = offP + durP;
  if (so > 1) so -= 1.;
  const double sd = 1. - durP;
  double pr = phase - so;
  if (pr < 0) pr += 1.;
  if (pr > sd) pr = 0.;
  else pr = (sd == 0) ? 0. : pr / sd;
  o.swing = pr;
  for (int k = 0; k < 3; ++k) o.pDes[k] = o.vDes[k] = o.pFoot_b[k] = o.vFoot_b[k] = 0.0;
  for (int upd = 0; upd < c.updates; ++upd) {
    // updateSwingTimes
    if (st.first_swing[j]) st.swing_time[j] = c.dtMPC * (double)(h - tk.gait_durations[0]);
    else {
      st.swing_time[j] = st.swing_time[j] - c.dt_update;
      if (st.swing_time[j] <= 0) st.first_swing[j] = 1;
    }
    // computeFootPlacement
    double vdw[2];
    for (int a = 0; a < 2; ++a) vdw[a] = R[a] * tk.v_des_robot[0] + R[3 + a] * tk.v_des_robot[1] + R[6 + a] * 0.0;
    for (int a = 0; a < 2; ++a) {
      const double rh = R[a] * hy[0] + R[3 + a] * hy[1] + R[6 + a] * hy[2];
      const double Pf = (pos[a] + rh) + v[a] * st.swing_time[j];
      double rel = c.place_gain_v * v[a] * 0.5 * (double)tk.gait_durations[0] * c.dtMPC + c.place_gain_err * (v[a] - vdw[a]);
      rel = fminf(fmaxf(rel, -c.place_max), c.place_max);
      st.pf[j][a] = Pf + rel;
    }
    st.pf[j][2] = 0.0;
    // computeFootDesiredPosition
    if (o.swing > 0) {
      if (st.first_swing[j]) {
        st.first_swing[j] = 0;
        for (int k = 0; k < 3; ++k) st.p0[j][k] = o.pFoot_w[k];
      }
      const double *p0 = st.p0[j], *pf = st.pf[j], ph = o.swing;
      for (int k = 0; k < 2; ++k) o.pDes[k] = bez(p0[k], pf[k], ph), o.vDes[k] = dbez(p0[k], pf[k], ph);
      if (ph < 0.5) o.pDes[2] = bez(p0[2], p0[2] + c.height, ph * 2), o.vDes[2] = dbez(p0[2], p0[2] + c.height, ph * 2);
      else o.pDes[2] = bez(p0[2] + c.height, pf[2], ph * 2 - 1), o.vDes[2] = dbez(p0[2] + c.height, pf[2], ph * 2 - 1);
      double d[3], e[3];
      for (int k = 0; k < 3; ++k) d[k] = o.pDes[k] - pos[k], e[k] = o.vDes[k] * 0.0 - v[k];
      for (int k = 0; k < 3; ++k) {
        o.pFoot_b[k] = (R[3 * k] * d[0] + R[3 * k + 1] * d[1] + R[3 * k + 2] * d[2]) + c.hip_width_offset[j][k];
        o.vFoot_b[k] = R[3 * k] * e[0] + R[3 * k + 1] * e[1] + R[3 * k + 2] * e[2];
      }
    }
    // setDesiredJointState
    if (o.swing > 0) {
      const double sideK = j == 0 ? -1.0 : 1.0;
      const double hr[3] = {c.hip_roll[0] - c.ik_hip_x, 0.0, c.hip_yaw[0][2] + c.hip_roll[2] * 2};
      const double f[3] = {o.pFoot_b[0] - hr[0], o.pFoot_b[1] - hr[1], o.pFoot_b[2] - hr[2]};
      const double d3 = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]), dyz = std::sqrt(f[1] * f[1] + f[2] * f[2]);
      const double dh = c.ik_horizontal, L = c.ik_link;
      const double dv = std::sqrt(std::max(0.00001, dyz * dyz - dh * dh)), dxz = std::sqrt(d3 * d3 - dh * dh);
      const double a1 = clamp1(dxz / (2.0 * L)), a2 = clamp1(dv / dxz);
      double div = std::abs(f[0]);
      div = (div == 0.0) ? 1e-6 : div;
      double ik[5];
      ik[0] = 0.0;
      ik[1] = asin_(clamp1(f[1] / dyz)) + asin_(clamp1(dh * sideK / dyz));
      ik[2] = acos_(a1) - acos_(a2) * f[0] / div;
      ik[3] = 2.0 * asin_(clamp1(dxz / 2.0 / L)) - PI;
      ik[4] = -q3 - q2;
      ik[2] = ik[2] - 0.3 * PI, ik[3] = ik[3] + 0.6 * PI, ik[4] = ik[4] - 0.3 * PI;
      for (int k = 0; k < 5; ++k) st.q_des[5 * j + k] = ik[k], o.kp[k] = c.kp[k], o.kd[k] = c.kd[k];
    } else {
      for (int k = 0; k < 5; ++k) o.kp[k] = 0.0, o.kd[k] = 0.0;
    }
  }
}

static void default_cfg(hmpc_swing &c) {
  memset(&c, 0, sizeof(c));
  c.dt_update = 0.001, c.dtMPC = 0.04, c.updates = 2, c.ticks_per_step = 40, c.subtick = 0;
  c.height = 0.15, c.place_gain_v = 1.75, c.place_gain_err = 0.1, c.place_max = 0.3;
  for (int leg = 0; leg < 2; ++leg) {
    c.hip_yaw[leg][0] = -0.005, c.hip_yaw[leg][1] = leg ? 0.057 : -0.057, c.hip_yaw[leg][2] = -0.126;
    c.hip_width_offset[leg][0] = -0.015, c.hip_width_offset[leg][1] = leg ? -0.055 : 0.055, c.hip_width_offset[leg][2] = 0.0;
  }
  c.hip_roll[0] = 0.0465, c.hip_roll[1] = 0.015, c.hip_roll[2] = -0.0705;
  c.ik_link = 0.22, c.ik_horizontal = 0.0205, c.ik_hip_x = 0.06;
  for (int k = 0; k < 5; ++k) c.kp[k] = k < 4 ? 30.0 : 20.0, c.kd[k] = 1.0;
}

static double urand(std::mt19937 &rng, double lo, double hi) { return lo + (hi - lo) * (double)(rng() % 1000003) / 1000003.0; }

static int self_test() {
  std::mt19937 rng(11);
  int bad = 0, cases = 0;
  for (int batch : {1, 24, 257})
    for (int motor = 0; motor < 2; ++motor)
      for (int updates : {1, 2})
        for (int variant = 0; variant < 2; ++variant) {
          const int h = 10;
          std::vector<hmpc_tick_inputs> ticks(batch);
          std::vector<hmpc_swing_state> state(batch);
          std::vector<double> tau(10 * batch), detail((size_t)batch * 32, -7.0);
          std::vector<hmpc_motor_cmd> cmd(batch);
          memset(cmd.data(), 0x5a, sizeof(hmpc_motor_cmd) * batch);
          for (int i = 0; i < batch; ++i) {
            hmpc_tick_inputs &t = ticks[i];
            memset(&t, 0, sizeof(t));
            const double roll = urand(rng, -0.1, 0.1), pitch = urand(rng, -0.1, 0.1), yaw = urand(rng, -3.0, 3.0);
            const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2), cy = std::cos(yaw / 2),
                         sy = std::sin(yaw / 2);
            const double q[4] = {cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy};
            const double M[9] = {1 - 2 * (q[2] * q[2] + q[3] * q[3]), 2 * (q[1] * q[2] - q[0] * q[3]),     2 * (q[1] * q[3] + q[0] * q[2]),
                                 2 * (q[1] * q[2] + q[0] * q[3]),     1 - 2 * (q[1] * q[1] + q[3] * q[3]), 2 * (q[2] * q[3] - q[0] * q[1]),
                                 2 * (q[1] * q[3] - q[0] * q[2]),     2 * (q[2] * q[3] + q[0] * q[1]),     1 - 2 * (q[1] * q[1] + q[2] * q[2])};
            for (int r = 0; r < 3; ++r)
              for (int cc = 0; cc < 3; ++cc) t.rBody[3 * r + cc] = M[3 * cc + r];
            for (int k = 0; k < 4; ++k) t.orientation[k] = q[k];
            for (int k = 0; k < 3; ++k) t.position[k] = urand(rng, -2, 2), t.vWorld[k] = urand(rng, -0.6, 0.6);
            t.position[2] = 0.55 + urand(rng, -0.03, 0.03);
            if (i % 9 == 4) t.vWorld[0] = 4.0, t.vWorld[1] = -4.0;  // (drives the touchdown clamp)
            for (int leg = 0; leg < 2; ++leg) {
              double *lq = t.leg_q + 5 * leg;
              lq[0] = urand(rng, -0.2, 0.2), lq[1] = urand(rng, -0.2, 0.2), lq[2] = urand(rng, 0.2, 1.0), lq[3] = urand(rng, -1.8, -0.6), lq[4] = urand(rng, 0.2, 1.0);
            }
            t.v_des_robot[0] = urand(rng, -0.5, 0.5), t.v_des_robot[1] = urand(rng, -0.2, 0.2);
            const int kind = i % 4;  // walking, walking with other offsets, an irregular table, standing
            t.gait_offsets[0] = kind == 1 ? 3 : 0, t.gait_offsets[1] = kind == 3 ? 0 : (kind == 2 ? 7 : 5);
            t.gait_durations[0] = kind == 3 ? 10 : (kind == 2 ? 6 : 5), t.gait_durations[1] = kind == 3 ? 10 : (kind == 2 ? 3 : 5);
            t.gait_iteration = (int)(rng() % 10);
            t.flags = motor ? HMPC_TICK_LEG_Q_MOTOR : 0;
            hmpc_swing_state &s = state[i];
            memset(&s, 0, sizeof(s));
            s.first_swing[0] = s.first_swing[1] = 1;
            if (variant) {  // in mid swing, or with a timer about to run out
              for (int leg = 0; leg < 2; ++leg) {
                s.first_swing[leg] = (int)(rng() % 3 == 0);
                s.swing_time[leg] = (rng() % 4 == 0) ? 0.0015 : urand(rng, 0.0, 0.2);
                for (int k = 0; k < 2; ++k) s.p0[leg][k] = t.position[k] + urand(rng, -0.2, 0.2), s.pf[leg][k] = t.position[k] + urand(rng, -0.2, 0.2);
                for (int k = 0; k < 5; ++k) s.q_des[5 * leg + k] = urand(rng, -1, 1);
              }
            }
            for (int k = 0; k < 10; ++k) tau[10 * i + k] = urand(rng, -20, 20);
          }
          SwingArgs a;
          memset(&a, 0, sizeof(a));
          default_cfg(a.cfg);
          a.cfg.updates = updates, a.cfg.ticks_per_step = variant ? 8 : 40, a.cfg.subtick = variant ? 3 : 0;
          a.batch = batch, a.horizon = h, a.tau = variant ? tau.data() : nullptr, a.cmd = cmd.data(), a.cmd_stride = 1, a.cmd_row = 0;
          a.detail = variant ? detail.data() : nullptr;
          std::vector<hmpc_swing_state> want_state = state;
          a.state = state.data();
          run_kernel(ticks, a);
          bool ok = true;
          int swinging = 0, clamped = 0;
          for (int i = 0; i < batch; ++i)
            for (int j = 0; j < 2; ++j) {
              LegOut o;
              plain_update(ticks[i], a.cfg, h, j, want_state[i], o);
              swinging += o.swing > 0;
              const double raw = 1.75 * ticks[i].vWorld[0] * 0.5 * (double)ticks[i].gait_durations[0] * 0.04;  // (the velocity term alone passes the clamp)
              clamped += raw + 0.1 * (ticks[i].vWorld[0] - 0.6) > 0.3;  // (|v_des_world| < 0.6)
              hmpc_motor_cmd w;
              for (int k = 0; k < 5; ++k) {
                const int jj = 5 * j + k;
                w.q[jj] = want_state[i].q_des[jj], w.dq[jj] = 0.0, w.Kp[jj] = o.kp[k], w.Kd[jj] = o.kd[k], w.tau[jj] = variant ? tau[10 * i + jj] : 0.0;
                ok = ok && memcmp(&w.q[jj], &cmd[i].q[jj], 8) == 0 && memcmp(&w.dq[jj], &cmd[i].dq[jj], 8) == 0 && memcmp(&w.Kp[jj], &cmd[i].Kp[jj], 8) == 0 &&
                     memcmp(&w.Kd[jj], &cmd[i].Kd[jj], 8) == 0 && memcmp(&w.tau[jj], &cmd[i].tau[jj], 8) == 0;
              }
              if (variant) {
                double row[16] = {o.swing};
                for (int k = 0; k < 3; ++k) row[1 + k] = o.pFoot_w[k], row[4 + k] = o.pDes[k], row[7 + k] = o.vDes[k], row[10 + k] = o.pFoot_b[k], row[13 + k] = o.vFoot_b[k];
                ok = ok && memcmp(row, &detail[(size_t)(2 * i + j) * 16], sizeof(row)) == 0;
              }
            }
          ok = ok && memcmp(state.data(), want_state.data(), sizeof(hmpc_swing_state) * batch) == 0;
          if (batch >= 24 && (swinging == 0 || clamped == 0)) ok = false, printf("the case lacks swinging legs (%d) or clamped touchdowns (%d)\n", swinging, clamped);
          if (!ok) printf("batch %d motor %d updates %d variant %d: differs from the plain loop\n", batch, motor, updates, variant);
          bad += !ok, ++cases;
        }
  printf("%d cases, %d problems\n", cases, bad);
  return bad != 0;
}

// file: int32 {batch, horizon, has_tau, 0}, hmpc_swing, ticks, state, then tau when present.  out: cmd, state, detail [batch][2][16].
static int from_file(const char *in_path, const char *out_path) {
  FILE *f = fopen(in_path, "rb");
  if (!f) return 2;
  int32_t hd[4];
  SwingArgs a;
  memset(&a, 0, sizeof(a));
  bool ok = fread(hd, sizeof(hd), 1, f) == 1 && fread(&a.cfg, sizeof(hmpc_swing), 1, f) == 1;
  if (!ok) return 3;
  const int batch = hd[0];
  std::vector<hmpc_tick_inputs> ticks(batch);
  std::vector<hmpc_swing_state> state(batch);
  std::vector<double> tau(10 * batch), detail((size_t)batch * 32);
  std::vector<hmpc_motor_cmd> cmd(batch);
  ok = fread(ticks.data(), sizeof(hmpc_tick_inputs), batch, f) == (size_t)batch && fread(state.data(), sizeof(hmpc_swing_state), batch, f) == (size_t)batch;
  if (ok && hd[2]) ok = fread(tau.data(), 8, 10 * batch, f) == (size_t)(10 * batch);
  fclose(f);
  if (!ok) return 3;
  a.batch = batch, a.horizon = hd[1], a.state = state.data(), a.tau = hd[2] ? tau.data() : nullptr, a.cmd = cmd.data(), a.cmd_stride = 1, a.cmd_row = 0;
  a.detail = detail.data();
  run_kernel(ticks, a);
  f = fopen(out_path, "wb");
  if (!f) return 2;
  fwrite(cmd.data(), sizeof(hmpc_motor_cmd), batch, f);
  fwrite(state.data(), sizeof(hmpc_swing_state), batch, f);
  fwrite(detail.data(), 8, detail.size(), f);
  fclose(f);
  return 0;
}

// the header's computeIK alone.  file: int32 {n, 0}, hmpc_swing, n x double[6] {pFoot_b[3], leg, q2, q3}.  out: n x double[5].
static int ik_from_file(const char *in_path, const char *out_path) {
  FILE *f = fopen(in_path, "rb");
  if (!f) return 2;
  int32_t hd[2];
  hmpc_swing c;
  if (fread(hd, sizeof(hd), 1, f) != 1 || fread(&c, sizeof(c), 1, f) != 1) return 3;
  std::vector<double> in((size_t)6 * hd[0]), out((size_t)5 * hd[0]);
  if (fread(in.data(), 8, in.size(), f) != in.size()) return 3;
  fclose(f);
  for (int i = 0; i < hd[0]; ++i) hmpc::swing_ik(&in[6 * i], c, (int)in[6 * i + 3], in[6 * i + 4], in[6 * i + 5], &out[5 * i]);
  f = fopen(out_path, "wb");
  if (!f) return 2;
  fwrite(out.data(), 8, out.size(), f);
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "ik")) return ik_from_file(argv[2], argv[3]);
  if (argc == 3) return from_file(argv[1], argv[2]);
  return self_test();
}
