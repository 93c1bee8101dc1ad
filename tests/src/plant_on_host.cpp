// tests/test_plant_kernel_on_host.py: csrc/hmpc_plant.h -- the plant step of the closed loop -- compiled for the CPU against
// tests/src/hip_lane_shim (one thread per lane) and
//   (no arguments)  run against a plain loop written from the comment above struct hmpc_plant in include/hector_mpc.h: batches 1, 24 and
//                   257 (a partial last workgroup), substeps 1 and 3, every flag combination, with and without per-instance mass, external
//                   wrench, explicit world_position_desired and the gait advance; instances that had fallen before, instances that fall on this
//                   step; summary rows that already hold counts.  Everything is compared as bit patterns.
//   (in out)        run on the inputs of a file the test wrote, outputs written to a file the test compares with tests/rollout_mirror.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "hmpc_plant.h"

using hmpc::PlantArgs;

static void run_kernel(std::vector<hmpc_tick_inputs> &ticks, PlantArgs a) {
  hipLaunchKernelGGL(hmpc::plant_step_kernel, dim3((a.batch + hmpc::PLANT_NT - 1) / hmpc::PLANT_NT), dim3(hmpc::PLANT_NT), 0, nullptr, ticks.data(), a);
}

// ---- the plain loop
struct V3 { double x, y, z; };
static V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 scale(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V3 rows(const double *R, V3 a) {  // R a
  return {(R[0] * a.x + R[1] * a.y) + R[2] * a.z, (R[3] * a.x + R[4] * a.y) + R[5] * a.z, (R[6] * a.x + R[7] * a.y) + R[8] * a.z};
}
static V3 cols(const double *R, V3 a) {  // R' a
  return {(R[0] * a.x + R[3] * a.y) + R[6] * a.z, (R[1] * a.x + R[4] * a.y) + R[7] * a.z, (R[2] * a.x + R[5] * a.y) + R[8] * a.z};
}
static V3 v3(const double *p) { return {p[0], p[1], p[2]}; }
static V3 v3f(const float *p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
static void put(double *p, V3 a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

static void plain_step(hmpc_tick_inputs &tk, const PlantArgs &a, int i) {
  const hmpc_plant &pl = a.plant;
  if (tk.flags & HMPC_TICK_FALLEN) return;
  const float *u = a.forces + (size_t)i * a.force_stride;
  const V3 FL = v3f(u), FR = v3f(u + 3), ML = v3f(u + 6), MR = v3f(u + 9);
  const double m = pl.device_mass ? pl.device_mass[i] : pl.mass;
  V3 Fext{0, 0, 0}, Text{0, 0, 0};
  if (pl.device_ext_wrench) Fext = v3(pl.device_ext_wrench + 6 * i), Text = v3(pl.device_ext_wrench + 6 * i + 3);
  const V3 I = v3(pl.inertia), cmd{tk.v_des_robot[0], tk.v_des_robot[1], 0.0};
  V3 p = v3(tk.position), v = v3(tk.vWorld), w = v3(tk.omegaWorld);
  double q0 = tk.orientation[0], q1 = tk.orientation[1], q2 = tk.orientation[2], q3 = tk.orientation[3];
  double R[9];
  for (int k = 0; k < 9; ++k) R[k] = tk.rBody[k];
  const V3 vdw0 = cols(R, cmd);
  const double base0 = a.wpd ? a.wpd[2 * i] : tk.world_position_desired[0], base1 = a.wpd ? a.wpd[2 * i + 1] : tk.world_position_desired[1];
  const double d = pl.dt_tick / (double)pl.substeps, hd = 0.5 * d;
  for (int s = 0; s < pl.substeps; ++s) {
    const V3 rL = sub(v3(tk.pFoot), p), rR = sub(v3(tk.pFoot + 3), p);
    const V3 tau = add(add(add(cross(rL, FL), ML), add(cross(rR, FR), MR)), Text);
    const V3 F = add(add(FL, FR), Fext);
    V3 tb = rows(R, tau);
    if (pl.flags & HMPC_PLANT_GYRO) {
      const V3 wb = rows(R, w);
      tb = sub(tb, cross(wb, V3{I.x * wb.x, I.y * wb.y, I.z * wb.z}));
    }
    const V3 alpha = cols(R, V3{tb.x / I.x, tb.y / I.y, tb.z / I.z});
    const V3 acc{F.x / m + 0.0, F.y / m + 0.0, F.z / m + (-pl.gravity)};
    w = add(w, scale(d, alpha));
    v = add(v, scale(d, acc));
    p = add(p, scale(d, v));
    const double e0 = -((w.x * q1 + w.y * q2) + w.z * q3), e1 = (w.x * q0 + w.y * q3) - w.z * q2, e2 = (w.y * q0 + w.z * q1) - w.x * q3,
                 e3 = (w.z * q0 + w.x * q2) - w.y * q1;
    q0 = q0 + hd * e0, q1 = q1 + hd * e1, q2 = q2 + hd * e2, q3 = q3 + hd * e3;
    const double n = std::sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    q0 = q0 / n, q1 = q1 / n, q2 = q2 / n, q3 = q3 / n;
    const double M[9] = {1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3),     2 * (q1 * q3 + q0 * q2),
                         2 * (q1 * q2 + q0 * q3),     1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1),
                         2 * (q1 * q3 - q0 * q2),     2 * (q2 * q3 + q0 * q1),     1 - 2 * (q1 * q1 + q2 * q2)};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[3 * r + c] = M[3 * c + r];
  }
  put(tk.position, p), put(tk.vWorld, v), put(tk.omegaWorld, w);
  tk.orientation[0] = q0, tk.orientation[1] = q1, tk.orientation[2] = q2, tk.orientation[3] = q3;
  for (int k = 0; k < 9; ++k) tk.rBody[k] = R[k];
  double sp = 2 * (q0 * q2 - q1 * q3);
  if (!(sp < 0.99999)) sp = 0.99999;
  if (sp < -0.99999) sp = -0.99999;
  tk.rpy[0] = hmpc::det_atan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2));
  tk.rpy[1] = hmpc::det_asin(sp);
  tk.rpy[2] = hmpc::det_atan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3));
  tk.world_position_desired[0] = base0 + pl.dt_tick * vdw0.x;
  tk.world_position_desired[1] = base1 + pl.dt_tick * vdw0.y;
  if (pl.advance_gait) tk.gait_iteration = (tk.gait_iteration + 1) % a.horizon;
  if (pl.flags & HMPC_PLANT_PLACE_FEET) {
    const V3 vdw = cols(R, cmd);
    for (int j = 0; j < 2; ++j) {
      int progress = tk.gait_iteration % a.horizon - tk.gait_offsets[j];
      if (progress < 0) progress += a.horizon;
      if (progress < tk.gait_durations[j]) continue;
      const V3 Pf = add(add(p, cols(R, v3(pl.hip[j]))), scale(0.0, v));
      double rx = ((v.x * 0.5) * (double)tk.gait_durations[0]) * pl.dtMPC + 0.02 * (v.x - vdw.x);
      double ry = ((v.y * 0.5) * (double)tk.gait_durations[0]) * pl.dtMPC + 0.02 * (v.y - vdw.y);
      const double p_rel_max = 0.4;
      rx = fminf(fmaxf(rx, -p_rel_max), p_rel_max);
      ry = fminf(fmaxf(ry, -p_rel_max), p_rel_max);
      tk.pFoot[3 * j] = Pf.x + rx, tk.pFoot[3 * j + 1] = Pf.y + ry, tk.pFoot[3 * j + 2] = 0.0;
    }
  }
  const bool fell = R[8] < pl.fall_cos;
  if (fell) tk.flags |= HMPC_TICK_FALLEN;
  if (a.summary) {
    int32_t *row = a.summary + 4 * i;
    if (fell && row[1] < 0) row[1] = row[0];
    row[0] += 1;
    const uint32_t code = a.status[i] & 0xffu;
    if (code != 0 && code != 6) row[2] += 1;
    const int32_t it = (int32_t)((a.status[i] >> 8) & 0xfffu);
    if (it > row[3]) row[3] = it;
  }
}

static double urand(std::mt19937 &rng, double lo, double hi) { return lo + (hi - lo) * (double)(rng() % 1000003) / 1000003.0; }

static int self_test() {
  std::mt19937 rng(7);
  int bad = 0, cases = 0;
  for (int batch : {1, 24, 257})
    for (int substeps : {1, 3})
      for (int flags = 0; flags < 4; ++flags)
        for (int variant = 0; variant < 2; ++variant) {
          const int h = 10, stride = variant ? 12 : 120;
          std::vector<hmpc_tick_inputs> ticks(batch);
          std::vector<float> forces((size_t)batch * stride);
          std::vector<uint32_t> status(batch);
          std::vector<double> wpd(2 * batch), mass(batch), ext(6 * batch);
          std::vector<int32_t> summary(4 * batch);
          for (int i = 0; i < batch; ++i) {
            hmpc_tick_inputs &t = ticks[i];
            memset(&t, 0, sizeof(t));
            const double roll = (i % 7 == 3) ? 1.2 : urand(rng, -0.1, 0.1), pitch = urand(rng, -0.1, 0.1), yaw = urand(rng, -3.0, 3.0);
            const double cr = std::cos(roll / 2), sr = std::sin(roll / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2), cy = std::cos(yaw / 2),
                         sy = std::sin(yaw / 2);
            double q[4] = {cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy};
            for (int k = 0; k < 4; ++k) t.orientation[k] = q[k];
            hmpc::plant_rbody(q, t.rBody);
            t.rpy[0] = roll, t.rpy[1] = pitch, t.rpy[2] = yaw;
            for (int k = 0; k < 3; ++k) t.position[k] = urand(rng, -2, 2), t.vWorld[k] = urand(rng, -0.3, 0.3), t.omegaWorld[k] = urand(rng, -0.5, 0.5);
            t.position[2] = 0.55 + urand(rng, -0.03, 0.03);
            for (int k = 0; k < 10; ++k) t.leg_q[k] = urand(rng, -1, 1);
            for (int leg = 0; leg < 2; ++leg) {
              t.pFoot[3 * leg] = t.position[0] + urand(rng, -0.1, 0.1), t.pFoot[3 * leg + 1] = t.position[1] + (leg ? -0.06 : 0.06), t.pFoot[3 * leg + 2] = 0.0;
            }
            t.v_des_robot[0] = (i % 4) ? urand(rng, -0.5, 0.5) : 0.0, t.v_des_robot[1] = urand(rng, -0.5, 0.5);
            t.yaw_rate_des = urand(rng, -0.3, 0.3), t.roll_des = 0.01, t.pitch_des = -0.01;
            t.world_position_desired[0] = t.position[0] + urand(rng, -0.1, 0.1), t.world_position_desired[1] = t.position[1] + urand(rng, -0.1, 0.1);
            const bool walking = i % 3 != 0;
            t.gait_offsets[0] = 0, t.gait_offsets[1] = walking ? 5 : 0, t.gait_durations[0] = walking ? 5 : 10, t.gait_durations[1] = walking ? 5 : 10;
            t.gait_iteration = (int)(rng() % 10);
            t.flags = (i % 2) | ((i % 11 == 5) ? HMPC_TICK_FALLEN : 0);
            for (int k = 0; k < stride; ++k) forces[(size_t)i * stride + k] = (float)urand(rng, -50, 50) * (k >= 6 && k < 12 ? 0.1f : 1.0f);
            status[i] = (uint32_t)((rng() % 3 == 0 ? rng() % 10 : 0) | ((rng() % 90) << 8) | ((rng() % 60) << 20));
            wpd[2 * i] = t.position[0] + urand(rng, -0.05, 0.05), wpd[2 * i + 1] = t.position[1] + urand(rng, -0.05, 0.05);
            mass[i] = urand(rng, 8, 13);
            for (int k = 0; k < 6; ++k) ext[6 * i + k] = urand(rng, -30, 30);
            summary[4 * i] = variant ? 5 : 0, summary[4 * i + 1] = (variant && i % 5 == 0) ? 2 : -1, summary[4 * i + 2] = variant, summary[4 * i + 3] = variant ? 40 : 0;
          }
          PlantArgs a;
          memset(&a, 0, sizeof(a));
          a.plant.dt_tick = 0.005, a.plant.dtMPC = 0.04, a.plant.substeps = substeps, a.plant.advance_gait = variant, a.plant.flags = flags;
          a.plant.mass = 9.0, a.plant.inertia[0] = 0.5413, a.plant.inertia[1] = 0.52, a.plant.inertia[2] = 0.0691, a.plant.gravity = 9.81;
          for (int leg = 0; leg < 2; ++leg) a.plant.hip[leg][0] = -0.005, a.plant.hip[leg][1] = leg ? 0.057 : -0.057, a.plant.hip[leg][2] = -0.126;
          a.plant.fall_cos = 0.5;
          a.plant.device_mass = variant ? mass.data() : nullptr, a.plant.device_ext_wrench = variant ? ext.data() : nullptr;
          a.batch = batch, a.horizon = h, a.forces = forces.data(), a.force_stride = stride, a.status = status.data();
          a.wpd = variant ? nullptr : wpd.data(), a.n_ticks = 1;
          std::vector<hmpc_tick_inputs> want = ticks, in = ticks;
          std::vector<int32_t> want_sum = summary;
          a.summary = summary.data();
          run_kernel(ticks, a);
          PlantArgs b = a;
          b.summary = want_sum.data();
          for (int i = 0; i < batch; ++i) plain_step(want[i], b, i);
          bool ok = memcmp(ticks.data(), want.data(), sizeof(hmpc_tick_inputs) * batch) == 0 && memcmp(summary.data(), want_sum.data(), 16 * batch) == 0;
          int fallen_before = 0, fell = 0, moved_feet = 0;
          for (int i = 0; i < batch; ++i) {
            if (in[i].flags & HMPC_TICK_FALLEN) {
              ++fallen_before;
              if (memcmp(&ticks[i], &in[i], sizeof(hmpc_tick_inputs)) != 0) ok = false, printf("a fallen instance changed\n");
            } else if (ticks[i].flags & HMPC_TICK_FALLEN) ++fell;
            if (memcmp(ticks[i].leg_q, in[i].leg_q, sizeof(in[i].leg_q)) != 0) ok = false, printf("leg_q changed\n");
            if (memcmp(ticks[i].pFoot, in[i].pFoot, sizeof(in[i].pFoot)) != 0) ++moved_feet;
          }
          if (!(flags & HMPC_PLANT_PLACE_FEET) && moved_feet) ok = false, printf("feet moved without PLACE_FEET\n");
          if (batch >= 24 && ((flags & HMPC_PLANT_PLACE_FEET) ? moved_feet == 0 : false)) ok = false, printf("no foot was placed\n");
          if (batch >= 24 && (fallen_before == 0 || fell == 0)) ok = false, printf("the case lacks fallen / falling instances\n");
          if (!ok) printf("batch %d substeps %d flags %d variant %d: differs from the plain loop\n", batch, substeps, flags, variant);
          bad += !ok, ++cases;
        }
  printf("%d cases, %d problems\n", cases, bad);
  return bad != 0;
}

// file: int32 {batch, horizon, force_stride, has_wpd, has_mass, has_ext}, hmpc_plant (its two pointers ignored), ticks, forces
// [batch][force_stride], status, summary, then wpd / mass / ext when present.  out: ticks, summary.
static int from_file(const char *in_path, const char *out_path) {
  FILE *f = fopen(in_path, "rb");
  if (!f) return 2;
  int32_t hd[6];
  PlantArgs a;
  memset(&a, 0, sizeof(a));
  bool ok = fread(hd, sizeof(hd), 1, f) == 1 && fread(&a.plant, sizeof(hmpc_plant), 1, f) == 1;
  if (!ok) return 3;
  const int batch = hd[0];
  std::vector<hmpc_tick_inputs> ticks(batch);
  std::vector<float> forces((size_t)batch * hd[2]);
  std::vector<uint32_t> status(batch);
  std::vector<int32_t> summary(4 * batch);
  std::vector<double> wpd(2 * batch), mass(batch), ext(6 * batch);
  ok = fread(ticks.data(), sizeof(hmpc_tick_inputs), batch, f) == (size_t)batch && fread(forces.data(), 4, forces.size(), f) == forces.size() &&
       fread(status.data(), 4, batch, f) == (size_t)batch && fread(summary.data(), 4, 4 * batch, f) == (size_t)(4 * batch);
  if (ok && hd[3]) ok = fread(wpd.data(), 8, 2 * batch, f) == (size_t)(2 * batch);
  if (ok && hd[4]) ok = fread(mass.data(), 8, batch, f) == (size_t)batch;
  if (ok && hd[5]) ok = fread(ext.data(), 8, 6 * batch, f) == (size_t)(6 * batch);
  fclose(f);
  if (!ok) return 3;
  a.plant.device_mass = hd[4] ? mass.data() : nullptr, a.plant.device_ext_wrench = hd[5] ? ext.data() : nullptr;
  a.batch = batch, a.horizon = hd[1], a.forces = forces.data(), a.force_stride = hd[2], a.status = status.data();
  a.wpd = hd[3] ? wpd.data() : nullptr, a.summary = summary.data(), a.n_ticks = 1;
  run_kernel(ticks, a);
  f = fopen(out_path, "wb");
  if (!f) return 2;
  fwrite(ticks.data(), sizeof(hmpc_tick_inputs), batch, f);
  fwrite(summary.data(), 4, 4 * batch, f);
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3) return from_file(argv[1], argv[2]);
  return self_test();
}
