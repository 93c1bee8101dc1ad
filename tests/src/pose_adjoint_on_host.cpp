// tests/test_pose_adjoint_kernel_on_host.py: csrc/hmpc_pose_adjoint.h -- everything of the pose-gradient kernel behind the assembly --
// compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop that states the definition once
// more, sequentially: h = 1, 3, 10 (HMAX = 10) and h = 11, 20 (HMAX = 20), NC = 2, 3, every output compared as bit patterns.  Variants:
// random data; zero upstream gradients (zeros out); a contact whose rows of grad_Fc are 0 (a swing contact: its frame and joint angles
// exactly 0); a NaN among the tabulated values (a NaN force upstream reaches the chain as NaN gradients: the run must end); a NaN
// grad_Fc (the run must end); the clamped pitch (a zero pitch row: grad_x0[1] does not reach q); an un-normalised quaternion.
#include "hmpc_pose_adjoint.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

template <int NC, int HM>
__global__ void pose_adjoint_test_kernel(const float *rec, const float *sc, const float *sc234, const float *ypsc, const float *R, const float *Acd,
                                         const float *Bcd, const double *gx0, const double *gtraj, const double *gw, const double *gal,
                                         const double *gA, const double *gB, const double *gr, const double *glim, const double *gFc, int h,
                                         double dt, double lt, double lh, const double *Ib, double *grec, double *gframes, double *grpy) {
  __shared__ hmpc::PoseAdjointWork<NC, HM> Wk;
  hmpc::pose_adjoint_of_instance<NC, HM, hmpc::PADJ_NT>(rec, sc, sc234, ypsc, R, Acd, Bcd, gx0, gtraj, gw, gal, gA, gB, gr, glim, gFc, h, dt, lt, lh,
                                                        Ib[0], Ib[1], Ib[2], Wk, grec, gframes, grpy);
}

static bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), 8 * a.size()) == 0; }

// the body rotation from a quaternion in binary32, as the assembly forms it
static void rotation(const float *q, float *R) {
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
  const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1.0f - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy, R[3] = txy + twz, R[4] = 1.0f - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0f - (txx + tyy);
}

template <int NC>
struct In {
  static constexpr int U = 6 * NC;
  std::vector<float> rec, sc, sc234, ypsc, R, Acd, Bcd;
  std::vector<double> gx0, gtraj, gw, gal, gA, gB, gr, glim, gFc;
  double dt, lt, lh, Ib[3];
  int h;
};

template <int NC>
struct Out {
  std::vector<double> rec, frames, rpy;
  explicit Out(int h) : rec(hmpc::RecLayout<NC>::NF + 12 * h, -7.0), frames(9 * (1 + NC), -7.0), rpy(3, -7.0) {}
  bool equals(const Out &o) const { return same(rec, o.rec) && same(frames, o.frames) && same(rpy, o.rpy); }
};

// 0 - (A' G A') / dt
static void inverse_adjoint(const double A[3][3], const double G[3][3], double dt, double out[3][3]) {
  double X[3][3];
  for (int m = 0; m < 3; ++m)
    for (int n = 0; n < 3; ++n) {
      double acc = 0.0;
      for (int a = 0; a < 3; ++a) acc = std::fma(A[a][m], G[a][n], acc);
      X[m][n] = acc;
    }
  for (int m = 0; m < 3; ++m)
    for (int k = 0; k < 3; ++k) {
      double acc = 0.0;
      for (int n = 0; n < 3; ++n) acc = std::fma(X[m][n], A[k][n], acc);
      out[m][k] = 0.0 - acc / dt;
    }
}

static void atan2_row(double n, double d, const double dn[4], const double dd[4], double row[4]) {
  const double den = std::fma(n, n, d * d);
  for (int k = 0; k < 4; ++k) row[k] = std::fma(d, dn[k], 0.0 - n * dd[k]) / den;
}

// the plain loop: the definition, sequentially
template <int NC>
static Out<NC> plain(const In<NC> &in) {
  using RL = hmpc::RecLayout<NC>;
  constexpr int U = 6 * NC;
  const int h = in.h;
  Out<NC> o(h);
  for (auto &v : o.rec) v = 0.0;
  double R[3][3];
  for (int k = 0; k < 9; ++k) R[k / 3][k % 3] = (double)in.R[k];
  auto GF = [&](int row, int col) { return in.gFc[(size_t)row * U + col]; };
  auto GB = [&](int a, int b) { return in.gB[(size_t)a * U + b]; };
  double P[NC + 1][3][3];
  for (int c = 0; c < NC; ++c) {
    const int cf = 3 * c, cmo = 3 * NC + 3 * c, b = (c < 2) ? 5 * c : 0;
    const double s0 = in.sc[2 * b], c0 = in.sc[2 * b + 1], s1 = in.sc[2 * b + 2], c1 = in.sc[2 * b + 3];
    const double sb = in.sc234[2 * (c & 1)], cb = in.sc234[2 * (c & 1) + 1];
    double Rf[3][3];
    const double t = s0 * s1, v = c0 * s1;
    Rf[0][0] = std::fma(c0, cb, 0.0 - t * sb), Rf[0][1] = 0.0 - s0 * c1, Rf[0][2] = std::fma(c0, sb, t * cb);
    Rf[1][0] = std::fma(s0, cb, v * sb), Rf[1][1] = c0 * c1, Rf[1][2] = std::fma(s0, sb, 0.0 - v * cb);
    Rf[2][0] = 0.0 - c1 * sb, Rf[2][1] = s1, Rf[2][2] = c1 * cb;
    if (NC == 3 && c == 2)
      for (int k = 0; k < 9; ++k) Rf[k / 3][k % 3] = (double)in.rec[RL::RH + k];
    const double sg = (c == 1) ? 1.0 : -1.0;
    double Gg[3][3], GRf[3][3];
    for (int j = 0; j < 3; ++j) {
      Gg[j][0] = GF(8 * c + 4, cmo + j);
      Gg[j][1] = GF(8 * c + 5, cmo + j) + sg * GF(8 * c + 6, cmo + j);
      Gg[j][2] = std::fma(0.0 - in.lt, GF(8 * c + 5, cf + j), (0.0 - in.lh) * GF(8 * c + 6, cf + j));
    }
    for (int a = 0; a < 3; ++a)
      for (int m = 0; m < 3; ++m) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc = std::fma(R[j][a], Gg[j][m], acc);
        GRf[a][m] = acc;
        o.frames[9 * (1 + c) + 3 * a + m] = acc;
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double acc = 0.0;
        for (int m = 0; m < 3; ++m) acc = std::fma(Gg[i][m], Rf[j][m], acc);
        P[c][i][j] = acc;
      }
    if (NC == 3 && c == 2) {
      for (int k = 0; k < 9; ++k) o.rec[RL::RH + k] = GRf[k / 3][k % 3];
      continue;
    }
    double a0 = 0.0, a1 = 0.0, ab = 0.0;
    for (int k = 0; k < 3; ++k) a0 = std::fma(GRf[0][k], 0.0 - Rf[1][k], a0);
    for (int k = 0; k < 3; ++k) a0 = std::fma(GRf[1][k], Rf[0][k], a0);
    const double e[3] = {c1 * sb, 0.0 - s1, 0.0 - c1 * cb}, f[3] = {s1 * sb, c1, 0.0 - s1 * cb};
    for (int k = 0; k < 3; ++k) a1 = std::fma(GRf[0][k], (0.0 - s0) * e[k], a1);
    for (int k = 0; k < 3; ++k) a1 = std::fma(GRf[1][k], c0 * e[k], a1);
    for (int k = 0; k < 3; ++k) a1 = std::fma(GRf[2][k], f[k], a1);
    for (int i = 0; i < 3; ++i) ab = std::fma(GRf[i][0], 0.0 - Rf[i][2], ab), ab = std::fma(GRf[i][2], Rf[i][0], ab);
    double *ja = o.rec.data() + RL::JA + 5 * c;
    ja[0] = a0, ja[1] = a1, ja[2] = ab, ja[3] = ab, ja[4] = ab;
  }
  {  // inertia
    double Gam[3][3], Mb[3][3], GI[3][3];
    for (int a = 0; a < 3; ++a)
      for (int m = 0; m < 3; ++m) {
        Mb[a][m] = (double)in.Bcd[(6 + a) * U + 3 * NC + m];
        double acc = 0.0;
        for (int c = 0; c < NC; ++c) {
          const float r0 = in.rec[RL::R + 0 * NC + c], r1 = in.rec[RL::R + 1 * NC + c], r2 = in.rec[RL::R + 2 * NC + c];
          const float cm[3][3] = {{0.0f, -r2, r1}, {r2, 0.0f, -r0}, {-r1, r0, 0.0f}};
          acc = acc + GB(6 + a, 3 * NC + 3 * c + m);
          for (int b = 0; b < 3; ++b) acc = std::fma(GB(6 + a, 3 * c + b), (double)cm[m][b], acc);
        }
        Gam[a][m] = acc;
      }
    inverse_adjoint(Mb, Gam, in.dt, GI);
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc = std::fma(GI[i][j] + GI[j][i], R[j][k], acc);
        P[NC][i][k] = acc * in.Ib[k];
      }
  }
  double GR[9];
  for (int e = 0; e < 9; ++e) {
    double g = 0.0;
    for (int p = 0; p <= NC; ++p) g = g + P[p][e / 3][e % 3];
    GR[e] = g, o.frames[e] = g;
  }
  // Euler
  double Ab[3][3], GAb[3][3], GRb[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Ab[a][b] = (double)in.Acd[a * 13 + 6 + b], GAb[a][b] = in.gA[a * 13 + 6 + b];
  inverse_adjoint(Ab, GAb, in.dt, GRb);
  const double cy = in.ypsc[0], sy = in.ypsc[1], cp = in.ypsc[2], sp = in.ypsc[3];
  double gy = 0.0, gp = 0.0;
  gy = std::fma(GRb[0][0], 0.0 - sy * cp, gy), gy = std::fma(GRb[0][1], 0.0 - cy, gy), gy = std::fma(GRb[1][0], cy * cp, gy), gy = std::fma(GRb[1][1], 0.0 - sy, gy);
  gp = std::fma(GRb[0][0], 0.0 - cy * sp, gp), gp = std::fma(GRb[1][0], 0.0 - sy * sp, gp), gp = std::fma(GRb[2][0], 0.0 - cp, gp);
  o.rpy[0] = in.gx0[0], o.rpy[1] = in.gx0[1] + gp, o.rpy[2] = in.gx0[2] + gy;
  const float qw = in.rec[RL::Q], qx = in.rec[RL::Q + 1], qy = in.rec[RL::Q + 2], qz = in.rec[RL::Q + 3];
  const double tw = (double)qw + (double)qw, tx = (double)qx + (double)qx, ty = (double)qy + (double)qy, tz = (double)qz + (double)qz;
  double J[3][4];
  {
    const float n0 = 2.0f * (qw * qx + qy * qz);
    const double d0 = 1.0 - (double)(2.0f * (qx * qx + qy * qy));
    const double dn[4] = {tx, tw, tz, ty}, dd[4] = {0.0, 0.0 - (tx + tx), 0.0 - (ty + ty), 0.0};
    atan2_row((double)n0, d0, dn, dd, J[0]);
    const float t = qw * qy - qx * qz;
    const double asd = 2.0 * (double)t, cosp = std::sqrt(std::fma(0.0 - asd, asd, 1.0));
    const double das[4] = {ty, 0.0 - tz, tw, 0.0 - tx};
    for (int k = 0; k < 4; ++k) J[1][k] = !(asd < 0.99999) ? 0.0 : das[k] / cosp;
    const float n2 = 2.0f * (qw * qz + qx * qy);
    const double d2 = 1.0 - (double)(2.0f * (qy * qy + qz * qz));
    const double dn2[4] = {tz, ty, tx, tw}, dd2[4] = {0.0, 0.0, 0.0 - (ty + ty), 0.0 - (tz + tz)};
    atan2_row((double)n2, d2, dn2, dd2, J[2]);
  }
  const double dR[4][9] = {{0.0, 0.0 - tz, ty, tz, 0.0, 0.0 - tx, 0.0 - ty, tx, 0.0},
                           {0.0, ty, tz, ty, 0.0 - (tx + tx), 0.0 - tw, tz, tw, 0.0 - (tx + tx)},
                           {0.0 - (ty + ty), tx, tw, tx, 0.0, tz, 0.0 - tw, tz, 0.0 - (ty + ty)},
                           {0.0 - (tz + tz), 0.0 - tw, tx, tw, 0.0 - (tz + tz), ty, tx, ty, 0.0}};
  for (int k = 0; k < 4; ++k) {
    double E = 0.0, acc = 0.0;
    for (int a = 0; a < 3; ++a) E = std::fma(J[a][k], o.rpy[a], E);
    for (int e = 0; e < 9; ++e) acc = std::fma(GR[e], dR[k][e], acc);
    o.rec[RL::Q + k] = acc + E;
  }
  for (int s = 0; s < 3; ++s) o.rec[RL::P + s] = in.gx0[3 + s], o.rec[RL::W + s] = in.gx0[6 + s], o.rec[RL::V + s] = in.gx0[9 + s];
  for (int t = 0; t < 3 * NC; ++t) o.rec[RL::R + t] = in.gr[t];
  for (int s = 0; s < 12; ++s) o.rec[RL::WT + s] = in.gw[s];
  for (int k = 0; k < U; ++k) o.rec[RL::AL + k] = in.gal[k];
  o.rec[RL::YAW] = 0.0;
  if (NC == 3) o.rec[RL::FMH] = in.glim[3 + 2];
  for (int t = 0; t < 12 * h; ++t) o.rec[RL::NF + t] = in.gtraj[t];
  return o;
}

template <int NC, int HM>
static int run(std::mt19937 &rng, std::initializer_list<int> horizons) {
  using RL = hmpc::RecLayout<NC>;
  constexpr int U = 6 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  for (int h : horizons)
    for (int variant = 0; variant < 7; ++variant) {
      In<NC> in;
      in.h = h, in.dt = (double)0.03f, in.lt = (double)0.09f, in.lh = (double)0.06f;
      in.Ib[0] = (double)0.5413f, in.Ib[1] = (double)0.52f, in.Ib[2] = (double)0.0691f;
      in.rec.assign(RL::NF + 12 * h, 0.f);
      for (auto &v : in.rec) v = uni(-0.4, 0.4);
      float *q = in.rec.data() + RL::Q;
      for (int k = 0; k < 4; ++k) q[k] = uni(-1, 1);
      {  // a unit quaternion, as far as binary32 goes; variant 6 shortens it (|2 t| <= |q|^2 < 1 keeps the stage's asin defined)
        const float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) / ((variant == 6) ? uni(0.6, 0.95) : 1.0f);
        for (int k = 0; k < 4; ++k) q[k] /= n;
      }
      if (variant == 5) q[0] = 0.70710678f, q[1] = 0.f, q[2] = 0.70710678f, q[3] = 0.f;  // 2 (qw qy - qx qz) = 1: the clamp holds
      in.R.resize(9), rotation(q, in.R.data());
      in.sc.resize(20), in.sc234.resize(4), in.ypsc.resize(4);
      for (int k = 0; k < 10; ++k) {
        const double a = uni(-3, 3);
        in.sc[2 * k] = (float)std::sin(a), in.sc[2 * k + 1] = (float)std::cos(a);
      }
      for (int k = 0; k < 2; ++k) {
        const double a = uni(-3, 3), b = uni(-1.5, 1.5);
        in.sc234[2 * k] = (float)std::sin(a), in.sc234[2 * k + 1] = (float)std::cos(a);
        in.ypsc[2 * k] = (float)std::cos(b), in.ypsc[2 * k + 1] = (float)std::sin(b);
      }
      in.Acd.resize(169), in.Bcd.resize(13 * U);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) in.Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : in.Bcd) v = uni(-0.4, 0.4);
      auto fill = [&](std::vector<double> &v, size_t n) {
        v.resize(n);
        for (auto &e : v) e = (double)uni(-1, 1) * 1.0000001;
      };
      fill(in.gx0, 13), fill(in.gtraj, (size_t)12 * h), fill(in.gw, 12), fill(in.gal, U), fill(in.gA, 169), fill(in.gB, 13 * U), fill(in.gr, 3 * NC);
      fill(in.glim, 3 + NC), fill(in.gFc, (size_t)8 * NC * U);
      if (variant == 1)
        for (auto *v : {&in.gx0, &in.gtraj, &in.gw, &in.gal, &in.gA, &in.gB, &in.gr, &in.glim, &in.gFc})
          for (auto &e : *v) e = 0.0;
      if (variant == 2)  // contact 1 swings at every step: its rows of grad_Fc are exact zeros
        for (int row = 8; row < 16; ++row)
          for (int k = 0; k < U; ++k) in.gFc[(size_t)row * U + k] = 0.0;
      if (variant == 3) in.gB[6 * U + rng() % (3 * U)] = NAN, in.gx0[rng() % 3] = NAN;  // what a NaN force leaves upstream
      if (variant == 4) in.gFc[(size_t)(8 * (rng() % NC) + 4 + rng() % 3) * U + rng() % U] = NAN;
      Out<NC> got(h);
      hipLaunchKernelGGL((pose_adjoint_test_kernel<NC, HM>), dim3(1), dim3(hmpc::PADJ_NT), 0, nullptr, in.rec.data(), in.sc.data(), in.sc234.data(),
                         in.ypsc.data(), in.R.data(), in.Acd.data(), in.Bcd.data(), in.gx0.data(), in.gtraj.data(), in.gw.data(), in.gal.data(),
                         in.gA.data(), in.gB.data(), in.gr.data(), in.glim.data(), in.gFc.data(), h, in.dt, in.lt, in.lh, in.Ib, got.rec.data(),
                         got.frames.data(), got.rpy.data());
      const Out<NC> want = plain<NC>(in);
      bool ok = true;
      if (!got.equals(want))
        ok = false, printf("NC %d HMAX %d h %d variant %d: differ from the plain loop (record %d frames %d rpy %d)\n", NC, HM, h, variant,
                           same(got.rec, want.rec), same(got.frames, want.frames), same(got.rpy, want.rpy));
      if (variant == 1) {
        bool z = true;
        for (const auto *v : {&got.rec, &got.frames, &got.rpy})
          for (double e : *v) z = z && e == 0.0;
        if (!z) ok = false, printf("NC %d HMAX %d h %d: zero upstream gradients and outputs that are not 0\n", NC, HM, h);
      }
      if (variant == 2) {
        bool z = true;
        for (int k = 0; k < 9; ++k) z = z && got.frames[9 * 2 + k] == 0.0;
        for (int k = 5; k < 10; ++k) z = z && got.rec[RL::JA + k] == 0.0;
        if (!z) ok = false, printf("NC %d HMAX %d h %d: a swing contact whose frame or joint angles are not 0\n", NC, HM, h);
      }
      if (variant == 5) {  // grad_x0[1] must not reach q: move it and compare the q slice
        In<NC> in2 = in;
        in2.gx0[1] += 3.0;
        const Out<NC> w2 = plain<NC>(in2);
        Out<NC> g2(h);
        hipLaunchKernelGGL((pose_adjoint_test_kernel<NC, HM>), dim3(1), dim3(hmpc::PADJ_NT), 0, nullptr, in2.rec.data(), in2.sc.data(), in2.sc234.data(),
                           in2.ypsc.data(), in2.R.data(), in2.Acd.data(), in2.Bcd.data(), in2.gx0.data(), in2.gtraj.data(), in2.gw.data(),
                           in2.gal.data(), in2.gA.data(), in2.gB.data(), in2.gr.data(), in2.glim.data(), in2.gFc.data(), h, in2.dt, in2.lt, in2.lh,
                           in2.Ib, g2.rec.data(), g2.frames.data(), g2.rpy.data());
        if (!g2.equals(w2) || memcmp(g2.rec.data() + RL::Q, got.rec.data() + RL::Q, 32) != 0 || g2.rpy[1] == got.rpy[1])
          ok = false, printf("NC %d HMAX %d h %d: a clamped pitch whose row is not 0\n", NC, HM, h);
      }
      if (variant == 0 || variant == 2 || variant == 5 || variant == 6)
        for (const auto *v : {&got.rec, &got.frames, &got.rpy})
          for (double e : *v)
            if (!std::isfinite(e) && ok) ok = false, printf("NC %d HMAX %d h %d variant %d: an output that is not finite\n", NC, HM, h, variant);
      if (got.rec[RL::YAW] != 0.0 || std::signbit(got.rec[RL::YAW])) ok = false, printf("NC %d HMAX %d h %d variant %d: the yaw word is not +0\n", NC, HM, h, variant);
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(41);
  const int bad = run<2, 10>(rng, {1, 3, 10}) + run<2, 20>(rng, {11, 20}) + run<3, 10>(rng, {1, 5, 10});
  printf("%d problems\n", bad);
  return bad != 0;
}
