// tests/test_model_adjoint_kernel_on_host.py: csrc/hmpc_model_adjoint.h -- everything of the model-gradient kernel behind the assembly --
// compiled for the CPU against tests/src/hip_lane_shim (one thread per lane) and run against a plain loop that states the definition once
// more, sequentially: h = 1, 3, 10 (HMAX = 10) and h = 20 (HMAX = 20), NC = 2, 3, every output compared as bit patterns.  Variants: random
// data; a zero dir (zeros out but c_1); a contact that is swing at every step (its columns of G_B exactly 0); a NaN force (the run must
// end); a NaN dir (the run must end); the rotation of an un-normalised quaternion.
#include "hmpc_model_adjoint.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

template <int NC, int HM>
__global__ void model_adjoint_test_kernel(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj, const float *r,
                                          const float *R, const float *u, const double *dir, int h, double dt, double mass, double *gA, double *gB,
                                          double *gr, double *gp, double *costate) {
  __shared__ hmpc::ModelAdjointKeep<NC, HM> Kp;
  __shared__ hmpc::ModelAdjointWork<NC, HM> Wk;
  hmpc::model_adjoint_of_instance<NC, HM, hmpc::MADJ_NT>(x0, Acd, Bcd, W, traj, r, R, u, dir, h, dt, mass, Kp, Wk, gA, gB, gr, gp, costate);
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
struct Out {
  static constexpr int U = 6 * NC;
  std::vector<double> gA, gB, gr, gp, co;
  Out() : gA(169, -7.0), gB(13 * U, -7.0), gr(3 * NC, -7.0), gp(4, -7.0), co(26, -7.0) {}
  bool equals(const Out &o) const { return same(gA, o.gA) && same(gB, o.gB) && same(gr, o.gr) && same(gp, o.gp) && same(co, o.co); }
};

// the plain loop: the definition, sequentially
template <int NC>
static Out<NC> plain(const std::vector<float> &x0, const std::vector<float> &Acd, const std::vector<float> &Bcd, const std::vector<float> &W,
                     const std::vector<float> &traj, const std::vector<float> &r, const float *R, const std::vector<float> &u,
                     const std::vector<double> &dir, int h, double dt, double mass) {
  constexpr int U = 6 * NC;
  Out<NC> o;
  std::vector<double> A(169), B(13 * U), q2(13, 0.0);
  for (int t = 0; t < 169; ++t) A[t] = (double)Acd[t];
  for (int t = 0; t < 13 * U; ++t) B[t] = (double)Bcd[t];
  for (int s = 0; s < 12; ++s) q2[s] = (double)W[s] + (double)W[s];
  std::vector<double> x(13 * (h + 1)), dx(13 * (h + 1), 0.0), c(13 * (h + 2), 0.0), d(13 * (h + 2), 0.0);
  for (int s = 0; s < 13; ++s) x[s] = (double)x0[s];
  for (int i = 0; i < h; ++i)
    for (int s = 0; s < 13; ++s) {
      double acc = 0.0;
      for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], x[13 * i + k], acc);
      for (int cc = 0; cc < U; ++cc) acc = std::fma(B[s * U + cc], (double)u[U * i + cc], acc);
      x[13 * (i + 1) + s] = acc;
      acc = 0.0;
      for (int k = 0; k < 13; ++k) acc = std::fma(A[s * 13 + k], dx[13 * i + k], acc);
      for (int cc = 0; cc < U; ++cc) acc = std::fma(B[s * U + cc], dir[U * i + cc], acc);
      dx[13 * (i + 1) + s] = acc;
    }
  for (int j = h; j >= 1; --j)  // rows j at 13 j
    for (int s = 0; s < 13; ++s) {
      double tc = 0.0, td = 0.0;
      for (int k = 0; k < 13; ++k) tc = std::fma(A[k * 13 + s], c[13 * (j + 1) + k], tc), td = std::fma(A[k * 13 + s], d[13 * (j + 1) + k], td);
      if (s < 12) {
        tc = std::fma(q2[s], x[13 * j + s] - (double)traj[12 * (j - 1) + s], tc);
        td = std::fma(q2[s], dx[13 * j + s], td);
      }
      c[13 * j + s] = tc, d[13 * j + s] = td;
    }
  for (int a = 0; a < 13; ++a) {
    for (int b = 0; b < 13; ++b) {
      double acc = 0.0;
      for (int i = 0; i < h; ++i) acc = std::fma(c[13 * (i + 1) + a], dx[13 * i + b], acc), acc = std::fma(d[13 * (i + 1) + a], x[13 * i + b], acc);
      o.gA[a * 13 + b] = acc;
    }
    for (int b = 0; b < U; ++b) {
      double acc = 0.0;
      for (int i = 0; i < h; ++i) acc = std::fma(c[13 * (i + 1) + a], dir[U * i + b], acc), acc = std::fma(d[13 * (i + 1) + a], (double)u[U * i + b], acc);
      o.gB[a * U + b] = acc;
    }
  }
  auto GB = [&](int a, int b) { return o.gB[a * U + b]; };
  auto Mb = [&](int a, int m) { return B[(6 + a) * U + 3 * NC + m]; };
  for (int cc = 0; cc < NC; ++cc) {
    double T[3][3];
    for (int m = 0; m < 3; ++m)
      for (int b = 0; b < 3; ++b) {
        double acc = 0.0;
        for (int a = 0; a < 3; ++a) acc = std::fma(Mb(a, m), GB(6 + a, 3 * cc + b), acc);
        T[m][b] = acc;
      }
    o.gr[0 * NC + cc] = T[2][1] - T[1][2], o.gr[1 * NC + cc] = T[0][2] - T[2][0], o.gr[2 * NC + cc] = T[1][0] - T[0][1];
  }
  double sm = 0.0;
  for (int cc = 0; cc < NC; ++cc)
    for (int a = 0; a < 3; ++a) sm = sm + GB(9 + a, 3 * cc + a);
  o.gp[0] = 0.0 - (sm * B[9 * U]) / mass;
  double Gam[3][3];
  for (int a = 0; a < 3; ++a)
    for (int m = 0; m < 3; ++m) {
      double acc = 0.0;
      for (int cc = 0; cc < NC; ++cc) {
        const float r0 = r[0 * NC + cc], r1 = r[1 * NC + cc], r2 = r[2 * NC + cc];
        const float cm[3][3] = {{0.0f, -r2, r1}, {r2, 0.0f, -r0}, {-r1, r0, 0.0f}};
        acc = acc + GB(6 + a, 3 * NC + 3 * cc + m);
        for (int b = 0; b < 3; ++b) acc = std::fma(GB(6 + a, 3 * cc + b), (double)cm[m][b], acc);
      }
      Gam[a][m] = acc;
    }
  for (int k = 0; k < 3; ++k) {
    double w[3], t[3], acc;
    for (int a = 0; a < 3; ++a) {
      acc = 0.0;
      for (int m = 0; m < 3; ++m) acc = std::fma(Mb(a, m), (double)R[3 * m + k], acc);
      w[a] = acc;
    }
    for (int a = 0; a < 3; ++a) {
      acc = 0.0;
      for (int m = 0; m < 3; ++m) acc = std::fma(Gam[a][m], w[m], acc);
      t[a] = acc;
    }
    acc = 0.0;
    for (int a = 0; a < 3; ++a) acc = std::fma(w[a], t[a], acc);
    o.gp[1 + k] = 0.0 - acc / dt;
  }
  for (int s = 0; s < 13; ++s) o.co[s] = c[13 + s], o.co[13 + s] = d[13 + s];
  return o;
}

template <int NC, int HM>
static int run(std::mt19937 &rng, std::initializer_list<int> horizons) {
  constexpr int U = 6 * NC;
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  for (int h : horizons)
    for (int variant = 0; variant < 6; ++variant) {
      std::vector<float> x0(13), Acd(169), Bcd(13 * U), W(13), traj(12 * h), r(3 * NC), u(U * h);
      std::vector<double> dir((size_t)U * h);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : traj) v = uni(-1, 1);
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.4, 0.4);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : r) v = uni(-0.3, 0.3);
      for (auto &v : u) v = uni(-50, 150);
      for (auto &v : dir) v = (double)uni(-1, 1);
      float q[4] = {uni(-1, 1), uni(-1, 1), uni(-1, 1), uni(-1, 1)}, R[9];
      if (variant != 5) {  // a unit quaternion, as far as binary32 goes; variant 5 leaves it un-normalised
        const float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (auto &v : q) v /= n;
      }
      rotation(q, R);
      if (variant == 1) for (auto &v : dir) v = 0.0;  // a zero dir
      if (variant == 2)                                // contact 0 swings at every step: no force, no direction
        for (int i = 0; i < h; ++i)
          for (int k = 0; k < 3; ++k) u[U * i + k] = 0.f, u[U * i + 3 * NC + k] = 0.f, dir[U * i + k] = 0.0, dir[U * i + 3 * NC + k] = 0.0;
      if (variant == 3) u[rng() % u.size()] = NAN;
      if (variant == 4) dir[rng() % dir.size()] = NAN;
      const double dt = (double)0.03f, mass = (double)uni(5, 15);
      Out<NC> got;
      hipLaunchKernelGGL((model_adjoint_test_kernel<NC, HM>), dim3(1), dim3(hmpc::MADJ_NT), 0, nullptr, x0.data(), Acd.data(), Bcd.data(), W.data(),
                         traj.data(), r.data(), R, u.data(), dir.data(), h, dt, mass, got.gA.data(), got.gB.data(), got.gr.data(), got.gp.data(),
                         got.co.data());
      const Out<NC> want = plain<NC>(x0, Acd, Bcd, W, traj, r, R, u, dir, h, dt, mass);
      bool ok = true;
      if (!got.equals(want))
        ok = false, printf("NC %d HMAX %d h %d variant %d: differ from the plain loop (A %d B %d r %d params %d costate %d)\n", NC, HM, h, variant,
                           same(got.gA, want.gA), same(got.gB, want.gB), same(got.gr, want.gr), same(got.gp, want.gp), same(got.co, want.co));
      if (variant == 1) {
        bool z = true;
        for (const auto *v : {&got.gA, &got.gB, &got.gr, &got.gp})
          for (double e : *v) z = z && e == 0.0;
        for (int s = 0; s < 13; ++s) z = z && got.co[13 + s] == 0.0;
        if (!z) ok = false, printf("NC %d HMAX %d h %d: a zero dir and outputs that are not 0\n", NC, HM, h);
      }
      if (variant == 2)
        for (int a = 0; a < 13; ++a)
          for (int k = 0; k < 3; ++k)
            if (got.gB[a * U + k] != 0.0 || got.gB[a * U + 3 * NC + k] != 0.0) ok = false, printf("NC %d HMAX %d h %d: G_B on a swing contact is not 0\n", NC, HM, h);
      if (variant == 0 || variant == 5)
        for (const auto *v : {&got.gA, &got.gB, &got.gr, &got.gp, &got.co})
          for (double e : *v)
            if (!std::isfinite(e)) ok = false;
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(37);
  const int bad = run<2, 10>(rng, {1, 3, 10}) + run<2, 20>(rng, {11, 20}) + run<3, 10>(rng, {1, 5, 10});
  printf("%d problems\n", bad);
  return bad != 0;
}
