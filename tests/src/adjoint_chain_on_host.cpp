// tests/test_adjoint_chain_kernel_on_host.py: csrc/hmpc_adjoint_chain.h -- everything of the multi-seed chain kernel behind the assembly
// -- compiled for the CPU against tests/src/hip_lane_shim (one thread per lane).  The oracle is model_adjoint_of_instance ->
// limit_adjoint_of_instance -> pose_adjoint_of_instance of the three single-seed headers under each seed alone (themselves pinned to plain
// loops by their own host tests): every output of every seed compared as bit patterns.  Shapes: (h 10, NC 2) standing, (10, 2) walking
// with a swing foot at step 0, (11 in HMAX 20, 2), (10, 3); S = 1, 2, one seed more than a sub-tile and the whole tile.  Variants: random
// inputs; a zero seed among them (a zero record gradient); a seed that lives on a swing contact alone; a NaN in one seed only (the other
// seeds' bits are the single-seed ones all the same); all ten limits active; an unloaded foot (eight active rows of rank 5); the clamped
// pitch of the quaternion map.  Every case runs with all detail arrays, with none and with two of them: the compact arrays keep their bits,
// and the slots behind the last seed stay untouched.
#include "hmpc_adjoint_chain.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace hmpc;

struct Inputs {
  const float *x0, *Acd, *Bcd, *W, *Fc, *u, *cap, *rec, *sc, *sc234, *ypsc, *R;
  const unsigned char *gait;
  int h;
  double act_tol, dt, mass, lt, lh, Ib[3];
};

// the three single-seed functions in the order the C calls run them, under one seed
template <int NC, int HM>
__global__ void single_kernel(Inputs in, const double *seed, const double *dir, const double *gx0, const double *gtraj, const double *gw,
                              const double *gal, double *gA, double *gB, double *gr, double *gp, double *costate, double *glim, double *gFc,
                              double *gbound, double *lam, double *nu, double *summary, double *grec, double *gframes, double *grpy) {
  using RL = RecLayout<NC>;
  __shared__ ModelAdjointKeep<NC, HM> Mk;
  __shared__ ModelAdjointWork<NC, HM> Mw;
  __shared__ LimitAdjointKeep<NC, HM> Lk;
  __shared__ LimitAdjointWork<NC, HM> Lw;
  __shared__ PoseAdjointWork<NC, HM> Pw;
  model_adjoint_of_instance<NC, HM, MADJ_NT>(in.x0, in.Acd, in.Bcd, in.W, in.rec + RL::NF, in.rec + RL::R, in.R, in.u, dir, in.h, in.dt, in.mass, Mk,
                                             Mw, gA, gB, gr, gp, costate);
  __syncthreads();
  limit_adjoint_of_instance<NC, HM, LADJ_NT>(in.x0, in.Acd, in.Bcd, in.W, in.rec + RL::NF, in.rec + RL::AL, in.Fc, in.u, in.gait, in.cap, dir, seed,
                                             in.h, in.act_tol, in.lt, in.lh, Lk, Lw, glim, gFc, gbound, lam, nu, summary);
  __syncthreads();
  pose_adjoint_of_instance<NC, HM, PADJ_NT>(in.rec, in.sc, in.sc234, in.ypsc, in.R, in.Acd, in.Bcd, gx0, gtraj, gw, gal, gA, gB, gr, glim, gFc, in.h,
                                            in.dt, in.lt, in.lh, in.Ib[0], in.Ib[1], in.Ib[2], Pw, grec, gframes, grpy);
}

template <int NC, int HM, int SUB>
__global__ void chain_kernel(Inputs in, ChainIo io, int ns) {
  using RL = RecLayout<NC>;
  __shared__ ChainKeep<NC, HM> Kp;
  __shared__ ChainWork<NC, HM, SUB> Wk;
  adjoint_chain_of_instance<NC, HM, CADJ_NT, SUB>(in.x0, in.Acd, in.Bcd, in.W, in.rec + RL::NF, in.rec + RL::AL, in.Fc, in.u, in.gait, in.cap, in.rec,
                                                  in.sc, in.sc234, in.ypsc, in.R, io, ns, in.h, in.act_tol, in.dt, in.mass, in.lt, in.lh, in.Ib[0],
                                                  in.Ib[1], in.Ib[2], Kp, Wk);
}

static const double UNTOUCHED = -7.0;
static void rotation(const float *q, float *R) {  // the body rotation from a quaternion in binary32, as the assembly forms it
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
  const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1.0f - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy, R[3] = txy + twz, R[4] = 1.0f - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0f - (txx + tyy);
}

enum Variant { RANDOM, ZERO_SEED, SWING_SEED, NAN_SEED, ALL_ACTIVE, UNLOADED, PITCH_CLAMP, N_VARIANTS };
enum Gait { STANDING, WALKING };
enum { N_OUT = 14, N_COMPACT = 6 };  // grec gframes grpy gparams glim summary | gA gB gr costate gFc gbound lam nu
static const char *OUT_NAME[N_OUT] = {"grad_record", "grad_frames", "grad_rpy", "grad_params", "grad_limits", "limit_summary", "grad_A",
                                      "grad_B",      "grad_r",      "costate",  "grad_Fc",     "grad_bound",  "lambda",        "nu"};

template <int NC, int HM, int SUB>
static int run(std::mt19937 &rng, const int h, const Gait gaitkind) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, C8 = 8 * NC, ST = 6 * NC;
  static_assert(SUB + 1 < ST, "a case with one seed more than a sub-tile");
  int bad = 0;
  auto uni = [&](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() % 100001) / 100000.0); };
  auto col = [&](int c, int k) { return k < 3 ? 3 * c + k : 3 * NC + 3 * c + (k - 3); };
  const size_t row[N_OUT] = {(size_t)RL::NF + 12 * h, 9 * (1 + NC), 3, MADJ_PARAMS, 3 + NC, LADJ_SUMMARY, 169, 13 * U, 3 * NC, MADJ_COSTATE,
                             (size_t)C8 * U, (size_t)10 * NC * h, (size_t)10 * NC * h, (size_t)10 * NC * h};
  for (int variant = 0; variant < N_VARIANTS; ++variant)
    for (int S : {1, 2, SUB + 1, ST}) {
      std::vector<float> x0(13), Acd(169), Bcd(13 * U), W(13), Fc(C8 * U, 0.f), u(U * h), cap(NC, 500.f), rec(RL::NF + 12 * h), sc(20), sc234(4),
          ypsc(4), R(9);
      std::vector<unsigned char> gait(NC * h, 1);
      for (auto &v : x0) v = uni(-1, 1);
      for (auto &v : rec) v = uni(-0.4, 0.4);
      for (int k = 0; k < U; ++k) rec[RL::AL + k] = uni(1e-6, 1e-3);
      float *q = rec.data() + RL::Q;
      for (int k = 0; k < 4; ++k) q[k] = uni(-1, 1);
      const float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int k = 0; k < 4; ++k) q[k] /= n;
      if (variant == PITCH_CLAMP) q[0] = 0.70710678f, q[1] = 0.f, q[2] = 0.70710678f, q[3] = 0.f;  // 2 (qw qy - qx qz) = 1: the clamp holds
      rotation(q, R.data());
      for (int k = 0; k < 10; ++k) {
        const double a = uni(-3, 3);
        sc[2 * k] = (float)std::sin(a), sc[2 * k + 1] = (float)std::cos(a);
      }
      for (int k = 0; k < 2; ++k) {
        const double a = uni(-3, 3), b = uni(-1.5, 1.5);
        sc234[2 * k] = (float)std::sin(a), sc234[2 * k + 1] = (float)std::cos(a);
        ypsc[2 * k] = (float)std::cos(b), ypsc[2 * k + 1] = (float)std::sin(b);
      }
      for (int s = 0; s < 13; ++s)
        for (int k = 0; k < 13; ++k) Acd[s * 13 + k] = (s == k ? 1.f : 0.f) + uni(-0.05, 0.05);
      for (auto &v : Bcd) v = (rng() % 3 == 0) ? 0.f : uni(-0.02, 0.02);
      for (auto &v : W) v = uni(0, 30);
      for (auto &v : u) v = uni(-50, 150);
      if (gaitkind == WALKING)  // contact 0 swings at steps 0 .. 4, contact 1 at steps 5 .. 9, and so on
        for (int i = 0; i < h; ++i) gait[NC * i + (i / 5) % 2] = 0;
      for (int c = 0; c < NC; ++c)
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k) Fc[(8 * c + j) * U + col(c, k)] = (rng() % 4 == 0) ? 0.f : uni(-1, 1);
      double act_tol = 40.0;  // random data: active sets of every size
      if (variant == ALL_ACTIVE) act_tol = 1e30, gait.assign(NC * h, 1);  // rank 6 on every leg-step: all ten limits active
      if (variant == UNLOADED) {  // eight rows spanning five dimensions; zero forces make rows 0-4, 6, 7, 8 active
        float basis[5][6];
        for (int b = 0; b < 5; ++b)
          for (int k = 0; k < 6; ++k) basis[b][k] = (k == b ? 1.f : 0.f) + (k == 5 ? (float)(b + 1) : 0.f);
        for (int j = 0; j < 8; ++j)
          for (int k = 0; k < 6; ++k)
            Fc[j * U + col(0, k)] = j < 5 ? basis[j][k] : (j == 5 ? basis[0][k] + basis[1][k] : (j == 6 ? basis[1][k] - basis[2][k] : basis[3][k] + basis[4][k]));
        for (int k = 0; k < U; ++k) u[k] = 0.f;
        gait[0] = 1;
        act_tol = 1e-3;
      }
      // per-seed inputs [S][..] with one instance per slice (the strides of a batch of one)
      const size_t nseed = (size_t)h * U;
      auto fill = [&](std::vector<double> &v, size_t cnt) {
        v.resize(cnt);
        for (auto &e : v) e = (double)uni(-1, 1) * 1.0000001;
      };
      std::vector<double> seeds, dir, gx0, gtraj, gw, gal;
      fill(seeds, S * nseed), fill(dir, S * nseed), fill(gx0, (size_t)S * 13), fill(gtraj, (size_t)S * 12 * h), fill(gw, (size_t)S * 12), fill(gal, (size_t)S * U);
      const int special = (S > 1) ? 1 : 0;  // the seed the variant is about
      if (variant == ZERO_SEED) {
        for (size_t t = 0; t < nseed; ++t) seeds[special * nseed + t] = 0.0, dir[special * nseed + t] = 0.0;
        for (int t = 0; t < 13; ++t) gx0[special * 13 + t] = 0.0;
        for (int t = 0; t < 12 * h; ++t) gtraj[(size_t)special * 12 * h + t] = 0.0;
        for (int t = 0; t < 12; ++t) gw[special * 12 + t] = 0.0;
        for (int t = 0; t < U; ++t) gal[special * U + t] = 0.0;
      }
      if (variant == NAN_SEED) {  // on a contact in stance, where the seed is read
        const int i = (int)(rng() % (unsigned)h), cc = gait[NC * i] ? 0 : 1;
        seeds[special * nseed + (size_t)U * i + col(cc, (int)(rng() % 6))] = NAN;
      }
      if (variant == SWING_SEED) {  // contact 0 swings at every step; the seed and its dir live on it alone
        for (int i = 0; i < h; ++i) gait[NC * i] = 0, gait[NC * i + 1] = 1;
        for (int i = 0; i < h; ++i)
          for (int c = 0; c < U; ++c) {
            const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3;
            if (cc != 0) seeds[special * nseed + (size_t)U * i + c] = 0.0, dir[special * nseed + (size_t)U * i + c] = 0.0;
          }
      }
      Inputs in = {x0.data(), Acd.data(), Bcd.data(), W.data(), Fc.data(), u.data(), cap.data(), rec.data(), sc.data(), sc234.data(), ypsc.data(),
                   R.data(), gait.data(), h, act_tol, (double)0.03f, (double)13.856f, (double)0.09f, (double)0.06f,
                   {(double)0.5413f, (double)0.52f, (double)0.0691f}};
      // the oracle, seed by seed
      std::vector<double> want[N_OUT];
      for (int k = 0; k < N_OUT; ++k) want[k].assign((size_t)S * row[k], UNTOUCHED);
      for (int s = 0; s < S; ++s) {
        double *o[N_OUT];
        for (int k = 0; k < N_OUT; ++k) o[k] = &want[k][(size_t)s * row[k]];
        hipLaunchKernelGGL((single_kernel<NC, HM>), dim3(1), dim3(CADJ_NT), 0, nullptr, in, &seeds[s * nseed], &dir[s * nseed], &gx0[s * 13],
                           &gtraj[(size_t)s * 12 * h], &gw[s * 12], &gal[s * U], o[6], o[7], o[8], o[3], o[9], o[4], o[10], o[11], o[12], o[13], o[5],
                           o[0], o[1], o[2]);
      }
      bool ok = true;
      for (unsigned mask : {0x3FFFu, 0x3Fu, 0x3Fu | (1u << 6) | (1u << 13)}) {  // all detail arrays, none, grad_A and nu alone
        std::vector<double> got[N_OUT];
        double *p[N_OUT];
        for (int k = 0; k < N_OUT; ++k) got[k].assign((size_t)(S + 1) * row[k], UNTOUCHED), p[k] = ((mask >> k) & 1) ? got[k].data() : nullptr;
        const ChainIo io = {seeds.data(), dir.data(), gx0.data(), gtraj.data(), gw.data(), gal.data(), p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7],
                            p[8], p[9], p[10], p[11], p[12], p[13], 1};
        hipLaunchKernelGGL((chain_kernel<NC, HM, SUB>), dim3(1), dim3(CADJ_NT), 0, nullptr, in, io, S);
        for (int k = 0; k < N_OUT; ++k) {
          if (!((mask >> k) & 1)) continue;
          for (int s = 0; s < S; ++s)
            if (memcmp(&got[k][(size_t)s * row[k]], &want[k][(size_t)s * row[k]], 8 * row[k]) != 0)
              ok = false, printf("NC %d h %d gait %d variant %d S %d mask %x seed %d: %s differs from the single-seed chain\n", NC, h, (int)gaitkind,
                                 variant, S, mask, s, OUT_NAME[k]);
          for (size_t t = (size_t)S * row[k]; t < got[k].size(); ++t)
            if (got[k][t] != UNTOUCHED) ok = false, printf("NC %d h %d variant %d S %d: wrote behind the last seed of %s\n", NC, h, variant, S, OUT_NAME[k]), t = got[k].size();
        }
      }
      for (int s = 1; s < S; ++s)  // lambda, c_1 and the lambda residual carry the same bits in every slice
        if (memcmp(&want[12][(size_t)s * row[12]], want[12].data(), 8 * row[12]) != 0 || memcmp(&want[9][(size_t)s * row[9]], want[9].data(), 8 * 13) != 0 ||
            memcmp(&want[5][(size_t)s * row[5]], want[5].data(), 8) != 0)
          ok = false, printf("NC %d h %d variant %d S %d: the seed-independent outputs differ between slices\n", NC, h, variant, S);
      if (variant == ZERO_SEED)
        for (size_t t = 0; t < row[0]; ++t)
          if (want[0][(size_t)special * row[0] + t] != 0.0) ok = false, printf("NC %d h %d S %d: a zero seed and a record gradient that is not 0\n", NC, h, S), t = row[0];
      if (variant == NAN_SEED && S > 1 && !std::isfinite(want[5][1]) )
        ok = false, printf("NC %d h %d S %d: a NaN in seed %d reached seed 0\n", NC, h, S, special);
      bool moved = false;  // keeps the comparison from passing on zeros
      for (size_t t = 0; t < row[0]; ++t) moved = moved || (want[0][t] != 0.0 && want[0][t] != UNTOUCHED);
      if (!moved && variant == RANDOM) ok = false, printf("NC %d h %d S %d: a record gradient of zeros\n", NC, h, S);
      bad += !ok;
    }
  return bad;
}

int main() {
  std::mt19937 rng(53);
  const int bad = run<2, 10, 5>(rng, 10, STANDING) + run<2, 10, 3>(rng, 10, WALKING) + run<2, 20, 2>(rng, 11, WALKING) + run<3, 10, 4>(rng, 10, STANDING);
  printf("%d problems\n", bad);
  return bad != 0;
}
