// hmpc_certificate.h -- the KKT certificate and the Lagrange multipliers of every solved instance (hmpc_kkt_certificate, DESIGN.md section
// 4.14): everything BEHIND the assembly, as device functions over plain LDS arrays, and the penalty kernel that turns the summaries into a
// mask for hmpc_sweep_select.  The kernel that assembles (hmpc_certificate.hip) calls certificate_of_instance with what the solve kernel's own
// stage function left in LDS; tests/src/certificate_on_host.cpp compiles this header for the CPU (one thread per lane) against a plain loop.
//
// It shares nothing with the solver but the assembly: the gradient comes from the prediction model by a costate recursion (never from H), the
// multipliers from a small non-negative least-squares problem per stance leg-step (never from the active-set iteration).
//
// Definition (fixed in include/hector_mpc.h; tests/certificate_mirror.py restates it in numpy).  Per instance, U = 6 NC, all binary64, every
// sum one ascending chain of explicit fma started at +0, dense:
//   x_1 .. x_h                 as hmpc_predict_states has them, un-rounded
//   q_i[s] = (w_s + w_s) (x_i[s] - traj[12 (i-1) + s])  (s < 12),  q_i[12] = 0;   p_h = q_h,  p_i[s] = q_i[s] + sum_k Acd[k][s] p_{i+1}[k]
//   grad_i[c] = fma(alpha_c + alpha_c, u_i[c], sum_k Bcd[k][c] p_{i+1}[k])
//   slacks s[i][c][0..9] and the stance rule: margins_of_instance (hmpc_margins.h)
//   stance leg-step (i, c): r = grad_i[cols(c)], n_j' = sigma_j' Fc[8 c + src(j')][cols(c)], active j' iff s_j' <= act_tol (NaN: not active);
//   lambda = argmin_{lambda >= 0} |r - N lambda|_2 over the active columns (nnls_leg_step), e = r - N lambda; swing: lambda = 0, e = 0
//   summary[0..3], where[0..1]: (value, index) maxima over the stance leg-steps, a NaN candidate counting as +inf.
// Mapping: lanes s < 13 run the forward and the backward chain (one barrier per step, x_i and p_i of all steps stay in LDS); all NT lanes
// share the U h gradient chains and the slacks; lane ls < NC h runs the NNLS of leg-step ls with its working set (Gram factor, the two
// right-hand sides) in an LDS slice of its own of NNLS_WORK doubles (an odd count: neighbouring lanes fall on different banks), lambda in
// the staged output; the passive set is a list of nibbles in a register.  No atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_margins.h"
#include "hmpc_record.h"

namespace hmpc {
constexpr int CERT_NT = DERIVED_NT;  // threads per workgroup (one workgroup per instance)
constexpr int CERT_WAVES = CERT_NT / 64;
constexpr int CERT_CLASSES = 4;  // stationarity, complementarity, primal violation, gradient scale
constexpr int CERT_WHERE = 2;    // positions of the first two
constexpr int CERT_CEILS = 3;    // the gradient scale has no ceiling
constexpr int NNLS_WORK = 33;    // doubles per lane: packed Gram factor (21), z (6), y (6)
constexpr int NNLS_STEPS = 32;   // outer steps at most, and inner steps at most, in total
constexpr double NNLS_PIVOT = 1e-12;

struct CertMax {
  double v;
  int idx;
};

// a candidate (NaN counting as +inf) replaces the incumbent iff its value is > the incumbent's, or == with a lower index
__device__ __forceinline__ CertMax cert_max(const CertMax inc, const CertMax cand) {
  const double v = (cand.v == cand.v) ? cand.v : margins_inf();
  const bool take = v > inc.v || (v == inc.v && cand.idx < inc.idx);
  return take ? CertMax{v, cand.idx} : inc;
}
// every candidate is >= 0: the incumbent before the first one
__device__ __forceinline__ CertMax cert_none() { return {-1.0, INT_MAX}; }

// row of the constraint block and sign of one-sided constraint j' < 10 (the order of the slack table)
__device__ __forceinline__ int cert_src(const int j) { return j < 5 ? j : (j < 9 ? j - 1 : 7); }
__device__ __forceinline__ double cert_sign(const int j) { return ((0x2E0 >> j) & 1) ? -1.0 : 1.0; }

// Multipliers of one stance leg-step, by one lane: Lawson-Hanson over the columns j' of `active` (bit j'), scanned in ascending j', ties
// to the lowest; the passive-set least squares through the Cholesky factor of its Gram matrix, a row appended per admitted column and
// rebuilt when columns leave.  A column whose pivot is below NNLS_PIVOT of its own diagonal is not admitted, nor is a seventh; a column
// whose first solution is not > 0 leaves again at once; both stay barred until lambda has moved.  A solution that is not finite, a
// factor that fails and the step caps end the loop.  lam[10] (any memory, indexed at run time) holds lambda >= 0 whenever the loop
// stops, and e = r - N lam is formed from that.  Fc: the block [8 NC][6 NC]; work: NNLS_WORK doubles of this lane's own.
template <int NC>
__device__ __forceinline__ void nnls_leg_step(const float *Fc, const int c, const double (&r)[6], const unsigned active, double *lam,
                                              double *work, double (&e)[6]) {
  constexpr int U = 6 * NC;
  const float *rows = Fc + 8 * c * U;
  double *Lf = work, *z = work + 21, *y = work + 27;  // L(a, b), b <= a, at a (a + 1) / 2 + b
  auto N = [&](const int j, const int k) -> double {
    const int col = (k < 3) ? 3 * c + k : 3 * NC + 3 * c + (k - 3);
    return cert_sign(j) * (double)rows[cert_src(j) * U + col];
  };
  auto dot_nn = [&](const int a, const int b) -> double {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = __builtin_fma(N(a, k), N(b, k), acc);
    return acc;
  };
  auto dot_nv = [&](const int a, const double(&v)[6]) -> double {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = __builtin_fma(N(a, k), v[k], acc);
    return acc;
  };
  unsigned plist = 0, pmask = 0, barred = 0;  // passive set: nibble a of plist = its a-th column, in the order of admission
  int m = 0;
  auto col_of = [&](const int a) -> int { return (int)((plist >> (4 * a)) & 15u); };
  auto residual = [&]() {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < 10; ++j) {
      const double lj = lam[j];
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[k] = __builtin_fma(N(j, k), lj, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = r[k] - acc[k];
  };
  // row m of the factor for column j; false (nothing changed) when its pivot is too small
  auto append = [&](const int j) -> bool {
    if (m >= 6) return false;
    const double djj = dot_nn(j, j);
    double ss = 0.0;
    double *row = Lf + m * (m + 1) / 2;
    for (int a = 0; a < m; ++a) {
      double v = dot_nn(col_of(a), j);
      const double *ra = Lf + a * (a + 1) / 2;
      for (int b = 0; b < a; ++b) v = __builtin_fma(-ra[b], row[b], v);
      v = v / ra[a];
      row[a] = v;
      ss = __builtin_fma(v, v, ss);
    }
    const double d = djj - ss;
    if (!(d >= NNLS_PIVOT * djj && d > 0.0)) return false;
    row[m] = __builtin_sqrt(d);
    plist |= (unsigned)j << (4 * m);
    pmask |= 1u << j;
    ++m;
    return true;
  };
  // z = argmin |r - N_P z|: L y = N_P' r, L' z = y; false when some z is not finite
  auto solve = [&]() -> bool {
    for (int a = 0; a < m; ++a) {
      double v = dot_nv(col_of(a), r);
      const double *ra = Lf + a * (a + 1) / 2;
      for (int b = 0; b < a; ++b) v = __builtin_fma(-ra[b], y[b], v);
      y[a] = v / ra[a];
    }
    bool finite = true;
    for (int a = m - 1; a >= 0; --a) {
      double v = y[a];
      for (int b = a + 1; b < m; ++b) v = __builtin_fma(-Lf[b * (b + 1) / 2 + a], z[b], v);
      v = v / Lf[a * (a + 1) / 2 + a];
      z[a] = v;
      finite = finite && (v - v == 0.0);
    }
    return finite;
  };
  for (int j = 0; j < 10; ++j) lam[j] = 0.0;
  residual();
  int outer = 0, inner = 0;
  bool stop = false;
  while (!stop && outer < NNLS_STEPS) {
    int js = -1;
    double wbest = 0.0;
    for (int j = 0; j < 10; ++j)
      if (((active & ~pmask & ~barred) >> j) & 1u) {
        const double w = dot_nv(j, e);
        if (w > wbest) wbest = w, js = j;
      }
    if (js < 0) break;
    ++outer;
    if (!append(js)) {
      barred |= 1u << js;
      continue;
    }
    if (!solve()) break;
    if (!(z[m - 1] > 0.0)) {  // the new column would get no weight: it leaves again, lambda has not moved
      --m;
      plist &= ~(15u << (4 * m));
      pmask &= ~(1u << js);
      barred |= 1u << js;
      continue;
    }
    for (;;) {
      int amin = -1, jmin = 16;
      double al = 0.0;
      for (int a = 0; a < m; ++a)
        if (!(z[a] > 0.0)) {
          const int ja = col_of(a);
          const double la = lam[ja];
          double t = la / (la - z[a]);
          if (!(t >= 0.0)) t = 0.0;
          if (amin < 0 || t < al || (t == al && ja < jmin)) amin = a, jmin = ja, al = t;
        }
      if (amin < 0) {
        for (int a = 0; a < m; ++a) lam[col_of(a)] = z[a];
        break;
      }
      if (inner >= NNLS_STEPS) {
        stop = true;
        break;
      }
      ++inner;
      unsigned keep = 0;
      int nk = 0;
      for (int a = 0; a < m; ++a) {
        const int ja = col_of(a);
        double v = __builtin_fma(al, z[a] - lam[ja], lam[ja]);
        if (!(v > 0.0) || a == amin) v = 0.0;
        lam[ja] = v;
        if (v > 0.0) keep |= (unsigned)ja << (4 * nk), ++nk;
      }
      plist = 0, pmask = 0, m = 0;
      for (int a = 0; a < nk && !stop; ++a)
        if (!append((int)((keep >> (4 * a)) & 15u))) stop = true;
      if (stop || !solve()) {
        stop = true;
        break;
      }
    }
    if (stop) break;
    residual();
    barred = 0;
  }
  residual();
}

// scratch of certificate_of_instance (LDS, or any memory all lanes see)
template <int NC, int HMAX>
struct CertScratch {
  double x[13 * (HMAX + 1)];  // x_0 .. x_h, un-rounded
  double p[13 * (HMAX + 1)];  // p_1 .. p_h at 13 i
  double slack[10 * NC * HMAX];
  double grad[6 * NC * HMAX];  // grad, lam and res: staged for coalesced stores
  double lam[10 * NC * HMAX];
  double res[6 * NC * HMAX];
  double work[NNLS_WORK * NC * HMAX];
  MarginMin wave_min[CERT_WAVES][MARGIN_CLASSES];
  CertMax wave_max[CERT_WAVES][CERT_CLASSES];
};

// The certificate of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): Acd[13][13], Bcd[13][6 NC],
// x0[13], W[12], traj[12 h], alpha[6 NC], Fc[8 NC][6 NC], u[h][6 NC], gait[NC h] bytes, cap[NC].  Out: grad_out[h][6 NC],
// lam_out[h][NC][10], res_out[h][NC][6], summary_out[4], where_out[2] (each may be nullptr).  Every lane of the workgroup calls it.
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void certificate_of_instance(const float *Acd, const float *Bcd, const float *x0, const float *W, const float *traj,
                                                        const float *alpha, const float *Fc, const float *u, const unsigned char *gait,
                                                        const float *cap, const int h, const double act_tol, CertScratch<NC, HMAX> &T,
                                                        double *grad_out, double *lam_out, double *res_out, double *summary_out,
                                                        int32_t *where_out) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  if (tid < 13) T.x[tid] = (double)x0[tid];
  __syncthreads();
  for (int i = 0; i < h; ++i) {  // states: the chain of hmpc_predict_states
    if (tid < 13) {
      const double *x = T.x + 13 * i;
      const float *ui = u + U * i;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma((double)Acd[tid * 13 + k], x[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma((double)Bcd[tid * U + c], (double)ui[c], acc);
      T.x[13 * (i + 1) + tid] = acc;
    }
    __syncthreads();
  }
  for (int i = h; i >= 1; --i) {  // costate
    if (tid < 13) {
      double q = 0.0;
      if (tid < 12) {
        const double w = (double)W[tid];
        q = (w + w) * (T.x[13 * i + tid] - (double)traj[12 * (i - 1) + tid]);
      }
      if (i < h) {
        const double *pn = T.p + 13 * (i + 1);
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma((double)Acd[k * 13 + tid], pn[k], acc);
        q = q + acc;
      }
      T.p[13 * i + tid] = q;
    }
    __syncthreads();
  }
  for (int t = tid; t < U * h; t += NT) {  // gradient
    const int i = t / U, c = t % U;
    const double *pn = T.p + 13 * (i + 1);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 13; ++k) acc = __builtin_fma((double)Bcd[k * U + c], pn[k], acc);
    const double al = (double)alpha[c];
    T.grad[t] = __builtin_fma(al + al, (double)u[t], acc);
  }
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, T.slack, T.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  CertMax best[CERT_CLASSES];
#pragma unroll
  for (int k = 0; k < CERT_CLASSES; ++k) best[k] = cert_none();
  for (int ls = tid; ls < NC * h; ls += NT) {
    const int i = ls / NC, c = ls % NC;
    double *lam = T.lam + 10 * ls, *res = T.res + 6 * ls;
    if (!stance(cap[c], gait[ls])) {  // its variables were eliminated
      for (int j = 0; j < 10; ++j) lam[j] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) res[k] = 0.0;
      continue;
    }
    const double *s = T.slack + 10 * ls;
    double r[6], e[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = T.grad[U * i + ((k < 3) ? 3 * c + k : 3 * NC + 3 * c + (k - 3))];
    unsigned active = 0;
    for (int j = 0; j < 10; ++j) active |= (s[j] <= act_tol) ? (1u << j) : 0u;
    nnls_leg_step<NC>(Fc, c, r, active, lam, T.work + NNLS_WORK * ls, e);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      res[k] = e[k];
      best[0] = cert_max(best[0], {__builtin_fabs(e[k]), 6 * ls + k});
      best[3] = cert_max(best[3], {__builtin_fabs(r[k]), 6 * ls + k});
    }
    for (int j = 0; j < 10; ++j) {
      const double sj = s[j];
      if ((active >> j) & 1u) best[1] = cert_max(best[1], {lam[j] * (sj > 0.0 ? sj : 0.0), 10 * ls + j});
      best[2] = cert_max(best[2], {(sj < 0.0) ? 0.0 - sj : ((sj == sj) ? 0.0 : sj), 10 * ls + j});  // max(0, -s); a NaN slack stays NaN
    }
  }
#pragma unroll
  for (int k = 0; k < CERT_CLASSES; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      CertMax other;
      other.v = __shfl_xor(best[k].v, off, 64);
      other.idx = __shfl_xor(best[k].idx, off, 64);
      best[k] = cert_max(best[k], other);
    }
    if ((tid & 63) == 0) T.wave_max[tid >> 6][k] = best[k];
  }
  __syncthreads();
  if (grad_out)
    for (int t = tid; t < U * h; t += NT) grad_out[t] = T.grad[t];
  if (lam_out)
    for (int t = tid; t < 10 * NC * h; t += NT) lam_out[t] = T.lam[t];
  if (res_out)
    for (int t = tid; t < 6 * NC * h; t += NT) res_out[t] = T.res[t];
  if (tid < CERT_CLASSES) {
    CertMax win = T.wave_max[0][tid];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) win = cert_max(win, T.wave_max[w][tid]);
    const bool none = win.idx == INT_MAX;
    if (summary_out) summary_out[tid] = none ? 0.0 : win.v;
    if (where_out && tid < CERT_WHERE) where_out[tid] = none ? -1 : win.idx;
  }
  __syncthreads();
}

// out[i] = +inf if for some k < 3 with a non-NaN ceil[k] the test summary[i][k] <= ceil[k] is false (a NaN summary masks), else
// penalty_in ? penalty_in[i] : +0.0.  One thread per instance; out may be penalty_in.
struct CertCeil {
  double v[CERT_CEILS];
};
template <int NT>
__global__ __launch_bounds__(NT) void certificate_penalty_kernel(const double *summary, const CertCeil ceil, const double *penalty_in,
                                                                 double *out, const int batch) {
  const int i = (int)(blockIdx.x * NT + threadIdx.x);
  if (i >= batch) return;
  bool pass = true;
#pragma unroll
  for (int k = 0; k < CERT_CEILS; ++k) {
    const double c = ceil.v[k];
    if (c == c) pass = pass && (summary[(size_t)CERT_CLASSES * i + k] <= c);
  }
  out[i] = pass ? (penalty_in ? penalty_in[i] : 0.0) : margins_inf();
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct CertificateOut {
  double *grad, *lambda, *resid, *summary;  // [batch][h][6 nc], [batch][h][nc][10], [batch][h][nc][6], [batch][4]
  int32_t *where;                           // [batch][2]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants, mu_inst) and `forces`; it writes `out` and nothing else.  Shapes: derived_shape (hmpc_derived_shape.h); anything else:
// hipErrorInvalidValue, nothing launched.
hipError_t launch_certificate(int nc, const KernelArgs &args, double act_tol, const CertificateOut &out, hipStream_t stream);
// out[batch] from summary[batch][4] and ceil[3]; penalty_in may be nullptr or out.
hipError_t launch_certificate_penalty(const double *summary, const double ceil[CERT_CEILS], const double *penalty_in, double *out, int batch,
                                      hipStream_t stream);
}  // namespace hmpc
#endif
