// hmpc_feedback.h -- the feedback gains of every solved instance (hmpc_feedback_gains) and the first-order force
// update built on them (hmpc_first_order_wrench): everything BEHIND the assembly, as device functions over plain LDS arrays.  The kernels
// that assemble (hmpc_feedback.hip) call feedback_of_instance / first_order_of_instance with what the solve kernel's own stage function
// left in LDS; tests/src/feedback_on_host.cpp compiles this header for the CPU (one thread per lane) against a plain loop.
//
// With the active set of the solved QP frozen, the MPC is an equality-constrained LQ problem whose constraints act on one leg-step's six
// variables only, so a Riccati recursion over 13 x 13 and U x U matrices gives du_0/dx_0 and du_0/dX_d exactly: no H, no H^-1, nothing
// of the solver.
//
// Definition (fixed in include/hector_mpc.h; tests/feedback_mirror.py restates it in numpy).  Per instance, U = 6 NC, all binary64, every
// sum one ascending chain of explicit fma started at +0.  A = Acd, B = Bcd, Q = diag(w + w, 0), R = diag(alpha + alpha).
//   slacks s[i][c][0..9], the stance rule: margins_of_instance (hmpc_margins.h); j' is active iff s_j' <= act_tol (NaN: not active)
//   stance leg-step (i, c): the active normals n_j' = sigma_j' Fc[8 c + src(j')][cols(c)] in ascending j', each reduced against the
//     vectors held by modified Gram-Schmidt applied twice, admitted (divided by its remaining length) iff fewer than six are held and
//     its squared remainder is > 0 and >= 1e-12 of its own squared length; then, until six are held, the unit vector e_k not yet taken
//     with the largest squared remainder (reduced the same way; > decides, so ties go to the lowest k), divided by its remaining length:
//     these are the columns of Z_{i,c}.  Swing: no columns.  Z_i puts Z_{i,c} on cols(c), contacts ascending; r_i = free_dims[i].
//     Sums over a column of Z_i run over the six rows of its contact, sums over a row of Z_i over the columns of its contact.
//   P_h = Q; for i = h-1 .. 0, with P = P_{i+1}:  PA = P A, PB = P B, W = R + B' PB, G = Z_i' (W Z_i), X = G^-1 (Z_i' B') through the
//     Cholesky factor of the lower triangle of G (pivot d_j = G_jj - sum_b L_jb^2, L_jj = sqrt(d_j); two triangular solves),
//     S_i = Z_i X, K_i = 0 - S_i PA (both exactly 0 when r_i = 0), and for i > 0  M_i = A + B K_i,  P_i = Q + PA' M_i evaluated on the
//     upper triangle and copied to the lower.
//   gain = K_0;  Psi_1 = S_0, Psi_{j+1} = Psi_j M_j';  ref_gain[j-1][c][s] = Psi_j[c][s] (w_s + w_s), s < 12.
//   summary[0] = min over all pivots of d_j / G_jj (NaN counting as 0; 1 with no pivot), summary[1] = max |K_0| (NaN counting as +inf).
// Every loop's trip count is fixed by (h, NC) and the number of held vectors (<= 6): nothing iterates on data.
// A step of the backward pass is riccati_gain_step + riccati_cost_step, which the adjoint (hmpc_adjoint.h) compiles too, with its vector
// recursion switched on.
// Mapping: the NC h Gram-Schmidt problems run one per lane before the backward pass (they do not depend on P), each on the 36 doubles
// of its own slot of Z; the products of a step are spread over all NT lanes, one output entry per lane and pass, a barrier between
// dependent products; the Cholesky factor is built column by column (lane a owns row a; one barrier per column), the 13 right-hand
// sides are solved one per lane with no barrier.  M_1 .. M_{h-1} stay in LDS for the forward chain of Psi; ref_gain rows are stored
// straight from Psi in coalesced passes.  No atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_certificate.h"
#include "hmpc_margins.h"
#include "hmpc_record.h"

namespace hmpc {
constexpr int FB_NT = DERIVED_NT;  // threads per workgroup (one workgroup per instance); lane 64 keeps the pivot minimum
static_assert(FB_NT > 64, "a lane of a second wave");
constexpr int FB_SUMMARY = 2;
constexpr double FB_DEPENDENT = 1e-12;

template <int NC>
__device__ __forceinline__ int fb_col(const int c, const int k) {
  return (k < 3) ? 3 * c + k : 3 * NC + 3 * c + (k - 3);
}

// Z_i of one step: where column b < r_i lies (its contact cb, its six entries), from the step's NC slots of Z, the normals each contact's
// leg-step holds and the first column of the second and third contact
__device__ __forceinline__ const double *fb_zcol(const double *Zi, const int hl0, const int hl1, const int hl2, const int o1, const int o2,
                                                 const int b, int &cb) {
  cb = (b >= o2) ? 2 : ((b >= o1) ? 1 : 0);
  const int hb = (cb == 2) ? hl2 : ((cb == 1) ? hl1 : hl0), ob = (cb == 2) ? o2 : ((cb == 1) ? o1 : 0);
  return Zi + 36 * cb + 6 * (hb + b - ob);
}

// what feedback_of_instance keeps from its first phase (LDS, or any memory all lanes see)
template <int NC, int HMAX>
struct FeedbackKeep {
  double A[169], B[13 * 6 * NC], q2[13], r2[6 * NC];  // Acd, Bcd, the diagonals of Q and R
  double Z[36 * NC * HMAX];                           // per leg-step: six vectors of six, the held normals first
  double slack[10 * NC * HMAX];
  MarginMin wave_min[FB_NT / 64][MARGIN_CLASSES];
  unsigned char held[NC * HMAX];  // normals held by leg-step (its free directions: vectors held .. 5); 6 for a swing leg-step
};

// scratch of the backward and the forward pass; may overlay the binary32 inputs of feedback_of_instance, which are not read again once
// the first phase has ended
template <int NC, int HMAX>
struct FeedbackWork {
  static constexpr int U = 6 * NC;
  double M[(HMAX > 1 ? HMAX - 1 : 1) * 169];  // M_1 .. M_{h-1}
  double P[169], PA[169], PB[13 * U];
  double W[U * U], WZ[U * U], G[U * U], Ld[U], piv[U];
  double X[U * 13], S[U * 13], K[U * 13], Psi[2][U * 13];
  double red[FB_NT];
};

// The free directions of one stance leg-step, by one lane: q[36] receives six orthonormal vectors, the admitted normals first; returns
// how many normals were admitted.  s: the ten slacks; Fc: the block [8 NC][6 NC].
template <int NC>
__device__ __forceinline__ int free_directions(const float *Fc, const int c, const double *s, const double act_tol, double *q) {
  constexpr int U = 6 * NC;
  const float *rows = Fc + 8 * c * U;
  int m = 0;
  auto reduce = [&](double(&v)[6]) {
    for (int pass = 0; pass < 2; ++pass)
      for (int a = 0; a < m; ++a) {
        const double *qa = q + 6 * a;
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) d = __builtin_fma(qa[k], v[k], d);
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = __builtin_fma(0.0 - d, qa[k], v[k]);
      }
  };
  auto norm2 = [](const double(&v)[6]) -> double {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = __builtin_fma(v[k], v[k], acc);
    return acc;
  };
  auto hold = [&](const double(&v)[6], const double rem2) {
    const double len = __builtin_sqrt(rem2);
#pragma unroll
    for (int k = 0; k < 6; ++k) q[6 * m + k] = v[k] / len;
    ++m;
  };
  for (int j = 0; j < 10; ++j) {
    if (!(s[j] <= act_tol)) continue;
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = cert_sign(j) * (double)rows[cert_src(j) * U + fb_col<NC>(c, k)];
    const double len2 = norm2(v);
    reduce(v);
    const double rem2 = norm2(v);
    if (m < 6 && rem2 > 0.0 && rem2 >= FB_DEPENDENT * len2) hold(v, rem2);
  }
  const int normals = m;
  unsigned taken = 0;
  for (int round = normals; round < 6; ++round) {
    int best = -1;
    double vb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rb = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if ((taken >> k) & 1u) continue;
      double v[6];
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) v[kk] = (kk == k) ? 1.0 : 0.0;
      reduce(v);
      const double rem2 = norm2(v);
      if (best < 0 || rem2 > rb) {
        best = k, rb = rem2;
#pragma unroll
        for (int kk = 0; kk < 6; ++kk) vb[kk] = v[kk];
      }
    }
    taken |= 1u << best;
    hold(vb, rb);
  }
  return normals;
}

// The first loop of free_directions once more, for the limit gradients (hmpc_limit_adjoint.h): the same decisions over the same chains,
// and which rows j' were admitted -- nibble b of `rows` is j_b, ascending.  q[36] receives the admitted normals' orthonormal vectors
// q_0 .. q_{m-1} only (bit for bit free_directions' first m); returns m.  A function of its own beside free_directions, which does not
// call it: an out-parameter there would change the machine code of the gains' and the adjoint's kernels (scripts/isa_hash.py --diff).
// tests/src/limit_adjoint_on_host.cpp pins the two against each other.  Change both or neither.
template <int NC>
__device__ __forceinline__ int admitted_normals(const float *Fc, const int c, const double *s, const double act_tol, double *q, unsigned &rows_out) {
  constexpr int U = 6 * NC;
  const float *rows = Fc + 8 * c * U;
  int m = 0;
  unsigned list = 0;
  for (int j = 0; j < 10; ++j) {
    if (!(s[j] <= act_tol)) continue;
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = cert_sign(j) * (double)rows[cert_src(j) * U + fb_col<NC>(c, k)];
    double len2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) len2 = __builtin_fma(v[k], v[k], len2);
    for (int pass = 0; pass < 2; ++pass)
      for (int a = 0; a < m; ++a) {
        const double *qa = q + 6 * a;
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) d = __builtin_fma(qa[k], v[k], d);
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = __builtin_fma(0.0 - d, qa[k], v[k]);
      }
    double rem2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) rem2 = __builtin_fma(v[k], v[k], rem2);
    if (m < 6 && rem2 > 0.0 && rem2 >= FB_DEPENDENT * len2) {
      const double len = __builtin_sqrt(rem2);
#pragma unroll
      for (int k = 0; k < 6; ++k) q[6 * m + k] = v[k] / len;
      list |= (unsigned)j << (4 * m);
      ++m;
    }
  }
  rows_out = list;
  return m;
}

// What the adjoint's vector recursion (hmpc_adjoint.h) adds to a step of the backward pass: l_i, p_{i+1}, where p_i and k_i go.  The gains
// leave it empty.
struct RiccatiVec {
  const double *ell = nullptr, *p = nullptr;
  double *p_next = nullptr, *k = nullptr;
};

// Step i of the backward pass up to K_i, by the NT lanes of the workgroup (every lane calls it; P = P_{i+1} in Wk.P on entry, behind a
// barrier; the caller puts a barrier behind it): PA, PB, W, G, the Cholesky factor, X, S_i (Wk.S), K_i (K[U][13]).  With
// riccati_cost_step the matrix step that feedback_of_instance and adjoint_of_instance share.  VEC: the vector recursion of hmpc_adjoint.h
// rides in the passes' spare lanes (Work then has v[U], y[U] too): v beside PA / PB, y = Z'v beside W / X, its triangular solves on
// lane 13 in the loop of the columns of X (a branch of its own would run behind them), k_i beside S, p_i beside P_i.  Without VEC none
// of that is compiled.
template <int NC, int HMAX, int NT, bool VEC, class Work>
__device__ __forceinline__ void riccati_gain_step(FeedbackKeep<NC, HMAX> &Kp, Work &Wk, const int i, double *K, double &pivmin,
                                                  const RiccatiVec vec) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  const double *A = Kp.A, *B = Kp.B;
  // normals held by each contact's leg-step, the first column of each contact in Z_i (the first contact's is 0), and r_i
  const int hl0 = (int)Kp.held[NC * i], hl1 = (int)Kp.held[NC * i + 1], hl2 = (NC == 3) ? (int)Kp.held[NC * i + NC - 1] : 6;
  const int o1 = 6 - hl0, o2 = o1 + 6 - hl1, r = o2 + 6 - hl2;
  const double *Zi = Kp.Z + 36 * NC * i;
  for (int t = tid; t < 169 + 13 * U + (VEC ? U : 0); t += NT) {  // PA = P A, PB = P B;  (VEC) v = l_i + B' p
    double acc = 0.0;
    if (t < 169) {
      const int k = t / 13, s = t % 13;
#pragma unroll
      for (int l = 0; l < 13; ++l) acc = __builtin_fma(Wk.P[k * 13 + l], A[l * 13 + s], acc);
      Wk.PA[t] = acc;
    } else if (!VEC || t < 169 + 13 * U) {
      const int k = (t - 169) / U, c = (t - 169) % U;
#pragma unroll
      for (int l = 0; l < 13; ++l) acc = __builtin_fma(Wk.P[k * 13 + l], B[l * U + c], acc);
      Wk.PB[t - 169] = acc;
    } else if constexpr (VEC) {
      const int c = t - 169 - 13 * U;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(B[k * U + c], vec.p[k], acc);
      Wk.v[c] = vec.ell[c] + acc;
    }
  }
  __syncthreads();
  if (r > 0) {  // (uniform)
    for (int t = tid; t < U * U + 13 * r + (VEC ? r : 0); t += NT) {  // W = R + B' PB;  X = Z' B';  (VEC) y = Z' v
      double acc = 0.0;
      if (t < U * U) {
        const int c = t / U, d = t % U;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(B[k * U + c], Wk.PB[k * U + d], acc);
        Wk.W[t] = (c == d) ? Kp.r2[c] + acc : acc;
      } else if (!VEC || t < U * U + 13 * r) {
        const int a = (t - U * U) / 13, s = (t - U * U) % 13;
        int ca;
        const double *za = fb_zcol(Zi, hl0, hl1, hl2, o1, o2, a, ca);
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = __builtin_fma(za[k], B[s * U + fb_col<NC>(ca, k)], acc);
        Wk.X[a * 13 + s] = acc;
      } else if constexpr (VEC) {
        const int a = t - U * U - 13 * r;
        int ca;
        const double *za = fb_zcol(Zi, hl0, hl1, hl2, o1, o2, a, ca);
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = __builtin_fma(za[k], Wk.v[fb_col<NC>(ca, k)], acc);
        Wk.y[a] = acc;
      }
    }
    __syncthreads();
    for (int t = tid; t < U * r; t += NT) {  // WZ = W Z
      const int c = t / r, b = t % r;
      int cb;
      const double *zb = fb_zcol(Zi, hl0, hl1, hl2, o1, o2, b, cb);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = __builtin_fma(Wk.W[c * U + fb_col<NC>(cb, k)], zb[k], acc);
      Wk.WZ[c * U + b] = acc;
    }
    __syncthreads();
    for (int t = tid; t < r * r; t += NT) {  // G = Z' WZ
      const int a = t / r, b = t % r;
      int ca;
      const double *za = fb_zcol(Zi, hl0, hl1, hl2, o1, o2, a, ca);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = __builtin_fma(za[k], Wk.WZ[fb_col<NC>(ca, k) * U + b], acc);
      Wk.G[a * U + b] = acc;
    }
    __syncthreads();
    // (the chains below run over all U slots with the terms outside their range switched off: the loads do not wait for each other)
    for (int j = 0; j < r; ++j) {  // Cholesky, column j: lane a >= j owns row a; L below the diagonal in G, its diagonal in Ld
      if (tid >= j && tid < r) {
        const double gjj = Wk.G[j * U + j];
        double ss = 0.0, acc = 0.0;
#pragma unroll
        for (int b = 0; b < U; ++b) {
          const double ljb = Wk.G[j * U + b], lab = Wk.G[tid * U + b];
          ss = (b < j) ? __builtin_fma(ljb, ljb, ss) : ss;
          acc = (b < j) ? __builtin_fma(lab, ljb, acc) : acc;
        }
        const double d = gjj - ss, ljj = __builtin_sqrt(d);
        if (tid == j) Wk.Ld[j] = ljj, Wk.piv[j] = d / gjj;
        else Wk.G[tid * U + j] = (Wk.G[tid * U + j] - acc) / ljj;
      }
      __syncthreads();
    }
    // Two copies of the two triangular solves, on purpose.  The second is the gains' own, kept verbatim: written over (col, ld) like the
    // first it compiles to other machine code for the kernels of hmpc_feedback.hip, whose hashes must stay (scripts/isa_hash.py --diff).
    // The first adds the vector y as a fourteenth lane of the same loop; as a branch of its own it would run behind the columns of X
    // (same wave), 25 % slower over the launch (profiles/r20/README.md).  Change both or neither, and check the hashes.
    if constexpr (VEC) {
      if (tid < 14) {  // the same two solves, with the same chains: lanes 0 .. 12 a column of X each, lane 13 the vector y beside them
        double *col = (tid < 13) ? Wk.X + tid : Wk.y;
        const int ld = (tid < 13) ? 13 : 1;
        for (int a = 0; a < r; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int b = 0; b < U; ++b) {
            const double l = Wk.G[a * U + b], x = col[b * ld];
            acc = (b < a) ? __builtin_fma(l, x, acc) : acc;
          }
          col[a * ld] = (col[a * ld] - acc) / Wk.Ld[a];
        }
        for (int a = r - 1; a >= 0; --a) {
          double acc = 0.0;
#pragma unroll
          for (int b = 0; b < U; ++b) {
            const double l = Wk.G[b * U + a], x = col[b * ld];
            acc = (b > a && b < r) ? __builtin_fma(l, x, acc) : acc;
          }
          col[a * ld] = (col[a * ld] - acc) / Wk.Ld[a];
        }
      }
    } else {
      if (tid < 13) {  // L y = X[:, tid], L' x = y, in place
        for (int a = 0; a < r; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int b = 0; b < U; ++b) {
            const double l = Wk.G[a * U + b], x = Wk.X[b * 13 + tid];
            acc = (b < a) ? __builtin_fma(l, x, acc) : acc;
          }
          Wk.X[a * 13 + tid] = (Wk.X[a * 13 + tid] - acc) / Wk.Ld[a];
        }
        for (int a = r - 1; a >= 0; --a) {
          double acc = 0.0;
#pragma unroll
          for (int b = 0; b < U; ++b) {
            const double l = Wk.G[b * U + a], x = Wk.X[b * 13 + tid];
            acc = (b > a && b < r) ? __builtin_fma(l, x, acc) : acc;
          }
          Wk.X[a * 13 + tid] = (Wk.X[a * 13 + tid] - acc) / Wk.Ld[a];
        }
      }
    }
    if (tid == 64)  // (a lane of the other wave: off the solves' path)
      for (int j = 0; j < r; ++j) {
        const double p = Wk.piv[j], v = (p == p) ? p : 0.0;
        pivmin = (v < pivmin) ? v : pivmin;
      }
    __syncthreads();
    for (int t = tid; t < 13 * U + (VEC ? U : 0); t += NT) {  // S = Z X;  (VEC) k_i = 0 - Z y
      const bool kvec = VEC && t >= 13 * U;
      const int c = kvec ? t - 13 * U : t / 13, s = t % 13;
      const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3, k = (c < 3 * NC) ? c % 3 : 3 + (c - 3 * NC) % 3;
      const int hc = (cc == 2) ? hl2 : ((cc == 1) ? hl1 : hl0), oc = (cc == 2) ? o2 : ((cc == 1) ? o1 : 0);
      const double *zrow = Kp.Z + 36 * (NC * i + cc) + 6 * hc + k;
      double acc = 0.0;
      if (kvec) {
        if constexpr (VEC) {
          for (int b = 0; b < 6 - hc; ++b) acc = __builtin_fma(zrow[6 * b], Wk.y[oc + b], acc);
          vec.k[c] = 0.0 - acc;
        }
        continue;
      }
      for (int b = 0; b < 6 - hc; ++b) acc = __builtin_fma(zrow[6 * b], Wk.X[(oc + b) * 13 + s], acc);
      Wk.S[t] = acc;
    }
    __syncthreads();
    for (int t = tid; t < 13 * U; t += NT) {  // K = 0 - S PA
      const int c = t / 13, s = t % 13;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(Wk.S[c * 13 + k], Wk.PA[k * 13 + s], acc);
      K[t] = 0.0 - acc;
    }
  } else {
    for (int t = tid; t < 13 * U; t += NT) Wk.S[t] = 0.0, K[t] = 0.0;
    if constexpr (VEC)
      if (tid < U) vec.k[tid] = 0.0;
  }
}

// The rest of step i behind riccati_gain_step and a barrier: M_i = A + B K_i into M[13][13], then (with_P) P_i = Q + PA' M_i into Wk.P,
// evaluated on the upper triangle and copied to the lower; (VEC) p_i beside it.  Ends with a barrier.
template <int NC, int HMAX, int NT, bool VEC, class Work>
__device__ __forceinline__ void riccati_cost_step(FeedbackKeep<NC, HMAX> &Kp, Work &Wk, const double *K, double *M, const bool with_P,
                                                  const RiccatiVec vec) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  const double *A = Kp.A, *B = Kp.B;
  for (int t = tid; t < 169; t += NT) {  // M_i = A + B K_i
    const int k = t / 13, s = t % 13;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < U; ++c) acc = __builtin_fma(B[k * U + c], K[c * 13 + s], acc);
    M[t] = A[t] + acc;
  }
  __syncthreads();
  for (int t = tid; t < 169 + (VEC ? 13 : 0); t += NT) {  // P_i = Q + PA' M_i, upper triangle, copied;  (VEC) p_i = M_i' p + K_i' l_i
    if constexpr (VEC) {
      if (t >= 169) {
        const int s = t - 169;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(M[k * 13 + s], vec.p[k], acc);
#pragma unroll
        for (int c = 0; c < U; ++c) acc = __builtin_fma(K[c * 13 + s], vec.ell[c], acc);
        vec.p_next[s] = acc;
        continue;
      }
      if (!with_P) continue;  // (P_0 is not needed)
    }
    const int s = t / 13, tt = t % 13;
    if (s > tt) continue;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 13; ++k) acc = __builtin_fma(Wk.PA[k * 13 + s], M[k * 13 + tt], acc);
    const double v = (s == tt) ? Kp.q2[s] + acc : acc;
    Wk.P[s * 13 + tt] = v, Wk.P[tt * 13 + s] = v;
  }
  __syncthreads();
}

// The gains of one instance, by the NT lanes of its workgroup.  In (LDS or any memory all lanes see): Acd[13][13], Bcd[13][6 NC], W[12],
// alpha[6 NC], Fc[8 NC][6 NC], u[h][6 NC], gait[NC h] bytes, cap[NC].  Out: gain_out[6 NC][13], ref_out[h][6 NC][12], free_out[h],
// summary_out[2].  Every lane of the workgroup calls it.  Wk may overlay the binary32 inputs (see FeedbackWork).
template <int NC, int HMAX, int NT>
__device__ __forceinline__ void feedback_of_instance(const float *Acd, const float *Bcd, const float *W, const float *alpha, const float *Fc,
                                                     const float *u, const unsigned char *gait, const float *cap, const int h,
                                                     const double act_tol, FeedbackKeep<NC, HMAX> &Kp, FeedbackWork<NC, HMAX> &Wk,
                                                     double *gain_out, double *ref_out, int32_t *free_out, double *summary_out) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  // ---- first phase: what the passes need of the inputs, in binary64; slacks; free directions
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < U) Kp.r2[tid] = (double)alpha[tid] + (double)alpha[tid];
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, Kp.slack, Kp.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  for (int ls = tid; ls < NC * h; ls += NT)
    Kp.held[ls] = stance(cap[ls % NC], gait[ls]) ? (unsigned char)free_directions<NC>(Fc, ls % NC, Kp.slack + 10 * ls, act_tol, Kp.Z + 36 * ls)
                                                 : (unsigned char)6;
  __syncthreads();  // the binary32 inputs are not read below
  if (free_out && tid < h) {
    int r = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) r += 6 - (int)Kp.held[NC * tid + c];
    free_out[tid] = r;
  }
  // ---- backward pass
  const double *A = Kp.A, *B = Kp.B;
  double pivmin = 1.0;  // (lane 64's is the one that counts)
  for (int t = tid; t < 169; t += NT) Wk.P[t] = (t % 14 == 0) ? Kp.q2[t / 13] : 0.0;
  __syncthreads();
  for (int i = h - 1; i >= 0; --i) {
    riccati_gain_step<NC, HMAX, NT, false>(Kp, Wk, i, Wk.K, pivmin, RiccatiVec{});
    __syncthreads();
    if (i > 0) {
      double *M = Wk.M + 169 * (i - 1);
      riccati_cost_step<NC, HMAX, NT, false>(Kp, Wk, Wk.K, M, true, RiccatiVec{});
    }
  }
  // ---- K_0, S_0: the gain, its maximum, and the forward chain of Psi
  double kmax = 0.0;
  for (int t = tid; t < 13 * U; t += NT) {
    const double kv = Wk.K[t], a = __builtin_fabs(kv), v = (a == a) ? a : margins_inf();
    if (gain_out) gain_out[t] = kv;
    kmax = (v > kmax) ? v : kmax;
    Wk.Psi[0][t] = Wk.S[t];
  }
  Wk.red[tid] = kmax;
  if (tid == 64) Wk.piv[0] = pivmin;
  __syncthreads();
  if (tid == 0 && summary_out) {
    double best = 0.0;
    for (int t = 0; t < NT; ++t) best = (Wk.red[t] > best) ? Wk.red[t] : best;
    summary_out[0] = Wk.piv[0], summary_out[1] = best;
  }
  int cur = 0;
  for (int j = 1; j <= h; ++j) {
    const double *Psi = Wk.Psi[cur];
    if (ref_out)
      for (int t = tid; t < 12 * U; t += NT) ref_out[(size_t)(j - 1) * 12 * U + t] = Psi[(t / 12) * 13 + t % 12] * Kp.q2[t % 12];
    if (j < h) {
      const double *M = Wk.M + 169 * (j - 1);
      double *nxt = Wk.Psi[cur ^ 1];
      for (int t = tid; t < 13 * U; t += NT) {
        const int c = t / 13, s = t % 13;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(Psi[c * 13 + k], M[s * 13 + k], acc);
        nxt[t] = acc;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// scratch of first_order_of_instance
template <int NC>
struct FirstOrderScratch {
  float wrench[6 * NC];
  double slack[10 * NC];
  MarginMin wave_min[FB_NT / 64][MARGIN_CLASSES];
};

// The first-order wrench of one instance, by the NT lanes of its workgroup: wrench[c] = (float)((double)u0[c] + chain_c), chain_c the
// ascending fma chain from +0 over gain[c][s] dx[s] (s < 13), then ref_gain[j][c][s] dt[12 j + s] (j < h, s < 12); worst = the least of
// the ten step-0 slacks of every stance contact at that wrench (+inf with none; a NaN slack never enters).  gain, ref_gain: any memory;
// dx[13], dt[12 h], u0[6 NC], Fc, gait (step 0), cap: LDS.
template <int NC, int NT>
__device__ __forceinline__ void first_order_of_instance(const double *gain, const double *ref_gain, const double *dx, const double *dt,
                                                        const float *u0, const float *Fc, const unsigned char *gait, const float *cap,
                                                        const int h, FirstOrderScratch<NC> &T, float *wrench_out, double *worst_out) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x;
  if (tid < U) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 13; ++s) acc = __builtin_fma(gain[tid * 13 + s], dx[s], acc);
    for (int j = 0; j < h; ++j) {
      const double *g = ref_gain + ((size_t)j * U + tid) * 12;
#pragma unroll
      for (int s = 0; s < 12; ++s) acc = __builtin_fma(g[s], dt[12 * j + s], acc);
    }
    T.wrench[tid] = (float)((double)u0[tid] + acc);
  }
  margins_of_instance<NC, NT>(Fc, T.wrench, gait, cap, 1, T.slack, T.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  if (wrench_out && tid < U) wrench_out[tid] = T.wrench[tid];
  if (worst_out && tid == 0) {
    double worst = margins_inf();
    for (int c = 0; c < NC; ++c)
      if (stance(cap[c], gait[c]))
        for (int j = 0; j < 10; ++j) worst = (T.slack[10 * c + j] < worst) ? T.slack[10 * c + j] : worst;
    *worst_out = worst;
  }
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
struct FeedbackOut {
  double *gain, *ref_gain, *summary;  // [batch][6 nc][13], [batch][h][6 nc][12], [batch][2]
  int32_t *free_dims;                 // [batch][h]
};
// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants, mu_inst) and `forces`; it writes `out` and nothing else.  Shapes: derived_shape (hmpc_derived_shape.h); anything else:
// hipErrorInvalidValue, nothing launched.
hipError_t launch_feedback(int nc, const KernelArgs &args, double act_tol, const FeedbackOut &out, hipStream_t stream);
// One launch over the batch: wrench[batch][6 nc], worst_slack[batch] from the gains in `gains`, the records of `args` (the solved ones),
// records_new (same stride) and step 0 of args.forces.  Same shapes as launch_feedback.
hipError_t launch_first_order(int nc, const KernelArgs &args, const unsigned char *records_new, const FeedbackOut &gains, float *wrench,
                              double *worst_slack, hipStream_t stream);
}  // namespace hmpc
#endif
