// hmpc_adjoint_multi.h -- the adjoint of the solve under several seeds at once (hmpc_solve_adjoint_multi): one
// matrix backward pass, and next to it the vector recursion and the forward pass of up to ST seeds; everything BEHIND the assembly, as
// device functions over plain LDS arrays.  The kernels that assemble (hmpc_adjoint_multi.hip) call adjoint_multi_of_instance with what the
// solve kernel's own stage function left in LDS; tests/src/adjoint_multi_on_host.cpp compiles this header for the CPU (one thread per
// lane) against adjoint_of_instance under each seed alone.
//
// Definition: by reference.  Seed s of a tile is, chain for chain, hmpc_adjoint.h's definition under that seed alone -- the same slacks,
// stance rule, active set, Z_i and matrix backward pass (riccati_gain_step / riccati_cost_step of hmpc_feedback.h, the gains' own
// instantiation, run ONCE per step), the same ascending fma chains from +0 for v, y, the two triangular solves, k_i, p_i, du_i, dx_i, x_i
// and the six outputs -- so every output of seed s is bit for bit what adjoint_of_instance returns under it.  The matrix pass does not
// read a seed, so summary[0] is the same for every seed of a launch.
// Mapping: one output entry per lane and pass.  Per step of the backward pass: v of every seed (ns U entries) in a pass of its own in
// front of the matrix step, y = Z'v (ns r entries) behind it with no barrier between it and the matrix step's first pass (they share no
// array); the ns pairs of triangular solves one per lane on the second wave, beside the matrix step's last pass K = -S PA (which reads
// neither G nor y) and in front of the barrier the step already has; k_i and p_i of every seed in one pass behind the cost step.  Two
// barriers per step more than the matrix pass alone.  The forward pass gives one lane to every (seed, row); x_j is shared by all seeds.
// Memory: K_i of every step stays in LDS; k_i of every seed is parked in the seed's own slice of dir in HBM -- written and read back by
// the same lane, du_i overwrites it -- and the seeds are read where step i needs them, never staged: see the count in DESIGN.md.  dx keeps
// two steps; the sums over steps (grad_weights, grad_alpha, max |dir|) are carried step by step by the lane that owns the entry.
// No atomics, no inline assembly.
#pragma once
#include "hmpc_adjoint.h"

namespace hmpc {

// seeds of one launch: one launch serves S <= U seeds
template <int NC>
constexpr int adjoint_seed_tile() {
  return 6 * NC;
}

// what adjoint_multi_of_instance keeps from its first phase beside FeedbackKeep
template <int HMAX>
struct AdjointMultiKeep {
  float traj[12 * HMAX], x0[16];
};

// scratch of the backward and the forward pass; may overlay the binary32 inputs, which are not read again once the first phase has ended
template <int NC, int HMAX, int ST>
struct AdjointMultiWork {
  static constexpr int U = 6 * NC;
  double K[HMAX * U * 13];  // K_0 .. K_{h-1}
  union {
    struct {
      double P[169], PA[169], M[169], PB[13 * U];
      double W[U * U], WZ[U * U], G[U * U], Ld[U], piv[U];
      double X[U * 13], S[U * 13];
      double v[ST * U], y[ST * U], p[2][ST * 13];  // per seed
    } b;  // the backward pass
    struct {
      double x[(HMAX + 1) * 13], dx[2][ST * 13], du[ST * U];
      double gw[ST * 12], ga[ST * U], dmax[ST * U], pivmin;
    } f;  // the forward pass
  } o;
};

// distance in doubles between the slices of two consecutive seeds, per array (seed-major layouts over the current batch)
struct AdjointMultiStride {
  size_t seed, x0, traj, weights, alpha, dir, summary;
};

// The adjoints of one instance under seeds 0 .. ns-1 of a tile (1 <= ns <= ST), by the NT lanes of its workgroup.  In: as
// adjoint_of_instance; seed, gx0 .. summary_out point at the instance's rows in the tile's first slice (any memory), St at the next
// slices.  dir must be writable memory that the writing lane reads back (k_i is parked there).  Every lane of the workgroup calls it.
template <int NC, int HMAX, int NT, int ST>
__device__ __forceinline__ void adjoint_multi_of_instance(const float *x0, const float *Acd, const float *Bcd, const float *W, const float *traj,
                                                          const float *alpha, const float *Fc, const float *u, const unsigned char *gait,
                                                          const float *cap, const double *seed, const int ns, const AdjointMultiStride St,
                                                          const int h, const double act_tol, FeedbackKeep<NC, HMAX> &Kp,
                                                          AdjointMultiKeep<HMAX> &Ak, AdjointMultiWork<NC, HMAX, ST> &Wk, double *gx0,
                                                          double *gtraj, double *gw, double *galpha, double *dir, double *summary_out) {
  constexpr int U = 6 * NC;
  static_assert(NT >= 64 + ST, "one lane of the second wave per seed for the triangular solves");
  const int tid = threadIdx.x;
  // ---- first phase: as adjoint_of_instance, without the seed
  for (int t = tid; t < 169; t += NT) Kp.A[t] = (double)Acd[t];
  for (int t = tid; t < 13 * U; t += NT) Kp.B[t] = (double)Bcd[t];
  if (tid < 13) Kp.q2[tid] = (tid < 12) ? (double)W[tid] + (double)W[tid] : 0.0;
  if (tid < U) Kp.r2[tid] = (double)alpha[tid] + (double)alpha[tid];
  if (tid < 13) Ak.x0[tid] = x0[tid];
  for (int t = tid; t < 12 * h; t += NT) Ak.traj[t] = traj[t];
  margins_of_instance<NC, NT>(Fc, u, gait, cap, h, Kp.slack, Kp.wave_min, nullptr, nullptr, nullptr);  // (begins and ends with a barrier)
  for (int ls = tid; ls < NC * h; ls += NT)
    Kp.held[ls] = stance(cap[ls % NC], gait[ls]) ? (unsigned char)free_directions<NC>(Fc, ls % NC, Kp.slack + 10 * ls, act_tol, Kp.Z + 36 * ls)
                                                 : (unsigned char)6;
  __syncthreads();  // the binary32 inputs but u are not read below
  // ---- backward pass
  const double *A = Kp.A, *B = Kp.B;
  auto &Bk = Wk.o.b;
  double pivmin = 1.0;  // (lane 64's is the one that counts)
  for (int t = tid; t < 169; t += NT) Bk.P[t] = (t % 14 == 0) ? Kp.q2[t / 13] : 0.0;
  for (int t = tid; t < ns * 13; t += NT) Bk.p[0][t] = 0.0;
  __syncthreads();
  int cur = 0;
  for (int i = h - 1; i >= 0; --i) {
    double *Ki = Wk.K + 13 * U * i;
    const double *p = Bk.p[cur];
    double *pn = Bk.p[cur ^ 1];
    const int hl0 = (int)Kp.held[NC * i], hl1 = (int)Kp.held[NC * i + 1], hl2 = (NC == 3) ? (int)Kp.held[NC * i + NC - 1] : 6;
    const int o1 = 6 - hl0, o2 = o1 + 6 - hl1, r = o2 + 6 - hl2;
    const double *Zi = Kp.Z + 36 * NC * i;
    for (int t = tid; t < ns * U; t += NT) {  // v = l_i + B' p
      const int sd = t / U, c = t % U;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(B[k * U + c], p[sd * 13 + k], acc);
      Bk.v[t] = seed[sd * St.seed + U * i + c] + acc;
    }
    __syncthreads();
    for (int t = tid; t < ns * r; t += NT) {  // y = Z' v
      const int sd = t / r, a = t % r;
      int ca;
      const double *za = fb_zcol(Zi, hl0, hl1, hl2, o1, o2, a, ca);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = __builtin_fma(za[k], Bk.v[sd * U + fb_col<NC>(ca, k)], acc);
      Bk.y[sd * U + a] = acc;
    }
    riccati_gain_step<NC, HMAX, NT, false>(Kp, Bk, i, Ki, pivmin, RiccatiVec{});  // (its barriers stand between y and the solves)
    if (r > 0 && tid >= 64 && tid < 64 + ns) {  // L y' = y, L' y'' = y', with the chains of X; beside K = -S PA
      double *col = Bk.y + (tid - 64) * U;
      for (int a = 0; a < r; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < U; ++b) {
          const double l = Bk.G[a * U + b], x = col[b];
          acc = (b < a) ? __builtin_fma(l, x, acc) : acc;
        }
        col[a] = (col[a] - acc) / Bk.Ld[a];
      }
      for (int a = r - 1; a >= 0; --a) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < U; ++b) {
          const double l = Bk.G[b * U + a], x = col[b];
          acc = (b > a && b < r) ? __builtin_fma(l, x, acc) : acc;
        }
        col[a] = (col[a] - acc) / Bk.Ld[a];
      }
    }
    __syncthreads();
    riccati_cost_step<NC, HMAX, NT, false>(Kp, Bk, Ki, Bk.M, true, RiccatiVec{});  // (M_0 as well; ends with a barrier)
    for (int t = tid; t < ns * (U + 13); t += NT) {  // k_i = 0 - Z y'' into dir;  p_i = M_i' p + K_i' l_i
      if (t < ns * U) {
        const int sd = t / U, c = t % U;
        const int cc = (c < 3 * NC) ? c / 3 : (c - 3 * NC) / 3, k = (c < 3 * NC) ? c % 3 : 3 + (c - 3 * NC) % 3;
        const int hc = (cc == 2) ? hl2 : ((cc == 1) ? hl1 : hl0), oc = (cc == 2) ? o2 : ((cc == 1) ? o1 : 0);
        const double *zrow = Kp.Z + 36 * (NC * i + cc) + 6 * hc + k;
        double acc = 0.0;
        if (r > 0)
          for (int b = 0; b < 6 - hc; ++b) acc = __builtin_fma(zrow[6 * b], Bk.y[sd * U + oc + b], acc);
        dir[sd * St.dir + U * i + c] = (r > 0) ? 0.0 - acc : 0.0;
      } else {
        const int sd = (t - ns * U) / 13, s = (t - ns * U) % 13;
        const double *li = seed + sd * St.seed + U * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(Bk.M[k * 13 + s], p[sd * 13 + k], acc);
#pragma unroll
        for (int c = 0; c < U; ++c) acc = __builtin_fma(Ki[c * 13 + s], li[c], acc);
        pn[sd * 13 + s] = acc;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  if (gx0)
    for (int t = tid; t < ns * 13; t += NT) gx0[(t / 13) * St.x0 + t % 13] = Bk.p[cur][t];
  __syncthreads();  // the backward pass' matrices are dead: the forward pass' arrays take their place
  // ---- forward pass
  auto &Fw = Wk.o.f;
  if (tid < 13) Fw.x[tid] = (double)Ak.x0[tid];
  for (int t = tid; t < ns * 13; t += NT) Fw.dx[0][t] = 0.0;
  for (int t = tid; t < ns * 12; t += NT) Fw.gw[t] = 0.0;
  for (int t = tid; t < ns * U; t += NT) Fw.ga[t] = 0.0, Fw.dmax[t] = 0.0;
  if (tid == 64) Fw.pivmin = pivmin;
  __syncthreads();
  cur = 0;
  for (int i = 0; i < h; ++i) {
    const double *dxi = Fw.dx[cur], *xi = Fw.x + 13 * i;
    double *dxn = Fw.dx[cur ^ 1];
    for (int t = tid; t < ns * U + 13; t += NT) {
      if (t < ns * U) {  // du_i = K_i dx_i + k_i (the lane that parked k_i reads it back)
        const int sd = t / U, c = t % U;
        const double *Kr = Wk.K + 13 * U * i + 13 * c;
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < 13; ++s) acc = __builtin_fma(Kr[s], dxi[sd * 13 + s], acc);
        double *slot = dir + sd * St.dir + U * i + c;
        const double dv = acc + *slot, a = __builtin_fabs(dv), m = (a == a) ? a : margins_inf();
        const double uv = (double)u[U * i + c];
        *slot = dv, Fw.du[t] = dv;
        Fw.ga[t] = __builtin_fma(uv + uv, dv, Fw.ga[t]);
        Fw.dmax[t] = (m > Fw.dmax[t]) ? m : Fw.dmax[t];
      } else {  // x_{i+1}, as hmpc_predict_states has it
        const int s = t - ns * U;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[s * 13 + k], xi[k], acc);
#pragma unroll
        for (int c = 0; c < U; ++c) acc = __builtin_fma(B[s * U + c], (double)u[U * i + c], acc);
        Fw.x[13 * (i + 1) + s] = acc;
      }
    }
    __syncthreads();
    for (int t = tid; t < ns * 13; t += NT) {  // dx_{i+1} = A dx_i + B du_i, and what the outputs take of it
      const int sd = t / 13, s = t % 13;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = __builtin_fma(A[s * 13 + k], dxi[sd * 13 + k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = __builtin_fma(B[s * U + c], Fw.du[sd * U + c], acc);
      dxn[t] = acc;
      if (s < 12) {
        if (gtraj) gtraj[sd * St.traj + 12 * i + s] = 0.0 - Kp.q2[s] * acc;
        const double e = Fw.x[13 * (i + 1) + s] - (double)Ak.traj[12 * i + s];
        Fw.gw[sd * 12 + s] = __builtin_fma(e + e, acc, Fw.gw[sd * 12 + s]);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  // ---- outputs
  if (gw)
    for (int t = tid; t < ns * 12; t += NT) gw[(t / 12) * St.weights + t % 12] = Fw.gw[t];
  if (galpha)
    for (int t = tid; t < ns * U; t += NT) galpha[(t / U) * St.alpha + t % U] = Fw.ga[t];
  if (summary_out && tid < ns) {
    double best = 0.0;
    for (int c = 0; c < U; ++c) best = (Fw.dmax[tid * U + c] > best) ? Fw.dmax[tid * U + c] : best;
    summary_out[tid * St.summary] = Fw.pivmin, summary_out[tid * St.summary + 1] = best;
  }
}

}  // namespace hmpc

#if defined(__HIPCC__)
#include "hmpc_kernel_args.h"
namespace hmpc {
// ceil(n_seeds / tile) launches over the batch on `stream`, tile = adjoint_seed_tile<nc>().  Of `args` the kernels read what
// launch_adjoint's does; they read seeds[n_seeds][batch][h][6 nc] and write the n_seeds slices behind the pointers of `out`, each laid out
// as launch_adjoint's outputs over args.batch.  Same shapes as launch_adjoint; anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_adjoint_multi(int nc, const KernelArgs &args, double act_tol, const double *seeds, int n_seeds, const AdjointOut &out,
                                hipStream_t stream);
}  // namespace hmpc
#endif
