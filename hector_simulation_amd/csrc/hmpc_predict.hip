// hmpc_predict.hip -- the predicted state trajectory and tracking cost of every instance (hmpc_predict_states).
//
// The solve kernel optimises over x_{i+1} = Acd x_i + Bcd u_i and leaves only the forces; this kernel rolls the same model out over
// whatever the force buffer holds.  It is a launch of its own (never part of hmpc_kernel, not a row of hmpc_variants.h) and it
// assembles by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that x0, Acd, Bcd, the weights
// and the trajectory are the very binary32 values the solve used, robot constants (hmpc_params) included.
//
// Arithmetic (fixed: tests/test_gpu_prediction.py restates it in numpy).  Per instance, U = 6 NC, state order rpy, position,
// angular velocity, velocity, gravity constant (SolverMPC.cpp:420):
//   x_0 = x0;  x_{i+1}[s] = sum_{k < 13} Acd[s][k] x_i[k] + sum_{c < U} Bcd[s][c] u_i[c]   for i = 0 .. h-1,
// in binary64, one ascending chain of explicit fma started at +0 (first the 13 state terms, then the U force terms), each step
// consuming the un-rounded binary64 x_i.  The chain is DENSE: the structural zeros of Acd / Bcd take part (a zero factor adds an
// exact +-0 to the chain, which leaves it as it is), so the arithmetic is the definition and not a property of the sparsity pattern.
//   states[inst][i][s] = (float) x_{i+1}[s]                                     (one rounding)
//   cost[inst][0] = sum_{s < 12} ( sum_i w_s (x_{i+1}[s] - X_d,i[s])^2 )        inner sum: acc = fma(w_s d, d, acc), i ascending;
//                                                                               outer: plain additions, s ascending
//   cost[inst][1] = sum_{c < U} ( sum_i alpha_c u_i[c]^2 )                      inner: acc = fma(alpha_c u, u, acc), i ascending;
//                                                                               outer: plain additions, c ascending
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves).  Lane s < 13 of wave 0 keeps row s
// of Acd and Bcd in registers and runs its chain; the 13 rows of a step run side by side, the h steps are dependent and exchange
// x_i through a double-buffered LDS array (one barrier per step).  Lanes 64 .. 64+U of wave 1 sum the force cost meanwhile.
// Traffic: the record and 6 NC h floats in (coalesced bursts), 13 h floats and 2 doubles out.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_predict.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct PredictLds {
  DerivedSmem<HMAX, NC> S;
  double x[2][16];            // x_i, un-rounded, ping-pong
  double part[16 + 6 * NC];   // per-state / per-component partial costs
  float u[6 * NC * HMAX];     // the instance's slot of the force buffer
  float out[13 * HMAX];       // states, rounded, staged for one coalesced store
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_predict_kernel(KernelArgs args, float *states, double *cost) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ PredictLds<HMAX, NC> L;
  static_assert(sizeof(PredictLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);

  if (tid >= 64 && tid < 64 + U) {  // force cost, one component per lane
    const int c = tid - 64;
    const double al = (double)rf[RL::AL + c];
    double acc = 0.0;
    for (int i = 0; i < h; ++i) {
      const double u = (double)L.u[U * i + c];
      acc = dfma(al * u, u, acc);
    }
    L.part[16 + c] = acc;
  }
  double arow[13], brow[U], w = 0.0, trk = 0.0;
  if (tid < 13) {
#pragma unroll
    for (int k = 0; k < 13; ++k) arow[k] = (double)A.Acd[tid * 13 + k];
#pragma unroll
    for (int c = 0; c < U; ++c) brow[c] = (double)A.Bcd[tid * U + c];
    w = (double)A.W[tid];
    L.x[0][tid] = (double)A.x0[tid];
  }
  __syncthreads();
  for (int i = 0; i < h; ++i) {
    if (tid < 13) {
      const double *x = L.x[i & 1];
      const float *u = L.u + U * i;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = dfma(arow[k], x[k], acc);
#pragma unroll
      for (int c = 0; c < U; ++c) acc = dfma(brow[c], (double)u[c], acc);
      L.x[(i + 1) & 1][tid] = acc;
      L.out[13 * i + tid] = (float)acc;
      if (tid < 12) {
        const double d = acc - (double)rf[RL::NF + 12 * i + tid];
        trk = dfma(w * d, d, trk);
      }
    }
    __syncthreads();
  }
  if (tid < 12) L.part[tid] = trk;
  __syncthreads();
  for (int t = tid; t < 13 * h; t += NT) states[(size_t)inst * 13 * h + t] = L.out[t];
  if (tid < 2) {  // lane 0: tracking cost, lane 1: force cost (adjacent doubles)
    const int lo = tid ? 16 : 0, n = tid ? U : 12;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += L.part[lo + k];
    cost[(size_t)inst * 2 + tid] = sum;
  }
}

}  // namespace

hipError_t launch_predict(int nc, const KernelArgs &args, float *states, double *cost, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !states || !cost || !args.forces || !args.records) return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_predict_kernel<H(), C()>), grid, block, 0, stream, args, states, cost);
  });
}

}  // namespace hmpc
