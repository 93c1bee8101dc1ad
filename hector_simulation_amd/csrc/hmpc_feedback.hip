// hmpc_feedback.hip -- the feedback gains of every instance (hmpc_feedback_gains): K_0 = du_0/dx_0 and
// du_0/dX_d of the QP that was solved, with its linearisation and the active set at the forces in the force buffer frozen; and the
// first-order wrench that applies them to a new record (hmpc_first_order_wrench).
//
// Launches of their own behind a solve (never part of hmpc_kernel, not rows of hmpc_variants.h).  Like the certificate kernel they
// assemble by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that Acd, Bcd, the weights, Alpha_K
// and the constraint block Fc are the very binary32 values the solve used, hmpc_params and the per-instance mu included.  Everything
// behind the assembly (slacks, free directions, the Riccati recursion, the forward chain; the arithmetic is fixed there) is
// feedback_of_instance of hmpc_feedback.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The scratch of the two
// passes overlays the assembly's Smem, which is dead once the first phase has widened what the passes read: 59 KB of LDS at (20, 2),
// two workgroups per CU.
// Traffic: the record and 6 NC h floats in (coalesced bursts); 6 NC (13 + 12 h) + 2 doubles and h ints out, K_0 and every ref_gain row
// stored from LDS in coalesced passes.  No atomics, no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_feedback.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct FbLds {
  union {
    DerivedSmem<HMAX, NC> S;    // the assembly, and the first phase of feedback_of_instance
    FeedbackWork<NC, HMAX> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_feedback_kernel(KernelArgs args, double act_tol, FeedbackOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ FbLds<HMAX, NC> L;
  static_assert(sizeof(FbLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
  feedback_of_instance<NC, HMAX, NT>(A.Acd, A.Bcd, A.W, rf + RL::AL, A.Fc, L.u, gait, L.cap, h, act_tol, L.Kp, L.o.Wk,
                                     out.gain + (size_t)inst * U * 13, out.ref_gain + (size_t)inst * h * U * 12,
                                     out.free_dims + (size_t)inst * h, out.summary + (size_t)inst * FB_SUMMARY);
}

template <int HMAX, int NC>
struct FoLds {
  DerivedSmem<HMAX, NC> S;
  FirstOrderScratch<NC> T;
  float x0n[13], trajn[12 * HMAX];  // of the new record
  double dx[13], dt[12 * HMAX];
  float u0[6 * NC];
  float cap[4];
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_first_order_kernel(KernelArgs args, const unsigned char *records_new, FeedbackOut gains,
                                                                      float *wrench, double *worst_slack) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ FoLds<HMAX, NC> L;
  static_assert(sizeof(FoLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  // the new record: x0' through the same stage function, its trajectory as it stands (no force slot: only u_0 is read, below)
  if (!derived_front(S, nullptr, args, records_new)) return;  // uniform
  if (tid < 13) L.x0n[tid] = A.x0[tid];
  for (int t = tid; t < 12 * h; t += NT) L.trajn[t] = rf[RL::NF + t];
  __syncthreads();
  // the record that was solved: x0, its trajectory, the constraint block, the gait and the caps
  derived_load_record(S, args.records, args.stride);
  if (tid < U) L.u0[tid] = args.forces[(size_t)inst * U * h + tid];
  __syncthreads();
  derived_assemble(S, args);
  if (tid < 13) L.dx[tid] = (double)L.x0n[tid] - (double)A.x0[tid];
  for (int t = tid; t < 12 * h; t += NT) L.dt[t] = (double)L.trajn[t] - (double)rf[RL::NF + t];
  derived_fill_caps(S, args, L.cap);
  __syncthreads();
  first_order_of_instance<NC, NT>(gains.gain + (size_t)inst * U * 13, gains.ref_gain + (size_t)inst * h * U * 12, L.dx, L.dt, L.u0, A.Fc,
                                  derived_gait(S, h), L.cap, h, L.T, wrench + (size_t)inst * U, worst_slack + inst);
}

}  // namespace

hipError_t launch_feedback(int nc, const KernelArgs &args, double act_tol, const FeedbackOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !out.gain || !out.ref_gain || !out.summary || !out.free_dims || !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_feedback_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, out);
  });
}

hipError_t launch_first_order(int nc, const KernelArgs &args, const unsigned char *records_new, const FeedbackOut &gains, float *wrench,
                              double *worst_slack, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !gains.gain || !gains.ref_gain || !wrench || !worst_slack || !records_new || !args.forces ||
      !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_first_order_kernel<H(), C()>), grid, block, 0, stream, args, records_new, gains, wrench, worst_slack);
  });
}

}  // namespace hmpc
