// hmpc_feedback.hip -- the feedback gains of every instance (hmpc_feedback_gains): K_0 = du_0/dx_0 and
// du_0/dX_d of the QP that was solved, with its linearisation and the active set at the forces in the force buffer frozen; and the
// first-order wrench that applies them to a new record (hmpc_first_order_wrench).
//
// Launches of their own behind a solve (never part of hmpc_kernel, not rows of hmpc_variants.h).  Like the certificate kernel they
// assemble by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the
// smallest Smem that serves (NC, HMAX) -- so that Acd, Bcd, the weights, Alpha_K and the constraint block Fc are the very binary32 values
// the solve used, hmpc_params and the per-instance mu included.  Everything behind the assembly (slacks, free directions, the Riccati
// recursion, the forward chain; the arithmetic is fixed there) is feedback_of_instance of hmpc_feedback.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The scratch of the two
// passes overlays the assembly's Smem, which is dead once the first phase has widened what the passes read: 59 KB of LDS at (20, 2),
// two workgroups per CU.
// Traffic: the record and 6 NC h floats in (coalesced bursts); 6 NC (13 + 12 h) + 2 doubles and h ints out, K_0 and every ref_gain row
// stored from LDS in coalesced passes.  No atomics, no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_feedback.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_certificate.hip: 12 reduced variables, a working set of one row)
template <int HMAX, int NC>
using FbSmem = Smem<12, HMAX, FB_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct FbLds {
  union {
    FbSmem<HMAX, NC> S;         // the assembly, and the first phase of feedback_of_instance
    FeedbackWork<NC, HMAX> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

// stage A0 as hmpc_kernel has it: the record, one coalesced burst into LDS (restated as in hmpc_predict.hip, for the reason given there)
template <int NT>
__device__ __forceinline__ void load_record(uint32_t *dst, const unsigned char *records, const size_t inst, const int stride) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(records + inst * (size_t)stride);
  const int nwords = stride >> 2;
  for (int t = threadIdx.x; t < nwords; t += NT) dst[t] = src[t];
}

template <int HMAX, int NC>
__global__ __launch_bounds__(FB_NT) void hmpc_feedback_kernel(KernelArgs args, double act_tol, FeedbackOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = FB_NT;
  __shared__ FbLds<HMAX, NC> L;
  auto &S = L.o.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec)) return;  // uniform
  load_record<NT>(S.u.a.rec, args.records, (size_t)inst, args.stride);
  for (int t = tid; t < U * h; t += NT) L.u[t] = args.forces[(size_t)inst * U * h + t];
  __syncthreads();
  Prof prof;
  stage_a_scalars<12, HMAX, NT, 1, NC, 1>(S, args, inst, h, prof);  // (ends with a barrier)
  const auto &A = S.u.a;
  const float *rf = reinterpret_cast<const float *>(A.rec);
  const unsigned char *gait = reinterpret_cast<const unsigned char *>(A.rec + RL::NF + 12 * h);
  if (tid < NC) L.cap[tid] = (NC == 3 && tid == 2) ? rf[RL::FMH] : args.f_max;
  feedback_of_instance<NC, HMAX, NT>(A.Acd, A.Bcd, A.W, rf + RL::AL, A.Fc, L.u, gait, L.cap, h, act_tol, L.Kp, L.o.Wk,
                                     out.gain + (size_t)inst * U * 13, out.ref_gain + (size_t)inst * h * U * 12,
                                     out.free_dims + (size_t)inst * h, out.summary + (size_t)inst * FB_SUMMARY);
}

template <int HMAX, int NC>
struct FoLds {
  FbSmem<HMAX, NC> S;
  FirstOrderScratch<NC> T;
  float x0n[13], trajn[12 * HMAX];  // of the new record
  double dx[13], dt[12 * HMAX];
  float u0[6 * NC];
  float cap[4];
};

template <int HMAX, int NC>
__global__ __launch_bounds__(FB_NT) void hmpc_first_order_kernel(KernelArgs args, const unsigned char *records_new, FeedbackOut gains,
                                                                 float *wrench, double *worst_slack) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = FB_NT;
  __shared__ FoLds<HMAX, NC> L;
  auto &S = L.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = reinterpret_cast<const float *>(A.rec);
  Prof prof;
  // the new record: x0' through the same stage function, its trajectory as it stands
  load_record<NT>(S.u.a.rec, records_new, (size_t)inst, args.stride);
  __syncthreads();
  stage_a_scalars<12, HMAX, NT, 1, NC, 1>(S, args, inst, h, prof);  // (ends with a barrier)
  if (tid < 13) L.x0n[tid] = A.x0[tid];
  for (int t = tid; t < 12 * h; t += NT) L.trajn[t] = rf[RL::NF + t];
  __syncthreads();
  // the record that was solved: x0, its trajectory, the constraint block, the gait and the caps
  load_record<NT>(S.u.a.rec, args.records, (size_t)inst, args.stride);
  if (tid < U) L.u0[tid] = args.forces[(size_t)inst * U * h + tid];
  __syncthreads();
  stage_a_scalars<12, HMAX, NT, 1, NC, 1>(S, args, inst, h, prof);
  if (tid < 13) L.dx[tid] = (double)L.x0n[tid] - (double)A.x0[tid];
  for (int t = tid; t < 12 * h; t += NT) L.dt[t] = (double)L.trajn[t] - (double)rf[RL::NF + t];
  if (tid < NC) L.cap[tid] = (NC == 3 && tid == 2) ? rf[RL::FMH] : args.f_max;
  __syncthreads();
  const unsigned char *gait = reinterpret_cast<const unsigned char *>(A.rec + RL::NF + 12 * h);
  first_order_of_instance<NC, NT>(gains.gain + (size_t)inst * U * 13, gains.ref_gain + (size_t)inst * h * U * 12, L.dx, L.dt, L.u0, A.Fc, gait,
                                  L.cap, h, L.T, wrench + (size_t)inst * U, worst_slack + inst);
}

}  // namespace

hipError_t launch_feedback(int nc, const KernelArgs &args, double act_tol, const FeedbackOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !out.gain || !out.ref_gain || !out.summary || !out.free_dims || !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(FB_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_feedback_kernel<10, 2>), grid, block, 0, stream, args, act_tol, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_feedback_kernel<20, 2>), grid, block, 0, stream, args, act_tol, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_feedback_kernel<10, 3>), grid, block, 0, stream, args, act_tol, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_first_order(int nc, const KernelArgs &args, const unsigned char *records_new, const FeedbackOut &gains, float *wrench,
                              double *worst_slack, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !gains.gain || !gains.ref_gain || !wrench || !worst_slack || !records_new || !args.forces ||
      !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(FB_NT);
  if (nc == 2 && args.horizon <= 10)
    hipLaunchKernelGGL((hmpc_first_order_kernel<10, 2>), grid, block, 0, stream, args, records_new, gains, wrench, worst_slack);
  else if (nc == 2 && args.horizon <= 20)
    hipLaunchKernelGGL((hmpc_first_order_kernel<20, 2>), grid, block, 0, stream, args, records_new, gains, wrench, worst_slack);
  else if (nc == 3 && args.horizon <= 10)
    hipLaunchKernelGGL((hmpc_first_order_kernel<10, 3>), grid, block, 0, stream, args, records_new, gains, wrench, worst_slack);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hmpc
