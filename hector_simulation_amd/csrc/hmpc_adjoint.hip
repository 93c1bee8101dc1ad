// hmpc_adjoint.hip -- the adjoint of the solve (hmpc_solve_adjoint): from a seed l = dL/du over the whole force
// trajectory, the gradients of L in the state, the reference trajectory, the weights and Alpha_K of the QP that was solved, with its
// linearisation and the active set at the forces in the force buffer frozen.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the gains' kernel it assembles by
// CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the smallest Smem
// that serves (NC, HMAX) -- so that x0, Acd, Bcd, the weights, the trajectory, Alpha_K and the constraint block Fc are the very binary32
// values the solve used, hmpc_params and the per-instance mu included.  Everything behind the assembly (the arithmetic is fixed there) is
// adjoint_of_instance of hmpc_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The scratch of the two
// passes overlays the assembly's Smem, which is dead once the first phase has widened what the passes read; K_i and k_i of every step
// stay in LDS for the forward pass (25 KB at (20, 2)), nothing goes to HBM scratch.
// Traffic: the record, 6 NC h floats and 6 NC h doubles in (coalesced bursts); 13 + 12 h + 12 + 6 NC + 6 NC h + 2 doubles out.  No atomics,
// no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_adjoint.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_feedback.hip)
template <int HMAX, int NC>
using AdjSmem = Smem<12, HMAX, FB_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct AdjLds {
  union {
    AdjSmem<HMAX, NC> S;       // the assembly, and the first phase of adjoint_of_instance
    AdjointWork<NC, HMAX> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  AdjointKeep<NC, HMAX> Ak;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(FB_NT) void hmpc_adjoint_kernel(KernelArgs args, double act_tol, const double *seed, AdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = FB_NT;
  __shared__ AdjLds<HMAX, NC> L;
  static_assert(sizeof(AdjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec)) return;  // uniform
  {
    // stage A0 as hmpc_kernel has it: the record, one coalesced burst into LDS (restated as in hmpc_predict.hip, for the reason given there)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(args.records + (size_t)inst * (size_t)args.stride);
    const int nwords = args.stride >> 2;
    for (int t = tid; t < nwords; t += NT) S.u.a.rec[t] = src[t];
  }
  for (int t = tid; t < U * h; t += NT) L.u[t] = args.forces[(size_t)inst * U * h + t];
  __syncthreads();
  Prof prof;
  stage_a_scalars<12, HMAX, NT, 1, NC, 1>(S, args, inst, h, prof);  // (ends with a barrier)
  const auto &A = S.u.a;
  const float *rf = reinterpret_cast<const float *>(A.rec);
  const unsigned char *gait = reinterpret_cast<const unsigned char *>(A.rec + RL::NF + 12 * h);
  if (tid < NC) L.cap[tid] = (NC == 3 && tid == 2) ? rf[RL::FMH] : args.f_max;
  const size_t i = (size_t)inst;
  adjoint_of_instance<NC, HMAX, NT>(A.x0, A.Acd, A.Bcd, A.W, rf + RL::NF, rf + RL::AL, A.Fc, L.u, gait, L.cap, seed + i * h * U, h, act_tol,
                                    L.Kp, L.Ak, L.o.Wk, out.grad_x0 + i * 13, out.grad_traj + i * h * 12, out.grad_weights + i * 12,
                                    out.grad_alpha + i * U, out.dir + i * h * U, out.summary + i * ADJ_SUMMARY);
}

}  // namespace

hipError_t launch_adjoint(int nc, const KernelArgs &args, double act_tol, const double *seed, const AdjointOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !seed || !out.grad_x0 || !out.grad_traj || !out.grad_weights || !out.grad_alpha || !out.dir ||
      !out.summary || !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(FB_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_adjoint_kernel<10, 2>), grid, block, 0, stream, args, act_tol, seed, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_adjoint_kernel<20, 2>), grid, block, 0, stream, args, act_tol, seed, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_adjoint_kernel<10, 3>), grid, block, 0, stream, args, act_tol, seed, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hmpc
