// hmpc_limit_adjoint.hip -- the limit gradients of the solve (hmpc_adjoint_limits): from the direction `dir` of the
// last adjoint and the seed it was made from, the gradients of its loss in the constraint block Fc and the bounds themselves and, through
// the assembly's rows, in mu, lt, lh and the Fz caps of the QP that was solved.
//
// A launch of its own behind hmpc_solve_adjoint (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the adjoint's kernel it
// assembles by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the
// smallest Smem that serves (NC, HMAX) -- so that x0, Acd, Bcd, the weights, Alpha_K and the constraint block Fc are the very binary32
// values the solve used, hmpc_params and the per-instance mu included.  Everything behind the assembly (the arithmetic is fixed there) is
// limit_adjoint_of_instance of hmpc_limit_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The passes' arrays and
// the staged outputs overlay the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic: the record, 6 NC h floats and 2 x 6 NC h doubles in (coalesced bursts); 3 + NC + 48 NC^2 + 30 NC h + 3 doubles out.  No atomics,
// no inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_limit_adjoint.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_adjoint.hip)
template <int HMAX, int NC>
using LadjSmem = Smem<12, HMAX, LADJ_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct LadjLds {
  union {
    LadjSmem<HMAX, NC> S;           // the assembly, and the first phase of limit_adjoint_of_instance
    LimitAdjointWork<NC, HMAX> Wk;  // the passes and the staged outputs
  } o;
  LimitAdjointKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(LADJ_NT) void hmpc_limit_adjoint_kernel(KernelArgs args, double act_tol, const double *dir, const double *seed,
                                                                     LimitAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = LADJ_NT;
  __shared__ LadjLds<HMAX, NC> L;
  static_assert(sizeof(LadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
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
  const size_t i = (size_t)inst, ls = (size_t)10 * NC * h;
  limit_adjoint_of_instance<NC, HMAX, NT>(A.x0, A.Acd, A.Bcd, A.W, rf + RL::NF, rf + RL::AL, A.Fc, L.u, gait, L.cap, dir + i * h * U,
                                          seed + i * h * U, h, act_tol, (double)args.lt, (double)args.lh, L.Kp, L.o.Wk,
                                          out.grad_limits + i * (3 + NC), out.grad_Fc + i * 8 * NC * U, out.grad_bound + i * ls,
                                          out.lambda + i * ls, out.nu + i * ls, out.summary + i * LADJ_SUMMARY);
}

}  // namespace

hipError_t launch_limit_adjoint(int nc, const KernelArgs &args, double act_tol, const double *dir, const double *seed, const LimitAdjointOut &out,
                                hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !dir || !seed || !out.grad_limits || !out.grad_Fc || !out.grad_bound || !out.lambda || !out.nu ||
      !out.summary || !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(LADJ_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_limit_adjoint_kernel<10, 2>), grid, block, 0, stream, args, act_tol, dir, seed, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_limit_adjoint_kernel<20, 2>), grid, block, 0, stream, args, act_tol, dir, seed, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_limit_adjoint_kernel<10, 3>), grid, block, 0, stream, args, act_tol, dir, seed, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hmpc
