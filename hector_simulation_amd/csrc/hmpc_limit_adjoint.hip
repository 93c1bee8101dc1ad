// hmpc_limit_adjoint.hip -- the limit gradients of the solve (hmpc_adjoint_limits): from the direction `dir` of the
// last adjoint and the seed it was made from, the gradients of its loss in the constraint block Fc and the bounds themselves and, through
// the assembly's rows, in mu, lt, lh and the Fz caps of the QP that was solved.
//
// A launch of its own behind hmpc_solve_adjoint (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the adjoint's kernel it
// assembles by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that x0, Acd, Bcd, the weights,
// Alpha_K and the constraint block Fc are the very binary32 values the solve used, hmpc_params and the per-instance mu included.
// Everything behind the assembly (the arithmetic is fixed there) is limit_adjoint_of_instance of hmpc_limit_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The passes' arrays and
// the staged outputs overlay the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic: the record, 6 NC h floats and 2 x 6 NC h doubles in (coalesced bursts); 3 + NC + 48 NC^2 + 30 NC h + 3 doubles out.  No atomics,
// no inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_limit_adjoint.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct LadjLds {
  union {
    DerivedSmem<HMAX, NC> S;        // the assembly, and the first phase of limit_adjoint_of_instance
    LimitAdjointWork<NC, HMAX> Wk;  // the passes and the staged outputs
  } o;
  LimitAdjointKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_limit_adjoint_kernel(KernelArgs args, double act_tol, const double *dir, const double *seed,
                                                                     LimitAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ LadjLds<HMAX, NC> L;
  static_assert(sizeof(LadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
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
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_limit_adjoint_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, dir, seed, out);
  });
}

}  // namespace hmpc
