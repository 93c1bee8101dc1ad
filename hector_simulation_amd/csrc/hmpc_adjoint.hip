// hmpc_adjoint.hip -- the adjoint of the solve (hmpc_solve_adjoint): from a seed l = dL/du over the whole force
// trajectory, the gradients of L in the state, the reference trajectory, the weights and Alpha_K of the QP that was solved, with its
// linearisation and the active set at the forces in the force buffer frozen.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the gains' kernel it assembles by
// CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that x0, Acd, Bcd, the weights, the trajectory,
// Alpha_K and the constraint block Fc are the very binary32 values the solve used, hmpc_params and the per-instance mu included.
// Everything behind the assembly (the arithmetic is fixed there) is adjoint_of_instance of hmpc_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  The scratch of the two
// passes overlays the assembly's Smem, which is dead once the first phase has widened what the passes read; K_i and k_i of every step
// stay in LDS for the forward pass (25 KB at (20, 2)), nothing goes to HBM scratch.
// Traffic: the record, 6 NC h floats and 6 NC h doubles in (coalesced bursts); 13 + 12 h + 12 + 6 NC + 6 NC h + 2 doubles out.  No atomics,
// no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_adjoint.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct AdjLds {
  union {
    DerivedSmem<HMAX, NC> S;   // the assembly, and the first phase of adjoint_of_instance
    AdjointWork<NC, HMAX> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  AdjointKeep<NC, HMAX> Ak;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_adjoint_kernel(KernelArgs args, double act_tol, const double *seed, AdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ AdjLds<HMAX, NC> L;
  static_assert(sizeof(AdjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
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
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_adjoint_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, seed, out);
  });
}

}  // namespace hmpc
