// hmpc_model_adjoint.hip -- the model gradients of the solve (hmpc_adjoint_model): from the direction `dir` of the
// last adjoint, the gradients of its loss in Acd and Bcd themselves and, through stage A2's B, in the foot positions, the mass and the
// body inertia of the QP that was solved.
//
// A launch of its own behind hmpc_solve_adjoint (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the adjoint's kernel it
// assembles by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that x0, Acd, Bcd and the weights
// are the very binary32 values the solve used, hmpc_params and the per-instance mu included.  Everything behind the assembly (the
// arithmetic is fixed there) is model_adjoint_of_instance of hmpc_model_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  x, dx, both costates
// and G_A, G_B overlay the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic: the record, 6 NC h floats and 6 NC h doubles in (coalesced bursts); 169 + 13 U + 3 NC + 4 + 26 doubles out.  No atomics, no
// inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_model_adjoint.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct MadjLds {
  union {
    DerivedSmem<HMAX, NC> S;        // the assembly, and the first phase of model_adjoint_of_instance
    ModelAdjointWork<NC, HMAX> Wk;  // the passes
  } o;
  ModelAdjointKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float R[12];             // quat_to_R of the record's quaternion
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_model_adjoint_kernel(KernelArgs args, double mass, const double *dir, ModelAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ MadjLds<HMAX, NC> L;
  static_assert(sizeof(MadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  derived_fill_rotation(S, L.R);
  __syncthreads();
  const size_t i = (size_t)inst;
  model_adjoint_of_instance<NC, HMAX, NT>(A.x0, A.Acd, A.Bcd, A.W, rf + RL::NF, rf + RL::R, L.R, L.u, dir + i * h * U, h, (double)args.dt, mass,
                                          L.Kp, L.o.Wk, out.grad_A + i * 169, out.grad_B + i * 13 * U, out.grad_r + i * 3 * NC,
                                          out.grad_params + i * MADJ_PARAMS, out.costate + i * MADJ_COSTATE);
}

}  // namespace

hipError_t launch_model_adjoint(int nc, const KernelArgs &args, double mass, const double *dir, const ModelAdjointOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !dir || !out.grad_A || !out.grad_B || !out.grad_r || !out.grad_params || !out.costate ||
      !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_model_adjoint_kernel<H(), C()>), grid, block, 0, stream, args, mass, dir, out);
  });
}

}  // namespace hmpc
