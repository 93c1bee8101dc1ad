// hmpc_adjoint_multi.hip -- the adjoint of the solve under several seeds (hmpc_solve_adjoint_multi): from seeds
// l_s = dL_s/du over the whole force trajectory, the gradients of every L_s in the state, the reference trajectory, the weights and
// Alpha_K of the QP that was solved -- slice s bit for bit what hmpc_adjoint.hip returns under l_s alone -- with the assembly, the
// Gram-Schmidt phase and the matrix backward pass run once per tile of seeds.
//
// A launch of its own behind a solve, like hmpc_adjoint.hip: it assembles by CALLING the solve kernel's own stage function -- the common
// front of hmpc_derived.h.  Everything behind the assembly is adjoint_multi_of_instance of hmpc_adjoint_multi.h.
// Mapping: one workgroup of 128 threads per instance and tile; a tile is 6 NC seeds, so that a Jacobian of one step's wrench is one
// launch.  Static LDS below 64 KB: K_i of every step stays there, k_i of every seed is parked in the seed's slice of dir (HBM).
// Traffic per instance and tile of ns seeds: the record and 6 NC h floats in; 2 x 6 NC h ns doubles of seeds in (once for v, once for
// p_i); 6 NC h ns doubles of dir written twice and read once; 13 + 12 h + 12 + 6 NC + 2 doubles out per seed.  No atomics, no inline
// assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_adjoint_multi.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct AdjMultiLds {
  union {
    DerivedSmem<HMAX, NC> S;                                 // the assembly, and the first phase of adjoint_multi_of_instance
    AdjointMultiWork<NC, HMAX, adjoint_seed_tile<NC>()> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  AdjointMultiKeep<HMAX> Ak;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

// seeds s0 .. s0 + ns - 1 of the launch's n_seeds; seeds and out point at slice 0
template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_adjoint_multi_kernel(KernelArgs args, double act_tol, const double *seeds, int s0, int ns,
                                                                        AdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT, ST = adjoint_seed_tile<NC>();
  __shared__ AdjMultiLds<HMAX, NC> L;
  static_assert(sizeof(AdjMultiLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (ns < 1 || ns > ST) return;  // uniform
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
  const size_t i = (size_t)inst, nb = (size_t)args.batch, hz = (size_t)h, s = (size_t)s0;
  const AdjointMultiStride St = {nb * hz * U, nb * 13, nb * hz * 12, nb * 12, nb * U, nb * hz * U, nb * ADJ_SUMMARY};
  adjoint_multi_of_instance<NC, HMAX, NT, ST>(A.x0, A.Acd, A.Bcd, A.W, rf + RL::NF, rf + RL::AL, A.Fc, L.u, gait, L.cap,
                                              seeds + s * St.seed + i * hz * U, ns, St, h, act_tol, L.Kp, L.Ak, L.o.Wk,
                                              out.grad_x0 + s * St.x0 + i * 13, out.grad_traj + s * St.traj + i * hz * 12,
                                              out.grad_weights + s * St.weights + i * 12, out.grad_alpha + s * St.alpha + i * U,
                                              out.dir + s * St.dir + i * hz * U, out.summary + s * St.summary + i * ADJ_SUMMARY);
}

}  // namespace

hipError_t launch_adjoint_multi(int nc, const KernelArgs &args, double act_tol, const double *seeds, int n_seeds, const AdjointOut &out,
                                hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || n_seeds < 1 || !seeds || !out.grad_x0 || !out.grad_traj || !out.grad_weights || !out.grad_alpha ||
      !out.dir || !out.summary || !args.forces || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_seed_tiles(nc, args.horizon, n_seeds, [&](auto H, auto C, int s0, int ns) {
    hipLaunchKernelGGL((hmpc_adjoint_multi_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, seeds, s0, ns, out);
  });
}

}  // namespace hmpc
