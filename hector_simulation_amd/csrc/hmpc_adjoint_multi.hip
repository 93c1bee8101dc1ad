// hmpc_adjoint_multi.hip -- the adjoint of the solve under several seeds (hmpc_solve_adjoint_multi): from seeds
// l_s = dL_s/du over the whole force trajectory, the gradients of every L_s in the state, the reference trajectory, the weights and
// Alpha_K of the QP that was solved -- slice s bit for bit what hmpc_adjoint.hip returns under l_s alone -- with the assembly, the
// Gram-Schmidt phase and the matrix backward pass run once per tile of seeds.
//
// A launch of its own behind a solve, like hmpc_adjoint.hip: it assembles by CALLING the solve kernel's own stage function,
// stage_a_scalars of hmpc_kernel.h, behind the record load of A0.  Everything behind the assembly is adjoint_multi_of_instance of
// hmpc_adjoint_multi.h.
// Mapping: one workgroup of 128 threads per instance and tile; a tile is 6 NC seeds, so that a Jacobian of one step's wrench is one
// launch.  Static LDS below 64 KB: K_i of every step stays there, k_i of every seed is parked in the seed's slice of dir (HBM).
// Traffic per instance and tile of ns seeds: the record and 6 NC h floats in; 2 x 6 NC h ns doubles of seeds in (once for v, once for
// p_i); 6 NC h ns doubles of dir written twice and read once; 13 + 12 h + 12 + 6 NC + 2 doubles out per seed.  No atomics, no inline
// assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_adjoint_multi.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_adjoint.hip)
template <int HMAX, int NC>
using AdjMultiSmem = Smem<12, HMAX, FB_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct AdjMultiLds {
  union {
    AdjMultiSmem<HMAX, NC> S;                                 // the assembly, and the first phase of adjoint_multi_of_instance
    AdjointMultiWork<NC, HMAX, adjoint_seed_tile<NC>()> Wk;  // the backward and the forward pass
  } o;
  FeedbackKeep<NC, HMAX> Kp;
  AdjointMultiKeep<HMAX> Ak;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

// seeds s0 .. s0 + ns - 1 of the launch's n_seeds; seeds and out point at slice 0
template <int HMAX, int NC>
__global__ __launch_bounds__(FB_NT) void hmpc_adjoint_multi_kernel(KernelArgs args, double act_tol, const double *seeds, int s0, int ns,
                                                                   AdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = FB_NT, ST = adjoint_seed_tile<NC>();
  __shared__ AdjMultiLds<HMAX, NC> L;
  static_assert(sizeof(AdjMultiLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec) || ns < 1 || ns > ST) return;  // uniform
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
  const int shape = (nc == 2 && args.horizon <= 10) ? 0 : (nc == 2 && args.horizon <= 20) ? 1 : (nc == 3 && args.horizon <= 10) ? 2 : -1;
  if (shape < 0) return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(FB_NT);
  const int tile = 6 * nc;
  for (int s0 = 0; s0 < n_seeds; s0 += tile) {
    const int ns = (n_seeds - s0 < tile) ? n_seeds - s0 : tile;
    if (shape == 0) hipLaunchKernelGGL((hmpc_adjoint_multi_kernel<10, 2>), grid, block, 0, stream, args, act_tol, seeds, s0, ns, out);
    else if (shape == 1) hipLaunchKernelGGL((hmpc_adjoint_multi_kernel<20, 2>), grid, block, 0, stream, args, act_tol, seeds, s0, ns, out);
    else hipLaunchKernelGGL((hmpc_adjoint_multi_kernel<10, 3>), grid, block, 0, stream, args, act_tol, seeds, s0, ns, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace hmpc
