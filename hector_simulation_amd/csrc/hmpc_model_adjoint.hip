// hmpc_model_adjoint.hip -- the model gradients of the solve (hmpc_adjoint_model): from the direction `dir` of the
// last adjoint, the gradients of its loss in Acd and Bcd themselves and, through stage A2's B, in the foot positions, the mass and the
// body inertia of the QP that was solved.
//
// A launch of its own behind hmpc_solve_adjoint (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the adjoint's kernel it
// assembles by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the
// smallest Smem that serves (NC, HMAX) -- so that x0, Acd, Bcd and the weights are the very binary32 values the solve used, hmpc_params
// and the per-instance mu included.  Everything behind the assembly (the arithmetic is fixed there) is model_adjoint_of_instance of
// hmpc_model_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.  x, dx, both costates
// and G_A, G_B overlay the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic: the record, 6 NC h floats and 6 NC h doubles in (coalesced bursts); 169 + 13 U + 3 NC + 4 + 26 doubles out.  No atomics, no
// inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_model_adjoint.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_adjoint.hip)
template <int HMAX, int NC>
using MadjSmem = Smem<12, HMAX, MADJ_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct MadjLds {
  union {
    MadjSmem<HMAX, NC> S;           // the assembly, and the first phase of model_adjoint_of_instance
    ModelAdjointWork<NC, HMAX> Wk;  // the passes
  } o;
  ModelAdjointKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float R[12];             // quat_to_R of the record's quaternion
};

template <int HMAX, int NC>
__global__ __launch_bounds__(MADJ_NT) void hmpc_model_adjoint_kernel(KernelArgs args, double mass, const double *dir, ModelAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = MADJ_NT;
  __shared__ MadjLds<HMAX, NC> L;
  static_assert(sizeof(MadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
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
  if (tid == NT - 1) {  // the body rotation, as stage A2 forms it
    float R[9], Rt[9];
    quat_to_R(rf + RL::Q, R, Rt);
#pragma unroll
    for (int k = 0; k < 9; ++k) L.R[k] = R[k];
  }
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
  const dim3 grid(args.batch), block(MADJ_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_model_adjoint_kernel<10, 2>), grid, block, 0, stream, args, mass, dir, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_model_adjoint_kernel<20, 2>), grid, block, 0, stream, args, mass, dir, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_model_adjoint_kernel<10, 3>), grid, block, 0, stream, args, mass, dir, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hmpc
