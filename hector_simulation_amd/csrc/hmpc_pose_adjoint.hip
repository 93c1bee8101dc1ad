// hmpc_pose_adjoint.hip -- the pose gradients of the solve (hmpc_adjoint_record): from what hmpc_solve_adjoint,
// hmpc_adjoint_model and hmpc_adjoint_limits last wrote, the gradient of the loss in every float of the packed record, the quaternion and
// the joint angles through stage A1 + A2 included.
//
// A launch of its own behind the three (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like their kernels it assembles by
// CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the smallest Smem
// that serves (NC, HMAX) -- so that the sines and cosines, the Euler tables, Acd and Bcd are the very binary32 values the solve used,
// hmpc_params included.  Everything behind the assembly (the arithmetic is fixed there) is pose_adjoint_of_instance of
// hmpc_pose_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.
// Traffic: the record and 13 + 12 h + 12 + 6 NC + 9 + 18 NC + 3 NC + 1 + 48 NC^2 doubles in (coalesced bursts); NF + 12 h + 9 (1 + NC) + 3
// doubles out.  No atomics, no inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_pose_adjoint.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_adjoint.hip)
template <int HMAX, int NC>
using PadjSmem = Smem<12, HMAX, PADJ_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct PadjLds {
  PadjSmem<HMAX, NC> S;           // the assembly: read until the chains have ended
  PoseAdjointWork<NC, HMAX> Wk;   // the staged gradients and outputs
  float R[12];                    // quat_to_R of the record's quaternion
};

template <int HMAX, int NC>
__global__ __launch_bounds__(PADJ_NT) void hmpc_pose_adjoint_kernel(KernelArgs args, PoseAdjointIn in, PoseAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = PADJ_NT;
  __shared__ PadjLds<HMAX, NC> L;
  static_assert(sizeof(PadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec)) return;  // uniform
  {
    // stage A0 as hmpc_kernel has it: the record, one coalesced burst into LDS (restated as in hmpc_model_adjoint.hip)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(args.records + (size_t)inst * (size_t)args.stride);
    const int nwords = args.stride >> 2;
    for (int t = tid; t < nwords; t += NT) S.u.a.rec[t] = src[t];
  }
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
  const size_t i = (size_t)inst, nrec = (size_t)(RL::NF + 12 * h);
  pose_adjoint_of_instance<NC, HMAX, NT>(rf, &A.sc[0][0], &A.sc234[0][0], A.ypsc, L.R, A.Acd, A.Bcd, in.grad_x0 + i * 13, in.grad_traj + i * 12 * h,
                                         in.grad_weights + i * 12, in.grad_alpha + i * U, in.grad_A + i * 169, in.grad_B + i * 13 * U,
                                         in.grad_r + i * 3 * NC, in.grad_limits + i * (3 + NC), in.grad_Fc + i * 8 * NC * U, h, (double)args.dt,
                                         (double)args.lt, (double)args.lh, (double)args.Ib[0], (double)args.Ib[1], (double)args.Ib[2], L.Wk,
                                         out.grad_record + i * nrec, out.grad_frames + i * 9 * (1 + NC), out.grad_rpy + i * 3);
}

}  // namespace

hipError_t launch_pose_adjoint(int nc, const KernelArgs &args, const PoseAdjointIn &in, const PoseAdjointOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !in.grad_x0 || !in.grad_traj || !in.grad_weights || !in.grad_alpha || !in.grad_A || !in.grad_B ||
      !in.grad_r || !in.grad_limits || !in.grad_Fc || !out.grad_record || !out.grad_frames || !out.grad_rpy || !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(PADJ_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_pose_adjoint_kernel<10, 2>), grid, block, 0, stream, args, in, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_pose_adjoint_kernel<20, 2>), grid, block, 0, stream, args, in, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_pose_adjoint_kernel<10, 3>), grid, block, 0, stream, args, in, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hmpc
