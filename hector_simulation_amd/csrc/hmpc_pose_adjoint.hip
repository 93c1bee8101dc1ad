// hmpc_pose_adjoint.hip -- the pose gradients of the solve (hmpc_adjoint_record): from what hmpc_solve_adjoint,
// hmpc_adjoint_model and hmpc_adjoint_limits last wrote, the gradient of the loss in every float of the packed record, the quaternion and
// the joint angles through stage A1 + A2 included.
//
// A launch of its own behind the three (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like their kernels it assembles by
// CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that the sines and cosines, the Euler tables,
// Acd and Bcd are the very binary32 values the solve used, hmpc_params included.  Everything behind the assembly (the arithmetic is fixed
// there) is pose_adjoint_of_instance of hmpc_pose_adjoint.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.
// Traffic: the record and 13 + 12 h + 12 + 6 NC + 9 + 18 NC + 3 NC + 1 + 48 NC^2 doubles in (coalesced bursts); NF + 12 h + 9 (1 + NC) + 3
// doubles out.  No atomics, no inline assembly, no matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_pose_adjoint.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct PadjLds {
  DerivedSmem<HMAX, NC> S;        // the assembly: read until the chains have ended
  PoseAdjointWork<NC, HMAX> Wk;   // the staged gradients and outputs
  float R[12];                    // quat_to_R of the record's quaternion
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_pose_adjoint_kernel(KernelArgs args, PoseAdjointIn in, PoseAdjointOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT;
  __shared__ PadjLds<HMAX, NC> L;
  static_assert(sizeof(PadjLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, nullptr, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  derived_fill_rotation(S, L.R);
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
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_pose_adjoint_kernel<H(), C()>), grid, block, 0, stream, args, in, out);
  });
}

}  // namespace hmpc
