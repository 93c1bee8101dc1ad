// hmpc_margins.hip -- the constraint margins of every instance (hmpc_constraint_margins): how far the forces in the
// force buffer are from each limit the QP was solved under -- friction pyramid, Mx, line contact, Fz floor and cap.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the prediction kernel it assembles
// by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the smallest
// Smem that serves (NC, HMAX) -- so that the constraint block Fc is the very binary32 block the solve used: foot rotations, the right-heel
// sign, hmpc_params and the per-instance mu included.  Everything behind the assembly (rows, slacks, minima; the arithmetic is fixed
// there) is margins_of_instance of hmpc_margins.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); one lane per (step, row) runs the
// U-term fma chain with Fc and u_i in LDS; the slacks are staged in LDS and stored in one coalesced pass.
// Traffic: the record and 6 NC h floats in (coalesced bursts), 10 NC h + 6 doubles and 6 ints out.  No atomics, no inline assembly, nothing
// kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_margins.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_predict.hip: 12 reduced variables, a working set of one row)
template <int HMAX, int NC>
using MarginsSmem = Smem<12, HMAX, MARGINS_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct MarginsLds {
  MarginsSmem<HMAX, NC> S;
  double slack[10 * NC * HMAX];                     // staged for one coalesced store
  MarginMin wave_min[MARGINS_WAVES][MARGIN_CLASSES];
  float u[6 * NC * HMAX];                           // the instance's slot of the force buffer
  float cap[4];                                     // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(MARGINS_NT) void hmpc_margins_kernel(KernelArgs args, double *slack, double *summary, int32_t *where) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = MARGINS_NT;
  __shared__ MarginsLds<HMAX, NC> L;
  auto &S = L.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX) return;  // uniform
  {
    // stage A0 as hmpc_kernel has it: the record, one coalesced burst into LDS (restated as in hmpc_predict.hip, for the reason given there)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(args.records + (size_t)inst * args.stride);
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
  margins_of_instance<NC, NT>(A.Fc, L.u, gait, L.cap, h, L.slack, L.wave_min, slack + (size_t)inst * 10 * NC * h,
                              summary + (size_t)inst * MARGIN_CLASSES, where + (size_t)inst * MARGIN_CLASSES);
}

}  // namespace

hipError_t launch_margins(int nc, const KernelArgs &args, double *slack, double *summary, int32_t *where, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !slack || !summary || !where || !args.forces || !args.records) return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(MARGINS_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_margins_kernel<10, 2>), grid, block, 0, stream, args, slack, summary, where);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_margins_kernel<20, 2>), grid, block, 0, stream, args, slack, summary, where);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_margins_kernel<10, 3>), grid, block, 0, stream, args, slack, summary, where);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_margin_penalty(const double *summary, const double floor[MARGIN_CLASSES], const double *penalty_in, double *out, int batch,
                                 hipStream_t stream) {
  if (!summary || !floor || !out || batch < 1) return hipErrorInvalidValue;
  MarginFloor f;
  for (int k = 0; k < MARGIN_CLASSES; ++k) f.v[k] = floor[k];
  hipLaunchKernelGGL((margin_penalty_kernel<PENALTY_NT>), dim3((batch + PENALTY_NT - 1) / PENALTY_NT), dim3(PENALTY_NT), 0, stream, summary, f,
                     penalty_in, out, batch);
  return hipGetLastError();
}

}  // namespace hmpc
