// hmpc_margins.hip -- the constraint margins of every instance (hmpc_constraint_margins): how far the forces in the
// force buffer are from each limit the QP was solved under -- friction pyramid, Mx, line contact, Fz floor and cap.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the prediction kernel it assembles
// by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that the constraint block Fc is the very
// binary32 block the solve used: foot rotations, the right-heel sign, hmpc_params and the per-instance mu included.  Everything behind
// the assembly (rows, slacks, minima; the arithmetic is fixed there) is margins_of_instance of hmpc_margins.h.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); one lane per (step, row) runs the
// U-term fma chain with Fc and u_i in LDS; the slacks are staged in LDS and stored in one coalesced pass.
// Traffic: the record and 6 NC h floats in (coalesced bursts), 10 NC h + 6 doubles and 6 ints out.  No atomics, no inline assembly, nothing
// kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_margins.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct MarginsLds {
  DerivedSmem<HMAX, NC> S;
  double slack[10 * NC * HMAX];                     // staged for one coalesced store
  MarginMin wave_min[MARGINS_WAVES][MARGIN_CLASSES];
  float u[6 * NC * HMAX];                           // the instance's slot of the force buffer
  float cap[4];                                     // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_margins_kernel(KernelArgs args, double *slack, double *summary, int32_t *where) {
  constexpr int NT = DERIVED_NT;
  __shared__ MarginsLds<HMAX, NC> L;
  static_assert(sizeof(MarginsLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  derived_fill_caps(S, args, L.cap);
  margins_of_instance<NC, NT>(A.Fc, L.u, derived_gait(S, h), L.cap, h, L.slack, L.wave_min, slack + (size_t)inst * 10 * NC * h,
                              summary + (size_t)inst * MARGIN_CLASSES, where + (size_t)inst * MARGIN_CLASSES);
}

}  // namespace

hipError_t launch_margins(int nc, const KernelArgs &args, double *slack, double *summary, int32_t *where, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !slack || !summary || !where || !args.forces || !args.records) return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_margins_kernel<H(), C()>), grid, block, 0, stream, args, slack, summary, where);
  });
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
