// hmpc_certificate.hip -- the KKT certificate of every instance (hmpc_kkt_certificate): the gradient of the QP
// objective at the forces in the force buffer, multipliers >= 0 on the active limits, the stationarity residual they leave and a
// per-instance summary that can mask the commands of a sweep.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the prediction and margins kernels it
// assembles by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h -- so that x0, Acd, Bcd, the weights,
// the trajectory and the constraint block Fc are the very binary32 values the solve used, hmpc_params and the per-instance mu included.
// Everything behind the assembly (costate, gradient, slacks, NNLS, maxima; the arithmetic is fixed there) is certificate_of_instance of
// hmpc_certificate.h: it checks the solver, it does not repeat it.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.
// Traffic: the record and 6 NC h floats in (coalesced bursts), 22 NC h + 4 doubles and 2 ints out, staged in LDS and stored in coalesced
// passes.  No atomics, no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_certificate.h"

namespace hmpc {
namespace {

template <int HMAX, int NC>
struct CertLds {
  DerivedSmem<HMAX, NC> S;
  CertScratch<NC, HMAX> T;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(DERIVED_NT) void hmpc_certificate_kernel(KernelArgs args, double act_tol, CertificateOut out) {
  using RL = RecLayout<NC>;
  constexpr int NT = DERIVED_NT;
  __shared__ CertLds<HMAX, NC> L;
  static_assert(sizeof(CertLds<HMAX, NC>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
  const size_t ls = (size_t)inst * NC * h;
  certificate_of_instance<NC, HMAX, NT>(A.Acd, A.Bcd, A.x0, A.W, rf + RL::NF, rf + RL::AL, A.Fc, L.u, gait, L.cap, h, act_tol, L.T,
                                        out.grad + 6 * ls, out.lambda + 10 * ls, out.resid + 6 * ls, out.summary + (size_t)inst * CERT_CLASSES,
                                        out.where + (size_t)inst * CERT_WHERE);
}

}  // namespace

hipError_t launch_certificate(int nc, const KernelArgs &args, double act_tol, const CertificateOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || !out.grad || !out.lambda || !out.resid || !out.summary || !out.where || !args.forces ||
      !args.records)
    return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_shape(nc, args.horizon, [&](auto H, auto C) {
    hipLaunchKernelGGL((hmpc_certificate_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, out);
  });
}

hipError_t launch_certificate_penalty(const double *summary, const double ceil[CERT_CEILS], const double *penalty_in, double *out, int batch,
                                      hipStream_t stream) {
  if (!summary || !ceil || !out || batch < 1) return hipErrorInvalidValue;
  CertCeil c;
  for (int k = 0; k < CERT_CEILS; ++k) c.v[k] = ceil[k];
  hipLaunchKernelGGL((certificate_penalty_kernel<PENALTY_NT>), dim3((batch + PENALTY_NT - 1) / PENALTY_NT), dim3(PENALTY_NT), 0, stream, summary,
                     c, penalty_in, out, batch);
  return hipGetLastError();
}

}  // namespace hmpc
