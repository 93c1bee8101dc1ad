// hmpc_certificate.hip -- the KKT certificate of every instance (hmpc_kkt_certificate): the gradient of the QP
// objective at the forces in the force buffer, multipliers >= 0 on the active limits, the stationarity residual they leave and a
// per-instance summary that can mask the commands of a sweep.
//
// A launch of its own behind a solve (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like the prediction and margins kernels it
// assembles by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over the
// smallest Smem that serves (NC, HMAX) -- so that x0, Acd, Bcd, the weights, the trajectory and the constraint block Fc are the very
// binary32 values the solve used, hmpc_params and the per-instance mu included.  Everything behind the assembly (costate, gradient, slacks,
// NNLS, maxima; the arithmetic is fixed there) is certificate_of_instance of hmpc_certificate.h: it checks the solver, it does not repeat it.
// Mapping: one workgroup of 128 threads per instance (stage_a_scalars needs lanes of two waves); see the header.
// Traffic: the record and 6 NC h floats in (coalesced bursts), 22 NC h + 4 doubles and 2 ints out, staged in LDS and stored in coalesced
// passes.  No atomics, no inline assembly, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_certificate.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_predict.hip: 12 reduced variables, a working set of one row)
template <int HMAX, int NC>
using CertSmem = Smem<12, HMAX, CERT_NT, 1, NC, 1>;

template <int HMAX, int NC>
struct CertLds {
  CertSmem<HMAX, NC> S;
  CertScratch<NC, HMAX> T;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
};

template <int HMAX, int NC>
__global__ __launch_bounds__(CERT_NT) void hmpc_certificate_kernel(KernelArgs args, double act_tol, CertificateOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = CERT_NT;
  __shared__ CertLds<HMAX, NC> L;
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
  const dim3 grid(args.batch), block(CERT_NT);
  if (nc == 2 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_certificate_kernel<10, 2>), grid, block, 0, stream, args, act_tol, out);
  else if (nc == 2 && args.horizon <= 20) hipLaunchKernelGGL((hmpc_certificate_kernel<20, 2>), grid, block, 0, stream, args, act_tol, out);
  else if (nc == 3 && args.horizon <= 10) hipLaunchKernelGGL((hmpc_certificate_kernel<10, 3>), grid, block, 0, stream, args, act_tol, out);
  else return hipErrorInvalidValue;
  return hipGetLastError();
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
