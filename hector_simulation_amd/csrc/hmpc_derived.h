// hmpc_derived.h -- what every kernel launched behind a solve does before its own arithmetic, and how its launcher picks the instantiation.
//
// The derived kernels (prediction, margins, certificate, gains, first-order wrench, the adjoints and their chain)
// rebuild the QP's data by CALLING the solve kernel's own stage function, stage_a_scalars of hmpc_kernel.h, behind the record load of
// stage A0, so that x0, Acd, Bcd, the weights, the trajectory and the constraint block Fc are the very binary32 values the solve used.
// This header is the one place that says how: the Smem they instantiate it over, the guard, the record burst, the force slot, the
// barrier and the call (derived_front), the tails several of them share (the record's float view, the gait bytes, the Fz caps, the
// body rotation), and the dispatch of a launch to the shape rule of hmpc_derived_shape.h.  hmpc_kernel keeps its own A0 lines: there
// they are no function, because moving them into one changed the machine code of four safe variants (profiles/r09/isa_hash.txt, README
// there).  That reason does not reach a function only these kernels call.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hmpc_derived_shape.h"  // DERIVED_NT, derived_shape, for_derived_shape
#include "hmpc_kernel.h"

namespace hmpc {

// the smallest Smem stage_a_scalars can be instantiated over: 12 reduced variables (two leg-steps: Smem wants an even count; the
// swing-elimination tables of larger instances are simply not filled, nothing in a derived kernel reads them), a working set of one row
template <int HMAX, int NC>
using DerivedSmem = Smem<12, HMAX, DERIVED_NT, 1, NC, 1>;

// stage A0 as hmpc_kernel has it: the record of this workgroup's instance out of `records`, one coalesced burst into LDS
template <int HMAX, int NC>
__device__ __forceinline__ void derived_load_record(DerivedSmem<HMAX, NC> &S, const unsigned char *records, const int stride) {
  const int tid = threadIdx.x, inst = blockIdx.x;
  const uint32_t *src = reinterpret_cast<const uint32_t *>(records + (size_t)inst * (size_t)stride);
  const int nwords = stride >> 2;
  for (int t = tid; t < nwords; t += DERIVED_NT) S.u.a.rec[t] = src[t];
}

// stages A1 + A2 on the record in S (ends with a barrier)
template <int HMAX, int NC>
__device__ __forceinline__ void derived_assemble(DerivedSmem<HMAX, NC> &S, const KernelArgs &args) {
  Prof prof;
  stage_a_scalars<12, HMAX, DERIVED_NT, 1, NC, 1>(S, args, blockIdx.x, args.horizon, prof);
}

// The common front.  false: this workgroup has no instance, or the launch does not fit the instantiation -- uniform, the caller returns.
// Otherwise the record of the instance (out of `records`), its slot of the force buffer into u[6 NC h] (nullptr: not loaded), a barrier,
// and the assembly.
template <int HMAX, int NC, class ForceSlot>
__device__ __forceinline__ bool derived_front(DerivedSmem<HMAX, NC> &S, ForceSlot u, const KernelArgs &args, const unsigned char *records) {
  constexpr int U = 6 * NC;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec)) return false;
  derived_load_record(S, records, args.stride);
  if constexpr (!std::is_same_v<ForceSlot, std::nullptr_t>) {
    for (int t = tid; t < U * h; t += DERIVED_NT) u[t] = args.forces[(size_t)inst * U * h + t];
  }
  __syncthreads();
  derived_assemble(S, args);
  return true;
}
template <int HMAX, int NC, class ForceSlot>
__device__ __forceinline__ bool derived_front(DerivedSmem<HMAX, NC> &S, ForceSlot u, const KernelArgs &args) {
  return derived_front(S, u, args, args.records);
}

// ---- the tails: views of the record in S, and what several families stage beside it.  No barrier in any: the caller places it.
template <int HMAX, int NC>
__device__ __forceinline__ const float *derived_record_floats(const DerivedSmem<HMAX, NC> &S) {
  return reinterpret_cast<const float *>(S.u.a.rec);
}
template <int HMAX, int NC>
__device__ __forceinline__ const unsigned char *derived_gait(const DerivedSmem<HMAX, NC> &S, const int h) {
  return reinterpret_cast<const unsigned char *>(S.u.a.rec + RecLayout<NC>::NF + 12 * h);
}
// cap[c] = the Fz cap of contact c: f_max for the feet, the record's own for the hand
template <int HMAX, int NC>
__device__ __forceinline__ void derived_fill_caps(const DerivedSmem<HMAX, NC> &S, const KernelArgs &args, float *cap) {
  const int tid = threadIdx.x;
  if (tid < NC) cap[tid] = (NC == 3 && tid == 2) ? derived_record_floats(S)[RecLayout<NC>::FMH] : args.f_max;
}
// R[0 .. 8] = the body rotation of the record's quaternion, as stage A2 forms it (one lane)
template <int HMAX, int NC>
__device__ __forceinline__ void derived_fill_rotation(const DerivedSmem<HMAX, NC> &S, float *Rout) {
  if (threadIdx.x == DERIVED_NT - 1) {
    float R[9], Rt[9];
    quat_to_R(derived_record_floats(S) + RecLayout<NC>::Q, R, Rt);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rout[k] = R[k];
  }
}

// ---- launchers.  launch(H, C) enqueues the kernel instantiated over <H(), C()> (std::integral_constant<int, ...>, the shape of
// hmpc_derived_shape.h); an unsupported shape launches nothing and is hipErrorInvalidValue
template <class F>
hipError_t for_derived_shape(int nc, int horizon, F &&launch) {
  return for_derived_shape(nc, horizon, hipErrorInvalidValue, [&](auto H, auto C) {
    launch(H, C);
    return hipGetLastError();
  });
}
// the same once per tile of 6 nc seeds: launch(H, C, s0, ns) for seeds s0 .. s0 + ns - 1 of n_seeds, until one fails
template <class F>
hipError_t for_derived_seed_tiles(int nc, int horizon, int n_seeds, F &&launch) {
  const int tile = 6 * nc;
  for (int s0 = 0; s0 < n_seeds; s0 += tile) {
    const int ns = (n_seeds - s0 < tile) ? n_seeds - s0 : tile;
    const hipError_t e = for_derived_shape(nc, horizon, [&](auto H, auto C) { launch(H, C, s0, ns); });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace hmpc
