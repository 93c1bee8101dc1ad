// hmpc_variants.hip -- instantiates the kernel family of hmpc_kernel.h.  Built once per group (-DHMPC_VARIANT_GROUP=k,
// hector_simulation_amd/build.py) into separate objects: the 2 900-line kernel template costs 5-20 s per instantiation, and
// the fifteen variants (21 kernels: a solve kernel each, an assembly-only one per fast variant) compile side by side instead of in
// one long translation unit.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_variants.h"

#ifndef HMPC_VARIANT_GROUP
#error "compile with -DHMPC_VARIANT_GROUP=0..3 (hector_simulation_amd/build.py does)"
#endif

namespace {
template <int NMAX, int HMAX, int NT, int QCAP, int NC, int BPT, Role ROLE>
Variant make_variant() {
  using SM = hmpc::Smem<NMAX, HMAX, NT, QCAP, NC, BPT>;
  static_assert(sizeof(SM) <= 160 * 1024, "LDS budget of a gfx950 CU");
  static_assert(BPT == 1 || NT >= 512 || sizeof(SM) <= 80 * 1024, "two workgroups per CU");
  // (the same shape test as SHAPE_HANDOVER / SPILLS / RESUMABLE in hmpc_kernel.h)
  constexpr bool handover = NMAX == 120 && NT == 256 && NC == 2 && BPT == 1 && QCAP != 0;
  static_assert(!handover || (QCAP < HMPC_QCAP_CONT) == (ROLE == Role::FAST || ROLE == Role::SWEEP), "hand-over: the fast variants save");
  static_assert((ROLE == Role::CONT) == (handover && QCAP >= HMPC_QCAP_CONT && QCAP < NMAX), "hand-over: the continuation variants resume");
  constexpr int MODE = ROLE == Role::SWEEP ? 1 : 0;
  kernel_fn assemble = nullptr;  // (the assembly-only debug kernel: hmpc_debug_assemble launches the fast variant's)
  if constexpr (ROLE == Role::FAST) assemble = hmpc::hmpc_kernel<NMAX, HMAX, NT, QCAP, true, NC, BPT, 0>;
  return Variant{NMAX, HMAX, NT, QCAP, NC, ROLE, hmpc::hmpc_kernel<NMAX, HMAX, NT, QCAP, false, NC, BPT, MODE>, assemble, sizeof(SM),
                 hmpc::DbgLayout<NMAX, NC>::TOTAL,
                 (handover && ROLE == Role::FAST) ? hmpc::SpillLayout<SM, NT, BPT>::stride_for(QCAP) : 0};
}
}  // namespace

#define HMPC_DEFINE_VARIANT(IDX, GRP, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE) HMPC_DEFINE_VARIANT_##GRP(IDX, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE)
#define HMPC_DEFINE_IT(IDX, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE) \
  Variant hmpc_variant_##IDX() { return make_variant<NMAX, HMAX, NT, QCAP, NC, BPT, Role::ROLE>(); }
#define HMPC_SKIP_IT(IDX, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE)
#if HMPC_VARIANT_GROUP == 0
#define HMPC_DEFINE_VARIANT_0 HMPC_DEFINE_IT
#else
#define HMPC_DEFINE_VARIANT_0 HMPC_SKIP_IT
#endif
#if HMPC_VARIANT_GROUP == 1
#define HMPC_DEFINE_VARIANT_1 HMPC_DEFINE_IT
#else
#define HMPC_DEFINE_VARIANT_1 HMPC_SKIP_IT
#endif
#if HMPC_VARIANT_GROUP == 2
#define HMPC_DEFINE_VARIANT_2 HMPC_DEFINE_IT
#else
#define HMPC_DEFINE_VARIANT_2 HMPC_SKIP_IT
#endif
#if HMPC_VARIANT_GROUP == 3
#define HMPC_DEFINE_VARIANT_3 HMPC_DEFINE_IT
#else
#define HMPC_DEFINE_VARIANT_3 HMPC_SKIP_IT
#endif
HMPC_VARIANT_TABLE(HMPC_DEFINE_VARIANT)
