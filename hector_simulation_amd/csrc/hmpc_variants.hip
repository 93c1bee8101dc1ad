// hmpc_variants.hip -- instantiates the kernel family of hmpc_kernel.h.  Built once per group (-DHMPC_VARIANT_GROUP=k,
// hector_simulation_amd/build.py) into separate objects: the kernel template (hmpc_kernel.h, 3 500 lines) costs 5-20 s per instantiation, and
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
  using VT = hmpc::VariantTraits<NMAX, HMAX, NT, QCAP, NC, BPT, ROLE>;
  kernel_fn assemble = nullptr;  // (the assembly-only debug kernel: hmpc_debug_assemble launches the fast variant's)
  if constexpr (ROLE == Role::FAST) assemble = hmpc::hmpc_kernel<NMAX, HMAX, NT, QCAP, true, NC, BPT, ROLE>;
  return Variant{NMAX, HMAX, NT, QCAP, NC, ROLE, VT::EGLOBAL, hmpc::hmpc_kernel<NMAX, HMAX, NT, QCAP, false, NC, BPT, ROLE>, assemble,
                 sizeof(typename VT::SM), hmpc::DbgLayout<NMAX, NC>::TOTAL, VT::SPILL_STRIDE, VT::READS_FRONT};
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
