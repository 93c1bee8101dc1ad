// hmpc_variants.h -- the table of kernel variants, shared between the host side (hmpc_plan.h picks, hmpc_launch.hip launches) and
// hmpc_variants.hip (instantiates; compiled once per group -DHMPC_VARIANT_GROUP=0..3 so that the groups build in parallel).
#pragma once
#include <stddef.h>

#include "hmpc_kernel_args.h"

#ifndef HMPC_QCAP_FAST
#define HMPC_QCAP_FAST 64  // working-set capacity of the fast 120-variable h <= 10 variant (49 KB LDS: three per CU)
#endif
// (HMPC_QCAP_CONT, the capacity of the CONTINUATION variant of the same shapes: hmpc_kernel_args.h, which the kernel sees as well)
// (not switches: each is pinned from both sides by the LDS budget and the staging areas that alias the solver state --
//  static_asserts of VariantTraits, hmpc_kernel.h -- 152 rows are what 160 KB leave next to the wide variant's mat-vec staging,
//  96 what 80 KB, two workgroups per CU, leave the three-contact one)
constexpr int HMPC_QCAP_WIDE = 152;  // ... of the 240-variable variant (double support over h = 11 .. 20)
constexpr int HMPC_QCAP_3C = 96;     // ... of the fast three-contact variant (256 threads, two register blocks each, <= 80 KB LDS: two per CU)

typedef void (*kernel_fn)(hmpc::KernelArgs);
using hmpc::Role;  // FAST, CONT, SAFE, SWEEP (hmpc_kernel_args.h); what follows from a row's role and shape: VariantTraits, hmpc_kernel.h
struct Variant {
  int nmax, hmax, nt, qcap, nc;
  Role role;
  bool e_global;  // the packed Schur inverse lives in KernelArgs::e_scratch, a slice per workgroup of the launch (VariantTraits::EGLOBAL)
  kernel_fn solve, assemble;  // assemble: the assembly-only debug kernel (FAST variants only, nullptr otherwise)
  size_t smem;
  int dbg_floats;
  size_t spill_stride;  // bytes of one hand-over slot (KernelArgs::spill) when this variant SAVES its state (FAST on the hand-over shape), 0 otherwise
  bool reads_front;     // takes stages A1 / A2 from KernelArgs::front where it is handed in (VariantTraits::READS_FRONT)
};

// index = position in hmpc_launch.hip's variants(); (NMAX, HMAX, NT, QCAP, NC, BPT, ROLE), group = translation unit that builds it.
// The groups are balanced by compile time (the two-blocks-per-thread and 512-thread variants are the slow ones).
#define HMPC_VARIANT_TABLE(X)                             \
  X(0, 0, 60, 10, 128, 60, 2, 1, FAST)                    \
  X(1, 0, 120, 10, 256, HMPC_QCAP_FAST, 2, 1, FAST)       \
  X(2, 0, 60, 20, 128, 60, 2, 1, FAST)                    \
  X(3, 1, 120, 20, 256, HMPC_QCAP_FAST, 2, 1, FAST)       \
  X(4, 1, 120, 10, 256, 120, 2, 1, SAFE)                  \
  X(5, 1, 120, 20, 256, 120, 2, 1, SAFE)                  \
  X(6, 2, 180, 10, 256, HMPC_QCAP_3C, 3, 2, FAST)         \
  X(7, 3, 180, 10, 512, 140, 3, 1, SAFE)                  \
  X(8, 3, 240, 20, 512, HMPC_QCAP_WIDE, 2, 2, FAST)       \
  X(9, 3, 240, 20, 512, 0, 2, 2, SAFE)                    \
  X(10, 2, 180, 10, 512, 0, 3, 1, SAFE)                   \
  X(11, 0, 120, 10, 256, HMPC_QCAP_CONT, 2, 1, CONT)      \
  X(12, 1, 120, 20, 256, HMPC_QCAP_CONT, 2, 1, CONT)      \
  X(13, 2, 120, 10, 256, HMPC_QCAP_FAST, 2, 1, SWEEP)     \
  X(14, 3, 60, 10, 128, 60, 2, 1, SWEEP)
constexpr int HMPC_VARIANT_GROUPS = 4;

#define HMPC_DECLARE_VARIANT(IDX, GRP, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE) Variant hmpc_variant_##IDX();
HMPC_VARIANT_TABLE(HMPC_DECLARE_VARIANT)
#undef HMPC_DECLARE_VARIANT
