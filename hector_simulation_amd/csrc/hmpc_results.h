// hmpc_results.h -- THE table of the results derived from a solve: per family its arrays, in the member order of the kernel's *Out struct
// (which is the argument order of its hmpc_set_device_* / hmpc_get_device_* / hmpc_download_* entries), and per array its element size
// and its elements per instance as a function of (contacts, horizon).  Every allocation and every copy of hmpc_results.hip takes its
// size from here; interface.py keeps the same table for the host arrays it allocates, and tests/test_result_layout_on_host.py compares
// the two line by line.  Plain values: no HIP runtime call and no hmpc_handle, so that tests/src/result_layout_on_host.cpp compiles this
// header for the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hmpc_plan.h"
#include "hmpc_record.h"

#pragma GCC visibility push(hidden)

namespace hmpc {

using RowFn = size_t (*)(size_t nc, size_t hz);  // elements per instance (per sweep group, for the selection)
struct ResultArray {
  const char *name;
  size_t elem;  // bytes per element
  RowFn row;
};

#define HMPC_ROW(expr) [](size_t nc, size_t hz) -> size_t { return (void)nc, (void)hz, (expr); }
constexpr size_t F32 = sizeof(float), F64 = sizeof(double), I32 = sizeof(int32_t), U32 = sizeof(uint32_t);

inline constexpr ResultArray PREDICTION_ROWS[] = {{"states", F32, HMPC_ROW(hz * 13)}, {"cost", F64, HMPC_ROW(2)}};
inline constexpr ResultArray SELECTION_ROWS[] = {{"index", I32, HMPC_ROW(1)}, {"score", F64, HMPC_ROW(1)}, {"forces", F32, HMPC_ROW(6 * nc * hz)},
                                                 {"status", U32, HMPC_ROW(1)}, {"states", F32, HMPC_ROW(hz * 13)}};
inline constexpr ResultArray MARGIN_ROWS[] = {{"slack", F64, HMPC_ROW(hz * nc * 10)}, {"summary", F64, HMPC_ROW(6)}, {"where", I32, HMPC_ROW(6)}};
inline constexpr ResultArray CERTIFICATE_ROWS[] = {{"grad", F64, HMPC_ROW(hz * 6 * nc)}, {"lambda", F64, HMPC_ROW(hz * nc * 10)},
                                                   {"resid", F64, HMPC_ROW(hz * nc * 6)}, {"summary", F64, HMPC_ROW(4)}, {"where", I32, HMPC_ROW(2)}};
inline constexpr ResultArray GAIN_ROWS[] = {{"gain", F64, HMPC_ROW(6 * nc * 13)}, {"ref_gain", F64, HMPC_ROW(hz * 6 * nc * 12)},
                                            {"summary", F64, HMPC_ROW(2)}, {"free_dims", I32, HMPC_ROW(hz)}};
inline constexpr ResultArray FIRST_ORDER_ROWS[] = {{"wrench", F32, HMPC_ROW(6 * nc)}, {"worst_slack", F64, HMPC_ROW(1)}};
inline constexpr ResultArray ADJOINT_ROWS[] = {{"grad_x0", F64, HMPC_ROW(13)}, {"grad_traj", F64, HMPC_ROW(hz * 12)}, {"grad_weights", F64, HMPC_ROW(12)},
                                               {"grad_alpha", F64, HMPC_ROW(6 * nc)}, {"dir", F64, HMPC_ROW(hz * 6 * nc)}, {"summary", F64, HMPC_ROW(2)}};
inline constexpr ResultArray MODEL_ROWS[] = {{"grad_A", F64, HMPC_ROW(13 * 13)}, {"grad_B", F64, HMPC_ROW(13 * 6 * nc)}, {"grad_r", F64, HMPC_ROW(3 * nc)},
                                             {"grad_params", F64, HMPC_ROW(4)}, {"costate", F64, HMPC_ROW(2 * 13)}};
inline constexpr ResultArray LIMIT_ROWS[] = {{"grad_limits", F64, HMPC_ROW(3 + nc)}, {"grad_Fc", F64, HMPC_ROW(8 * nc * 6 * nc)},
                                             {"grad_bound", F64, HMPC_ROW(hz * nc * 10)}, {"lambda", F64, HMPC_ROW(hz * nc * 10)},
                                             {"nu", F64, HMPC_ROW(hz * nc * 10)}, {"summary", F64, HMPC_ROW(3)}};
inline constexpr ResultArray RECORD_ROWS[] = {{"grad_record", F64, HMPC_ROW((size_t)rec_fixed_floats((int)nc) + 12 * hz)},
                                              {"grad_frames", F64, HMPC_ROW((1 + nc) * 9)}, {"grad_rpy", F64, HMPC_ROW(3)}};
#undef HMPC_ROW

// the chain of the multi-seed adjoint: the member order of struct hmpc_adjoint_chain, every row the record, model or limit row it is
constexpr ResultArray renamed(const char *name, const ResultArray &a) { return {name, a.elem, a.row}; }
constexpr int CHAIN_COMPACT = 6;  // the first six are always produced, the other eight only into a caller's buffer
constexpr int ADJOINT_ARRAYS = sizeof(ADJOINT_ROWS) / sizeof(ADJOINT_ROWS[0]);
inline constexpr ResultArray CHAIN_ROWS[] = {RECORD_ROWS[0], RECORD_ROWS[1], RECORD_ROWS[2], MODEL_ROWS[3], LIMIT_ROWS[0], renamed("limit_summary", LIMIT_ROWS[5]),
                                             MODEL_ROWS[0], MODEL_ROWS[1], MODEL_ROWS[2], MODEL_ROWS[4],
                                             LIMIT_ROWS[1], LIMIT_ROWS[2], LIMIT_ROWS[3], LIMIT_ROWS[4]};
constexpr int CHAIN_ARRAYS = sizeof(CHAIN_ROWS) / sizeof(CHAIN_ROWS[0]);

// the families; [0, N_SINGLE) are the ones whose arrays the handle keeps as OutputBuffers, one row per instance of max_batch (the
// multi-seed adjoint and its chain have one row per (seed, instance) and grow with the seed count)
enum Family { F_PREDICTION, F_SELECTION, F_MARGINS, F_CERTIFICATE, F_GAINS, F_FIRST_ORDER, F_ADJOINT, F_MODEL_ADJOINT, F_LIMIT_ADJOINT, F_RECORD_ADJOINT,
              N_SINGLE, F_ADJOINT_MULTI = N_SINGLE, F_ADJOINT_CHAIN, N_FAMILIES };
struct ResultFamily {
  const char *name;  // (the suffix of its hmpc_download_* entry)
  ResultNode node;   // its node of ResultState's graph
  int n;
  const ResultArray *arrays;
};
template <int N>
constexpr ResultFamily family(const char *name, ResultNode node, const ResultArray (&a)[N]) { return {name, node, N, a}; }
inline constexpr ResultFamily FAMILIES[N_FAMILIES] = {
    family("prediction", ResultNode::PREDICTION, PREDICTION_ROWS), family("selection", ResultNode::SELECTION, SELECTION_ROWS),
    family("margins", ResultNode::MARGINS, MARGIN_ROWS), family("certificate", ResultNode::CERTIFICATE, CERTIFICATE_ROWS),
    family("gains", ResultNode::GAINS, GAIN_ROWS), family("first_order", ResultNode::FIRST_ORDER, FIRST_ORDER_ROWS),
    family("adjoint", ResultNode::ADJOINT, ADJOINT_ROWS), family("adjoint_model", ResultNode::MODEL_ADJOINT, MODEL_ROWS),
    family("adjoint_limits", ResultNode::LIMIT_ADJOINT, LIMIT_ROWS), family("adjoint_record", ResultNode::RECORD_ADJOINT, RECORD_ROWS),
    family("adjoint_multi", ResultNode::ADJOINT_MULTI, ADJOINT_ROWS), family("adjoint_chain_multi", ResultNode::ADJOINT_CHAIN, CHAIN_ROWS)};
constexpr int MAX_SINGLE_ARRAYS = 6, MAX_ARRAYS = 14;  // the most arrays of a family of [0, N_SINGLE), and of any

constexpr bool family_sizes_fit() {
  for (int f = 0; f < N_FAMILIES; ++f)
    if (FAMILIES[f].n > (f < N_SINGLE ? MAX_SINGLE_ARRAYS : MAX_ARRAYS)) return false;
  return true;
}
static_assert(family_sizes_fit(), "MAX_SINGLE_ARRAYS / MAX_ARRAYS hold every family of the table");

// bytes of `rows` rows of array k of a family
inline size_t array_bytes(const ResultFamily &fam, int k, int nc, int hz, size_t rows) {
  return rows * fam.arrays[k].row((size_t)nc, (size_t)hz) * fam.arrays[k].elem;
}

}  // namespace hmpc

#pragma GCC visibility pop
