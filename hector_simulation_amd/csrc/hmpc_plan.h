// hmpc_plan.h -- what a solve decides before it launches anything: which variant a batch runs on, the size-class launches, the lengths
// of the device-side lists, which status words are repaired, and which derived results are still valid.  Plain functions of plain
// values: no HIP runtime call and no hmpc_handle, so that tests/src/plan_on_host.cpp compiles this header for the CPU and checks every rule.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"
#include "hmpc_variants.h"

#pragma GCC visibility push(hidden)  // (the inline functions of this header are no exports of the library)

// The kernel family (instantiated in hmpc_variants.hip, one translation unit per group so that the build runs in parallel).
// NMAX = reduced variables held on chip (6 per stance leg-step); 120 -> 256-thread workgroups (210 register blocks),
// 60 (single support over h <= 10) -> 128-thread workgroups (55 blocks).  QCAP = working-set capacity: the fast variants
// hold 64 rows (49-50 KB LDS, 168 VGPRs: three workgroups per CU, also at h = 20); the "safe"
// variants hold NMAX rows (can never overflow)
// and re-solve the few instances the fast pass flags (hmpc_resolve_failed).
// The extension with a third (hand) contact -- BASELINE config 5, 180 variables x 240 rows at h = 10 -- runs 256-thread
// workgroups with two register blocks per thread (465 blocks, two workgroups per CU; round 2: 512 threads, one per CU --
// still the shape of its safe pass).  BPT = blocks per thread, see hmpc_kernel.h.
constexpr int N_VARIANTS = 15;
constexpr int N_FAST = 4;       // two-contact fast variants [0, N_FAST), their safe variants N_FAST + (h > 10)
constexpr int V3_FAST = 6, V3_SAFE = 7;
// double support over more than ten steps (two contacts, 121 .. 240 reduced variables, h <= 20): 820 register blocks on 512
// threads, two each, one workgroup per CU; working set up to HMPC_QCAP_WIDE rows (what 160 KB of LDS leave room for).
constexpr int V2_WIDE = 8;
// QCAP = 0: working set as large as the variable count with the packed Schur inverse in GLOBAL memory (a scratch slice per
// workgroup; 231 KB for 240 variables -- more than a CU's LDS): the safe pass of the wide variant, and the second safe pass of
// the three-contact one (whose LDS-resident safe variant holds 140 of 180 possible rows)
constexpr int V2_WIDE_SAFE = 9, V3_SAFE_G = 10;
// the CONTINUATION variants of the 120-variable shapes (h <= 10, h <= 20): working set of HMPC_QCAP_CONT = 96 rows, 70 KB of LDS = two
// workgroups per CU; they take over -- state and all -- the solves whose working set outgrew the fast variants' 64 rows, run block
// rounds of up to 96 rows on them, and leave what outgrows them in turn (HMPC_S_WORKSET again) to the 120-row safe variants
constexpr int V2_CONT = 11;  // + (h > 10)
// command sweeps (hmpc_solve_command_sweep): a workgroup solves a chunk of instances that share state and gait on ONE
// inverse -- the 120-variable h <= 10 shape and the 60-variable (single support) one
constexpr int V2_SWEEP_120 = 13, V2_SWEEP_60 = 14;

// longest-first dispatch (hmpc_set_dispatch_order, on by default): only where a launch has a tail to shorten -- more instances
// than the ~512-1536 workgroup slots of the chip -- and not beyond what the one-workgroup sort handles in a few microseconds
constexpr int DISPATCH_ORDER_MIN_BATCH = 512, DISPATCH_ORDER_MAX_BATCH = 32768;
constexpr int REPAIR_GRID_CAP = 65536;  // workgroups of the device-side safe launch = most instances it can repair per solve (until round 6: 2 048; workgroups beyond the flagged count leave at once)
constexpr double SAFE_PASS_RELAX = 1e-6;  // first safe pass (device- and host-driven): bounds moved outward by this, exact re-solve + exact KKT check at its end
constexpr int SPILL_SLOT_CAP = 32768;   // hand-over slots per handle at most (101 KB each for 120 variables: 3.3 GB of the 288 GB); instances beyond it are re-solved cold
constexpr int EGLOBAL_CHUNK = 512;         // host-driven safe pass of the global-E variants: instances per launch (118 MB of scratch at 240 variables)
constexpr int DEVICE_REG_MIN_HORIZON = 10;  // device-side chain: the regularisation launches are enqueued for longer horizons only (device_reg_steps)
constexpr int REG_LIST_CAP = 256;  // device-side chain: instances per solve whose Hessian is not positive definite that get the regularisation launches (the rest: hmpc_resolve_failed)
constexpr int REPAIR_GRID_CAP_WIDE = 4096;  // ... of the wide variant's, whose safe pass keeps 231 KB per workgroup in global memory (0.95 GB of 288: the list mixes size classes, so a small cap could leave a wide instance behind 256 others unrepaired -- ADVICE round 5)

// ---------------------------------------------------------------------------------------------------- which variant
// Two-contact size classes: 0 = up to 60 reduced variables, 1 = up to 120, 2 = up to 240 (6 variables per stance leg-step; the class
// byte KernelArgs::cls counts leg-steps: [0, 10], [11, 20], [21, 255]).
constexpr int SIZE_CLASSES = 3;
inline constexpr int CLS_FIRST[SIZE_CLASSES] = {0, 11, 21}, CLS_LAST = 255;
inline int size_class(int n_reduced) { return n_reduced <= 60 ? 0 : (n_reduced <= HMPC_MAX_VARS ? 1 : 2); }

// the one map from (horizon beyond ten steps, size class) to the fast variant: <60,10> <120,10> <60,20> <120,20> are variants 0 .. 3,
// class 2 is the wide variant; a command sweep (h <= 10 only) runs the SWEEP variant of the class
inline int fast_variant(bool long_h, int cls, bool sweep = false) {
  if (sweep) return cls == 0 ? V2_SWEEP_60 : V2_SWEEP_120;
  return cls == 2 ? V2_WIDE : (long_h ? 2 : 0) + cls;
}

// the fast variant of a batch: the one that holds its widest reduced QP, max_stance (< 0: the host does not know it and plans for
// HMPC_MAX_VARS).  Of the variants that hold it this is the one with the smallest LDS footprint: smem grows with (NMAX, HMAX).
inline int pick_variant(int nc, int horizon, int max_stance) {
  if (nc == 3) return V3_FAST;
  const bool long_h = horizon > 10;
  const int cls = size_class(max_stance < 0 ? HMPC_MAX_VARS : max_stance);
  if (cls == 2 && !long_h) return N_FAST - 1;  // oversize batches are reported per instance (HMPC_S_TOO_LARGE)
  return fast_variant(long_h, cls);  // (class 2: double support beyond ten steps, the wide variant)
}

// the variant of a list launch of the continuation (role CONT) or the safe pass (SAFE): the safe variants hold a working set as
// large as the variable count -- for 240 variables only in global memory; ultimate = the three-contact safe pass's second level,
// whose working set cannot overflow either (global memory as well)
inline int repair_variant(Role role, int nc, int horizon, int max_stance, bool ultimate = false) {
  const int long_h = horizon > 10 ? 1 : 0;
  if (role == Role::CONT) return V2_CONT + long_h;
  if (pick_variant(nc, horizon, max_stance) == V2_WIDE) return V2_WIDE_SAFE;
  if (nc == 3) return ultimate ? V3_SAFE_G : V3_SAFE;
  return N_FAST + long_h;
}

// The size-class launches of a two-contact batch whose widest reduced QP only the device knows: every class of the family runs over
// the whole batch, a workgroup whose instance belongs to another one leaving at once.  Ordinary solves: classes 0, 1 (h <= 10, the
// second takes everything above ten leg-steps) or 0, 1, 2 (h > 10); command sweeps: the h <= 10 classes on the SWEEP variants.
struct ClassLaunch {
  int vi, lo, hi;  // variant, KernelArgs::cls_lo / cls_hi
};
inline int class_launches(bool sweep, bool long_h, ClassLaunch l[SIZE_CLASSES]) {
  const int n = (long_h && !sweep) ? 3 : 2;
  for (int k = 0; k < n; ++k) l[k] = {fast_variant(long_h, k, sweep), CLS_FIRST[k], k + 1 < n ? CLS_FIRST[k + 1] - 1 : CLS_LAST};
  return n;
}

// ---------------------------------------------------------------------------------------------------- the device-side lists
// the flagged list of the device-side chain: flag_list_cap entries, then REG_LIST_CAP more for the instances the safe launch ends as
// HMPC_S_INDEFINITE; the two counters sit next to each other (one memset clears both)
inline int flag_list_cap(int max_batch) { return max_batch < REPAIR_GRID_CAP ? max_batch : REPAIR_GRID_CAP; }
// workgroups of the chain's list launches: min(batch, REPAIR_GRID_CAP), fewer for the wide variant, whose safe pass keeps 231 KB of
// global scratch per workgroup; workgroups beyond the flagged count leave at once
inline int device_list_len(int batch, bool wide) {
  const int n = batch < REPAIR_GRID_CAP ? batch : REPAIR_GRID_CAP;
  return (wide && n > REPAIR_GRID_CAP_WIDE) ? REPAIR_GRID_CAP_WIDE : n;
}
inline int reg_list_len(int batch) { return batch < REG_LIST_CAP ? batch : REG_LIST_CAP; }

// longest-first dispatch: only where the tail of a launch matters (small and medium batches), and not for batches known to hold
// single-support QPs only: those solve in one or two iterations, there is nothing to sort and the extra launch costs a walking batch 1-4 %
inline bool orders_dispatch(int mode, bool have_buffers, int batch, int nc, int max_stance, bool external_qp) {
  const bool small_qps_only = nc == 2 && max_stance >= 0 && max_stance <= 60;
  return mode != 0 && have_buffers && batch > DISPATCH_ORDER_MIN_BATCH && batch <= DISPATCH_ORDER_MAX_BATCH && !small_qps_only && !external_qp;
}

// ---------------------------------------------------------------------------------------------------- what gets repaired
// an HMPC_S_MAXITER status is the CALLER's answer (not re-solved) exactly when the kernel says so: the caller's cap was the
// bound in force, i.e. the iteration count reached it (hmpc_kernel.h: `capped`; the variants' own bounds are 4 m + 16 and up)
inline bool capped_by_caller(int iter_cap, uint32_t status) {
  return iter_cap > 0 && (int)HMPC_STATUS_ITERS(status) >= iter_cap && (int)HMPC_STATUS_ITERS(status) <= iter_cap + 1;
}
// flagged: what a solve kernel leaves for a repair pass (and counts in KernelArgs::flagged) -- working set full, the variant's own
// iteration bound, infeasible, KKT check.  A solve that ran into the caller's own iteration cap (hmpc_set_max_iterations) is the
// caller's answer; one that hit the VARIANT's bound under a generous cap is re-solved like any other.
inline bool flagged(uint32_t status, int iter_cap) {
  const uint32_t c = HMPC_STATUS_CODE(status);
  return c == HMPC_S_WORKSET || (c == HMPC_S_MAXITER && !capped_by_caller(iter_cap, status)) || c == HMPC_S_INFEASIBLE || c == HMPC_S_KKT;
}
// needs_repair: what hmpc_resolve_failed takes up -- the flagged ones and HMPC_S_INDEFINITE, which only a SAFE variant's sweeps end an
// instance as (a device-side chain that left it there: short horizon, or a full regularisation list).  Its relaxed passes re-run what is
// still `flagged`: regularisation has had its turn by then.  A caller that looks at the status of a FAST launch alone (the legacy tick)
// may ask either: a fast variant never ends HMPC_S_INDEFINITE, it flags such a Hessian through its KKT check.
inline bool needs_repair(uint32_t status, int iter_cap) { return flagged(status, iter_cap) || HMPC_STATUS_CODE(status) == HMPC_S_INDEFINITE; }

inline bool params_ok(const hmpc_params &p) {
  auto pos = [](float v) { return v > 0.0f && v < 1e30f; };
  return pos(p.mass) && pos(p.inertia[0]) && pos(p.inertia[1]) && pos(p.inertia[2]) && pos(p.mu) && p.lt == p.lt && p.lh == p.lh &&
         p.gravity == p.gravity && fabsf(p.lt) < 1e30f && fabsf(p.lh) < 1e30f && fabsf(p.gravity) < 1e30f;
}

// ---------------------------------------------------------------------------------------------------- what is still valid
// Which results on the device belong to the CURRENT batch and its LAST solve.  Every result is a node of one graph, stated once as the
// table of each node's parents below; whatever replaces a node makes everything behind it stale.  Nothing outside this struct writes the
// facts.  (hmpc_resolve_failed repairs the solve in place and invalidates nothing; a bare launch that is no solve --
// hmpc_debug_phase_cycles without device repair -- does not count as one.)
enum class ResultNode : int { SOLVE, PREDICTION, SELECTION, MARGINS, CERTIFICATE, GAINS, FIRST_ORDER, ADJOINT, MODEL_ADJOINT, LIMIT_ADJOINT, RECORD_ADJOINT, ADJOINT_MULTI, ADJOINT_CHAIN, N };
constexpr int RESULT_NODES = (int)ResultNode::N, RESULT_MAX_PARENTS = 3;
// the parents of every node, in the order of ResultNode (N = none; the solve's parent is the batch itself: on_batch).  The record
// gradients read the adjoint, the model gradients and the limit gradients; the chain reads the multi-seed adjoint alone.
inline constexpr ResultNode RESULT_PARENTS[RESULT_NODES][RESULT_MAX_PARENTS] = {
    /* SOLVE */ {ResultNode::N, ResultNode::N, ResultNode::N},
    /* PREDICTION */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* SELECTION */ {ResultNode::PREDICTION, ResultNode::N, ResultNode::N},
    /* MARGINS */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* CERTIFICATE */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* GAINS */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* FIRST_ORDER */ {ResultNode::GAINS, ResultNode::N, ResultNode::N},
    /* ADJOINT */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* MODEL_ADJOINT */ {ResultNode::ADJOINT, ResultNode::N, ResultNode::N},
    /* LIMIT_ADJOINT */ {ResultNode::ADJOINT, ResultNode::N, ResultNode::N},
    /* RECORD_ADJOINT */ {ResultNode::ADJOINT, ResultNode::MODEL_ADJOINT, ResultNode::LIMIT_ADJOINT},
    /* ADJOINT_MULTI */ {ResultNode::SOLVE, ResultNode::N, ResultNode::N},
    /* ADJOINT_CHAIN */ {ResultNode::ADJOINT_MULTI, ResultNode::N, ResultNode::N},
};
constexpr uint32_t result_bit(ResultNode n) { return 1u << (int)n; }
constexpr bool result_behind(ResultNode d, ResultNode a) {  // d is a descendant of a (parents precede their children in ResultNode)
  for (int k = 0; k < RESULT_MAX_PARENTS; ++k) {
    const ResultNode p = RESULT_PARENTS[(int)d][k];
    if (p != ResultNode::N && (p == a || result_behind(p, a))) return true;
  }
  return false;
}
struct ResultDescendants {
  uint32_t of[RESULT_NODES];  // result_bit of every node behind node n
};
constexpr ResultDescendants result_descendants() {
  ResultDescendants t{};
  for (int a = 0; a < RESULT_NODES; ++a)
    for (int d = 0; d < RESULT_NODES; ++d)
      if (result_behind((ResultNode)d, (ResultNode)a)) t.of[a] |= 1u << d;
  return t;
}
inline constexpr ResultDescendants RESULT_BEHIND = result_descendants();  // (worked out by the compiler: a solve pays one AND for it)

class ResultState {
 public:
  // the three generic moves (hmpc_results.hip calls them with the node its family table names)
  bool has(ResultNode n) const { return (valid & result_bit(n)) != 0; }
  void set(ResultNode n) {  // n has been enqueued anew: it stands, whatever was made from the one before is stale
    invalidate(RESULT_BEHIND.of[(int)n]);
    valid |= result_bit(n);
    if (n == ResultNode::ADJOINT) adjoint_selected = -1;  // (a single launch; on_select_adjoint names its slice afterwards)
  }
  void retarget(ResultNode n) { invalidate(result_bit(n) | RESULT_BEHIND.of[(int)n]); }  // the caller moved n's buffers: whatever was computed went elsewhere

  void on_batch() { retarget(ResultNode::SOLVE); }  // the handle holds another batch
  void on_solve() { set(ResultNode::SOLVE); }       // every solve of a batch: its forces are newer than anything derived
  void on_predict() { set(ResultNode::PREDICTION); }
  void on_select(int groups) { set(ResultNode::SELECTION), select_groups = groups; }
  void on_margins() { set(ResultNode::MARGINS); }
  void on_certificate() { set(ResultNode::CERTIFICATE); }
  void on_gains() { set(ResultNode::GAINS); }
  void on_first_order() { set(ResultNode::FIRST_ORDER); }
  void on_adjoint() { set(ResultNode::ADJOINT); }  // (independent of the gains and the wrench)
  void on_model_adjoint() { set(ResultNode::MODEL_ADJOINT); }
  void on_limit_adjoint() { set(ResultNode::LIMIT_ADJOINT); }    // (independent of the model gradients)
  void on_record_adjoint() { set(ResultNode::RECORD_ADJOINT); }  // (the C entry point asks can_record_adjoint first)
  // A multi-seed adjoint is a node of its own behind the solve, in buffers of its own.  The CURRENT adjoint -- the parent of the model, limit
  // and record gradients -- is whichever came last of a single launch (on_adjoint) and a selected slice of the multi-seed one
  // (on_select_adjoint; the C entry point asks has_adjoint_multi and the range of s first).  A new multi-seed launch or new buffers for it
  // overwrite or move a selected slice, so a current adjoint that is a selection falls with them; one from a single launch does not.
  void on_adjoint_multi(int seeds) { set(ResultNode::ADJOINT_MULTI), adjoint_multi_seeds = seeds, drop_selection(); }
  void on_select_adjoint(int s) { set(ResultNode::ADJOINT), adjoint_selected = s; }
  // The chain of the multi-seed adjoint (hmpc_adjoint_chain_multi) is a node behind it alone, in buffers of its own: it reads the multi-seed
  // adjoint's slices where they stand and touches neither the current adjoint, a selection, nor the single-seed model, limit and record
  // nodes; none of those touches it.  (The C entry point asks has_adjoint_multi first.)
  void on_adjoint_chain() { set(ResultNode::ADJOINT_CHAIN); }
  void retarget_prediction() { retarget(ResultNode::PREDICTION); }
  void retarget_selection() { retarget(ResultNode::SELECTION); }
  void retarget_margins() { retarget(ResultNode::MARGINS); }
  void retarget_certificate() { retarget(ResultNode::CERTIFICATE); }
  void retarget_gains() { retarget(ResultNode::GAINS); }
  void retarget_first_order() { retarget(ResultNode::FIRST_ORDER); }
  void retarget_adjoint() { retarget(ResultNode::ADJOINT); }  // (a selection goes too: the current adjoint is gone either way)
  void retarget_adjoint_multi() { retarget(ResultNode::ADJOINT_MULTI), drop_selection(); }
  void retarget_adjoint_chain() { retarget(ResultNode::ADJOINT_CHAIN); }
  void retarget_model_adjoint() { retarget(ResultNode::MODEL_ADJOINT); }
  void retarget_limit_adjoint() { retarget(ResultNode::LIMIT_ADJOINT); }
  void retarget_record_adjoint() { retarget(ResultNode::RECORD_ADJOINT); }

  bool has_solve() const { return has(ResultNode::SOLVE); }              // a solve of the current batch has been enqueued
  bool has_prediction() const { return has(ResultNode::PREDICTION); }    // ... and a prediction behind it
  bool has_selection() const { return has(ResultNode::SELECTION); }      // ... and a selection behind that prediction
  bool has_margins() const { return has(ResultNode::MARGINS); }
  bool has_certificate() const { return has(ResultNode::CERTIFICATE); }
  bool has_gains() const { return has(ResultNode::GAINS); }
  bool has_first_order() const { return has(ResultNode::FIRST_ORDER); }  // ... a first-order wrench behind those gains
  bool has_adjoint() const { return has(ResultNode::ADJOINT); }          // the current adjoint: a single launch's or a selected slice
  bool has_model_adjoint() const { return has(ResultNode::MODEL_ADJOINT); }
  bool has_limit_adjoint() const { return has(ResultNode::LIMIT_ADJOINT); }
  // the record gradients are the one node with three parents: all three inputs must stand
  bool can_record_adjoint() const { return has(ResultNode::ADJOINT) && has(ResultNode::MODEL_ADJOINT) && has(ResultNode::LIMIT_ADJOINT); }
  bool has_record_adjoint() const { return has(ResultNode::RECORD_ADJOINT); }
  bool has_adjoint_multi() const { return has(ResultNode::ADJOINT_MULTI); }
  int adjoint_multi_seeds_enqueued() const { return has_adjoint_multi() ? adjoint_multi_seeds : 0; }  // ... and its seeds
  // a chain stands only as long as the multi-seed adjoint it was made from does (on_adjoint_chain does not ask)
  bool has_adjoint_chain() const { return has(ResultNode::ADJOINT_MULTI) && has(ResultNode::ADJOINT_CHAIN); }
  int selected_adjoint_seed() const { return has_adjoint() ? adjoint_selected : -1; }  // the slice the current adjoint is (-1: a single launch's, or none)
  int selected_groups() const { return has_selection() ? select_groups : 0; }  // groups of that selection

 private:
  uint32_t valid = 0;  // result_bit(n) of every node that stands
  int select_groups = 0, adjoint_multi_seeds = 0, adjoint_selected = -1;
  void invalidate(uint32_t nodes) {
    valid &= ~nodes;
    if (nodes & result_bit(ResultNode::ADJOINT)) adjoint_selected = -1;
  }
  // the selection rule: a current adjoint that is a slice of the multi-seed one goes when that slice is overwritten or moved
  void drop_selection() {
    if (adjoint_selected >= 0) retarget(ResultNode::ADJOINT);
  }
};

#pragma GCC visibility pop
