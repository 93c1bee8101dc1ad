// hmpc_launch.hip -- what a solve enqueues: one launch of a variant, the fast pass with its size classes, the repair steps over a list of
// flagged instances, the device-side chain that strings them together behind a solve or a command sweep, and the host-driven repair of
// hmpc_resolve_failed.  The decisions themselves (which variant, which classes, what is repaired) are hmpc_plan.h's.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>
#include <vector>

#include "hmpc_builder_launch.h"
#include "hmpc_front.h"
#include "hmpc_handle.h"
#include "hmpc_variants.h"

std::string &hip_error_text() {
  thread_local std::string text;
  return text;
}

const Variant *variants() {
#define HMPC_VARIANT_ENTRY(IDX, ...) hmpc_variant_##IDX(),
  static const Variant v[] = {HMPC_VARIANT_TABLE(HMPC_VARIANT_ENTRY)};
#undef HMPC_VARIANT_ENTRY
  static_assert(sizeof(v) / sizeof(v[0]) == N_VARIANTS, "hmpc_variants.h");
  return v;
}

int settle(hmpc_handle *h) {
  HIP_TRY(hipStreamSynchronize(h->last_stream));
  return HMPC_OK;
}

int enter_stream(hmpc_handle *h, hipStream_t stream) {
  if (stream == h->last_stream) return HMPC_OK;
  const int rc = settle(h);
  if (rc == HMPC_OK) h->last_stream = stream;
  return rc;
}

int scratch(hmpc_handle *h, size_t bytes, void **out) {
  HIP_TRY(h->d_scratch.reserve((bytes + 4095) & ~(size_t)4095, nullptr, /*whole_device=*/true));
  *out = h->d_scratch.get();
  return HMPC_OK;
}

void set_problem_args(const hmpc_handle *h, hmpc::KernelArgs &a) {
  a.records = h->d_records;
  a.stride = (int)h->stride;
  a.batch = h->batch;
  a.horizon = h->setup.horizon;
  a.dt = h->setup.dt;
  a.f_max = h->setup.f_max;
  a.forces = h->d_forces.get();
  a.inv_mass = 1.0f / h->params.mass;  // (binary32 division, correctly rounded: the value the reference's 1.f / 9.f folds to for the default)
  a.Ib[0] = h->params.inertia[0], a.Ib[1] = h->params.inertia[1], a.Ib[2] = h->params.inertia[2];
  a.mu = h->params.mu, a.lt = h->params.lt, a.lh = h->params.lh, a.gravity = h->params.gravity;
  a.mu_inst = h->d_mu_inst;
}

// One launch of variants()[vi].  A list launch of the CONTINUATION variant resumes the listed instances whose fast solve handed its
// state over (KernelArgs::resume = 2) and leaves every other one alone; where nothing can have been handed over it launches nothing.
int launch(hmpc_handle *h, hipStream_t stream, int vi, const LaunchOpt &o) {
  const Variant &v = variants()[vi];
  const int grid_all = o.assemble_only ? 1 : (o.d_index_list ? o.n_list : ((o.sweep_k > 0 && o.sweep_phase == 0) ? h->batch / o.sweep_k : h->batch));
  if (grid_all < 1) return HMPC_OK;
  // EGLOBAL variants keep NMAX (NMAX + 1) / 2 doubles of global scratch per WORKGROUP (231 KB for 240 variables): a host-driven
  // safe pass over thousands of flagged instances goes through the list in chunks that reuse one bounded buffer (stream order
  // keeps the chunks apart).  The device-driven pass (d_list_count) is one launch, capped by its caller.
  const int chunk = (v.e_global && o.d_index_list && !o.d_list_count && grid_all > EGLOBAL_CHUNK) ? EGLOBAL_CHUNK : grid_all;
  if (v.e_global)  // one slice of packed triangle per workgroup of this launch
    RC_TRY(grow(h, h->d_escratch, (size_t)chunk * ((size_t)v.nmax * (v.nmax + 1) / 2) * sizeof(double)));
  // hand-over slots: allocated on the first launch of a variant that saves its state (one slot per instance of the handle).
  // The per-instance slot table is written by EVERY ordinary launch of such a variant (-1 where nothing was saved), also when
  // saving itself is off for the launch, so that a later safe pass never meets an entry of an earlier batch.
  if (o.assemble_only && !v.assemble) return HMPC_E_ARG;
  if ((v.role == Role::SWEEP) != (o.sweep_k > 0)) return HMPC_E_ARG;
  const bool can_save = v.spill_stride > 0 && !o.assemble_only && !o.d_index_list;
  const bool saves = can_save && h->handover && !h->d_ext_H;
  if (can_save && !h->d_spill_slot.get()) {
    // filled on the launch's own stream, which is the stream that reads it next: no fill on the null stream, no wait on the host
    HIP_TRY(h->d_spill_slot.alloc((size_t)h->max_batch));
    const hipError_t e = hipMemsetAsync(h->d_spill_slot.get(), 0xff, (size_t)h->max_batch * sizeof(int), stream);
    if (e != hipSuccess) h->d_spill_slot.reset();  // (never a table that exists but was not filled)
    HIP_TRY(e);
  }
  if (saves && (!h->d_spill.get() || h->spill_stride < v.spill_stride)) {
    const int cap = h->max_batch < SPILL_SLOT_CAP ? h->max_batch : SPILL_SLOT_CAP;
    HIP_TRY(h->d_spill.reserve((size_t)cap * v.spill_stride, stream, /*whole_device=*/true));
    h->spill_stride = v.spill_stride, h->spill_cap = cap;
  }
  kernel_fn fn = o.assemble_only ? v.assemble : v.solve;
  if (!h->attrs_set[vi]) {
    HIP_TRY(hipFuncSetAttribute((const void *)v.solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.smem));
    if (v.assemble) HIP_TRY(hipFuncSetAttribute((const void *)v.assemble, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.smem));
    h->attrs_set[vi] = true;
  }
  hmpc::KernelArgs a;
  a.status = h->d_status.get();
  a.x64 = h->d_x64.get();
  a.obj64 = h->d_obj64.get();
  a.dbg_index = o.dbg_index;
  a.dbg_f = h->d_dbg_f.get();
  a.dbg_i = h->d_dbg_i.get();
  a.prof = h->d_prof.get();
  a.warm = (o.warm < 0) ? h->warm : o.warm;
  a.index_list = o.d_index_list;
  if (!o.d_index_list && !o.assemble_only && o.longest_first) a.index_list = h->d_order.get();
  a.wset = (h->tick_warm && !o.assemble_only && o.carry_wset) ? h->d_wset.get() : nullptr;
  a.flagged = h->d_flagged.get();
  a.wset_shift = h->tick_shift;
  a.relax = o.relax;
  a.flag_list = o.record_flagged ? h->d_flag_list.get() : nullptr;
  a.flag_count = o.record_flagged ? h->d_flag_count.get() : nullptr;
  a.flag_cap = o.record_flagged ? flag_list_cap(h->max_batch) : 0;
  a.list_count = o.d_list_count;
  a.ext_H = h->d_ext_H, a.ext_g = h->d_ext_g, a.ext_Fc = h->d_ext_Fc, a.ext_ld = h->ext_ld;
  a.iter_cap = h->iter_cap;
  a.cls = (o.cls_hi >= 0) ? h->d_cls.get() : nullptr;
  a.cls_lo = o.cls_lo, a.cls_hi = o.cls_hi;
  a.e_scratch = h->d_escratch.get();
  a.spill = nullptr, a.spill_stride = 0, a.spill_cap = 0, a.spill_slot = nullptr, a.resume = 0;
  if (can_save) {
    a.spill_slot = h->d_spill_slot.get();
    if (saves) a.spill = h->d_spill.get(), a.spill_stride = h->spill_stride, a.spill_cap = h->spill_cap;
  } else if (v.role == Role::CONT) {
    // nothing was handed over (hand-over off / no slots), or the pass is one that must not resume: nothing to do
    if (!o.d_index_list || !h->handover || !h->d_spill.get() || !h->d_spill_slot.get() || o.relax != 0.0 || h->d_ext_H) return HMPC_OK;
    a.spill = h->d_spill.get(), a.spill_stride = h->spill_stride, a.spill_cap = h->spill_cap, a.spill_slot = h->d_spill_slot.get();
    a.resume = 2;
  }
  a.skip_ok = o.skip_ok;
  if (o.d_index_list && !h->d_reg_rho.get()) HIP_TRY(h->d_reg_rho.alloc((size_t)h->max_batch));  // (safe variants: where a pivot that is not positive is left)
  a.reg_step = o.reg_step, a.reg_rho = h->d_reg_rho.get();
  a.reg_list = nullptr, a.reg_count = nullptr, a.reg_cap = 0;
  if (o.list_indefinite && h->d_flag_list.get() && h->d_flag_count.get())
    a.reg_list = h->d_flag_list.get() + flag_list_cap(h->max_batch), a.reg_count = h->d_flag_count.get() + 1, a.reg_cap = REG_LIST_CAP;
  a.sweep_k = o.sweep_k > 0 ? o.sweep_k : 1, a.sweep_phase = o.sweep_phase, a.sweep_m = h->d_sweep_m.get();
  // (never derived from "the buffer exists": only the caller that has just enqueued the prologue on this stream says so)
  a.front = (o.front_ready && v.reads_front && !o.assemble_only && !o.d_index_list && o.sweep_k == 0 && !h->d_ext_H)
                ? reinterpret_cast<const hmpc::FrontScalars *>(h->d_front.get()) : nullptr;
  set_problem_args(h, a);
  for (int off = 0; off < grid_all; off += chunk) {
    const int grid = (grid_all - off < chunk) ? grid_all - off : chunk;
    if (off > 0) a.index_list = o.d_index_list + off;  // (only list launches are ever chunked)
    hipLaunchKernelGGL(fn, dim3(grid), dim3(v.nt), v.smem, stream, a);
    HIP_TRY(hipGetLastError());
  }
  return HMPC_OK;
}

// Stages A1 / A2 of every instance of the batch in one launch ahead of the fast pass (front_scalars_kernel): a third small launch on the
// solve's stream next to the dispatch order's.  Two contacts only; not for the external QP, whose constraint block comes from outside.
int enqueue_front(hmpc_handle *h, hipStream_t stream, const int *vis, int n, bool *ready) {
  *ready = false;
  if (!h->front_prologue || h->nc != 2 || h->d_ext_H || h->batch < 1) return HMPC_OK;
  bool reads = false;
  for (int k = 0; k < n; ++k) reads = reads || variants()[vis[k]].reads_front;
  if (!reads) return HMPC_OK;
  RC_TRY(grow(h, h->d_front, (size_t)h->max_batch * sizeof(hmpc::FrontScalars)));
  hmpc::KernelArgs ka;
  memset(&ka, 0, sizeof(ka));
  set_problem_args(h, ka);  // (the very values the solve kernels assemble from)
  const hmpc::FrontArgs fa = {ka.records, ka.stride, ka.batch, ka.horizon, ka.dt, ka.f_max, {ka.Ib[0], ka.Ib[1], ka.Ib[2]}, ka.lt, ka.lh};
  HIP_TRY(hmpc::launch_front_scalars(fa, reinterpret_cast<hmpc::FrontScalars *>(h->d_front.get()), stream));
  *ready = true;
  return HMPC_OK;
}

// the size classes of a two-contact batch whose widest reduced QP only the device knows (records built on the device or handed in by
// pointer): every variant of the family runs over the whole batch, a workgroup whose instance belongs to another one leaving at once
static bool by_class(const hmpc_handle *h) { return h->nc == 2 && h->max_stance < 0 && h->d_cls.get(); }

// The fast pass of one solve: one launch of variant `vi` over the batch, or (by_class) the size-class launches --
// of class_launches (hmpc_plan.h).  A command sweep (o.sweep_k > 0; vi and the class variants are SWEEP variants) runs each launch in
// its two phases, the first of which lists nothing.
// The hand-over slot table must describe the CURRENT solve for the whole batch: the continuation pass resumes instance i from slot i
// when the table says i and the status word says "working set full" -- an entry an earlier batch left, met by a status word of this
// solve from a launch that does not rewrite the table (the 60-variable, wide, sweep and external-QP launches; the workgroups of a
// size-class launch that leave early), would continue the old QP's state against the new record.  So the table is cleared first,
// unless the solve is ONE launch of a saving variant, which rewrites every entry itself.
int enqueue_fast(hmpc_handle *h, hipStream_t stream, int vi, bool classes, LaunchOpt o) {
  const bool sweep = o.sweep_k > 0;
  ClassLaunch l[SIZE_CLASSES] = {{vi, 0, -1}};
  const int n = classes ? class_launches(sweep, h->setup.horizon > 10, l) : 1;
  if ((n > 1 || variants()[l[0].vi].spill_stride == 0) && h->d_spill_slot.get() && h->batch > 0)
    HIP_TRY(hipMemsetAsync(h->d_spill_slot.get(), 0xff, (size_t)h->batch * sizeof(int), stream));
  if (classes && !h->cls_valid)
    HIP_TRY(hmpc::launch_classify_records(h->d_records, (int)h->stride, h->batch, h->setup.horizon, h->setup.f_max, h->d_cls.get(), stream));
  o.front_ready = false;
  if (!sweep) {  // (the SWEEP variants run the two stages themselves)
    int vis[SIZE_CLASSES];
    for (int k = 0; k < n; ++k) vis[k] = l[k].vi;
    RC_TRY(enqueue_front(h, stream, vis, n, &o.front_ready));
  }
  const bool record_flagged = o.record_flagged;
  for (int k = 0; k < n; ++k) {
    o.cls_lo = l[k].lo, o.cls_hi = l[k].hi;
    if (sweep) {
      o.sweep_phase = 0, o.record_flagged = false;
      const int rc = launch(h, stream, l[k].vi, o);
      if (rc != HMPC_OK) return rc;
      o.sweep_phase = 1, o.record_flagged = record_flagged;
    }
    const int rc = launch(h, stream, l[k].vi, o);
    if (rc != HMPC_OK) return rc;
  }
  h->results.on_solve();  // (every solve of a batch starts here)
  return HMPC_OK;
}

// The repair steps over a list of flagged instances (the device-side chain's list, trimmed on the device by its counter, or a list
// the host uploaded), in the order each chain calls them.
// (1) continuation: instances whose working set outgrew the fast variant go on, from the state it handed over, on the variant with
//     96 rows and block rounds of its own (two per CU).  *taken = whether the step applies (the safe pass behind it then leaves
//     alone what it solved), also when the launch finds nothing to resume.
static int continuation_pass(hmpc_handle *h, hipStream_t stream, const LaunchOpt &s, bool *taken) {
  *taken = h->nc == 2 && h->handover && h->d_spill.get();
  return *taken ? launch(h, stream, repair_variant(Role::CONT, h->nc, h->setup.horizon, h->max_stance), s) : HMPC_OK;
}

// (2) the safe pass.  Where the host knows the batch's widest reduced QP (or the family has one safe variant) that is one launch.  A
// two-contact batch at h > 10 whose sizes only the DEVICE knows (by_class) may hold both <= 120-variable instances and double-support
// ones with up to 240: the list is then run twice, once per safe variant, each workgroup leaving at once unless its instance's size
// class belongs to the variant -- a wide instance must never reach the 120-variable kernel (it would end as HMPC_S_TOO_LARGE with zero
// forces, which nothing re-solves).
static int safe_pass(hmpc_handle *h, hipStream_t stream, LaunchOpt s, bool ultimate = false) {
  if (!by_class(h) || h->setup.horizon <= 10) return launch(h, stream, repair_variant(Role::SAFE, h->nc, h->setup.horizon, h->max_stance, ultimate), s);
  s.cls_lo = 0, s.cls_hi = CLS_FIRST[2] - 1;
  const int rc = launch(h, stream, N_FAST + 1, s);
  if (rc != HMPC_OK) return rc;
  s.cls_lo = CLS_FIRST[2], s.cls_hi = CLS_LAST;
  if (s.d_list_count && s.n_list > REPAIR_GRID_CAP_WIDE) s.n_list = REPAIR_GRID_CAP_WIDE;  // (one launch: bounded scratch)
  return launch(h, stream, V2_WIDE_SAFE, s);
}

// (3) instances whose Hessian is not positive definite (the safe variants' sweeps found a pivot <= 0 and ended them as
// HMPC_S_INDEFINITE) get the reference's two regularised QPs (KernelArgs::reg_step): H + rho I, then one more QP with the gradient
// g - rho x_1 (QProblem.cpp:1753-1860, QProblemB.cpp:1999-2031)
static int reg_steps(hmpc_handle *h, hipStream_t stream, LaunchOpt s) {
  s.relax = 0.0, s.warm = 1, s.skip_ok = 0, s.list_indefinite = false;
  for (int step = 1; step <= 2; ++step) {
    s.reg_step = step;
    const int rc = safe_pass(h, stream, s);
    if (rc != HMPC_OK) return rc;
  }
  return HMPC_OK;
}

// the device-side chain's list: what the fast launches flagged
static LaunchOpt device_list(const hmpc_handle *h) {
  LaunchOpt s;
  s.d_index_list = h->d_flag_list.get();
  s.d_list_count = h->d_flag_count.get();
  s.n_list = device_list_len(h->batch, pick_variant(h) == V2_WIDE);
  return s;
}

// The device-side chain's regularisation steps run over a short list of their own (REG_LIST_CAP entries, its counter next to the
// flagged counter, filled by the safe launch), so the two launches are a few hundred workgroups that leave at once when it is empty.
// Two launches = ~4 us of dispatch latency per solve even when their list is empty (scripts/dev/chain_overhead.py: the whole chain
// 11 -> 15 us at b8192, 6 -> 10 us at b1024), so only where such Hessians occur: horizons beyond 10 steps (binary32 round-off in H
// grows with the horizon; 107 of 4 096 double-support h = 20 instances at 10x the input ranges, none in any h <= 10 stress row up to
// 10x -- 20 000 instances).  A shorter-horizon handle would leave such an instance HMPC_S_INDEFINITE for hmpc_resolve_failed.
static int device_reg_steps(hmpc_handle *h, hipStream_t stream, LaunchOpt s) {
  if (h->setup.horizon <= DEVICE_REG_MIN_HORIZON) return HMPC_OK;
  s.d_index_list = h->d_flag_list.get() + flag_list_cap(h->max_batch);
  s.d_list_count = h->d_flag_count.get() + 1;
  s.n_list = reg_list_len(h->batch);
  return reg_steps(h, stream, s);
}

// The dispatch order of the solve about to be enqueued (LaunchOpt::longest_first).  Keyed by the iteration counts of the previous solve
// when that was of a batch of this size (the caller's contract: instance i of this tick is instance i of the last one); otherwise -- a
// cold handle, another batch size, mode 2 -- by the cost predicted from the records themselves (predicted_cost_bucket: no previous solve needed)
static int enqueue_dispatch_order(hmpc_handle *h, hipStream_t stream) {
  const bool from_previous = h->dispatch_order == 1 && h->order_batch == h->batch;
  if (!from_previous) {
    if (!h->d_keys.get()) HIP_TRY(h->d_keys.alloc((size_t)h->max_batch));
    HIP_TRY(hmpc::launch_predicted_cost(h->d_records, (int)h->stride, h->batch, h->setup.horizon, h->nc, h->d_keys.get(), stream));
  }
  HIP_TRY(hmpc::launch_dispatch_order(h->d_status.get(), h->batch, h->d_order.get(), from_previous ? nullptr : h->d_keys.get(), stream));
  return HMPC_OK;
}

// The device-side chain (hmpc_set_device_repair): the fast launches of variant `vi` with the options `o` list what they flag, the repair
// steps follow over that list (trimmed on the device by the counter: workgroups beyond it leave at once) -- no host round trip.  One
// stream per handle at a time: the list and its counter belong to the handle, two solves of one handle in flight on two streams would
// race on them.  Without device repair it is the fast launches alone.
//  * continuation: the instances whose working set the fast variant handed over go on first, with the block start (what differs from the
//    fast variant is capacity, periodic rebuild of E, in-kernel perturbation); the safe pass then leaves alone what that solved;
//  * relax_safe: the safe pass starts with every bound moved outward by SAFE_PASS_RELAX (1 + frac(0.618 row)).  What reaches it are the
//    instances that cycle at degenerate vertices (the continuation's budget, a KKT check): perturbed, they take ~150 iterations instead
//    of up to 480, and the kernel's epilogue re-solves on the final working set with the EXACT bounds and repeats the exact KKT check --
//    measured at 6x the input ranges: 8.8 -> 6.9 ms for the whole chain AND 3 -> 0 of 8 192 left flagged (10x: 19.5 -> 14.6 ms,
//    10 -> 1); every one of them HMPC_S_OK, exact (profiles/r06/range_scale.txt).  The safe pass is cold either way;
//  * mode2_stops: under device-repair mode 2 the chain ends behind the continuation, the safe pass is left to hmpc_resolve_failed /
//    hmpc_download.
static int enqueue_chain(hmpc_handle *h, hipStream_t stream, int vi, LaunchOpt o, bool continuation, bool relax_safe, bool mode2_stops) {
  const bool repair = h->device_repair != 0;
  if (repair) HIP_TRY(hipMemsetAsync(h->d_flag_count.get(), 0, 2 * sizeof(unsigned int), stream));
  h->order_valid = false;
  if (o.longest_first) {
    const int rc = enqueue_dispatch_order(h, stream);
    if (rc != HMPC_OK) return rc;
    h->order_valid = true;
  }
  h->order_batch = o.sweep_k > 0 ? 0 : h->batch;  // (natural order inside a sweep; the next ordinary solve starts from the predictor)
  o.record_flagged = repair;
  int rc = enqueue_fast(h, stream, vi, by_class(h), o);
  if (rc != HMPC_OK || !repair) return rc;
  LaunchOpt s = device_list(h);
  s.carry_wset = o.carry_wset;
  if (continuation) {
    s.warm = 1;
    bool cont = false;
    rc = continuation_pass(h, stream, s, &cont);
    if (rc != HMPC_OK) return rc;
    if (cont) s.skip_ok = 1;
  }
  if (mode2_stops && h->device_repair == 2) return HMPC_OK;
  s.relax = relax_safe ? SAFE_PASS_RELAX : 0.0, s.warm = 0, s.list_indefinite = true;
  rc = safe_pass(h, stream, s);
  if (rc != HMPC_OK) return rc;
  return device_reg_steps(h, stream, s);
}

// One solve of the current batch, enqueued on `stream` -- what hmpc_solve does and what hmpc_time_solve times:
//  * widest reduced QP known (host-uploaded records, or hmpc_set_max_reduced_vars >= 0): one launch of the variant
//    that holds it;
//  * unknown (records built on the device or handed in by device pointer; two contacts): the instances' size classes are
//    on the device (from the record builder, else counted here from the gait bytes) and EVERY variant of the family is
//    launched over the whole batch -- a workgroup whose instance belongs to another variant leaves at once -- so that a
//    walking sweep built on the device runs on the 60-variable kernel without the host ever seeing a gait table;
//  * device repair: the whole chain -- continuation, then the relaxed safe pass unless mode 2 leaves that to the host.
int enqueue_solve(hmpc_handle *h, hipStream_t stream, bool carry_wset) {
  LaunchOpt o;
  o.carry_wset = carry_wset;
  o.longest_first = orders_dispatch(h->dispatch_order, h->d_order.get() != nullptr, h->batch, h->nc, h->max_stance, h->d_ext_H != nullptr);
  return enqueue_chain(h, stream, pick_variant(h), o, /*continuation=*/true, /*relax_safe=*/true, /*mode2_stops=*/true);
}

// Command sweeps (the SWEEP variants): phase 0 forms every group's M = H^-1 once (one workgroup per group) and leaves it in HBM, phase 1
// solves every instance with its group's M (one workgroup per instance, stages H and S skipped).
int enqueue_command_sweep(hmpc_handle *h, hipStream_t stream, int group_size) {
  // single-support sweeps (max_stance <= 60): the 60-variable kernel (six workgroups per CU).  Records whose sizes only the device
  // knows (max_stance < 0): every group runs on the sweep variant of its size class, the one hmpc_solve's size-class launches give its
  // instances -- what keeps the results the bits of hmpc_solve's (a member whose gait differs from its group's first record's may
  // land in the other launch: it is reported there, never solved)
  const bool small = h->max_stance >= 0 && h->max_stance <= 60;
  const int vi = fast_variant(/*long_h=*/false, small ? 0 : 1, /*sweep=*/true);
  const size_t need = (size_t)(h->batch / group_size) * 36 * (size_t)variants()[vi].nt * sizeof(double);  // (V2_SWEEP_120 has the wider workgroups)
  RC_TRY(grow(h, h->d_sweep_m, need));
  LaunchOpt o;
  o.sweep_k = group_size;  // (natural order inside a sweep)
  // whatever a sweep flags is repaired as an independent instance (its record is complete).  Sweeps save nothing: no continuation; their
  // safe pass is cold and EXACT; and it runs under device-repair mode 2 as well (nothing else would repair a sweep on the device)
  return enqueue_chain(h, stream, vi, o, /*continuation=*/false, /*relax_safe=*/false, /*mode2_stops=*/false);
}

// The host-driven repair: the status words come to the host, what needs_repair (hmpc_plan.h) is re-solved over an uploaded list with the
// same steps as the device-side chain's, then the steps only the host drives.  It repairs the solve in place: no result is invalidated.
int resolve_failed(hmpc_handle *h, int *n_resolved) {
  int src = settle(h);
  if (src != HMPC_OK) return src;
  std::vector<uint32_t> st(h->batch);
  HIP_TRY(hipMemcpy(st.data(), h->d_status.get(), (size_t)h->batch * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<int> idx;
  for (int i = 0; i < h->batch; ++i)
    if (needs_repair(st[i], h->iter_cap)) idx.push_back(i);
  if (idx.empty()) return HMPC_OK;
  int *d_idx = nullptr;  // lives in the handle's scratch: nothing to free on the error paths below
  {
    void *sp = nullptr;
    const int rc = scratch(h, idx.size() * sizeof(int), &sp);
    if (rc != HMPC_OK) return rc;
    d_idx = (int *)sp;
  }
  HIP_TRY(hipMemcpy(d_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
  // (launch parameters; the handle's own warm-start setting is not touched)
  LaunchOpt so;
  so.d_index_list = d_idx, so.n_list = (int)idx.size(), so.warm = 1;  // (first pass: with the block start; the perturbed passes below start cold)
  bool cont = false;
  int rc = continuation_pass(h, h->last_stream, so, &cont);
  if (rc != HMPC_OK) return rc;
  if (cont) so.skip_ok = 1;
  // (the same launch as the device-side chain's: cold, bounds perturbed by SAFE_PASS_RELAX, exact re-solve at its end -- see enqueue_solve)
  so.relax = SAFE_PASS_RELAX, so.warm = 0;
  rc = safe_pass(h, h->last_stream, so);
  if (rc != HMPC_OK) return rc;
  // ... then, for what is still flagged, the exact pass with the block start (the first safe pass of rounds 4-6a)
  so.relax = 0.0, so.warm = 1, so.skip_ok = 2;  // (an answer that is only ok-relaxed gets the exact attempt as well)
  rc = safe_pass(h, h->last_stream, so);
  so.skip_ok = 0;
  if (rc != HMPC_OK) return rc;
  if ((src = settle(h)) != HMPC_OK) return src;
  if (n_resolved) *n_resolved = (int)idx.size();
  // each later pass: copy the status words back, keep the members of idx whose code `keep` accepts, upload them, run `pass` over
  // them (a copy of `so` with that list), synchronise; *ran = whether anything was kept
  auto rerun = [&](auto keep, auto pass, bool *ran) -> int {
    std::vector<int> sub;
    HIP_TRY(hipMemcpy(st.data(), h->d_status.get(), (size_t)h->batch * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i : idx)
      if (keep(st[i])) sub.push_back(i);
    *ran = !sub.empty();
    if (sub.empty()) return HMPC_OK;
    HIP_TRY(hipMemcpy(d_idx, sub.data(), sub.size() * sizeof(int), hipMemcpyHostToDevice));
    LaunchOpt o = so;
    o.n_list = (int)sub.size();
    const int prc = pass(o);
    return prc != HMPC_OK ? prc : settle(h);
  };
  bool ran = false;
  // A Hessian that is not positive definite (found by the safe variants' sweeps: HMPC_S_INDEFINITE; the fast variants diverge on it
  // and flag it through their KKT check): the reference's qpOASES run regularises, and so do two more launches here
  rc = rerun([](uint32_t w) { return HMPC_STATUS_CODE(w) == HMPC_S_INDEFINITE; },
             [&](const LaunchOpt &o) { return reg_steps(h, h->last_stream, o); }, &ran);
  if (rc != HMPC_OK) return rc;
  // last resort for instances that cycle at a degenerate vertex even with the full-size working set: bounds moved outward
  // by 1e-7, 1e-6, then 1e-5 (a different amount per row), reported as HMPC_S_OK_RELAXED.  For three contacts first a second level:
  // instances whose working set outgrew even the LDS-resident safe variant (140 of 180 rows); once that has run, the relax levels
  // run on the same variant (ultimate)
  bool ultimate = false;
  if (h->nc == 3) {
    rc = rerun([](uint32_t w) { return HMPC_STATUS_CODE(w) == HMPC_S_WORKSET; },
               [&](const LaunchOpt &o) { return safe_pass(h, h->last_stream, o, /*ultimate=*/true); }, &ultimate);
    if (rc != HMPC_OK) return rc;
  }
  // (with the exact re-solve that ends a relaxed pass -- see the kernel -- a larger perturbation costs nothing when its working
  //  set turns out to be optimal for the exact bounds: such an instance is reported HMPC_S_OK, exact)
  for (const double relax : {1e-7, 1e-6, 1e-5}) {
    rc = rerun(
        [&](uint32_t w) { return flagged(w, h->iter_cap); },
        [&](LaunchOpt o) {
          o.relax = relax, o.warm = 0;
          return safe_pass(h, h->last_stream, o, ultimate);
        },
        &ran);
    if (rc != HMPC_OK || !ran) return rc;
  }
  return HMPC_OK;
}
