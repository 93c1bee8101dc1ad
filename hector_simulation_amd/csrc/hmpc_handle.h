// hmpc_handle.h -- what the host units of libhector_mpc_hip.so share and nobody outside sees: the handle, the error string, the options
// of one launch, and what hmpc_launch.hip (what a solve enqueues) offers hmpc_capi.hip (the batched C ABI) and hmpc_results.hip (the results
// derived from a solve).  Everything here is hidden.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/hector_mpc.h"
#include "hmpc_device_buffer.h"
#include "hmpc_kernel_args.h"
#include "hmpc_certificate.h"
#include "hmpc_feedback.h"
#include "hmpc_adjoint.h"
#include "hmpc_adjoint_multi.h"
#include "hmpc_adjoint_chain.h"
#include "hmpc_model_adjoint.h"
#include "hmpc_limit_adjoint.h"
#include "hmpc_pose_adjoint.h"
#include "hmpc_margins.h"
#include "hmpc_plan.h"
#include "hmpc_results.h"

#pragma GCC visibility push(hidden)

std::string &hip_error_text();  // what hmpc_last_hip_error reports: per thread (hmpc_launch.hip)

#define HIP_TRY(expr)                                                                                    \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) {                                                                              \
      hip_error_text() = std::string(#expr) + ": " + hipGetErrorString(_e);                              \
      return HMPC_E_HIP;                                                                                 \
    }                                                                                                    \
  } while (0)

#define RC_TRY(expr)                       \
  do {                                     \
    const int _rc = (expr);                \
    if (_rc != HMPC_OK) return _rc;        \
  } while (0)

struct hmpc_handle {  // (opaque to callers: its constructor and destructor are not exported)
  problem_setup setup{};
  int nc = 2;  // contacts per horizon step: 2 (reference) or 3 (hand-contact extension)
  int max_batch = 0, device = 0, batch = 0;
  size_t stride = 0;
  DeviceBuffer<unsigned char> d_record_store;    // the handle's own records (uploads, the record builder)
  const unsigned char *d_records = nullptr;      // the current batch's: d_record_store, or the caller's (hmpc_set_device_records)
  OutputBuffer<float> d_forces;                  // the caller's, hmpc_set_device_outputs, else the handle's own (allocated at create)
  OutputBuffer<uint32_t> d_status;
  DeviceBuffer<double> d_x64, d_obj64;
  DeviceBuffer<float> d_dbg_f;
  DeviceBuffer<int> d_dbg_i;
  DeviceBuffer<long long> d_prof;
  int warm = 1;    // block warm start of the working set (default on)
  DeviceBuffer<signed char> d_wset;  // working sets carried from tick to tick (hmpc_set_tick_warm_start), [max_batch][8 nc h]
  int tick_warm = 0, tick_shift = 0;
  int auto_resolve = 1;  // hmpc_download re-solves flagged instances with the safe variant (default on)
  int max_stance = -1;  // max reduced variables of the current batch (known only for host-uploaded records; else -1)
  hipStream_t last_stream = nullptr;  // the stream of the last enqueued call: moved by enter_stream, waited for by settle, by nothing else
  bool attrs_set[N_VARIANTS] = {};
  // persistent device scratch for the host-pointer convenience entry points (grown on demand): no allocation per call and nothing to
  // leak on an early error return
  DeviceBuffer<unsigned char> d_scratch;
  // number of instances the solve kernels have flagged (working set full / max-iter / infeasible / KKT) since the handle
  // was created; monotonically increasing device counter, hmpc_download compares it with the value it saw last and
  // skips the status scan of the safe pass when nothing new was flagged
  DeviceBuffer<unsigned int> d_flagged;
  unsigned int flagged_seen = 0;
  // device-side safe pass (hmpc_set_device_repair): list of the instances the last fast launch flagged + its counter
  int device_repair = 0;
  DeviceBuffer<int> d_flag_list;
  DeviceBuffer<unsigned int> d_flag_count;
  // parity hook (hmpc_debug_solve_external_qp): device copies of caller-supplied QP data, only set during that call
  const float *d_ext_H = nullptr, *d_ext_g = nullptr, *d_ext_Fc = nullptr;
  int ext_ld = 0;
  int iter_cap = 0;  // hmpc_set_max_iterations: cap on the active-set iterations of every solve (0 = the variant's own bound)
  // hmpc_set_dispatch_order: 1 = workgroups take the instances longest-previous-solve first (d_order, rebuilt at the head of
  // every solve from the status words the previous solve of a batch of the same size left; order_batch = that size, 0 = none)
  int dispatch_order = 1, order_batch = 0;
  bool order_valid = false;
  DeviceBuffer<int> d_order;
  DeviceBuffer<unsigned char> d_keys;  // predicted cost bucket per instance (cold-handle order), allocated on first use
  // size classes of a device-resident batch whose widest reduced QP the host was not told (hmpc_set_max_reduced_vars < 0):
  // stance leg-steps per instance, written on the device by the record builder (cls_valid) or, for records handed in by
  // pointer, by classify_records_kernel at the head of every solve
  DeviceBuffer<unsigned char> d_cls;
  int cls_valid = 0;
  // packed Schur inverses of the EGLOBAL safe variants: [e_slices][nmax (nmax + 1) / 2] doubles, grown on demand
  DeviceBuffer<double> d_escratch;
  // hand-over of full working sets (KernelArgs::spill): one slot per instance (slot = instance index), allocated on the first
  // launch of a variant that saves its state; spill_stride = bytes per slot of the allocation, spill_cap = slots
  DeviceBuffer<unsigned char> d_spill;
  DeviceBuffer<int> d_spill_slot;
  size_t spill_stride = 0;
  int spill_cap = 0;
  int handover = 1;  // hmpc_set_handover (default on)
  hmpc_params params{};  // robot / contact constants (hmpc_set_params; defaults = the reference's literals)
  const float *d_mu_inst = nullptr;  // hmpc_set_instance_mu: per-instance friction parameter in HBM (caller-owned), nullptr = params.mu for all
  DeviceBuffer<double> d_reg_rho;  // Hessians that are not positive definite: the pivot the safe variant found, then rho of hmpc_resolve_failed's regularisation steps, per instance (allocated with the first list launch)
  ResultState results;  // which of the derived results belong to the current batch and its last solve (hmpc_plan.h)
  // The results derived from a solve (hmpc_results.hip).  Their families, arrays and shapes are the table of hmpc_results.h and stated
  // nowhere else; d_result[family][k] is array k of a family of [0, N_SINGLE): the caller's buffer (hmpc_set_device_<family>) or the
  // handle's own, allocated for max_batch rows by the first call that needs it.
  OutputBuffer<unsigned char> d_result[hmpc::N_SINGLE][hmpc::MAX_SINGLE_ARRAYS];
  // hmpc_set_sweep_margin_floor: hmpc_tick_sweep_device masks the commands whose margins miss the floor (penalty: scratch of the handle)
  bool sweep_floor_on = false;
  double sweep_floor[hmpc::MARGIN_CLASSES] = {};
  DeviceBuffer<double> d_sweep_penalty;
  double cert_act_tol = 1e-3;  // hmpc_set_certificate_tolerance
  // hmpc_set_sweep_certificate_ceiling: hmpc_tick_sweep_device masks the commands whose certificate exceeds the ceiling (same scratch)
  bool sweep_ceil_on = false;
  double sweep_ceil[hmpc::CERT_CEILS] = {};
  // multi-seed adjoint (hmpc_solve_adjoint_multi): the arrays of the adjoint once per seed, seed-major over the CURRENT batch
  // ([n_seeds][batch][...]); to the caller's buffers (hmpc_set_device_adjoint_multi, room for adjm_caller_seeds slices) or the handle's
  // own, reserved for (n_seeds, max_batch) by the launch that needs them (adjm_own_seeds = what they hold room for)
  DeviceBuffer<double> d_adjm_own[hmpc::ADJOINT_ARRAYS];
  double *adjm_caller[hmpc::ADJOINT_ARRAYS] = {};
  int adjm_caller_seeds = 0, adjm_own_seeds = 0;
  // chain of the multi-seed adjoint (hmpc_adjoint_chain_multi): the arrays of struct hmpc_adjoint_chain in its member order, seed-major
  // over the CURRENT batch; the compact ones to the caller's buffers (hmpc_set_device_adjoint_chain_multi, room for chain_caller_seeds
  // slices) or the handle's own, reserved for (n_seeds, max_batch) by the launch that needs them (chain_own_seeds = what they hold room
  // for); the detail ones to the caller's buffers only.  chain_written = the arrays the chain that stands wrote.
  DeviceBuffer<double> d_chain_own[hmpc::CHAIN_COMPACT];
  double *chain_caller[hmpc::CHAIN_ARRAYS] = {};
  int chain_caller_seeds = 0, chain_own_seeds = 0;
  bool chain_written[hmpc::CHAIN_ARRAYS] = {};
  // closed loop (hmpc_rollout_device, hmpc_plant.hip): a tick's clamped world_position_desired [max_batch][2] and torques [max_batch][10]
  // between its solve and its plant step; the handle's own log buffers, for max_batch x roll_own_ticks rows (hmpc_get_device_rollout);
  // the caller's (hmpc_set_device_rollout); and where the last rollout logged, which is what hmpc_download_rollout copies
  DeviceBuffer<double> d_roll_wpd, d_roll_tau, d_roll_state, d_roll_taulog;
  DeviceBuffer<float> d_roll_wrench;
  DeviceBuffer<uint32_t> d_roll_status;
  DeviceBuffer<int32_t> d_roll_summary;
  int roll_own_ticks = 0;
  hmpc_rollout_log roll_caller{}, roll_last{};
  int roll_last_batch = 0, roll_last_ticks = 0;
  // closed-loop command sweeps (hmpc_rollout_sweep_device, hmpc_rollout_score.hip): the expanded ticks the rollout advances and their copy
  // from before it (each hmpc_tick_inputs[max_batch]: not the shared scratch, they outlive n solves), cost [max_batch][4] and score
  // [max_batch]; allocated by the first sweep.  rsw_batch = the instances of the last sweep (0: none yet).  rscore_batch, rscore_ticks =
  // the shape of the log hmpc_rollout_score_device scored last (what hmpc_rollout_select_device takes a caller's log to have)
  DeviceBuffer<unsigned char> d_rsw_ticks, d_rsw_ticks0;
  DeviceBuffer<double> d_rsw_cost, d_rsw_score;
  int rsw_batch = 0, rscore_batch = 0, rscore_ticks = 0;
  // swing legs in a rollout (hmpc_set_rollout_swing, hmpc_swing.hip): the constants, copied; the caller's state [batch] and command log
  // [batch][n_ticks] (may be nullptr).  swing_on = false: a rollout enqueues nothing for them.
  bool swing_on = false;
  hmpc_swing swing_cfg{};
  hmpc_swing_state *swing_state = nullptr;
  hmpc_motor_cmd *swing_cmd_log = nullptr;
  // stages A1 / A2 ahead of the fast two-contact launches (front_scalars_kernel, hmpc_front.hip): one FrontScalars block per instance,
  // [max_batch], allocated by the first solve that enqueues the prologue.  Written and read inside ONE enqueue on one stream
  // (enqueue_front, then the launches whose LaunchOpt says front_ready): no later call reads it, so no block can be stale.
  DeviceBuffer<unsigned char> d_front;
  int front_prologue = 1;  // hmpc_debug_set_front_prologue: 0 = every launch runs the two stages in the kernel
  DeviceBuffer<double> d_sweep_m;  // command sweeps: every group's M = H^-1, [groups][36][threads per workgroup] doubles (grown on demand)
};

// the fast variant of the handle's batch (the only place a handle is mapped to a fast variant)
inline int pick_variant(const hmpc_handle *h) { return pick_variant(h->nc, h->setup.horizon, h->max_stance); }

struct LaunchOpt {
  bool assemble_only = false;
  int dbg_index = 0;
  const int *d_index_list = nullptr;  // workgroup b solves instance d_index_list[b] (the repair passes over flagged instances)
  int n_list = 0;
  double relax = 0.0;
  int warm = -1;           // -1 = the handle's setting, 0/1 = override for this launch (the safe pass chooses per pass without touching the handle)
  bool carry_wset = true;  // false keeps a repeated launch of the same batch from consuming/advancing the tick-to-tick working sets
  const unsigned int *d_list_count = nullptr;
  bool record_flagged = false;
  bool longest_first = false;  // workgroup b takes instance h->d_order.get()[b] (enqueue_solve, hmpc_set_dispatch_order)
  int cls_lo = 0, cls_hi = -1;  // cls_hi >= 0: only instances whose size class lies in [cls_lo, cls_hi] (h->d_cls.get())
  int skip_ok = 0;         // list launch: instances an earlier pass over the same list solved are left alone (1: ok / ok-relaxed, 2: ok only)
  int sweep_k = 0, sweep_phase = 0;  // command sweep: group size; phase 0 = one workgroup per group forms M, 1 = one per instance solves with it (a SWEEP variant)
  bool list_indefinite = false;  // device-side chain, safe launch: instances ended as HMPC_S_INDEFINITE are appended to the handle's short list
  bool front_ready = false;  // the caller has just enqueued the prologue for the whole batch on this stream (enqueue_front): a variant that reads it gets KernelArgs::front
  int reg_step = 0;        // safe pass over an index list: regularisation step 1 / 2 for instances whose Hessian is not positive definite (KernelArgs::reg_step)
};

// ---- hmpc_launch.hip
const Variant *variants();  // [N_VARIANTS], in the order of HMPC_VARIANT_TABLE
// THE STREAM RULE (include/hector_mpc.h, "Streams"), kept by settle and enter_stream and by nothing else: no
// other line of the library decides to wait for h->last_stream, and none assigns it.
//  * settle: the host is about to write, read, free or reallocate device memory of the handle: waits until everything enqueued for the
//    handle has finished.
//  * enter_stream: the call enqueues on `stream`.  The same stream as the last call's: nothing (no wait, no launch -- stream order does
//    it).  Another one: settle first, since what is enqueued next writes the handle's memory from the new stream.  Then `stream` is the
//    handle's stream.  A call enters its stream BEFORE it grows a buffer or launches.
int settle(hmpc_handle *h);
int enter_stream(hmpc_handle *h, hipStream_t stream);
//  * grow: a buffer whose users are the handle's own calls grows to at least `bytes` (contents undefined).  The old allocation is freed,
//    so the handle is settled first; a buffer that is large enough costs nothing.
template <class T>
int grow(hmpc_handle *h, DeviceBuffer<T> &b, size_t bytes) {
  if (b.get() && bytes <= b.bytes()) return HMPC_OK;
  if (b.get()) RC_TRY(settle(h));
  HIP_TRY(b.alloc((bytes + sizeof(T) - 1) / sizeof(T)));  // (frees the old allocation, which nothing uses any more)
  return HMPC_OK;
}
// A new buffer with every byte set (DeviceBuffer::alloc_filled) whose first reader is a kernel on a stream that is not known yet and is, as
// a rule, NON-BLOCKING: the null stream, on which hipMemset fills, does not order such a stream.  Whether a device memset has finished
// when hipMemset returns is promised nowhere: hip_runtime_api.h documents the call without a word on completion, and the CUDA runtime API
// it mirrors says the opposite outright (its "API synchronization behavior" notes: memsets of device memory may be asynchronous with
// respect to the host).  The fill cannot be put on the reader's stream -- hmpc_create, hmpc_set_tick_warm_start and hmpc_set_device_repair
// take none -- so the null stream is synchronised behind it.  Once per buffer; a call that finds its buffers allocated never gets here.
// (A call that HAS a stream fills on it instead: the hand-over slot table in launch(), hmpc_reset_tick_warm_start.)
template <class T>
hipError_t alloc_filled_done(DeviceBuffer<T> &b, size_t count, int byte) {
  hipError_t e = b.alloc_filled(count, byte);
  if (e == hipSuccess && (e = hipStreamSynchronize(nullptr)) != hipSuccess) b.reset();
  return e;
}
// returns a device buffer of at least `bytes` owned by the handle (contents undefined).  Its earlier users are the handle's own calls: the
// caller has settled the handle or entered its stream before it writes the buffer
int scratch(hmpc_handle *h, size_t bytes, void **out);
// What stage A of a kernel reads of the handle: the batch, the problem shape and the robot / contact constants.  One place, so that the
// prediction and margins kernels assemble from the very values the solve kernels do.
void set_problem_args(const hmpc_handle *h, hmpc::KernelArgs &a);
int launch(hmpc_handle *h, hipStream_t stream, int vi, const LaunchOpt &o);                       // one launch of variants()[vi]
// The prologue of a fast pass whose launches are the variants vis[0 .. n): front_scalars_kernel over the current batch on `stream`, when
// at least one of them reads it (and the handle's switch is on, no external QP is set).  *ready = whether it was enqueued: what the
// caller passes on as LaunchOpt::front_ready to the launches that follow on the same stream, and to nothing else.
int enqueue_front(hmpc_handle *h, hipStream_t stream, const int *vis, int n, bool *ready);
int enqueue_fast(hmpc_handle *h, hipStream_t stream, int vi, bool classes, LaunchOpt o);          // the fast pass of one solve
int enqueue_solve(hmpc_handle *h, hipStream_t stream, bool carry_wset);                           // what hmpc_solve enqueues
int enqueue_command_sweep(hmpc_handle *h, hipStream_t stream, int group_size);                    // what hmpc_solve_command_sweep enqueues (group_size > 1)
int resolve_failed(hmpc_handle *h, int *n_resolved);                                              // the host-driven repair of hmpc_resolve_failed (device set, batch > 0)
// ---- hmpc_swing.hip
// tick k of a rollout: the swing launch of hmpc_set_rollout_swing behind the tick's torque launch (nothing when the setting is off)
int rollout_swing_tick(hmpc_handle *h, const void *device_ticks, int batch, int k, int n_ticks, int ticks_per_step, int subtick0, hipStream_t stream);

#pragma GCC visibility pop
