/*
 * hector_mpc.h -- C ABI of libhector_mpc_hip.so: MI355X (gfx950) batched force-and-moment MPC QP solver for
 * HECTOR's convex-MPC loop.  Plain pointers and sizes only; no torch / Eigen / C++ types cross this boundary.
 *
 * Two surfaces:
 *  (1) the reference's own interface, byte-for-byte the same signatures, so hector_control links against this
 *      library instead of its ConvexMPC/convexMPC_interface.cpp + SolverMPC.cpp + qpOASES and nothing else changes:
 *        setup_problem / update_problem_data / get_solution / update_solver_settings
 *            -> Hector_ROS_Simulation/hector_control/ConvexMPC/convexMPC_interface.h:39-43
 *        solve_mpc(update_data_t*, problem_setup*), get_q_soln()   (C++ linkage in the reference)
 *            -> ConvexMPC/SolverMPC.h:56,63    (exported here additionally as C symbols hmpc_solve_mpc / hmpc_get_q_soln
 *               and, under the north-star name, solveDenseMPC)
 *        problem_setup, update_data_t PODs -> ConvexMPC/convexMPC_interface.h:11-37
 *  (2) a handle-based, re-entrant BATCHED interface (names are ours) over packed records
 *      (hector_simulation_amd/records.py documents the layout; hmpc_pack_record builds one from the reference's
 *      argument list).
 *
 * Every function returns 0 on success or a negative hmpc_error; nothing throws across this boundary
 * (the reference throws std::runtime_error for horizon > 19, SolverMPC.cpp:140-143: here setup returns/records
 * HMPC_E_HORIZON and get_solution keeps returning the previous values).
 */
#ifndef HECTOR_MPC_H
#define HECTOR_MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define K_MAX_GAIT_SEGMENTS 36 /* convexMPC_interface.h:3 */
#define HMPC_MAX_HORIZON 20    /* device scratch is sized for this (reference: 10 hard-coded, cap 19) */
#define HMPC_MAX_VARS 120      /* reduced QP variables (6 per stance leg-step) the fast on-chip variants hold (two contacts; 180 with three) */
#define HMPC_MAX_VARS_WIDE 240 /* ... the wide variant (double support over h = 11 .. 20): picked when the batch needs it -- from the gait
                                  tables of host-uploaded records, hmpc_set_max_reduced_vars, or per instance on the device */

/* ---- reference PODs (convexMPC_interface.h:11-37), same field order and types ---- */
struct problem_setup {
  float dt;
  float mu; /* ignored by the reference (mu = 2.0 is hard-coded, SolverMPC.cpp:488); ignored here too */
  float f_max;
  int horizon;
};

struct update_data_t {
  float p[3];
  float v[3];
  float q[4];
  float w[3];
  float r[6];
  float joint_angles[10];
  float yaw;
  float weights[12];
  float traj[12 * K_MAX_GAIT_SEGMENTS];
  float Alpha_K[12];
  unsigned char gait[K_MAX_GAIT_SEGMENTS];
  unsigned char hack_pad[1000];
  int max_iterations;
  double rho, sigma, solver_alpha, terminate;
};

/* ---- (1) reference interface, convexMPC_interface.h:39-43 ---- */
void setup_problem(double dt, int horizon, double mu, double f_max);
void update_problem_data(double *p, double *v, double *q, double *w, double *r, double *joint_angles, double yaw,
                         double *weights, double *state_trajectory, double *Alpha_K, int *gait);
double get_solution(int index);
void update_solver_settings(int max_iter, double rho, double sigma, double solver_alpha, double terminate,
                            double use_jcqp);
/* SolverMPC.h:56,63 under C names (the C++-linkage solve_mpc/get_q_soln are exported too, see hmpc_capi) */
void hmpc_solve_mpc(struct update_data_t *update, struct problem_setup *setup);
void solveDenseMPC(struct update_data_t *update, struct problem_setup *setup);
double *hmpc_get_q_soln(void);
/* extra: status word of the last legacy solve (see HMPC_STATUS_*), never part of the reference.
 * The process-global solver behind the reference interface runs on the device named by the environment variable
 * HMPC_DEVICE (default 0).  On a flagged solve it prints the reference's "failed to solve!" line and, like the
 * reference (SolverMPC.cpp:714-732), still scatters the last iterate; HMPC_S_OK_RELAXED counts as solved. */
uint32_t hmpc_last_status(void);

/* ---- (2) batched interface ---- */
typedef struct hmpc_handle hmpc_handle;

enum hmpc_error {
  HMPC_OK = 0,
  HMPC_E_ARG = -1,      /* null pointer / bad size */
  HMPC_E_HORIZON = -2,  /* horizon < 1 or > HMPC_MAX_HORIZON */
  HMPC_E_BATCH = -3,    /* batch > max_batch */
  HMPC_E_HIP = -4,      /* HIP runtime error (hmpc_last_hip_error) */
  HMPC_E_NO_DEVICE = -5 /* no gfx950 device visible: the library has NO CPU fallback */
};

/* per-instance status word written by the kernel: bits 0-7 code, 8-19 active-set iterations, 20-31 final |W| */
#define HMPC_STATUS_CODE(s) ((s) & 0xffu)
#define HMPC_STATUS_ITERS(s) (((s) >> 8) & 0xfffu)
#define HMPC_STATUS_NACTIVE(s) (((s) >> 20) & 0xfffu)
enum hmpc_status_code {
  HMPC_S_OK = 0,
  HMPC_S_MAXITER = 1,     /* iteration cap hit (reference analogue: nWSR = 500 exhausted) */
  HMPC_S_INFEASIBLE = 2,  /* constraints inconsistent */
  HMPC_S_TOO_LARGE = 3,   /* more reduced variables than the variant the batch was launched with holds (only when
                             hmpc_set_max_reduced_vars named a smaller size than the batch really contains) */
  HMPC_S_KKT = 4,         /* final KKT check outside tolerance (rows outside the working set, the residual of the rows in it,
                             multiplier signs; relative to the force scale) */
  HMPC_S_WORKSET = 5,     /* more simultaneously active constraints than the FAST variant's on-chip working set holds (64 rows; 96
                             with three contacts, 152 in the wide variant).  The safe pass holds as many rows as there are
                             variables -- in LDS for 120 variables, in global memory for 180 / 240 -- and cannot overflow */
  HMPC_S_SWEEP_MISMATCH = 7, /* hmpc_solve_command_sweep: the record differs from its chunk's first record outside the trajectory; not solved.
                                Terminal: forces 0, not counted as flagged, never re-solved by a repair pass; the instance's tick-to-tick
                                working set (hmpc_set_tick_warm_start) is cleared */
  HMPC_S_INDEFINITE = 8,  /* the reduced Hessian, assembled in binary32 as the reference assembles it (SolverMPC.cpp:560-570), is NOT
                             positive definite: a sweep pivot of the safe pass came out <= 0 (seen with 20-step horizons at 10x the
                             nominal input ranges: rounding at 6e-8 |H| against a smallest eigenvalue of ~2 alpha).  An intermediate
                             state: the safe pass -- hmpc_resolve_failed / hmpc_download, or (horizons > 10) the device-side chain of
                             hmpc_set_device_repair(h, 1) -- answers it the way the reference's qpOASES run does (H + rho I, then one
                             step with g - rho x_1: QProblem.cpp:1753-1860) and reports HMPC_S_OK; seen by a caller only where those
                             two QPs fail as well (forces zeroed) */
  HMPC_S_REG_STEP = 9,    /* (internal to hmpc_resolve_failed: between the two regularised QPs of an HMPC_S_INDEFINITE instance) */
  HMPC_S_OK_RELAXED = 6   /* solved only after every bound was moved outward by <= 2e-5 (relative for the Fz cap) AND the exact
                             re-solve on the working set so found did not pass the exact KKT check: the last-resort pass of
                             hmpc_resolve_failed for instances cycling at a degenerate vertex.  (When the exact re-solve passes --
                             every case seen up to 10x the nominal input ranges -- the instance is HMPC_S_OK, exact.) */
};

size_t hmpc_record_stride(int horizon);  /* bytes per packed record: (54+12h)*4 + 2h rounded up to 16 */
/* packs one record from the reference's update_problem_data argument list (double -> float, int -> u8 narrowing
 * exactly as convexMPC_interface.cpp:83-103) */
int hmpc_pack_record(void *record, int horizon, const double *p, const double *v, const double *q, const double *w,
                     const double *r, const double *joint_angles, double yaw, const double *weights,
                     const double *state_trajectory, const double *Alpha_K, const int *gait);

int hmpc_create(hmpc_handle **out, const struct problem_setup *setup, int max_batch, int device);

/* Robot and contact constants of the formulation.  The reference hard-codes every one of them in its solver source (and ignores
 * problem_setup.mu): a payload, friction or foot-geometry sweep needs a recompile there.  Here they are data of the handle; the
 * defaults are the reference's literals, and a handle that was never given anything else assembles bit for bit the QP it
 * assembled before the struct existed (tests/test_gpu_assembly.py).  The CPU oracle takes the same struct (orc_set_params), so
 * non-default values are checked bitwise as well. */
struct hmpc_params {
  float mass;       /* 9.0                      SolverMPC.cpp:423  (B_ct: v' += F / mass) */
  float inertia[3]; /* 0.5413, 0.5200, 0.0691   RobotState.cpp:45  (body inertia, diagonal) */
  float mu;         /* 2.0                      SolverMPC.cpp:488  (friction pyramid rows 0-3 are (-+mu, 0, 1) F >= 0, i.e. |F_t| <= F_z / mu: the
                                                 reference's 2.0 is a friction coefficient of 0.5 -- convention kept; problem_setup.mu is ignored, as there) */
  float lt, lh;     /* 0.09, 0.06               SolverMPC.cpp:489-490 (toe / heel lever arms of the line-contact rows 5, 6) */
  float gravity;    /* 9.81                     SolverMPC.cpp:420  (the constant 13th state) */
};
void hmpc_default_params(struct hmpc_params *p);
/* takes effect with the next solve of the handle; p == NULL restores the defaults.  mass, inertia, mu > 0 and finite, else HMPC_E_ARG */
int hmpc_set_params(hmpc_handle *h, const struct hmpc_params *p);
int hmpc_get_params(const hmpc_handle *h, struct hmpc_params *p);
/* TERRAIN SWEEPS: a friction parameter per INSTANCE -- device_mu[batch] floats in HBM, caller-owned, read by every later solve of the
 * handle in place of hmpc_params.mu until it is set to NULL again (instance i of the current batch uses device_mu[i]; values must
 * be > 0).  H and its inverse do not depend on mu -- only the friction rows (-+mu, 0, 1) of the constraint block do -- so the
 * records of one hmpc_solve_command_sweep group may differ in their mu as well as in their trajectory: one state under many commands
 * on many floors, one inverse. */
int hmpc_set_instance_mu(hmpc_handle *h, const float *device_mu);
/* ... for the process-global solver behind the reference interface (applies from the next setup_problem / solve on) */
int hmpc_legacy_set_params(const struct hmpc_params *p);

/* ---- extension beyond the reference: a third (hand) contact per horizon step -- BASELINE.json config 5, the
 * loco-manipulation shape 180 variables x 240 rows at h = 10.  The reference has no code for it;
 * the formulation is the reference's own with one more contact: B_ct gains the hand's force / moment columns
 * (SolverMPC.cpp:312-331 with a third r), the hand gets the left foot's 8-row block (SolverMPC.cpp:488-548) expressed
 * in its contact frame Rhand (body frame, row-major) with its own force cap, gait gets a third flag per step.
 * Component order within a step: [F_left F_right F_hand M_left M_right M_hand]; r[3*axis + contact]; Alpha_K has 18
 * entries in that order; gait[3*step + contact].  h <= 10.  Rows f1-f3 (tick builder, wrench, torques) are two-foot only. */
#define HMPC_MAX_VARS_3C 180
int hmpc_create_ex(hmpc_handle **out, const struct problem_setup *setup, int max_batch, int device, int n_contacts);
int hmpc_contacts(const hmpc_handle *h);
size_t hmpc_record_stride_ex(int horizon, int n_contacts); /* n_contacts 3: (73+12h)*4 + 3h rounded up to 16 */
int hmpc_pack_record_ex(void *record, int horizon, int n_contacts, const double *p, const double *v, const double *q,
                        const double *w, const double *r, const double *joint_angles, double yaw, const double *weights,
                        const double *state_trajectory, const double *Alpha_K, const int *gait, const double *Rhand,
                        double f_max_hand);
int hmpc_destroy(hmpc_handle *h);
/* host records -> device: waits for whatever is enqueued for the handle (STREAMS below), then copies; the copy has finished on return */
int hmpc_upload_records(hmpc_handle *h, const void *host_records, int batch);
/* use records that already live in HBM (no copy; pointer must stay valid until the solve finishes) */
int hmpc_set_device_records(hmpc_handle *h, const void *device_records, int batch);
/* optional: write forces/status into caller-owned device buffers instead of the handle's own */
int hmpc_set_device_outputs(hmpc_handle *h, float *device_forces, uint32_t *device_status);
/* asynchronous: enqueue assembly+solve of the current batch on `stream` (a hipStream_t, NULL = default stream) */
int hmpc_solve(hmpc_handle *h, void *stream);
/* waits for `stream` work, copies forces [batch][12h] float and status [batch] to host (either may be NULL) */
int hmpc_download(hmpc_handle *h, float *forces, uint32_t *status);
/* COMMAND SWEEPS (round 6): the current batch is B = G x group_size records in G groups of group_size CONSECUTIVE records that
 * share the robot state, foot positions, joint angles, weights and gait table and differ in the reference trajectory only -- one
 * state under many commands: ConvexMPCLocomotion.cpp:351-406 builds state_trajectory from the velocity / yaw-rate commands, while
 * A_qp, B_qp, H = 2(B'SB + alpha) and the constraint block depend on the state and the gait alone (SolverMPC.cpp:398-447, 488-570),
 * so only g = 2 B'S (A_qp x0 - X_d) changes inside a group and M = H^-1 is a property of the GROUP.  Two launches on `stream`:
 * one workgroup per group forms M once and leaves it in HBM (74 KB per group; a per-handle buffer grown on demand), then one
 * workgroup per instance -- the chip as full as for independent solves -- assembles its own g, takes M from its group's slot
 * instead of assembling and inverting H (55 % of an independent solve) and runs the block start and the active-set iteration as
 * they stand: forces and status words are BIT-IDENTICAL to hmpc_solve's.  A record that differs from its group's first record
 * anywhere but in the trajectory is not solved: status HMPC_S_SWEEP_MISMATCH, forces 0 (checked on the device, word by word; the
 * padding bytes after the gait table are not part of the record and are ignored).  The mismatch is terminal: nothing re-solves it.
 * Records handed in by device pointer without a size hint run per size class, on the variants hmpc_solve gives them.  A sweep hands
 * no working set over: it clears the handle's hand-over slot table first.
 * Flagged instances are repaired as independent ones (hmpc_download / hmpc_set_device_repair).  Two-contact handles, horizon <= 10;
 * batch % group_size must be 0; group_size 1 is hmpc_solve.  A per-call CPU solver has no counterpart: the reference assembles and
 * factorises H for every command. */
int hmpc_solve_command_sweep(hmpc_handle *h, int group_size, void *stream);
/* hint for device-resident records: the widest reduced QP (6 x stance leg-steps) in the batch: one launch of the variant
 * that holds it.  -1 = unknown (the state after hmpc_set_device_records / hmpc_build_records_device): two-contact handles
 * then route every instance on the device -- its stance leg-steps are counted there (by the record builder, or from the
 * records' gait bytes at the head of the solve) and each variant of the family (60 / 120 / at h > 10 also 240 variables)
 * is launched over the whole batch, a workgroup leaving at once when its instance belongs to another variant.
 * hmpc_upload_records derives the hint from the gait tables itself. */
int hmpc_set_max_reduced_vars(hmpc_handle *h, int n_reduced);
/* Working-set start of the active-set solver.  on = 1 (default): every moment / line-contact row violated at the
 * unconstrained minimiser enters at once (block warm start); on = 0: cold start from the empty set, one row per
 * iteration, as the reference's qpOASES call does.  Same optimum either way (strictly convex QP). */
int hmpc_set_warm_start(hmpc_handle *h, int on);
/* Warm start ACROSS ticks (the reference cold-starts every tick, SolverMPC.cpp:702).
 * Default off.  When on, every solve leaves each instance's final working set in HBM (one signed byte per constraint
 * row) and the next solve of the same handle starts instance k from the set instance k ended with: its Schur matrix
 * is formed and inverted at once, rows whose multiplier comes out negative are released, and the dual active-set
 * iteration continues from there.  horizon_shift = how many horizon steps the gait table advanced between the two
 * solves (rows of step i start from saved step i + shift).  Same optimum as a cold start (the QP is strictly convex);
 * only the iteration count changes.  A saved set that has become rank deficient under the new data is discarded for
 * that instance.  hmpc_reset_tick_warm_start forgets all saved sets (e.g. before an unrelated batch). */
int hmpc_set_tick_warm_start(hmpc_handle *h, int on, int horizon_shift);
int hmpc_reset_tick_warm_start(hmpc_handle *h);
/* Safe pass: waits for the last solve, then re-solves every instance whose status is working-set-full / max-iter /
 * infeasible / KKT and overwrites its forces and status in place.  The passes, each over what the one before left flagged
 * (round 6): (1) instances that handed their state over (hmpc_set_handover) are CONTINUED on the 96-row variant; (2) the
 * large-working-set variant (capacity = number of variables: cannot overflow; the Schur inverse is rebuilt from scratch every
 * 48 working-set changes, so that hundreds of them do not add up round-off), cold, with every bound moved outward by a relative
 * 1e-6 (a different amount per row: separates the coinciding vertices at which the exact problem makes Goldfarb-Idnani cycle --
 * the instances that reach this pass are the degenerate ones), ending with an exact re-solve on the working set it found:
 * HMPC_S_OK when that passes the exact KKT check -- every one of the 8 192 at 6x the nominal input ranges --, HMPC_S_OK_RELAXED
 * otherwise; (3) the same variant on the EXACT bounds, started by the block start, for relaxed and flagged instances alike;
 * (4) instances whose reduced Hessian is not positive definite (HMPC_S_INDEFINITE, found by the sweeps of (2)): the reference's
 * regularisation, two more launches -- H + rho I with rho = |H|_F sqrt(1e3 * 2.221e-16), then the same QP with the gradient
 * g - rho x_1 (qpOASES QProblem.cpp:1753-1860, QProblemB.cpp:1418-1431, 1999-2031 under Options::setToMPC) -- within 6e-8 of what
 * the reference returns for them; (5) up to three last-resort passes with the bounds moved by 1e-7, 1e-6, 1e-5, cold.  Measured at 1x .. 10x the nominal input
 * ranges (scripts/stress.py, profiles/r06/stress.txt, 28 shapes x ranges of 1 024 instances): every instance qpOASES solves ends
 * HMPC_S_OK.  On 4 096 per row (stress_4096.txt): the same up to 6x; at 10x five rows keep ONE instance flagged KKT, and two
 * instances end HMPC_S_OK_RELAXED 3e-3 / 8e-3 from qpOASES' forces (7 of 114 688; an ok-relaxed answer satisfies the bounds to 2e-5
 * but need not be close to the exact optimum where the problem is that degenerate: check for the code where that matters).
 * *n_resolved (may be NULL) =
 * how many were re-solved.  hmpc_download does this automatically unless hmpc_set_auto_resolve(h, 0). */
int hmpc_resolve_failed(hmpc_handle *h, int *n_resolved);
/* Dispatch order of the workgroups of a solve.  mode 1 (default), longest first: the instances are started in the order of
 * the active-set iterations their PREVIOUS solve took (most first; read on the device from the status words the previous
 * solve of this handle left, one small sorting launch at the head of each solve).  An MPC tick resembles the tick before it,
 * so the solves that will run longest start first and the short ones fill the last, partly occupied round of workgroup
 * slots -- what bounds small and medium batches is that tail (2 048 three-contact instances are four rounds of 512 resident
 * workgroups and one 87-iteration straggler: 1.18 M solves/s in natural order, 1.66 M with a hint one tick old).  mode 0:
 * instance b runs in workgroup b.  Results do not depend on the mode, nor on whether the assumption holds (instance i of
 * this solve = instance i of the previous one, as for hmpc_set_tick_warm_start): any status words give a valid order, a
 * stale one merely stops helping.  The first solve of a handle and the first after a change of the batch size -- no previous
 * solve to go by -- are ordered by a COST PREDICTED FROM THE RECORDS (round 5): the forward acceleration the tick asks for,
 * (v_x commanded - v_x) + 2 x mean foot x, and the body's tilt, which is what the iteration count of this QP follows
 * (correlation 0.8 on the bench's sets; hmpc_builder.h predicted_cost_bucket) -- so a cold handle, and the first tick of a
 * device-built pipeline, are ordered too.  mode 2: always by the predictor (never by a previous solve).  Batches of at
 * most 512 instances (they fit the chip's workgroup slots at once), of more than 32 768, and batches known to hold
 * single-support QPs only (<= 60 reduced variables: one or two iterations each, nothing to sort) run in natural order.
 * The reference has no counterpart (one QP per call). */
int hmpc_set_dispatch_order(hmpc_handle *h, int mode);

/* Cap on the active-set iterations of every later solve of the handle -- the analogue of the reference's nWSR = 500
 * (SolverMPC.cpp:706).  0 (default) = the kernel variant's own bound.  Block rounds and switch passes of the block start
 * count as one iteration each and always complete; the cap is tested before every single-row iteration after them.  An
 * instance that would need more ends as HMPC_S_MAXITER with its last iterate in the force buffer and is NOT re-solved by
 * the safe pass -- neither by hmpc_download's host-driven one nor by the device-side one (hmpc_set_device_repair).
 * hmpc_legacy_set_max_iterations sets the same cap for the process-global solver behind setup_problem / update_problem_data.
 * The legacy update_solver_settings(max_iter, ...) does NOT: as in the reference (convexMPC_interface.cpp:112-118 stores its
 * arguments, nothing reads them; the qpOASES path uses a fixed nWSR, SolverMPC.cpp:706) it is inert, so that a drop-in caller
 * passing a small JCQP-style max_iter still gets full solves. */
int hmpc_set_max_iterations(hmpc_handle *h, int max_iter);
int hmpc_legacy_set_max_iterations(int max_iter);
int hmpc_set_auto_resolve(hmpc_handle *h, int on);
/* Hand-over of a full working set (round 6; default on).  A fast two-contact variant (<= 120 reduced variables) whose working
 * set is full (HMPC_STATUS_NACTIVE = 64) when another row is violated no longer throws its work away: it writes its live
 * Goldfarb-Idnani state -- x, multipliers, working set, the packed Schur inverse and the register-resident H^-1 -- to the
 * instance's slot of a per-handle buffer in HBM (101 KB per instance of max_batch, allocated at the first solve; at most
 * 32 768 slots) and flags the instance HMPC_S_WORKSET as before; the safe pass -- the device-side one of hmpc_set_device_repair or
 * the host-driven one of hmpc_resolve_failed / hmpc_download -- then CONTINUES that solve on the variant whose working set cannot
 * overflow instead of re-solving it cold without the block start: same optimum (the QP is strictly convex), a fraction of the
 * iterations (the reference's qpOASES run needs up to 190 working-set changes for such an instance, SolverMPC.cpp:699-712; the
 * continuation the 20-40 that were still missing).  on = 0: the round-5 behaviour (flag, re-solve cold).  Three-contact handles
 * and the wide variant (> 120 reduced variables) always take the cold path. */
int hmpc_set_handover(hmpc_handle *h, int on);
/* Device-side safe pass (default off for a plain handle): when on, hmpc_solve enqueues, behind the fast launch and on the
 * same stream, the safe variant over the list of instances the fast launch flagged (the list and its length stay on the
 * device; workgroups beyond the length leave at once) -- device-resident outputs, hmpc_download_async and the group
 * exchange then see repaired forces/status without any host involvement.  Costs one 4-byte memset and one (normally
 * empty) extra launch per solve; repairs every flagged instance of batches up to 65 536 (the wide variant's instances, whose safe
 * pass keeps 231 KB of global scratch per workgroup: the first 4 096 positions of the flagged list, 0.95 GB of scratch allocated with
 * the first such solve), the rest stay flagged for
 * hmpc_resolve_failed / hmpc_download.  Instances whose working set merely outgrew the fast variant are CONTINUED, not
 * re-solved (hmpc_set_handover): first the continuation variant over the flagged list (96-row working set, two workgroups per
 * CU), then the safe variant over what is still flagged: cold, bounds moved outward by a relative 1e-6 and an exact re-solve
 * on the working set found (pass (2) of hmpc_resolve_failed: HMPC_S_OK, or HMPC_S_OK_RELAXED when the exact KKT check fails
 * on that set: a solved instance whose bounds were off by <= 2e-6 relative; not seen on any measured set), and -- for horizons beyond
 * 10 steps, where such Hessians occur -- two more short launches for the instances whose Hessian is not positive definite (pass (4)
 * of hmpc_resolve_failed; up to 256 per solve, the rest and any such instance of a shorter-horizon handle stay HMPC_S_INDEFINITE for
 * hmpc_resolve_failed).  Every launch of the chain is trimmed on the device by a counter: with nothing flagged their workgroups leave
 * at once, and a nominal solve pays 11-15 us of dispatch latency for the chain (scripts/dev/chain_overhead.py).  on = 2: the continuation pass only -- what it does not finish
 * (~0.5 % of the instances at 6x the nominal input ranges: degenerate vertices, working sets beyond 96 rows) stays FLAGGED in
 * the status word for hmpc_resolve_failed / hmpc_download; a cold re-solve of such an instance takes hundreds of iterations on a
 * single workgroup, milliseconds at the tail of the stream, which a device-resident pipeline may prefer not to wait for. */
int hmpc_set_device_repair(hmpc_handle *h, int on);
/* NOTE (device repair): the list of flagged instances and its counter belong to the handle -- keep the solves of ONE handle
 * on one stream at a time (use one handle per stream to overlap launches, as bench.py does). */
/* STREAMS.  A handle remembers the stream of its last enqueued call -- every entry point that takes a `stream`, hmpc_download_async and
 * the upload variants included; the blocking host-pointer entries (hmpc_build_records, hmpc_body_wrench, hmpc_leg_torques,
 * hmpc_debug_assemble) enqueue on the null stream.  A call waits on the host for that stream FIRST
 *   - if it frees or reallocates device memory the handle owns (a buffer that has to grow: the groups' H^-1 of a command sweep, the safe
 *     variants' scratch, the handle's own rollout log; hmpc_destroy);
 *   - if it writes device memory the handle owns from the host (hmpc_upload_records, hmpc_build_records, hmpc_body_wrench,
 *     hmpc_leg_torques, the host-driven repair of hmpc_resolve_failed / hmpc_download) or reads it to the host (every hmpc_download_*);
 *   - if it enqueues on ANOTHER stream than that one: what it enqueues writes the handle's memory from the new stream.
 * So a handle may be moved from one stream to the next, and a blocking entry may be called while work is pending, without any
 * synchronisation by the caller FOR THE HANDLE'S MEMORY.  A call on the SAME stream as the one before waits for nothing and enqueues
 * nothing extra: stream order does it (one handle per stream, as bench.py runs, never waits).  hmpc_reset_tick_warm_start does not wait
 * either: it clears the saved sets on the handle's stream, behind the solve that may still write them.  Buffers that are filled when
 * they are allocated (hmpc_create, the first hmpc_set_tick_warm_start(on) / hmpc_set_device_repair(on)) are complete when the call
 * returns: a solve on any stream may follow at once.  (The hand-over slot table of a handle's first solve is filled on that solve's stream.)
 * What stays the caller's business: the caller's OWN buffers (records, outputs, seeds, ticks, logs handed in by pointer -- valid and
 * ordered until the stream has passed them); two calls of one handle in flight on two streams at once (see the note above: the second
 * call waits for the first, it does not overlap it); and where a result belongs -- put a result call on the solve's stream. */
/* Stream-ordered variants for pipelining host batches (two handles on two streams: the copies of one overlap the solve
 * of the other).  The host buffers should be pinned (hipHostMalloc / hipHostRegister) for the copies to be asynchronous
 * and must stay valid until the stream reaches them.  hmpc_download_async does not run the safe pass: check the status
 * words after synchronising and call hmpc_resolve_failed + hmpc_download for a batch that has flagged instances. */
int hmpc_upload_records_async(hmpc_handle *h, const void *host_records, int batch, void *stream);
/* ... every pitch_bytes-th record of a larger host array (pitch_bytes >= hmpc_record_stride and a multiple of 4, else HMPC_E_ARG): record k of the
 * batch is read at host_records + k * pitch_bytes -- one strided copy, no host staging (what a striped device group uses). */
int hmpc_upload_records_strided_async(hmpc_handle *h, const void *host_records, int batch, size_t pitch_bytes, void *stream);
int hmpc_download_async(hmpc_handle *h, float *forces, uint32_t *status, void *stream);
int hmpc_get_device_outputs(hmpc_handle *h, float **device_forces, uint32_t **device_status);
int hmpc_batch(const hmpc_handle *h);
int hmpc_horizon(const hmpc_handle *h);
/* average kernel time in ms of `reps` back-to-back launches of the current batch measured with HIP events on
 * `stream` (used by bench.py for the roofline object) */
int hmpc_time_solve(hmpc_handle *h, void *stream, int reps, float *ms_per_launch);


/* ---- the rows either side of the solve, batched on the device ----
 * hmpc_tick_inputs = everything ConvexMPCLocomotion::updateMPCIfNeeded reads to build one MPC tick
 * (ConvexMPC/ConvexMPCLocomotion.cpp:283-406): state estimate, leg joint angles, foot positions, commands, the
 * persistent world_position_desired, and the Gait parameters of ConvexMPC/GaitGenerator.cpp:85-113. */
struct hmpc_tick_inputs {
  double position[3], vWorld[3], omegaWorld[3], orientation[4], rpy[3];
  double rBody[9];        /* row-major, world -> body (orientation_tools.h:182-200) */
  /* Joint angles, left 0-4, right 5-9, AS updateMPCIfNeeded READS THEM: data[leg].q of the LegController
   * (ConvexMPCLocomotion.cpp:288-296).  On the reference's live path that is NOT the motor angle: updateData() hands
   * data[leg].q BY REFERENCE to computeLegJacobianAndPosition, which adds (+0.3, -0.6, +0.3) * 3.14159 to joints 2-4 in place
   * (common/LegController.cpp:48-52, 108-113) before the MPC runs; the MPC then adds its own offsets (:302-308) and the
   * solver a third time (SolverMPC.cpp:382-388) -- SURVEY A.9 "triple offset", reproduced, not fixed.  So pass either
   *   - data[leg].q after the LegController update (flags = 0), or
   *   - the raw motor angles state->motorState[].q with HMPC_TICK_LEG_Q_MOTOR set in `flags`: the builder then applies the
   *     LegController's first offset itself (same constant 3.14159, same operation order).
   * hmpc_leg_torques takes the Jacobian's argument, i.e. the MOTOR angle before that offset (LegController.cpp:108-113). */
  double leg_q[10];
  double pFoot[6];        /* world foot positions, [leg][axis] */
  double v_des_robot[2];  /* stateDes[6], stateDes[7] */
  double yaw_rate_des;    /* stateDes[11] */
  double roll_des, pitch_des; /* stateDes[3], stateDes[4] */
  double world_position_desired[2];
  int gait_offsets[2], gait_durations[2], gait_iteration;
  int flags;              /* HMPC_TICK_* bits (was padding: 0 keeps the previous meaning) */
};
#define HMPC_TICK_LEG_Q_MOTOR 1 /* leg_q holds raw motor angles: apply LegController.cpp:111-113's offset first */
#define HMPC_TICK_FALLEN 2      /* set by the plant step (hmpc_plant_step_device) once the body has tipped over; the builder tests bit 0 only */
/* f1+f2: builds the packed records of `batch` ticks on the device into the handle's own record buffer (which becomes
 * the current batch) and returns the clamped world_position_desired (ConvexMPCLocomotion.cpp:336-346) per instance.
 * host_ticks / wpd_out are host pointers (wpd_out may be NULL); the _device form takes device pointers and a stream. */
int hmpc_build_records(hmpc_handle *h, const struct hmpc_tick_inputs *host_ticks, int batch, double dtMPC, double *wpd_out);
int hmpc_build_records_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, double *device_wpd_out,
                              void *stream);
/* f3: f_ff[batch][2][6] = -rBody [GRF; GRM] from the forces of the last solve (ConvexMPCLocomotion.cpp:419-440) */
int hmpc_body_wrench(hmpc_handle *h, const double *host_rBody, double *host_f_ff);
int hmpc_body_wrench_device(hmpc_handle *h, const double *device_rBody, double *device_f_ff, void *stream);
/* f3, with the joint torques: f_ff as above, then tau[batch][2][5] = J_fm' f_ff with the force-moment Jacobian of
 * common/LegController.cpp:108-167 evaluated at leg_q[batch][10] (LegController.cpp:57-61).  f_ff may be NULL.
 * leg_q here is what computeLegJacobianAndPosition RECEIVES: the raw motor angles (it adds its 3.14159-based offset
 * itself) -- not the hmpc_tick_inputs.leg_q of a flags = 0 tick, which already carries that offset. */
int hmpc_leg_torques(hmpc_handle *h, const double *host_rBody, const double *host_leg_q, double *host_f_ff, double *host_tau);
int hmpc_leg_torques_device(hmpc_handle *h, const double *device_rBody, const double *device_leg_q, double *device_f_ff,
                            double *device_tau, void *stream);
/* f1+f2 -> solve -> f3 in one call, device-resident end to end: builds the records of `batch` ticks (device_ticks:
 * hmpc_tick_inputs[batch] in HBM) into the handle, solves them -- every instance on the smallest kernel variant that holds
 * its reduced QP, decided on the device from the gait table the builder has just generated: a walking sweep runs on the
 * 60-variable variant with no host hint -- and writes f_ff[batch][2][6] (may be NULL) and the stance feed-forward torques
 * tau[batch][2][5] (rBody and the joint angles are read from the tick structs; leg_q per the tick's HMPC_TICK_LEG_Q_MOTOR
 * flag).  device_wpd_out (may be NULL) receives the clamped world_position_desired.  Three or four launches on `stream`, no
 * host synchronisation: forces, status, f_ff and tau are valid once the stream reaches them.  With hmpc_set_device_repair
 * the torques are computed from repaired forces.  Two-contact handles only. */
int hmpc_tick_solve_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, double *device_wpd_out,
                           double *device_f_ff, double *device_tau, void *stream);
/* ---- the predicted state trajectory and tracking cost of every instance ----
 * The QP minimises over an h-step prediction of the body state; these calls return it.  Per instance, with U = 6 * contacts,
 * x0[13], Acd[13][13], Bcd[13][U] THE binary32 values the solve kernel assembles for the record (hmpc_params included; the prediction
 * kernel calls the solve kernel's own assembly stage) and u_i[U] step i of the handle's force buffer as it stands:
 *   x_0 = x0;   x_{i+1}[s] = sum_{k<13} Acd[s][k] x_i[k] + sum_{c<U} Bcd[s][c] u_i[c],   i = 0 .. h-1,
 * evaluated in binary64 as one ascending chain of fused multiply-adds started at +0 (state terms, then force terms; every term, the
 * structural zeros too), each step taking the un-rounded x_i.  State order as the reference's (SolverMPC.cpp:420): roll pitch yaw,
 * position, angular velocity, velocity, gravity constant.
 *   states[batch][h][13]  binary32; row i = x_{i+1}, rounded once (column 12 is x0[12], the gravity constant, in every row)
 *   cost[batch][2]        binary64, from the un-rounded states, in a fixed summation order:
 *                         cost[0] = sum_{s<12} sum_i weights[s] (x_{i+1}[s] - traj[12 i + s])^2       (tracking)
 *                         cost[1] = sum_{c<U} sum_i Alpha_K[c] u_i[c]^2                               (force)
 * cost[0] + cost[1] is the reference's QP objective plus the constant the QP drops (the cost of applying no force).  The states are
 * the model's own prediction; the binary32 matrix powers inside H and g (the reference's A_qp, B_qp) differ from it by their
 * round-off, 5e-7 absolute on states of order 1.
 * The prediction is a pure function of (record, hmpc_params, force buffer): it does not depend on launch shape, dispatch order or on
 * which pass wrote the forces.  An instance whose status word is not HMPC_S_OK / HMPC_S_OK_RELAXED is predicted all the same, from
 * whatever its slot of the force buffer holds -- the last iterate, or zeros (HMPC_S_TOO_LARGE, HMPC_S_SWEEP_MISMATCH,
 * HMPC_S_INDEFINITE): check the status words.
 *
 * hmpc_predict_states enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing: put
 * it on the solve's stream, behind the solve and the device-side repair (hmpc_set_device_repair) if that is on.  It reads the forces
 * where the solve wrote them (hmpc_set_device_outputs is honoured).  HMPC_E_ARG, nothing enqueued, when no solve -- hmpc_solve,
 * hmpc_solve_command_sweep, hmpc_tick_solve_device, hmpc_debug_solve_external_qp -- has been enqueued since the current batch was set.
 * hmpc_set_device_prediction: caller-owned device buffers for later predictions (either may be NULL = the handle's own, which are
 * allocated for max_batch by the first call that needs them; never inside hmpc_solve).  hmpc_get_device_prediction: where the next
 * prediction goes.  hmpc_download_prediction waits for the stream of the last call, then copies (either pointer may be NULL);
 * HMPC_E_ARG when nothing has been predicted since the last solve of the current batch.  It does NOT run the safe pass: for repaired
 * forces call hmpc_download (or hmpc_resolve_failed) first, then hmpc_predict_states again.
 * Device groups: per member, through hmpc_group_member. */
int hmpc_predict_states(hmpc_handle *h, void *stream);
int hmpc_set_device_prediction(hmpc_handle *h, float *device_states, double *device_cost);
int hmpc_get_device_prediction(hmpc_handle *h, float **device_states, double **device_cost);
int hmpc_download_prediction(hmpc_handle *h, float *states, double *cost);
/* ... of the process-global solver behind setup_problem / update_problem_data: component (0..12) of the state predicted for
 * `step` (0..horizon-1: x_{step+1}) under the last solution.  Predicts lazily, once per solve, on first use (one launch, one
 * copy).  0 before the first solve and for out-of-range arguments, as get_solution. */
double hmpc_legacy_predicted_state(int step, int component);
/* ---- the constraint margins of every solved instance ----
 * How far the forces in the force buffer are from each limit the QP was solved under.  Per instance, with NC contacts, U = 6 NC,
 * Fc[8 NC][U] THE binary32 constraint block the solve kernel assembles for the record (hmpc_params and hmpc_set_instance_mu included;
 * the margins kernel calls the solve kernel's own assembly stage) and u_i[U] step i of the handle's force buffer as it stands:
 *   c_{i,r} = sum_{k<U} Fc[r][k] u_i[k],   r = 8 c + j: row j of contact c,
 * evaluated in binary64 as one ascending chain of fused multiply-adds started at +0 (every term, the structural zeros too).
 * Contact c is in stance at step i by the rule that sizes the QP: ub7 = fl32(cap_c * (float)gait[NC i + c]) is not within 1e-4 of
 * zero (cap_c = f_max for the feet, the record's own cap for the hand).  Ten one-sided slacks per leg-step, >= 0 when the limit holds:
 *   slack[batch][h][NC][10]  binary64
 *     [0..3]  c_{8c+0..3}                                friction pyramid (Fz -+ mu Fx, Fz -+ mu Fy >= 0)
 *     [4]     c_{8c+4}                                   Mx >= 0
 *     [5]     (double)0.01f - c_{8c+4}                   Mx <= 0.01
 *     [6],[7] 0.0 - c_{8c+5},  0.0 - c_{8c+6}            line contact: toe, heel (<= 0)
 *     [8]     c_{8c+7}                                   Fz floor (the row is 2 Fz >= 0)
 *     [9]     (double)ub7 - c_{8c+7}                     Fz cap
 *   All ten are +inf for a swing leg-step: its variables were eliminated, these rows are no constraints of the QP.
 *   summary[batch][6] binary64, where[batch][6] int32: per class the lexicographic (value, index) minimum over the stance leg-steps,
 *   index = 10 NC i + 10 c + j'.  A candidate replaces the incumbent iff its value is < the incumbent's, or == with a lower index, so
 *   a NaN never enters and the result does not depend on the order of the reduction.  No candidate: +inf and where = -1.
 *     [0] friction        j' 0..3          [1] Mx            j' 4, 5          [2] line contact   j' 6, 7
 *     [3] Fz floor        j' 8             [4] Fz cap        j' 9
 *     [5] friction headroom fraction: per stance leg-step with slack[8] > 0, m / (0.5 * slack[8]) (one IEEE division), m = the least
 *         of slack[0..3] by <, started at +inf; index = 10 NC i + 10 c.  1 = no tangential force, 0 = on the pyramid.
 * The result is a pure function of (record, hmpc_params, per-instance mu, force buffer).  An instance whose status word is not
 * HMPC_S_OK / HMPC_S_OK_RELAXED is computed all the same, from whatever its slot of the force buffer holds: check the status words.
 * After hmpc_debug_solve_external_qp the margins are still against the handle's OWN assembly of the record, not the block handed in.
 *
 * hmpc_constraint_margins enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing.
 * It reads the forces where the solve wrote them (hmpc_set_device_outputs is honoured) and needs no prediction.  HMPC_E_ARG, nothing
 * enqueued, when no solve has been enqueued since the current batch was set (the rule of hmpc_predict_states).
 * hmpc_set_device_margins: caller-owned device buffers for later margins (any may be NULL = the handle's own, allocated for max_batch
 * by the first call that needs them; never inside hmpc_solve).  hmpc_get_device_margins: where the next margins go; any pointer may be
 * NULL.  hmpc_download_margins waits for the stream of the last call, then copies (any pointer may be NULL); HMPC_E_ARG when nothing
 * has been computed since the last solve of the current batch.  It does NOT run the safe pass.
 * hmpc_margin_penalty enqueues one launch: device_penalty_out[i] = +inf if for some k with a non-NaN floor[k] the test
 * summary[i][k] >= floor[k] is false (a NaN summary therefore masks), else device_penalty_in[i] (+0.0 when device_penalty_in is NULL).
 * In-place is allowed.  The output is a device_penalty of hmpc_sweep_select.  HMPC_E_ARG without margins of the last solve.
 * hmpc_set_sweep_margin_floor: floor[6] for hmpc_tick_sweep_device, NULL = off (the default).  When set, the tick enqueues the
 * margins and the penalty between its prediction and its selection; the penalty goes to scratch of the handle and the caller's
 * device_penalty is its device_penalty_in.  When off the tick enqueues exactly the launches it did without.
 * Device groups: per member, through hmpc_group_member. */
int hmpc_constraint_margins(hmpc_handle *h, void *stream);
int hmpc_set_device_margins(hmpc_handle *h, double *device_slack, double *device_summary, int32_t *device_where);
int hmpc_get_device_margins(hmpc_handle *h, double **device_slack, double **device_summary, int32_t **device_where);
int hmpc_download_margins(hmpc_handle *h, double *slack, double *summary, int32_t *where);
int hmpc_margin_penalty(hmpc_handle *h, const double floor[6], const double *device_penalty_in, double *device_penalty_out, void *stream);
int hmpc_set_sweep_margin_floor(hmpc_handle *h, const double floor[6]);
/* ... of the process-global solver behind setup_problem / update_problem_data: slack j (0..9) of `contact` (0, 1) at `step`
 * (0..horizon-1) under the last solution.  Computed lazily, once per solve, on first use (one launch, one copy).  0 before the first
 * solve and for out-of-range arguments, as get_solution. */
double hmpc_legacy_constraint_slack(int step, int contact, int j);
/* ---- the KKT certificate and the Lagrange multipliers of every solved instance ----
 * Whether the forces in the force buffer minimise the QP, and the QP's dual solution.  Per instance, let NC be the number of contacts
 * and U = 6 NC.  Let x0, Acd, Bcd, Fc, the weights w[12], the trajectory, Alpha_K[U], the gait and the caps be the binary32 values the
 * solve kernel's assembly stage builds for the record (hmpc_params and hmpc_set_instance_mu included), and u_i[U] step i of the force
 * buffer as it stands.  Everything below is binary64.  Every sum is one ascending chain of explicit fused multiply-adds started at +0,
 * dense, with the structural zeros taking part.
 *   1. States.  x_1 .. x_h exactly as hmpc_predict_states defines them, un-rounded.
 *   2. Costate.  q_i[s] = (w_s + w_s) (x_i[s] - traj[12 (i-1) + s]) for s < 12, q_i[12] = 0, for i = 1 .. h.  p_h = q_h.  For
 *      i = h-1 .. 1: p_i[s] = q_i[s] + sum_{k<13} Acd[k][s] p_{i+1}[k] (the chain runs first; one addition follows).
 *   3. Gradient.  For i = 0 .. h-1 and c < U: grad_i[c] = fma(alpha_c + alpha_c, u_i[c], sum_{k<13} Bcd[k][c] p_{i+1}[k]).  This is the
 *      gradient of cost[0] + cost[1] of the prediction; in exact arithmetic it equals H u + g of the reference's QP.
 *   4. Slacks.  s[i][c][0..9] and the stance rule are exactly those of hmpc_constraint_margins.
 *   5. Multipliers of stance leg-step (i, c).  cols(c) = {3c, 3c+1, 3c+2, 3NC+3c, 3NC+3c+1, 3NC+3c+2}; r = grad_i[cols(c)] in R^6;
 *      n_j' = sigma_j' Fc[8c + src(j')][cols(c)] with src = (0,1,2,3,4,4,5,6,7,7) and sigma = (+,+,+,+,+,-,-,-,+,-) (rows 8c .. 8c+7 of
 *      Fc are zero outside cols(c)).  The active set is A = { j' : s[j'] <= act_tol }; a NaN slack is not active.
 *      lambda_A = argmin over lambda >= 0 of |r - N_A lambda|_2, e = r - N_A lambda_A; elsewhere lambda_j' = 0.  With A empty, e = r.
 *      A swing leg-step has lambda = 0 and e = 0: its variables were eliminated.  e is unique (the residual of a projection on a closed
 *      convex cone); lambda is unique iff the active normals are linearly independent.  Stationarity of the QP at u means e = 0 on
 *      every stance leg-step.
 *   6. Algorithm.  Lawson-Hanson active-set NNLS over the columns of A in ascending j', ties to the lowest j'.  The passive-set least
 *      squares goes through the Cholesky factor of the <= 6 x 6 Gram matrix.  A column whose pivot falls below 1e-12 of its own
 *      diagonal is not admitted: a dependent normal never enters the passive set, so |P| <= 6.  A column admitted and given no
 *      positive weight by its first solution leaves again at once; a column refused either way is not proposed again until lambda
 *      has moved.  At most 32 outer and 32 inner steps in total; a solution that is not finite ends the loop.  Whatever lambda >= 0 the
 *      loop holds when it stops is the answer, and e is recomputed from that lambda (dense over the ten j', ascending): any lambda >= 0
 *      is a valid certificate and the residual reported is the residual of the lambda reported, so a NaN or an iteration cap can make
 *      a certificate pessimistic but never wrong.  The loop terminates on NaN input.
 *   7. act_tol: hmpc_set_certificate_tolerance, default 1e-3 -- derived, not tuned: >= 8 x the slack that binary32 rounding of a force at
 *      the cap leaves on an active row (500 N * 2^-24 * |row|_1 <~ 1.2e-4), and 5 x below half the Mx window (0.005), above which both
 *      sides of row 4 would be active at once.  HMPC_E_ARG unless 0 < act_tol < 0.005.
 *   8. summary[batch][4] binary64 and where[batch][2] int32: maxima over the stance leg-steps.  A candidate v counts as +inf when it is
 *      NaN; it replaces the incumbent iff it is greater, or equal with a lower index.  No candidate: 0 and -1.  The reduction does
 *      not depend on its order.
 *        [0] stationarity: max |e_k|; where[0] = 6 (NC i + c) + k.
 *        [1] complementarity: max over active j' of lambda_j' * max(s_j', 0); where[1] = 10 NC i + 10 c + j'.
 *        [2] primal violation: max of max(0, -s_j') over all ten slacks (a NaN slack is a NaN candidate).
 *        [3] gradient scale: max |grad_i[c]| over the stance variables, for callers who want a relative test.
 * Outputs: grad[batch][h][U], lambda[batch][h][NC][10], resid[batch][h][NC][6] (= e), summary, where; all binary64 except where.  The
 * result is a pure function of (record, hmpc_params, per-instance mu, force buffer, act_tol).  Instances that are not HMPC_S_OK are
 * computed all the same.
 *
 * hmpc_kkt_certificate enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance, sharing nothing with the solver
 * but the assembly stage) and synchronises nothing.  It reads the forces where the solve wrote them and needs neither a prediction nor
 * margins.  HMPC_E_ARG, nothing enqueued, when no solve of the current batch has been enqueued.
 * hmpc_set_device_certificate: caller-owned device buffers for later certificates (any may be NULL = the handle's own, allocated for
 * max_batch by the first call that needs them; never inside hmpc_solve).  hmpc_get_device_certificate: where the next certificate
 * goes; any pointer may be NULL.  hmpc_download_certificate waits for the stream of the last call, then copies (any pointer may be
 * NULL); HMPC_E_ARG when nothing has been computed since the last solve of the current batch.  It does NOT run the safe pass.
 * hmpc_certificate_penalty enqueues one launch: device_penalty_out[i] = +inf if for some k < 3 with a non-NaN ceil[k] the test
 * summary[i][k] <= ceil[k] is false (a NaN summary therefore masks), else device_penalty_in[i] (+0.0 when device_penalty_in is NULL).
 * In-place is allowed.  The output is a device_penalty of hmpc_sweep_select.  HMPC_E_ARG without a certificate of the last solve.
 * hmpc_set_sweep_certificate_ceiling: ceil[3] for hmpc_tick_sweep_device, NULL = off (the default).  When set, the tick enqueues the
 * certificate and its penalty between its prediction and its selection, behind the margin penalty when a margin floor is set as well
 * (chained through the same scratch of the handle).  When off the tick enqueues exactly the launches it did without.
 * Device groups: per member, through hmpc_group_member. */
int hmpc_kkt_certificate(hmpc_handle *h, void *stream);
int hmpc_set_device_certificate(hmpc_handle *h, double *device_grad, double *device_lambda, double *device_resid, double *device_summary,
                                int32_t *device_where);
int hmpc_get_device_certificate(hmpc_handle *h, double **device_grad, double **device_lambda, double **device_resid, double **device_summary,
                                int32_t **device_where);
int hmpc_download_certificate(hmpc_handle *h, double *grad, double *lambda, double *resid, double *summary, int32_t *where);
int hmpc_set_certificate_tolerance(hmpc_handle *h, double act_tol);
int hmpc_certificate_penalty(hmpc_handle *h, const double ceil[3], const double *device_penalty_in, double *device_penalty_out, void *stream);
int hmpc_set_sweep_certificate_ceiling(hmpc_handle *h, const double ceil[3]);
/* ... of the process-global solver behind setup_problem / update_problem_data: multiplier j (0..9) of `contact` (0, 1) at `step`
 * (0..horizon-1), and summary[0] (the stationarity residual), of the last solution.  Computed lazily, once per solve, on first use (one
 * launch, two copies).  0 before the first solve and for out-of-range arguments, as get_solution. */
double hmpc_legacy_multiplier(int step, int contact, int j);
double hmpc_legacy_stationarity(void);
/* ---- the feedback gains of every solved instance; first-order force updates ----
 * At the optimum the MPC also defines a local linear policy: how the step-0 wrench changes when the state estimate or the reference
 * trajectory moves a little while the active limits stay the same.  Per instance, let NC be the number of contacts and U = 6 NC.  Let
 * Acd[13][13], Bcd[13][U], Fc, the weights w[12], Alpha_K[U], the gait and the caps be the binary32 values the solve kernel's assembly
 * stage builds for the record (hmpc_params and hmpc_set_instance_mu included), and u_i[U] step i of the force buffer as it stands.
 * Everything below is binary64.  Every sum is one ascending chain of explicit fused multiply-adds started at +0; sums over a column
 * (row) of Z_i run over the six rows (the columns) of its contact, all others are dense.
 *   1. Slacks, stance rule, active set: exactly hmpc_kkt_certificate's.  j' is active iff s[i][c][j'] <= act_tol, the value of
 *      hmpc_set_certificate_tolerance; a NaN slack is not active.
 *   2. Free directions of stance leg-step (i, c).  The active normals n_j' (as in the certificate) are orthonormalised in R^6 in
 *      ascending j' by modified Gram-Schmidt applied twice.  A normal is admitted, divided by its remaining length, iff fewer than six
 *      vectors are held, its squared remainder is > 0 and it is >= 1e-12 of the normal's own squared length (the certificate's dependence
 *      rule).  The basis is completed with unit vectors e_k: each time the one not yet taken whose squared remainder (reduced the same
 *      way) is largest, ties to the lowest k, divided by its remaining length, until six vectors are held.  These completions are the
 *      columns of Z_{i,c} (6 x (6 - m)); a swing leg-step has none.  Z_i (U x r_i) places every Z_{i,c} on cols(c), contacts
 *      ascending.  free_dims[i] = r_i.
 *   3. Backward pass.  Q = diag(w + w, 0) (13 x 13), R = diag(Alpha_K + Alpha_K), P_h = Q.  For i = h-1 .. 0, with P = P_{i+1}:
 *      PA = P Acd, PB = P Bcd, W = R + Bcd' PB, G_i = Z_i' (W Z_i), factored by Cholesky from its lower triangle (pivot d_j = G_jj -
 *      sum_{b<j} L_jb^2, L_jj = sqrt(d_j)); X = G_i^-1 (Z_i' Bcd') by two triangular solves; S_i = Z_i X (U x 13); K_i = 0 - S_i PA
 *      (S_i and K_i are exactly 0 when r_i = 0).  For i > 0: M_i = Acd + Bcd K_i, P_i = Q + PA' M_i, evaluated on the upper triangle
 *      and copied to the lower.
 *   4. Outputs.  gain[batch][U][13] = K_0 = du_0/dx_0.  ref_gain[batch][h][U][12]: row j-1 is Psi_j[c][s] (w_s + w_s) for s < 12, with
 *      Psi_1 = S_0 and Psi_{j+1} = Psi_j M_j'; it is du_0/dtraj of step j (traj[12 (j-1) + s]).  free_dims[batch][h], int32.
 *      summary[batch][2]: [0] the smallest ratio d_j / G_jj over the pivots of every G_i (1 when no G_i exists; a NaN ratio counts as
 *      0), [1] max |K_0| (a NaN entry counts as +inf).
 *   5. Meaning.  These are the derivatives of the QP's solution in (x_0, X_d) with the linearisation (Acd, Bcd, Fc) and the active set
 *      frozen: exact wherever the active set is locally constant.  At a weakly active limit the solution has one-sided derivatives only,
 *      and the gain reported is the frozen set's.  Rows of a swing contact are exactly 0, and N_A' K_0 = 0 for the active normals of
 *      every stance leg-step of step 0: a first-order update stays on the active limits.  The result is a pure function of (record,
 *      hmpc_params, per-instance mu, force buffer, act_tol).  Instances that are not HMPC_S_OK are computed all the same.
 *   6. Termination.  Every loop's trip count is fixed by (h, NC) and the number of vectors held; nothing iterates on data, so NaN input
 *      ends like any other.
 *
 * hmpc_feedback_gains enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance, sharing nothing with the solver
 * but the assembly stage: no H, no H^-1) and synchronises nothing.  It reads the forces where the solve wrote them.  HMPC_E_ARG, nothing
 * enqueued, when no solve of the current batch has been enqueued.
 * hmpc_set_device_gains: caller-owned device buffers for later gains (any may be NULL = the handle's own, allocated for max_batch by
 * the first call that needs them; never inside hmpc_solve); moving the buffers makes gains already computed stale.
 * hmpc_get_device_gains: where the next gains go; any pointer may be NULL.  hmpc_download_gains waits for the stream of the last call,
 * then copies (any pointer may be NULL); HMPC_E_ARG when nothing has been computed since the last solve of the current batch.  It does
 * NOT run the safe pass.
 *
 * hmpc_first_order_wrench enqueues ONE launch: device_records_new is `batch` records of the handle's stride in HBM, the same robots a
 * moment later.  The kernel assembles x0' of the new record through the same stage function; dx = (double)x0' - (double)x0 as it is
 * (a yaw that wraps is the caller's business, as in the reference); dt_j = (double)traj'_j - (double)traj_j.
 *   wrench[batch][U] = (float)((double)u_0[c] + chain_c), chain_c the ascending chain of fused multiply-adds from +0 over
 *   gain[c][s] dx[s] (s < 13), then ref_gain[j][c][s] dt_j[s] (j < h ascending, s < 12): identical records give step 0 of the force
 *   buffer bit for bit.  worst_slack[batch]: the least of the ten step-0 slacks of every stance contact at that wrench (binary32, as
 *   stored), against the ORIGINAL record's Fc and caps; +inf with no stance contact; a NaN slack never enters.  What to do when it goes
 *   negative is the caller's decision.
 * It needs gains of the last solve of the current batch (HMPC_E_ARG otherwise, and for a NULL pointer; nothing enqueued), and changes
 * neither the force buffer nor any result state but its own.  hmpc_set_device_first_order / hmpc_download_first_order: as above.
 * Device groups: per member, through hmpc_group_member. */
int hmpc_feedback_gains(hmpc_handle *h, void *stream);
int hmpc_set_device_gains(hmpc_handle *h, double *device_gain, double *device_ref_gain, double *device_summary, int32_t *device_free_dims);
int hmpc_get_device_gains(hmpc_handle *h, double **device_gain, double **device_ref_gain, double **device_summary,
                          int32_t **device_free_dims);
int hmpc_download_gains(hmpc_handle *h, double *gain, double *ref_gain, double *summary, int32_t *free_dims);
int hmpc_first_order_wrench(hmpc_handle *h, const void *device_records_new, void *stream);
int hmpc_set_device_first_order(hmpc_handle *h, float *device_wrench, double *device_worst_slack);
int hmpc_download_first_order(hmpc_handle *h, float *wrench, double *worst_slack);
/* ... of the process-global solver behind setup_problem / update_problem_data: entry [component][state] (0..11, 0..12) of K_0 of the
 * last solution.  Computed lazily, once per solve, on first use (one launch, one copy).  0 before the first solve and for
 * out-of-range arguments, as get_solution. */
double hmpc_legacy_feedback_gain(int component, int state);
/* ---- the adjoint of the solve: loss gradients in the state, the reference, the weights and Alpha_K ----
 * A sweep or a learning loop has a scalar loss L(u) over the whole force trajectory and wants its gradient in what it tunes.  With the
 * active limits frozen the solution map is that of an equality-constrained LQ problem, and ONE backward / forward sweep turns the seed
 * dL/du into all of those gradients.  Per instance, let NC be the number of contacts and U = 6 NC.  The assembly (x0, Acd, Bcd, Fc, w[12],
 * traj, Alpha_K[U], gait, caps; hmpc_params and hmpc_set_instance_mu included) enters exactly as for hmpc_feedback_gains, and u_i[U] is step
 * i of the force buffer as it stands.  The seed l[batch][h][U], binary64, is a caller-owned device pointer and stands for dL/du.
 * Everything below is binary64.  Every sum is one ascending chain of explicit fused multiply-adds started at +0; "a ; b" continues
 * chain a with the terms of b.  A = Acd, B = Bcd, q2 = (w + w, 0), l_i = l[i][.].
 *   1. Slacks, stance rule, active set and free directions Z_i: exactly hmpc_feedback_gains' (items 1, 2), with the same act_tol.
 *   2. Matrix backward pass: exactly hmpc_feedback_gains' (item 3), chain for chain: P_h = Q, then PA, PB, W, G_i, the Cholesky factor,
 *      S_i, K_i, M_i, P_i; M_0 = A + B K_0 is formed as well (P_0 is not).
 *   3. Vector backward pass, p_h = 0.  For i = h-1 .. 0, with p = p_{i+1}:
 *        v[c]   = l_i[c] + sum_{k<13} B[k][c] p[k]
 *        y[a]   = sum_k Z_i[k][a] v[k] over the six rows of column a's contact; y <- G_i^-1 y through the Cholesky factor: the two
 *                 triangular solves of the gains' X, with their chains (forward: b < a ascending; backward: a < b < r_i ascending)
 *        k_i[c] = 0 - sum_b Z_i[c][b] y[b] over the columns of c's contact (exactly 0 when r_i = 0)
 *        p_i[s] = sum_{k<13} M_i[k][s] p[k] ; sum_{c<U} K_i[c][s] l_i[c]
 *   4. Forward pass, dx_0 = 0.  For i = 0 .. h-1:
 *        du_i[c]     = (sum_{s<13} K_i[c][s] dx_i[s]) + k_i[c]
 *        dx_{i+1}[s] = sum_{k<13} A[s][k] dx_i[k] ; sum_{c<U} B[s][c] du_i[c]
 *      x_1 .. x_h exactly as hmpc_predict_states defines them, un-rounded.
 *   5. Outputs.
 *        grad_x0[batch][13]      = p_0
 *        grad_traj[batch][h][12]   row j-1: 0 - q2[s] dx_j[s]                                   (d/d traj[12 (j-1) + s])
 *        grad_weights[batch][12] = sum_{j=1..h} (e + e) dx_j[s],  e = x_j[s] - traj[12 (j-1) + s]
 *        grad_alpha[batch][U]    = sum_{i<h} (u_i[c] + u_i[c]) du_i[c]
 *        dir[batch][h][U]        = du_i.  It is -Z (Z'HZ)^-1 Z' l of the condensed QP; the gradient in any other parameter theta is
 *                                  sum dir . d(Hu + g)/d theta: hmpc_adjoint_model below returns it for r, the mass and the body inertia
 *                                  (gravity is grad_x0[12]) and hmpc_adjoint_limits further below for mu, lt, lh and the Fz caps, which
 *                                  enter through the constraint block; left to the caller are the orientation and the joint angles
 *                                  (through grad_A, grad_B, grad_x0 and grad_Fc of these calls) by these three alone;
 *                                  hmpc_adjoint_record, behind all three, chains them through the assembly.
 *        summary[batch][2]       [0] the smallest pivot ratio: hmpc_feedback_gains' summary[0], bit for bit; [1] max |dir| (a NaN
 *                                  entry counts as +inf).
 *   6. Meaning.  The outputs are the derivatives of L(u*(x0, X_d, w, Alpha_K)) with the linearisation (Acd, Bcd, Fc) and the active
 *      set frozen: exact wherever the active set is locally constant; at a weakly active limit there are one-sided derivatives only and
 *      the frozen set's is reported, as for the gains.  The seed e_c at step 0 returns row c of the gains (grad_x0 = gain[c][.],
 *      grad_traj[j] = ref_gain[j][c][.]).  Rows of dir on swing contacts are exactly 0, finite seed entries on swing contacts change no
 *      output bit, and a zero seed gives zeros.  No loop iterates on data, so NaN input ends like any other.  The result is a pure
 *      function of (record, hmpc_params, per-instance mu, force buffer, act_tol, seed).
 *
 * hmpc_solve_adjoint enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing.  It
 * reads the forces where the solve wrote them and needs no gains.  HMPC_E_ARG, nothing enqueued: a NULL seed, or no solve of the
 * current batch has been enqueued.  One seed per call (several: hmpc_solve_adjoint_multi below).
 * hmpc_set_device_adjoint: caller-owned device buffers for later adjoints (any may be NULL = the handle's own, allocated for max_batch
 * by the first call that needs them; never inside hmpc_solve); moving the buffers makes an adjoint already computed stale, as do every
 * solve and every new batch.  The gains and the first-order wrench are not touched by any of these calls, nor they by theirs.
 * hmpc_get_device_adjoint: where the next adjoint goes; any pointer may be NULL.  hmpc_download_adjoint waits for the stream of the last
 * call, then copies (any pointer may be NULL); HMPC_E_ARG when nothing has been computed since the last solve of the current batch.  It
 * does NOT run the safe pass.  With no batch set (batch = 0) it copies nothing and returns HMPC_OK, as hmpc_download_gains does; the
 * launch itself is refused there, there being no solve.
 * Device groups: per member, through hmpc_group_member.  There is no accessor on the process-global solver behind setup_problem /
 * update_problem_data: a seed has no place in that interface. */
int hmpc_solve_adjoint(hmpc_handle *h, const double *device_seed, void *stream);
int hmpc_set_device_adjoint(hmpc_handle *h, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                            double *device_grad_alpha, double *device_dir, double *device_summary);
int hmpc_get_device_adjoint(hmpc_handle *h, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                            double **device_grad_alpha, double **device_dir, double **device_summary);
int hmpc_download_adjoint(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, double *grad_alpha, double *dir,
                          double *summary);
/* ---- multi-seed adjoint: several loss gradients of the same solve behind one matrix backward pass ----
 * hmpc_solve_adjoint under n_seeds seeds at once: the Jacobian of a step's wrench (unit seeds), Gauss-Newton on a vector residual,
 * several losses on one sweep.  The assembly, the free directions and the matrix backward pass do not depend on the seed and run once
 * per launch; each seed's vector recursion and forward pass run beside them.
 *   Definition.  Seed s is, chain for chain, items 3-5 of hmpc_solve_adjoint's contract above: every output of slice s is bit for bit
 *   what hmpc_solve_adjoint returns under that seed alone (summary[s][.][0] is therefore the same for every s).
 *   Layouts, seed-major over the CURRENT batch: device_seeds[n_seeds][batch][h][U]; grad_x0[n_seeds][batch][13],
 *   grad_traj[n_seeds][batch][h][12], grad_weights[n_seeds][batch][12], grad_alpha[n_seeds][batch][U], dir[n_seeds][batch][h][U],
 *   summary[n_seeds][batch][2], all binary64: slice s of every array has exactly the layout of a single-seed call on the current batch.
 *   The seeds must not overlap the outputs.
 * hmpc_solve_adjoint_multi enqueues ceil(n_seeds / (6 NC)) launches on `stream` -- ONE for n_seeds <= U -- and synchronises nothing.
 * HMPC_E_ARG, nothing enqueued: NULL seeds, n_seeds outside 1 .. HMPC_ADJOINT_MAX_SEEDS, no solve of the current batch, more seeds than
 * the caller's buffers hold, or inside a solve on an external constraint block.  hmpc_solve_adjoint, its buffers, what
 * hmpc_get_device_adjoint returns and an adjoint it computed are not touched.
 * hmpc_set_device_adjoint_multi: caller-owned device buffers with room for n_seeds slices (any may be NULL = the handle's own, reserved
 * for (n_seeds, max_batch) by the launch that needs them and grown by a later launch with more seeds; never inside hmpc_solve; with all
 * six NULL n_seeds is not read).  HMPC_E_ARG when a buffer is given and n_seeds lies outside 1 .. HMPC_ADJOINT_MAX_SEEDS.
 * hmpc_get_device_adjoint_multi: slice 0 of where the multi-seed adjoint is or goes next (one of the handle's own that no launch has
 * reserved yet: NULL) and the seeds of the one that stands (0: none); any pointer may be NULL.  hmpc_download_adjoint_multi waits for the
 * stream of the last call, then copies the slices of the seeds enqueued (any pointer may be NULL); HMPC_E_ARG when no multi-seed
 * adjoint stands; with no batch set it copies nothing and returns HMPC_OK.
 * A multi-seed adjoint goes stale on every solve, every new batch and every hmpc_set_device_adjoint_multi.
 * hmpc_select_adjoint_seed(h, s) makes slice s of the multi-seed adjoint that stands the handle's CURRENT adjoint: pointer arithmetic on
 * the host, no launch, no copy.  hmpc_adjoint_model, hmpc_adjoint_limits, hmpc_adjoint_record and hmpc_download_adjoint then behave
 * exactly as after hmpc_solve_adjoint under that seed; hmpc_adjoint_limits is handed the seed's own slice, device_seeds + s batch h U.
 * The current adjoint is whichever came last of hmpc_solve_adjoint and a selection; a selection makes model, limit and record gradients
 * stale as a new adjoint does, and falls with the multi-seed adjoint it points into (also when a new hmpc_solve_adjoint_multi overwrites
 * it).  HMPC_E_ARG: s outside 0 .. n_seeds - 1, or no multi-seed adjoint stands.  Behind a selection the three downstream launches are one
 * seed each; hmpc_adjoint_chain_multi below runs them for every seed at once.
 * Device groups: per member, through hmpc_group_member; nothing on the process-global interface. */
#define HMPC_ADJOINT_MAX_SEEDS 240
int hmpc_solve_adjoint_multi(hmpc_handle *h, const double *device_seeds, int n_seeds, void *stream);
int hmpc_set_device_adjoint_multi(hmpc_handle *h, int n_seeds, double *device_grad_x0, double *device_grad_traj, double *device_grad_weights,
                                  double *device_grad_alpha, double *device_dir, double *device_summary);
int hmpc_get_device_adjoint_multi(hmpc_handle *h, int *n_seeds, double **device_grad_x0, double **device_grad_traj, double **device_grad_weights,
                                  double **device_grad_alpha, double **device_dir, double **device_summary);
int hmpc_download_adjoint_multi(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, double *grad_alpha, double *dir,
                                double *summary);
int hmpc_select_adjoint_seed(hmpc_handle *h, int s);
/* ---- model gradients of the solve: foot positions, mass, body inertia, Acd and Bcd themselves ----
 * Behind hmpc_solve_adjoint: the gradient of the same loss in what enters the QP through the prediction model.  With the active set
 * frozen and du = dir of the last adjoint, dL/dtheta = <G_A, dA/dtheta> + <G_B, dB/dtheta> for every theta that enters through A = Acd
 * and B = Bcd only; the constraint block does not depend on r, the mass or the inertia, so no multipliers are needed.  Per instance, NC
 * contacts, U = 6 NC; the assembly enters exactly as for hmpc_solve_adjoint (hmpc_params and hmpc_set_instance_mu included), u_i[U] is step
 * i of the force buffer as it stands, du_i[U] step i of the adjoint's dir buffer as it stands.  Everything below is binary64.  Every sum
 * is one ascending chain of explicit fused multiply-adds started at +0; "a ; b" continues chain a with the terms of b; q2 = (w + w, 0).
 *   1. Forward pass, x_0 = x0, dx_0 = 0.  For i = 0 .. h-1:
 *        x_{i+1}[s]  = sum_{k<13} A[s][k] x_i[k] ; sum_{c<U} B[s][c] u_i[c]          (exactly hmpc_predict_states', un-rounded)
 *        dx_{i+1}[s] = sum_{k<13} A[s][k] dx_i[k] ; sum_{c<U} B[s][c] du_i[c]        (item 4 of the adjoint, over the stored dir)
 *   2. Backward pass, c_{h+1} = d_{h+1} = 0.  For j = h .. 1, with t_c[s] = sum_{k<13} A[k][s] c_{j+1}[k], t_d likewise over d_{j+1}:
 *        c_j[s] = fma(q2[s], x_j[s] - traj[12 (j-1) + s], t_c[s])   for s < 12;   c_j[12] = t_c[12]
 *        d_j[s] = fma(q2[s], dx_j[s], t_d[s])                       for s < 12;   d_j[12] = t_d[12]
 *   3. Accumulation: per entry one chain over i = 0 .. h-1, per step the c term, then the d term:
 *        G_A[a][b] = sum_i ( c_{i+1}[a] dx_i[b] ; d_{i+1}[a] x_i[b] )                 (13 x 13)
 *        G_B[a][c] = sum_i ( c_{i+1}[a] du_i[c] ; d_{i+1}[a] u_i[c] )                 (13 x U)
 *   4. Chain rules.  Mb[a][m] = B[6+a][3 NC + m] is the assembled dt Iinv.  r_c[k] is the record's r[k NC + c] and cm_c = {0, -r_c[2],
 *      r_c[1]; r_c[2], 0, -r_c[0]; -r_c[1], r_c[0], 0} the cross matrix as the assembly writes it, binary32, widened.  R is the binary32
 *      rotation the assembly forms from the record's quaternion, widened.
 *        T_c[m][b]       = sum_{a<3} Mb[a][m] G_B[6+a][3c+b]
 *        grad_r[.][c]    = (T_c[2][1] - T_c[1][2], T_c[0][2] - T_c[2][0], T_c[1][0] - T_c[0][1])
 *        grad_mass       = 0 - (s B[9][0]) / mass,  s = +0 + G_B[9][0] + G_B[10][1] + G_B[11][2] + G_B[9][3] + ... (c ascending, then a),
 *                          mass the handle's hmpc_params value widened
 *        Gam[a][m]       = per c ascending: + G_B[6+a][3 NC + 3c + m], then ; sum_{b<3} G_B[6+a][3c+b] cm_c[m][b]   (zero entries included)
 *        w_k[a]          = sum_{m<3} Mb[a][m] R[m][k];   t_k[a] = sum_{m<3} Gam[a][m] w_k[m]
 *        grad_inertia[k] = 0 - (sum_{a<3} w_k[a] t_k[a]) / dt,  dt widened: exact for an un-normalised quaternion too
 *   5. Outputs: grad_A[batch][13][13] = G_A;  grad_B[batch][13][U] = G_B;  grad_r[batch][3][NC] in the record's order [axis][contact];
 *      grad_params[batch][4] = (grad_mass, grad_inertia[0..2]);  costate[batch][2][13] = (c_1, d_1).
 *   6. Meaning.  d L / d theta of L(u*(theta)) with the active set frozen, theta entering through Acd and Bcd: the foot positions, the
 *      mass and the inertia as the assembly uses them (first-order; the assembly's binary32 rounding is not differentiated), and through
 *      grad_A / grad_B the orientation or any parameterisation of the caller's.  A' d_1 is the adjoint's grad_x0 up to rounding.  The
 *      gradient in the gravity state is grad_x0[12] of the adjoint: nothing new is needed.  A zero seed gives zeros; columns of G_B on a
 *      contact that is swing at every step are exactly 0 (u and dir are 0 there).  No loop iterates on data, so NaN input ends like any
 *      other.  The result is a pure function of (record, hmpc_params, per-instance mu, force buffer, dir buffer).
 *      What enters through the constraint block instead (mu, lt, lh, the Fz caps) is hmpc_adjoint_limits' below.
 *
 * hmpc_adjoint_model enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing.  It reads
 * dir where the last adjoint wrote it.  HMPC_E_ARG, nothing enqueued: no adjoint of the last solve of the current batch has been enqueued
 * (every solve, every new batch and hmpc_set_device_adjoint make an adjoint stale).
 * hmpc_set_device_adjoint_model: caller-owned device buffers for later calls (any may be NULL = the handle's own, allocated for max_batch
 * by the first call that needs them; never inside hmpc_solve); moving the buffers makes model gradients already computed stale, as do
 * every solve, every new batch, every hmpc_solve_adjoint (a new seed) and hmpc_set_device_adjoint.
 * hmpc_get_device_adjoint_model: where the next model gradients go; any pointer may be NULL.  hmpc_download_adjoint_model waits for the
 * stream of the last call, then copies (any pointer may be NULL); HMPC_E_ARG when nothing has been computed since the last adjoint.  It
 * does NOT run the safe pass.  With no batch set (batch = 0) it copies nothing and returns HMPC_OK.
 * Device groups: per member, through hmpc_group_member.  There is no accessor on the process-global solver. */
int hmpc_adjoint_model(hmpc_handle *h, void *stream);
int hmpc_set_device_adjoint_model(hmpc_handle *h, double *device_grad_A, double *device_grad_B, double *device_grad_r,
                                  double *device_grad_params, double *device_costate);
int hmpc_get_device_adjoint_model(hmpc_handle *h, double **device_grad_A, double **device_grad_B, double **device_grad_r,
                                  double **device_grad_params, double **device_costate);
int hmpc_download_adjoint_model(hmpc_handle *h, double *grad_A, double *grad_B, double *grad_r, double *grad_params, double *costate);
/* ---- limit gradients of the solve: friction, foot length, the Fz caps, the constraint block itself ----
 * Behind hmpc_solve_adjoint: the gradient of the same loss in what enters the QP through the constraint block.  Per stance leg-step
 * (i, c), v = u_i[cols(c)], the ten one-sided slacks are s_j'(v) = n_j' . v + beta_j' with n_j' = sigma_j' Fc[8c + src(j')][cols(c)] (src
 * and sigma of hmpc_kkt_certificate) and beta = (0, 0, 0, 0, 0, (double)0.01f, 0, 0, 0, (double)ub7); the QP is min f(u) s.t. s >= 0.  With
 * the admitted active normals frozen, stationarity reads grad f = sum lambda_j' n_j'; for the loss L(u) with seed l = dL/du and the
 * adjoint's dir, rho_i = l_i + (H dir)_i and rho_i[cols(c)] = sum nu_j' n_j' on every stance leg-step (exact when dir and l belong
 * together), and
 *   dL/dtheta = (what hmpc_solve_adjoint / hmpc_adjoint_model return)
 *               - sum_{i,c,j'} lambda_j' (dn_j'/dtheta . dir_i[cols(c)]) - sum_{i,c,j'} nu_j' (dn_j'/dtheta . v + dbeta_j'/dtheta).
 * One stance leg-step with only the Fz cap active (n_9 = (0, 0, -2, 0, 0, 0)), dir = 0 and the seed e_Fz: nu_9 = -0.5, dL/dub7 = +0.5.
 * Per instance, NC contacts, U = 6 NC; the assembly enters exactly as for hmpc_solve_adjoint (hmpc_params and hmpc_set_instance_mu
 * included), u_i[U] is step i of the force buffer as it stands, du_i[U] step i of the adjoint's dir buffer as it stands, l_i[U] step i of
 * device_seed.  Everything below is binary64.  Every sum is one ascending chain of explicit fused multiply-adds started at +0; trip
 * counts are fixed by (h, NC) and the number of admitted normals (<= 6): no loop iterates on data.
 *   1. Forward and backward pass: items 1 and 2 of hmpc_adjoint_model, chain for chain: x_j, dx_j over the stored dir, then c_j, d_j.
 *   2. Gradient and residual, a2 = alpha + alpha:
 *        grad_i[k] = fma(a2[k], u_i[k],  sum_{a<13} B[a][k] c_{i+1}[a])
 *        hd_i[k]   = fma(a2[k], du_i[k], sum_{a<13} B[a][k] d_{i+1}[a])
 *        rho_i[k]  = l_i[k] + hd_i[k]
 *   3. Slacks, stance rule, active set: hmpc_constraint_margins' and hmpc_kkt_certificate's (j' active iff s_j' <= act_tol, NaN: not
 *      active), with the handle's act_tol (hmpc_set_certificate_tolerance).
 *   4. Admitted normals: the adjoint's own -- the decisions of hmpc_feedback_gains' item 2 (modified Gram-Schmidt applied twice, rule
 *      1e-12, at most six, ascending j').  q_0 .. q_{m-1} are the orthonormal vectors held, j_0 < .. < j_{m-1} the admitted rows.
 *   5. Multipliers.  T[a][b] = sum_{k<6} q_a[k] n_{j_b}[k] for a <= b, y_a = sum_{k<6} q_a[k] rhs[k]; for a = m-1 down to 0
 *        x_a = (y_a - sum_{b = a+1 .. m-1} T[a][b] x_b) / T[a][a].
 *      rhs = grad_i[cols(c)] gives lambda_{j_a} = x_a: the frozen set's multiplier, no sign constraint, reported as it comes;
 *      rhs = rho_i[cols(c)] gives nu_{j_a} = x_a.  Rows not admitted and swing leg-steps get exact zeros.
 *      Residual of either: e[k] = rhs[k] - sum_{b<m} n_{j_b}[k] x_b.
 *   6. Row gradients.  One chain per entry over i ascending and, inside a step, over the j' of the row ascending (rows 4 and 7 of a
 *      contact serve two j'), zero multipliers included:
 *        grad_Fc[8c + src(j')][col_k] <- fma(0 - sigma_j' lambda_j', du_i[col_k], .), then fma(0 - sigma_j' nu_j', (double)u_i[col_k], .)
 *      Entries outside the row's own cols(c) are exact zeros.
 *   7. Bound gradients.  grad_bound[i][c][j'] = 0 - nu_j' is dL/dbeta_j', raising beta_j' loosening limit j': index 5 is the Mx window,
 *      index 9 is ub7.
 *   8. Chain rules (the assembly's formulas are differentiated, not its binary32 rounding), G = grad_Fc:
 *        grad_mu     = over c ascending from +0: + G[8c+1][3c] - G[8c+0][3c] + G[8c+3][3c+1] - G[8c+2][3c+1]; also the gradient in the
 *                      instance's own mu under hmpc_set_instance_mu
 *        grad_lt     = (sum_c sum_{k<3} G[8c+5][3c+k] (double)Fc[8c+5][3c+k]) / lt;  grad_lh the same over row 6 and lh.  lt, lh: the handle's
 *                      hmpc_params values widened; a zero lt / lh gives what IEEE division gives (0/0 = NaN, x/0 = +-inf)
 *        grad_cap[c] = sum_i grad_bound[i][c][9] (double)(float)gait[NC i + c]
 *        grad_limits[batch][3 + NC] = (mu, lt, lh, cap_0 .. cap_{NC-1}).  f_max is cap_0 + cap_1; the hand's cap is cap_2.
 *   9. summary[batch][3]: maxima over the stance leg-steps, a NaN candidate counting as +inf, 0 with no candidate:
 *        [0] |grad - sum lambda n|_inf;  [1] |rho - sum nu n|_inf -- 0 in exact arithmetic when the seed is the one dir was made from: the
 *        caller's consistency check;  [2] max |grad_Fc|.
 *  10. Meaning.  The frozen-set derivatives, as for hmpc_feedback_gains, hmpc_solve_adjoint and hmpc_adjoint_model.  At a leg-step
 *      whose active rows are dependent (an unloaded foot: eight rows, rank 5) the admitted subset's gradient is reported.  Flagged
 *      instances are computed all the same.  The joint angles and the orientation go through grad_Fc (with grad_A, grad_B, grad_x0).
 *      The result is a pure function of (record, hmpc_params, per-instance mu, force buffer, dir buffer, seed, act_tol).
 *
 * hmpc_adjoint_limits enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing.  It reads
 * dir where the last adjoint wrote it and device_seed[batch][h][U] (binary64, caller-owned): the seed that adjoint was given, passed again
 * -- summary[1] tells whether it was.  HMPC_E_ARG, nothing enqueued: device_seed is NULL, or no adjoint of the last solve of the current
 * batch has been enqueued (every solve, every new batch and hmpc_set_device_adjoint make an adjoint stale).
 * hmpc_set_device_adjoint_limits: caller-owned device buffers for later calls (any may be NULL = the handle's own, allocated for max_batch
 * by the first call that needs them; never inside hmpc_solve): grad_limits[max_batch][3 + NC], grad_Fc[max_batch][8 NC][U], grad_bound,
 * lambda and nu [max_batch][horizon][NC][10], summary[max_batch][3].  Moving the buffers makes limit gradients already computed stale, as
 * do every solve, every new batch, every hmpc_solve_adjoint (a new seed) and hmpc_set_device_adjoint; hmpc_adjoint_model does not.
 * hmpc_get_device_adjoint_limits: where the next limit gradients go; any pointer may be NULL.  hmpc_download_adjoint_limits waits for the
 * stream of the last call, then copies (any pointer may be NULL); HMPC_E_ARG when nothing has been computed since the last adjoint.  It
 * does NOT run the safe pass.  With no batch set (batch = 0) it copies nothing and returns HMPC_OK.
 * Device groups: per member, through hmpc_group_member.  There is no accessor on the process-global solver. */
int hmpc_adjoint_limits(hmpc_handle *h, const double *device_seed, void *stream);
int hmpc_set_device_adjoint_limits(hmpc_handle *h, double *device_grad_limits, double *device_grad_Fc, double *device_grad_bound,
                                   double *device_lambda, double *device_nu, double *device_summary);
int hmpc_get_device_adjoint_limits(hmpc_handle *h, double **device_grad_limits, double **device_grad_Fc, double **device_grad_bound,
                                   double **device_lambda, double **device_nu, double **device_summary);
int hmpc_download_adjoint_limits(hmpc_handle *h, double *grad_limits, double *grad_Fc, double *grad_bound, double *lambda, double *nu,
                                 double *summary);
/* ---- pose gradients of the solve: orientation, joint angles, the whole record ----
 * Behind hmpc_solve_adjoint, hmpc_adjoint_model and hmpc_adjoint_limits: their outputs chained through stage A1 + A2 of the assembly, so
 * that the gradient of the same loss comes back IN EVERY FLOAT OF THE PACKED RECORD: p, v, q, w, r, the joint angles, the weights,
 * Alpha_K, the trajectory, and for three contacts the hand frame and the hand's cap.  grad_x0[0:3] of the adjoint is the gradient in the
 * Euler angles with the linearisation frozen; the quaternion also moves Acd (through Rb^-1(yaw, pitch)), Bcd (through I_w^-1 = (R I_b
 * R')^-1) and Fc (through the rows R Rf_c), and grad_record's q slice is the total.  Per instance, NC contacts, U = 6 NC; the buffers of
 * the three calls enter as they stand.  Everything below is binary64; every sum is one ascending chain of explicit fused multiply-adds
 * started at +0; trip counts are fixed by NC.  What is differentiated is the assembly's formula, not its binary32 rounding; the
 * assembly's own tabulated binary32 values enter widened: (s_k, c_k) the sine and cosine of joint angle k as the assembly holds them,
 * (s_b, c_b) those of a2 + a3 + a4 of a leg, (cy, sy, cp, sp) of yaw and pitch, R the rotation it forms from the record's quaternion,
 * Ab = Acd[0:3][6:9], Mb = Bcd[6:9][3 NC .. 3 NC + 2].  G_F = grad_Fc, cf = 3c, cmo = 3 NC + 3c, sigma_c = +1 for c = 1 and -1 otherwise (the
 * sign of the heel row's moment part), lt, lh, dt, I_b the handle's values widened.
 *   1. Foot frames.  For a foot c < 2 with joints 0 = 5c .. 4 = 5c + 4, t = s0 s1, v = c0 s1:
 *        Rf_c = { fma(c0, cb, 0 - t sb), 0 - s0 c1, fma(c0, sb, t cb);  fma(s0, cb, v sb), c0 c1, fma(s0, sb, 0 - v cb);  0 - c1 sb, s1, c1 cb }
 *      which is Rz(a0) Rx(a1) Ry(a2 + a3 + a4), what the assembly's expanded products equal.  Rf_2 is the record's Rhand, widened.
 *   2. Constraint block -> frames.  Gg_c[j][0] = G_F[8c+4][cmo+j];  Gg_c[j][1] = G_F[8c+5][cmo+j] + sigma_c G_F[8c+6][cmo+j];
 *        Gg_c[j][2] = fma(0 - lt, G_F[8c+5][cf+j], (0 - lh) G_F[8c+6][cf+j])                                    (j < 3)
 *        G_Rf[c][a][m] = sum_{j<3} R[j][a] Gg_c[j][m];      P_c[i][j] = sum_{m<3} Gg_c[i][m] Rf_c[j][m]
 *   3. Joint angles (c < 2), e = (c1 sb, 0 - s1, 0 - c1 cb), f = (s1 sb, c1, 0 - s1 cb):
 *        grad_ja[5c]       = sum_{k<3} G_Rf[c][0][k] (0 - Rf_c[1][k]) ; sum_{k<3} G_Rf[c][1][k] Rf_c[0][k]
 *        grad_ja[5c+1]     = sum_k G_Rf[c][0][k] ((0 - s0) e[k]) ; sum_k G_Rf[c][1][k] (c0 e[k]) ; sum_k G_Rf[c][2][k] f[k]
 *        grad_ja[5c+2..4]  = sum_{i<3} ( G_Rf[c][i][0] (0 - Rf_c[i][2]) ; G_Rf[c][i][2] Rf_c[i][0] )      one number, three times: the offsets
 *                            and the fmod of the assembly have derivative 1
 *   4. Inertia -> body rotation.  Gam as item 4 of hmpc_adjoint_model;  X[m][n] = sum_{a<3} Mb[a][m] Gam[a][n];  Y[m][k] = sum_{n<3}
 *        X[m][n] Mb[k][n];  G_Iw = 0 - Y / dt;  P_NC[i][k] = (sum_{j<3} (G_Iw[i][j] + G_Iw[j][i]) R[j][k]) I_b[k]
 *        G_R[i][j] = +0 + P_0[i][j] + .. + P_NC[i][j]
 *   5. Euler-rate map.  X'[m][n] = sum_a Ab[a][m] grad_A[a][6+n];  Y'[m][k] = sum_n X'[m][n] Ab[k][n];  G_Rb = 0 - Y' / dt;  with Rb =
 *        {cy cp, -sy, 0; sy cp, cy, 0; -sp, 0, 1} (roll does not enter):
 *        G_yaw   = G_Rb[0][0] (0 - sy cp) ; G_Rb[0][1] (0 - cy) ; G_Rb[1][0] (cy cp) ; G_Rb[1][1] (0 - sy)
 *        G_pitch = G_Rb[0][0] (0 - cy sp) ; G_Rb[1][0] (0 - sy sp) ; G_Rb[2][0] (0 - cp)
 *        grad_rpy = (grad_x0[0], grad_x0[1] + G_pitch, grad_x0[2] + G_yaw)
 *   6. Euler angles -> quaternion (qw, qx, qy, qz as the record holds them, un-normalised or not; t* = q* + q*).  The assembly's own
 *      binary32 numerators and denominators, widened: n0 = 2 (qw qx + qy qz), d0 = 1 - 2 (qx qx + qy qy), t = qw qy - qx qz, n2 = 2 (qw qz +
 *      qx qy), d2 = 1 - 2 (qy qy + qz qz) (d0, d2: the binary32 product subtracted in binary64, as the assembly does).
 *        J[0][k] = fma(d0, dn0[k], 0 - n0 dd0[k]) / fma(n0, n0, d0 d0),   dn0 = (tx, tw, tz, ty),  dd0 = (0, 0 - 2 tx, 0 - 2 ty, 0)
 *        J[1][k] = exactly 0 where the assembly's clamp !(2 t < 0.99999) holds, else das[k] / sqrt(fma(0 - 2 t, 2 t, 1)),  das = (ty, 0 - tz, tw, 0 - tx)
 *        J[2][k] = as J[0] over n2, d2,   dn2 = (tz, ty, tx, tw),  dd2 = (0, 0, 0 - 2 ty, 0 - 2 tz)
 *        E[k] = J[0][k] grad_rpy[0] ; J[1][k] grad_rpy[1] ; J[2][k] grad_rpy[2]
 *   7. Body rotation -> quaternion.  grad_q[k] = (sum over (i, j) row-major of G_R[i][j] dR[i][j]/dq_k) + E[k], dR/dq that of the polynomial
 *      R = {1 - ty qy - tz qz, tx qy - tz qw, ...}, zero entries included; no normalisation is differentiated.
 *   8. Outputs.  grad_record[batch][NF + 12 h] in the float order of the packed record (NF = 54 for two contacts, 73 for three): p, w, v <-
 *      grad_x0[3:6], [6:9], [9:12];  q <- grad_q;  r <- grad_r;  joint angles <- grad_ja;  yaw <- +0 (the solve never reads it);  weights <-
 *      grad_weights;  Alpha_K <- grad_alpha;  Rhand <- G_Rf[2];  f_max_hand <- grad_limits[3 + 2];  trajectory <- grad_traj.
 *      grad_frames[batch][1 + NC][9] = G_R, then G_Rf[c] per contact, row-major: for callers with their own leg kinematics.
 *      grad_rpy[batch][3] as item 5: the total gradient in the Euler angles.
 *   9. Meaning.  The frozen-set derivatives, as for the three calls behind it.  A contact that is swing at every step contributes exact
 *      zeros; a zero seed upstream gives zeros everywhere; no loop iterates on data, so NaN input ends like any other.  The gradients in
 *      the gait bytes and in f_max of the feet are not part of it (the latter is grad_limits' cap_0 + cap_1).  The result is a pure
 *      function of (record, hmpc_params, per-instance mu, the nine upstream buffers).
 *
 * hmpc_adjoint_record enqueues ONE launch on `stream` (a kernel of its own, 128 threads per instance) and synchronises nothing.  It reads
 * grad_x0, grad_traj, grad_weights, grad_alpha, grad_A, grad_B, grad_r, grad_limits and grad_Fc where the three calls last wrote them.
 * HMPC_E_ARG, nothing enqueued: hmpc_solve_adjoint, hmpc_adjoint_model and hmpc_adjoint_limits have not all three been enqueued behind
 * the last adjoint of the last solve of the current batch, or the handle is inside a solve on an external constraint block.
 * hmpc_set_device_adjoint_record: caller-owned device buffers for later calls (any may be NULL = the handle's own, allocated for max_batch
 * by the first call that needs them; never inside hmpc_solve).  Moving the buffers makes record gradients already computed stale, as
 * does whatever makes one of the three inputs stale or new: every solve, every new batch, every hmpc_solve_adjoint, hmpc_adjoint_model
 * and hmpc_adjoint_limits, and the three hmpc_set_device_adjoint* calls of theirs.
 * hmpc_get_device_adjoint_record: where the next record gradients go; any pointer may be NULL.  hmpc_download_adjoint_record waits for
 * the stream of the last call, then copies (any pointer may be NULL); HMPC_E_ARG when nothing has been computed since.  It does NOT run
 * the safe pass.  With no batch set (batch = 0) it copies nothing and returns HMPC_OK.
 * Device groups: per member, through hmpc_group_member.  There is no accessor on the process-global solver. */
int hmpc_adjoint_record(hmpc_handle *h, void *stream);
int hmpc_set_device_adjoint_record(hmpc_handle *h, double *device_grad_record, double *device_grad_frames, double *device_grad_rpy);
int hmpc_get_device_adjoint_record(hmpc_handle *h, double **device_grad_record, double **device_grad_frames, double **device_grad_rpy);
int hmpc_download_adjoint_record(hmpc_handle *h, double *grad_record, double *grad_frames, double *grad_rpy);
/* ---- the chain of the multi-seed adjoint: model, limit and record gradients of every seed behind one assembly ----
 * Behind hmpc_solve_adjoint_multi: for every seed of the multi-seed adjoint that stands, the chain hmpc_adjoint_model ->
 * hmpc_adjoint_limits -> hmpc_adjoint_record, so that the Jacobian of a step's wrench in every float of the record is two calls.  The
 * record load, the assembly, the forward chain x_j, the tracking costate c_j, grad_i, the slacks, the active set, the admitted normals
 * and lambda do not depend on the seed and are formed once per launch; each seed's dx_j, d_j, rho, nu, outer-product sums and chain
 * rules run beside them, their intermediates never leaving the chip unless a detail buffer asks for them.
 *   Definition, by reference: no arithmetic of its own.  Were the handle's state hmpc_select_adjoint_seed(h, s), then hmpc_adjoint_model,
 *   then hmpc_adjoint_limits(h, device_seeds + s batch h U), then hmpc_adjoint_record, slice s of every array below is bit for bit what
 *   the matching array of those three calls holds (items 1-5 of the model gradients, 1-9 of the limit gradients, 1-8 of the record
 *   gradients).  lambda, costate[.][0] and limit_summary[.][0] therefore carry the same bits in every slice.
 *   Layouts, seed-major over the CURRENT batch, all binary64; slice s of every array has exactly the layout of the single-seed call on
 *   the current batch.  Compact (always produced): grad_record[n_seeds][batch][NF + 12 h], grad_frames[n_seeds][batch][1 + NC][9],
 *   grad_rpy[n_seeds][batch][3] (hmpc_adjoint_record's), grad_params[n_seeds][batch][4] (hmpc_adjoint_model's),
 *   grad_limits[n_seeds][batch][3 + NC], limit_summary[n_seeds][batch][3] (hmpc_adjoint_limits').  Detail (written only where the caller
 *   gives a buffer): grad_A[..][13][13], grad_B[..][13][U], grad_r[..][3][NC], costate[..][2][13] (hmpc_adjoint_model's); grad_Fc[..][8 NC][U],
 *   grad_bound, lambda, nu[..][h][NC][10] (hmpc_adjoint_limits').
 *   Inputs: dir, grad_x0, grad_traj, grad_weights and grad_alpha of the multi-seed adjoint, where it last wrote them; device_seeds
 *   [n_seeds][batch][h][U], the seeds that adjoint was given, passed again (limit_summary[s][.][1] tells whether they were); the force
 *   buffer, the record, hmpc_params, the per-instance mu and the certificate tolerance, as the single-seed calls read them.  The seeds
 *   must not overlap the outputs.
 * hmpc_adjoint_chain_multi enqueues ceil(n_seeds / (6 NC)) launches on `stream` -- ONE for n_seeds <= U -- and synchronises nothing.
 * HMPC_E_ARG, nothing enqueued and no buffer touched: NULL seeds, no multi-seed adjoint of the last solve of the current batch stands,
 * caller-owned buffers that hold fewer seeds than that adjoint has, or inside a solve on an external constraint block.
 * hmpc_set_device_adjoint_chain_multi: caller-owned device buffers with room for n_seeds slices.  A NULL compact member is the handle's
 * own buffer, reserved for (n_seeds, max_batch) by the launch that needs it and grown by a later launch with more seeds, never inside
 * hmpc_solve; a NULL detail member means "not written".  NULL device_buffers: all members NULL (n_seeds is not read then).  HMPC_E_ARG
 * when a buffer is given and n_seeds lies outside 1 .. HMPC_ADJOINT_MAX_SEEDS.
 * hmpc_get_device_adjoint_chain_multi: slice 0 of where the chain is or goes next (a compact member of the handle's own that no launch
 * has reserved yet, and a detail member not given: NULL) and the seeds of the chain that stands (0: none); either pointer may be NULL.
 * hmpc_download_adjoint_chain_multi waits for the stream of the last call, then copies the slices of the seeds enqueued; any member may be
 * NULL.  HMPC_E_ARG, nothing copied: no chain stands, or a detail array is asked for that was not written.  With no batch set it copies
 * nothing and returns HMPC_OK.  It runs no safe pass.
 * The chain goes stale on every solve, every new batch, every hmpc_solve_adjoint_multi, every hmpc_set_device_adjoint_multi and every
 * hmpc_set_device_adjoint_chain_multi.  It touches neither the current adjoint, a selection, nor the single-seed model, limit and record
 * gradients and their buffers, and none of those touches it: hmpc_select_adjoint_seed keeps working beside it, with the bits it has.
 * For one or two seeds the selection and the three single-seed launches remain the advice (DESIGN.md section 4.21 has the break-even).
 * Device groups: per member, through hmpc_group_member; nothing on the process-global interface. */
struct hmpc_adjoint_chain {
  /* compact: always produced */
  double *grad_record, *grad_frames, *grad_rpy, *grad_params, *grad_limits, *limit_summary;
  /* detail: written only where the caller gives a buffer */
  double *grad_A, *grad_B, *grad_r, *costate;
  double *grad_Fc, *grad_bound, *lambda, *nu;
};
int hmpc_adjoint_chain_multi(hmpc_handle *h, const double *device_seeds, void *stream);
int hmpc_set_device_adjoint_chain_multi(hmpc_handle *h, int n_seeds, const struct hmpc_adjoint_chain *device_buffers);
int hmpc_get_device_adjoint_chain_multi(hmpc_handle *h, int *n_seeds, struct hmpc_adjoint_chain *device_buffers);
int hmpc_download_adjoint_chain_multi(hmpc_handle *h, const struct hmpc_adjoint_chain *host_buffers);
/* ---- the best command of every sweep group, picked on the device ----
 * A command sweep solves one robot state under many candidate commands and the prediction scores each (cost[batch][2]); these calls
 * take the planner's last step without a trip to the host.  The current batch is G = batch / group_size groups of group_size
 * CONSECUTIVE instances.  For instance i of group g, with U = 6 * contacts:
 *   score_i = (cost[i][0] + cost[i][1]) + device_penalty[i]     two plain binary64 additions in that order; cost = the handle's current
 *                                                               prediction; device_penalty = double[batch] in HBM, caller-owned: the
 *                                                               caller's own term (e.g. the distance of a command from the operator's);
 *                                                               NULL = only the first addition is made
 *   eligible  <=>  the status code is HMPC_S_OK or HMPC_S_OK_RELAXED, and score_i is finite (a NaN or +-inf penalty masks a command)
 *   winner     =   the eligible instance of smallest score; equal scores (==, so -0 equals +0) are broken by the lowest index
 * Outputs per group:
 *   index[g]            the winner's position in its group, 0 .. group_size-1, or -1 when the group has no winner
 *   score[g]            the winner's score, or +inf
 *   forces[g][U h]      a bit copy of the winner's slot of the force buffer, or +0
 *   status[g]           the winner's status word, or HMPC_SELECT_NONE
 *   states[g][h][13]    a bit copy of the winner's predicted states, or +0
 * The result is a pure function of cost, states, status, forces, penalty and group_size: it does not depend on the workgroup size or
 * on the order of the reduction (a lexicographic (score, index) minimum over the eligible instances; ineligible ones never enter a
 * comparison).
 *
 * hmpc_sweep_select enqueues ONE launch on `stream` (a kernel of its own, one workgroup per group) and synchronises nothing.  Forces
 * and status are read where the solve wrote them (hmpc_set_device_outputs is honoured), the prediction where the last prediction went.
 * Any contact count and any horizon; it may follow hmpc_solve as well as a sweep (it only groups consecutive instances).  HMPC_E_ARG,
 * nothing enqueued: group_size < 1, batch % group_size != 0, or no prediction enqueued since the last solve of the current batch (the
 * rule of hmpc_download_prediction: a later solve, a new batch or hmpc_set_device_prediction each ask for a new prediction, and every
 * new prediction for a new selection).
 * hmpc_set_device_selection: caller-owned device buffers for later selections, each for as many groups as will be selected (any may
 * be NULL = the handle's own, allocated for max_batch groups by the first call that needs them; never inside hmpc_solve).
 * hmpc_get_device_selection: where the next selection goes, and *n_groups = the groups of the last selection (0 when nothing has been
 * selected since the last prediction); any pointer may be NULL.  hmpc_download_selection waits for the stream of the last call, then
 * copies (any pointer may be NULL); HMPC_E_ARG when nothing has been selected since the last prediction.  It does NOT run the safe pass.
 * Device groups: per member, through hmpc_group_member (a sweep group never spans two members: hmpc_group_solve_command_sweep). */
#define HMPC_SELECT_NONE 0xffffffffu
int hmpc_sweep_select(hmpc_handle *h, int group_size, const double *device_penalty, void *stream);
int hmpc_set_device_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states);
int hmpc_get_device_selection(hmpc_handle *h, int32_t **index, double **score, float **forces, uint32_t **status, float **states,
                              int *n_groups);
int hmpc_download_selection(hmpc_handle *h, int32_t *index, double *score, float *forces, uint32_t *status, float *states);
/* One candidate command: the five command fields of hmpc_tick_inputs, in their order. */
struct hmpc_command {
  double v_des_robot[2];
  double yaw_rate_des;
  double roll_des, pitch_des;
};
/* Ticks and candidate commands in HBM in, the best command's torques in HBM out -- hmpc_tick_solve_device for ONE robot state under K
 * commands.  device_ticks: hmpc_tick_inputs[n_ticks]; device_commands: hmpc_command[n_ticks][group_size].  Instance g K + k of the new
 * current batch (n_ticks * group_size instances) is built from ticks[g] with its five command fields replaced by commands[g][k],
 * everything else copied: its record is bit for bit what hmpc_build_records_device builds from ticks expanded that way by the caller.
 * Launches on the one stream, no host synchronisation: the expansion (into scratch of the handle) and the record builder; the sweep
 * solve exactly as hmpc_solve_command_sweep enqueues it (per-class routing, and the device-side repair chain when
 * hmpc_set_device_repair is on); the prediction; the selection with device_penalty[n_ticks * group_size] (or NULL); and the joint
 * torques of hmpc_tick_solve_device over the n_ticks winner force rows, rBody and the joint angles read from device_ticks.
 * Outputs: f_ff[n_ticks][2][6] (may be NULL), tau[n_ticks][2][5], device_wpd_out[n_ticks][2] (may be NULL): the clamped
 * world_position_desired of each tick, the value hmpc_build_records returns for it (it does not depend on the command).  Which command
 * won, its score, forces, status word and predicted states: hmpc_get_device_selection / hmpc_download_selection.  A tick with no
 * eligible command gets index -1, and f_ff and tau computed from zero forces.
 * HMPC_E_ARG for a three-contact handle or a horizon above 10 (the sweep's limits); HMPC_E_BATCH when n_ticks * group_size > max_batch. */
int hmpc_tick_sweep_device(hmpc_handle *h, const void *device_ticks, int n_ticks, const struct hmpc_command *device_commands,
                           int group_size, double dtMPC, const double *device_penalty, double *device_wpd_out, double *device_f_ff,
                           double *device_tau, void *stream);
/* ---- closed loop on the device: plant step, foot placement, tick log (csrc/hmpc_plant.h) ----
 * hmpc_tick_solve_device takes tick structs in HBM to forces in HBM; hmpc_plant_step_device takes (tick structs, step-0 forces) to the
 * tick structs of the NEXT tick, in place, and hmpc_rollout_device chains n ticks of both on one stream.  The plant is the single rigid
 * body the MPC predicts with (SolverMPC.cpp:312-331), integrated semi-implicitly with a quaternion attitude.  Its constants are the
 * PLANT'S OWN (struct hmpc_plant, binary64), independent of the handle's hmpc_params: the plant may be heavier than the MPC believes,
 * per instance (device_mass), and may be pushed (device_ext_wrench).  The plant has no legs: leg_q is never changed -- the joint angles
 * enter the QP only through the foot rotations -- and a stance foot keeps its pFoot bit for bit.
 *
 * One launch, one thread per instance, 256 threads per workgroup, nothing synchronised.  ALL arithmetic is binary64, every operation a
 * correctly rounded IEEE operation (+ - * / sqrt; no contraction), in exactly the order written here; a * b + c * d + e * f below always
 * means ((a * b) + (c * d)) + (e * f), x cross y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0), vectors are handled component by
 * component.  Per instance i, tick struct tk:
 *   If tk.flags & HMPC_TICK_FALLEN: nothing of tk and nothing of its summary row changes.  Otherwise:
 *   m = device_mass ? device_mass[i] : mass;  (F_ext, tau_ext) = device_ext_wrench ? its row i (force, then torque about the centre of mass,
 *   world frame) : six times +0.0 (added all the same);  I = inertia, g = gravity.
 *   u0[0..11] = forces[i * force_stride + 0..11] widened from float: F_L = u0[0..2], F_R = u0[3..5], M_L = u0[6..8], M_R = u0[9..11], world
 *   frame, applied as they stand whatever the status word (the rule of hmpc_predict_states).
 *   p = position, v = vWorld, w = omegaWorld, q = orientation (body -> world, scalar first), R = rBody (row-major, world -> body).
 *   R0 = R as read;  vdw0[a] = R0[a] * v_des_robot[0] + R0[3 + a] * v_des_robot[1] + R0[6 + a] * 0.0,  a = 0, 1   (the builder's expression)
 *   d = dt_tick / (double)substeps;  hd = 0.5 * d.        Then `substeps` times:
 *     1.  r_L = pFoot[0..2] - p;  r_R = pFoot[3..5] - p
 *     2.  tau = ((r_L cross F_L + M_L) + (r_R cross F_R + M_R)) + tau_ext
 *     3.  F = (F_L + F_R) + F_ext
 *     4.  tb[k] = R[3k] * tau[0] + R[3k + 1] * tau[1] + R[3k + 2] * tau[2]
 *     5.  with HMPC_PLANT_GYRO:  wb[k] = R[3k] * w[0] + R[3k + 1] * w[1] + R[3k + 2] * w[2];  Iw[k] = I[k] * wb[k];  tb = tb - (wb cross Iw)
 *     6.  ab[k] = tb[k] / I[k];  alpha[k] = R[k] * ab[0] + R[3 + k] * ab[1] + R[6 + k] * ab[2]
 *     7.  a[k] = F[k] / m + (k == 2 ? -g : 0.0)
 *     8.  w = w + d * alpha
 *     9.  v = v + d * a
 *     10. p = p + d * v
 *     11. with (q0, q1, q2, q3) = q and the NEW w:   e0 = -(w0 * q1 + w1 * q2 + w2 * q3),   e1 = (w0 * q0 + w1 * q3) - w2 * q2,
 *         e2 = (w1 * q0 + w2 * q1) - w0 * q3,   e3 = (w2 * q0 + w0 * q2) - w1 * q1     ((0, w) (x) q, Hamilton product)
 *         q[k] = q[k] + hd * e[k];   n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);   q[k] = q[k] / n
 *     12. R = transpose of M(q), the polynomial of orientation_tools.h:182-200:
 *         M = [ 1 - 2 (q2 q2 + q3 q3),  2 (q1 q2 - q0 q3),      2 (q1 q3 + q0 q2)     ]
 *             [ 2 (q1 q2 + q0 q3),      1 - 2 (q1 q1 + q3 q3),  2 (q2 q3 - q0 q1)     ]
 *             [ 2 (q1 q3 - q0 q2),      2 (q2 q3 + q0 q1),      1 - 2 (q1 q1 + q2 q2) ]
 *   Once per tick, after the sub-steps:
 *     rpy[0] = det_atan2(2 (q0 q1 + q2 q3), 1 - 2 (q1 q1 + q2 q2));   s = 2 (q0 q2 - q1 q3), s = 0.99999 unless s < 0.99999,
 *     then s = -0.99999 if s < -0.99999, rpy[1] = det_asin(s);
 *     rpy[2] = det_atan2(2 (q0 q3 + q1 q2), 1 - 2 (q2 q2 + q3 q3))     -- the formulas of the solve kernel's quat_to_rpy (SolverMPC.cpp:338-341)
 *     over csrc/hmpc_math.h's deterministic routines, with the clamp of s made TWO-SIDED: the reference (and the solve kernel, which keeps
 *     its clamp bit for bit) limits s from above only, and at pitch -90 degrees rounding takes s below -1, where asin is NaN -- a plant that
 *     is pushed over must not hand NaN to the next solve.  (rpy is the one output a libm restatement matches to a few ulp only.)
 *     world_position_desired[a] = base[a] + dt_tick * vdw0[a], base = device_wpd ? device_wpd[2 i + a] (the builder's clamped value,
 *     ConvexMPCLocomotion.cpp:336-346) : the tick's own -- ConvexMPCLocomotion.cpp:50-54 on the rBody BEFORE the step.
 *     If advance_gait: gait_iteration = (gait_iteration + 1) % horizon of the handle.
 *     With HMPC_PLANT_PLACE_FEET, for each leg j that is in swing at step 0 of the NEW gait phase (progress = gait_iteration % horizon -
 *     gait_offsets[j], + horizon if negative; swing <=> not progress < gait_durations[j] -- GaitGenerator.cpp:85-103), with the NEW p, v, R:
 *       vdw[a] = R[a] * v_des_robot[0] + R[3 + a] * v_des_robot[1] + R[6 + a] * 0.0;   rh[k] = R[k] * hip[j][0] + R[3 + k] * hip[j][1] + R[6 + k] * hip[j][2]
 *       Pf[k] = (p[k] + rh[k]) + v[k] * 0.0                                              (swingTimeRemaining = 0)
 *       rel[a] = ((v[a] * 0.5) * (double)gait_durations[0]) * dtMPC + 0.02 * (v[a] - vdw[a]);   rel[a] = (double)fminf(fmaxf((float)rel[a], (float)-0.4), (float)0.4)
 *       pFoot[j] = (Pf[0] + rel[0], Pf[1] + rel[1], +0.0)        -- ConvexMPCLocomotion.cpp:148-164, the float narrowing of its clamp kept.
 *     A leg in stance keeps its pFoot: a foot freezes where it was placed on the tick it touches down.
 *     If the new R[8] < fall_cos: flags |= HMPC_TICK_FALLEN  (FSM.cpp:78-87).
 *     Summary row (int32[4], ACCUMULATED, never initialised by the step: start it at {0, -1, 0, 0}):  if the flag was set just now and
 *     row[1] < 0: row[1] = row[0];  row[0] += 1;  row[2] += 1 when HMPC_STATUS_CODE(status[i]) is neither HMPC_S_OK nor HMPC_S_OK_RELAXED;
 *     row[3] = max(row[3], HMPC_STATUS_ITERS(status[i])).  So: ticks stepped, first fall tick or -1, ticks not solved, largest iteration count.
 *
 * hmpc_plant_step_device: device_ticks = hmpc_tick_inputs[batch] in HBM, advanced in place.  device_forces NULL = the handle's force buffer
 * with force_stride = 12 * horizon (the argument is ignored then); else force_stride >= 12 floats between instances.  device_status NULL =
 * the handle's.  device_wpd NULL = the tick's own world_position_desired.  device_summary [batch][4] may be NULL.  Passing forces and
 * status explicitly makes the step usable without a solve.  HMPC_E_ARG, nothing enqueued: NULL handle, ticks or plant, batch < 0,
 * substeps < 1, force_stride < 12 with explicit forces, batch > max_batch when the handle's own forces or status are read, a three-contact
 * handle.  It does not replace the handle's batch. */
#define HMPC_PLANT_GYRO 1       /* step 5: the gyroscopic term */
#define HMPC_PLANT_PLACE_FEET 2 /* foot placement for the legs in swing */
struct hmpc_plant {
  double dt_tick;      /* 0.005: seconds per tick */
  double dtMPC;        /* 0.04: seconds per horizon step, read by the foot placement only; hmpc_rollout_device puts its own argument here */
  int substeps;        /* 1: integrator sub-steps per tick, >= 1 */
  int advance_gait;    /* 0 or 1: this tick ends a horizon step (hmpc_rollout_device sets it per tick) */
  int flags;           /* 0: HMPC_PLANT_* bits */
  int reserved;        /* 0 */
  double mass;         /* 9 */
  double inertia[3];   /* (0.5413, 0.5200, 0.0691) */
  double gravity;      /* 9.81 */
  double hip[2][3];    /* Biped.h getHipYawLocation: (-0.005, -0.057, -0.126) for leg 0, y negated for leg 1; body frame */
  double fall_cos;     /* 0.5 */
  const double *device_mass;        /* NULL, or double[batch] in HBM: overrides `mass` per instance */
  const double *device_ext_wrench;  /* NULL, or double[batch][6] in HBM: world-frame force, then torque about the centre of mass */
};
void hmpc_default_plant(struct hmpc_plant *p);
int hmpc_plant_step_device(hmpc_handle *h, void *device_ticks, int batch, const struct hmpc_plant *plant, const float *device_forces,
                           int force_stride, const uint32_t *device_status, const double *device_wpd, int32_t *device_summary,
                           void *stream);
/* The log of a rollout: device pointers, each may be NULL (= not logged).  Row (i, k) = instance i, tick k:
 *   state   [batch][n_ticks][12] double: rpy, position, omegaWorld, vWorld AFTER tick k's plant step
 *   wrench  [batch][n_ticks][12] float:  the step-0 forces of tick k as the plant read them
 *   status  [batch][n_ticks]     uint32: the status word of tick k
 *   tau     [batch][n_ticks][10] double: the joint torques of tick k
 *   summary [batch][4]           int32:  as in the plant step; initialised to {0, -1, 0, 0} on the stream at the start of the rollout
 * An instance that has fallen keeps being solved and logged, with its frozen state. */
struct hmpc_rollout_log {
  double *state;
  float *wrench;
  uint32_t *status;
  double *tau;
  int32_t *summary;
};
/* n_ticks closed-loop ticks on ONE stream: for k = 0 .. n_ticks - 1 what hmpc_tick_solve_device enqueues, then the plant step (which also
 * writes row k of the log) with advance_gait = ((subtick0 + k + 1) % ticks_per_step == 0); plant->advance_gait and plant->dtMPC are not
 * read.  No host synchronisation, no hipGraph, and no hipMalloc after the first call (the clamped world_position_desired and the torques
 * of a tick go through two small buffers of the handle).  With hmpc_set_tick_warm_start on, the tick after an advance is solved with
 * horizon_shift = 1 and every other one with 0 -- tick 0 with 0; the handle is left with the shift of the last tick.  With
 * hmpc_set_device_repair on the plant reads repaired forces.  log == NULL: the handle's own log buffers (hmpc_get_device_rollout, allocated
 * here on first need); else the caller's, rows as above.  The current batch becomes device_ticks' last tick, as after hmpc_tick_solve_device.
 * Two-contact handles only.  HMPC_E_ARG, nothing enqueued: n_ticks < 1, ticks_per_step < 1, subtick0 < 0, plant->substeps < 1, a
 * three-contact handle, batch > max_batch or < 0, a NULL handle, ticks or plant (plant == NULL is NOT the default plant).
 * hmpc_get_device_rollout: the handle's own log buffers, (re)allocated for max_batch x n_ticks when they hold fewer ticks -- outside the
 * solve; the pointers stay valid until a call with a larger n_ticks, here or in a rollout or sweep with log == NULL.  Such a growth frees
 * the old buffers, so the handle forgets a last rollout that logged into any of them (one logged wholly into the caller's buffers stays):
 * until the next rollout, hmpc_download_rollout and the score and selection with log == NULL return HMPC_E_ARG, as before the first
 * rollout; the old contents are not copied over.  hmpc_set_device_rollout: caller-owned buffers for the rollouts that
 * pass log == NULL (NULL member = the handle's own; log == NULL = all the handle's own).  hmpc_download_rollout waits for the stream of
 * the last rollout, then copies its log (any pointer may be NULL; a member that was not logged: HMPC_E_ARG); HMPC_E_ARG before the first.
 * Device groups: per member, through hmpc_group_member. */
int hmpc_rollout_device(hmpc_handle *h, void *device_ticks, int batch, int n_ticks, double dtMPC, int ticks_per_step, int subtick0,
                        const struct hmpc_plant *plant, const struct hmpc_rollout_log *log, void *stream);
int hmpc_set_device_rollout(hmpc_handle *h, const struct hmpc_rollout_log *log);
int hmpc_get_device_rollout(hmpc_handle *h, int n_ticks, struct hmpc_rollout_log *log);
int hmpc_download_rollout(hmpc_handle *h, double *state, float *wrench, uint32_t *status, double *tau, int32_t *summary);
/* ---- closed-loop command sweeps: score rollouts, pick the best on the device (csrc/hmpc_rollout_score.h) ----
 * hmpc_rollout_device leaves a log; hmpc_rollout_score_device turns the log of every instance into a cost, hmpc_rollout_select_device picks
 * the cheapest instance of every group of consecutive instances, and hmpc_rollout_sweep_device chains expansion (robot states x candidate
 * commands), rollout, score and selection on one stream: "which command keeps it up over the next second" without the log leaving the device.
 *
 * THE SCORE.  One launch, one wave of 64 lanes per instance, four waves per workgroup, nothing synchronised, nothing allocated.  ALL
 * arithmetic is binary64, every operation a correctly rounded IEEE operation (+ - * / and rint, ties to even; no contraction), in exactly the
 * order written here; a * b + c * d + e * f means ((a * b) + (c * d)) + (e * f).  W = 64 is a constant of this definition (not of the
 * hardware), TWO_PI = 6.283185307179586.  Per instance i, with tk = ticks0[i] -- the tick struct AS IT WAS BEFORE THE ROLLOUT (the rollout
 * advances its ticks in place: score against a copy) --, c = the hmpc_rollout_cost, n = n_ticks, and the log's rows (i, k):
 *   R0 = tk.rBody;   vdw[a] = R0[a] * tk.v_des_robot[0] + R0[3 + a] * tk.v_des_robot[1] + R0[6 + a] * 0.0,  a = 0, 1   (the builder's expression)
 *   Row k, k = 0 .. n - 1:
 *     t = (double)(k + 1) * c.dt_tick
 *     ref = (tk.roll_des, tk.pitch_des, tk.rpy[2] + t * tk.yaw_rate_des, tk.position[0] + t * vdw[0], tk.position[1] + t * vdw[1], c.height,
 *            0.0, 0.0, tk.yaw_rate_des, vdw[0], vdw[1], 0.0)          (the columns of the log's state row: rpy, position, omegaWorld, vWorld)
 *     e[s] = state[i][k][s] - ref[s],  s = 0 .. 11;   then for s = 2 only:  e[2] = e[2] - TWO_PI * rint(e[2] / TWO_PI)
 *     trk_k = +0.0, then for s = 0 .. 11 in this order:  trk_k = trk_k + (c.w_state[s] * e[s]) * e[s]
 *     eff_k = +0.0, then, when log.wrench is not NULL, for j = 0 .. 11:  u = (double)wrench[i][k][j];  eff_k = eff_k + (c.w_wrench[j] * u) * u
 *             then, when log.tau is not NULL, for j = 0 .. 9:  u = tau[i][k][j];  eff_k = eff_k + (c.w_tau[j] * u) * u
 *   Sums over the ticks, the same for trk (giving cost[0], tracking) and eff (giving cost[1], effort):
 *     P[l] = +0.0 for l = 0 .. W - 1;   for k = 0 .. n - 1 in ascending order:  P[k % W] = P[k % W] + trk_k      (a lane without a tick keeps +0.0)
 *     for off = 32, 16, 8, 4, 2, 1:   P'[l] = P[l] + P[l ^ off] for every l at once, then P = P'
 *     cost = P[0]      (IEEE addition is commutative, so every P[l] ends with the same bits)
 *   cost[2] = +0.0, then for s = 0 .. 11:  cost[2] = cost[2] + (c.w_terminal[s] * e[s]) * e[s]  with the e of row n - 1     (terminal)
 *   cost[3] = (summary[i][1] >= 0 ? c.fall_penalty : 0.0) + (summary[i][2] > 0 ? (double)summary[i][2] * c.unsolved_penalty : 0.0), or +0.0
 *             when log.summary is NULL.  (The comparisons keep 0 * inf from occurring: an infinite penalty masks exactly the instances it is for.)
 *   score = ((cost[0] + cost[1]) + cost[2]) + cost[3]
 * A NaN anywhere in a row that carries weight gives a NaN score; with the default fall_penalty a fallen instance scores +inf.  Either masks
 * the instance in the selection below.
 *
 * hmpc_rollout_score_device: device_ticks0 = hmpc_tick_inputs[batch], log = the rows to score (log == NULL: where the handle's last
 * hmpc_rollout_device logged, and batch and n_ticks must be that rollout's), device_cost [batch][4] and device_score [batch] binary64,
 * caller-owned, either may be NULL (= not written).  HMPC_E_ARG, nothing enqueued: a NULL handle, ticks0 or cost, batch < 0, n_ticks < 1,
 * log.state NULL, or log == NULL with no rollout yet or another batch or n_ticks than the last rollout's.  It does not replace the handle's batch.
 *
 * THE SELECTION.  One launch, one workgroup per group g = instances g K .. g K + K - 1 (K = group_size):
 *   s_i      = score[i] + penalty[i]        one binary64 addition; with device_penalty NULL no addition is made
 *   eligible <=> s_i is finite
 *   winner   = the eligible instance of smallest s_i; equal values (==, so -0 equals +0) are broken by the lowest index
 * a lexicographic (s, index) minimum over the eligible instances -- ineligible ones never enter a comparison --, so the result does not
 * depend on the workgroup size or on the order of the reduction; any group_size (each thread strides over its group).  Outputs: the
 * members of struct hmpc_rollout_choice, caller-owned device pointers, each may be NULL (= not written); per group
 *   index [groups]        int32:   the winner's position in its group, or -1 when the group has no winner
 *   score [groups]        double:  the winner's s_i, or +inf
 *   wrench[groups][12]    float:   a bit copy of the winner's row of tick 0 of log.wrench, or +0
 *   tau   [groups][10]    double:  a bit copy of the winner's row of tick 0 of log.tau -- the torques to apply NOW --, or +0
 *   summary[groups][4]    int32:   a bit copy of the winner's row of log.summary, or {0, -1, 0, 0}
 * hmpc_rollout_select_device: log == NULL = where the handle's last hmpc_rollout_device logged, with its n_ticks as the row count per
 * instance, and batch must be that rollout's; log != NULL = the caller's, rows per instance = the n_ticks of the handle's last
 * hmpc_rollout_score_device, whose batch it must share.  HMPC_E_ARG, nothing enqueued: a NULL handle, score or choice, batch < 0,
 * group_size < 1, batch % group_size != 0, no such rollout / score call or another batch, or choice->wrench, ->tau or ->summary asked
 * for with the log member behind it NULL.
 *
 * THE CHAIN.  hmpc_rollout_sweep_device, on the one stream and without host synchronisation: (1) device_ticks [n_states] x
 * device_commands [n_states][K] are expanded as hmpc_tick_sweep_device expands them -- instance g K + k = ticks[g] with its five command
 * fields replaced by commands[g][k] --, twice, into two buffers of the handle's own (NOT its shared scratch: they must outlive n solves;
 * allocated for max_batch instances by the first sweep, never inside hmpc_solve); (2) hmpc_rollout_device over the first copy with
 * log == NULL and the arguments given here; (3) the score with ticks0 = the second copy, into the handle's own cost and score; (4) the
 * selection with device_penalty [n_states * K] (or NULL) into `choice`.  device_ticks is not modified.  plant->device_mass and
 * plant->device_ext_wrench are indexed by EXPANDED instance.  hmpc_get_device_rollout_sweep: the handle's buffers of the last sweep -- the
 * expanded ticks after the rollout, cost [n_states K][4], score [n_states K] -- (any pointer may be NULL; HMPC_E_ARG before the first
 * sweep); the log is hmpc_download_rollout's.  Two-contact handles only.  HMPC_E_BATCH when n_states * K > max_batch.  HMPC_E_ARG, nothing
 * enqueued: a NULL handle, ticks, commands, plant, cost or choice, n_states < 1, K < 1, and every argument error of hmpc_rollout_device. */
struct hmpc_rollout_cost {
  double w_state[12];      /* the reference's Q (100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1): weight per column of the log's state row */
  double w_terminal[12];   /* 0: extra weight on the last tick */
  double w_wrench[12];     /* the reference's Alpha (1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, six times 1e-2): weight on the logged step-0 wrench */
  double w_tau[10];        /* 0: weight on the logged joint torques */
  double height;           /* 0.55: reference z */
  double dt_tick;          /* 0.005: seconds per tick */
  double fall_penalty;     /* +inf: a fallen instance is masked */
  double unsolved_penalty; /* 0: per unsolved tick */
};
struct hmpc_rollout_choice {
  int32_t *index;
  double *score;
  float *wrench;
  double *tau;
  int32_t *summary;
};
void hmpc_default_rollout_cost(struct hmpc_rollout_cost *c);
int hmpc_rollout_score_device(hmpc_handle *h, const void *device_ticks0, int batch, int n_ticks, const struct hmpc_rollout_cost *cost,
                              const struct hmpc_rollout_log *log, double *device_cost, double *device_score, void *stream);
int hmpc_rollout_select_device(hmpc_handle *h, const double *device_score, const double *device_penalty, int batch, int group_size,
                               const struct hmpc_rollout_log *log, const struct hmpc_rollout_choice *choice, void *stream);
int hmpc_rollout_sweep_device(hmpc_handle *h, const void *device_ticks, int n_states, const struct hmpc_command *device_commands, int K,
                              int n_ticks, double dtMPC, int ticks_per_step, int subtick0, const struct hmpc_plant *plant,
                              const struct hmpc_rollout_cost *cost, const double *device_penalty, const struct hmpc_rollout_choice *choice,
                              void *stream);
int hmpc_get_device_rollout_sweep(hmpc_handle *h, void **ticks_final, double **cost, double **score);
/* ---- swing legs on the device: Bezier targets, inverse kinematics, complete motor commands (csrc/hmpc_swing.h) ----
 * hmpc_tick_solve_device ends in forces and the stance feed-forward torques; the reference's controller ends in a COMPLETE command per joint
 * (tau, q, dq, Kp, Kd -- LowlevelCmd, common/LegController.cpp:90-97), and for a leg in swing that command is a joint-angle target with gains:
 * swingLegController::updateSwingLeg() of common/SwingLegController.cpp (line numbers below are that file's unless another is named).  One
 * launch performs it for every instance: thread g -> instance g / 2, leg g % 2 (0 = left), 256 threads per workgroup, nothing synchronised,
 * plain loads and stores.  The two legs of an instance share only what they read.
 *
 * THE ARITHMETIC IS A CONTRACT, as the plant's: ALL of it binary64, every operation a correctly rounded IEEE operation (+ - * / sqrt and
 * comparisons; no contraction), evaluated as C evaluates the expressions written here -- parentheses first, operators of equal precedence
 * from left to right, so a * b * c is (a * b) * c and a + b - c is (a + b) - c.  Trigonometry: sincos(x) = det_sincos, asin(v) = det_asin(v),
 * acos(v) = det_atan2(sqrt((1 - v) * (1 + v)), v) of csrc/hmpc_math.h (a libm restatement agrees to a few ulp only).  PI3 = 3.14159 (the
 * LegController's), PI = 3.141592653589793 (M_PI, the IK's).  clamp1(v) = max(-1, min(v, 1)) as std::max / std::min order their
 * arguments: t = (1 < v) ? 1 : v;  clamp1 = (-1 < t) ? t : -1  (a NaN comes out as -1).
 * Per instance i and leg j, tick struct tk, constants c (struct hmpc_swing), state st (struct hmpc_swing_state of instance i, of which leg
 * j reads and writes only its own entries), h = the handle's horizon, R = tk.rBody (row-major, world -> body), pos = tk.position, v = tk.vWorld:
 *   1. Joint angles (the rule of hmpc_tick_solve_device's torques).  q0, q1 = tk.leg_q[5 j + 0, 1]; with tk.flags & HMPC_TICK_LEG_Q_MOTOR
 *      q2 = leg_q[5 j + 2] + 0.3 * PI3, q3 = leg_q[5 j + 3] - 0.6 * PI3, q4 = leg_q[5 j + 4] + 0.3 * PI3 (LegController.cpp:111-113), else as stored.
 *   2. Foot position.  (sk, ck) = sincos(qk), k = 0 .. 4;  side = (j == 0) ? 1.0 : -1.0;  data[leg].p of LegController.cpp:190-193:
 *        A = c0 * c2 - s0 * s1 * s2;   B = c0 * s2 + c2 * s0 * s1;   C = c2 * s0 + c0 * s1 * s2;   D = s0 * s2 - c0 * c2 * s1
 *        p[0] = -(3 * c0) / 200 - (9 * s4 * (c3 * A - s3 * B)) / 250 - (11 * c0 * s2) / 50 - (side * s0) / 50 - (11 * c3 * B) / 50
 *               - (11 * s3 * A) / 50 - (9 * c4 * (c3 * B + s3 * A)) / 250 - (23 * c1 * side * s0) / 1000 - (11 * c2 * s0 * s1) / 50
 *        p[1] = (c0 * side) / 50 - (9 * s4 * (c3 * C - s3 * D)) / 250 - (3 * s0) / 200 - (11 * s0 * s2) / 50 - (11 * c3 * D) / 50
 *               - (11 * s3 * C) / 50 - (9 * c4 * (c3 * D + s3 * C)) / 250 + (23 * c0 * c1 * side) / 1000 + (11 * c0 * c2 * s1) / 50
 *        p[2] = (23 * side * s1) / 1000 - (11 * c1 * c2) / 50 - (9 * c4 * (c1 * c2 * c3 - c1 * s2 * s3)) / 250
 *               + (9 * s4 * (c1 * c2 * s3 + c1 * c3 * s2)) / 250 - (11 * c1 * c2 * c3) / 50 + (11 * c1 * s2 * s3) / 50 - 3.0 / 50.0
 *      u[k] = c.hip_yaw[j][k] + p[k];   pFoot_w[k] = pos[k] + (R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2]), k = 0, 1;   pFoot_w[2] = +0.0   (:59-68)
 *   3. Swing sub-phase (GaitGenerator.cpp:54-79, 109-113).  cur = tk.gait_iteration * c.ticks_per_step + c.subtick;  per = c.ticks_per_step * h;
 *      phase = (double)(cur % per) / (double)per;   offP = (double)tk.gait_offsets[j] / (double)h;   durP = (double)tk.gait_durations[j] / (double)h
 *      so = offP + durP;  if so > 1: so = so - 1.;    sd = 1. - durP;    pr = phase - so;  if pr < 0: pr = pr + 1.
 *      swing = (pr > sd) ? 0. : (sd == 0 ? 0. : pr / sd)     -- the inner test is deviation 2 below
 *   4. - 6a.  `c.updates` times, u = 0 .. updates - 1 (the reference calls updateSwingLeg() once per foot: twice a tick; what an update reads
 *      of the tick does not change, so only these state steps repeat):
 *      4.  Timer (:80-91).  if st.first_swing[j]: st.swing_time[j] = c.dtMPC * (double)(h - tk.gait_durations[0])
 *          else: st.swing_time[j] = st.swing_time[j] - c.dt_update;  if st.swing_time[j] <= 0: st.first_swing[j] = 1
 *      5.  Touchdown point (:96-126).  vdw[a] = R[a] * tk.v_des_robot[0] + R[3 + a] * tk.v_des_robot[1] + R[6 + a] * 0.0, a = 0, 1 (the builder's expression)
 *          rh[k] = R[k] * c.hip_yaw[j][0] + R[3 + k] * c.hip_yaw[j][1] + R[6 + k] * c.hip_yaw[j][2];    Pf[k] = (pos[k] + rh[k]) + v[k] * st.swing_time[j]
 *          rel[a] = c.place_gain_v * v[a] * 0.5 * (double)tk.gait_durations[0] * c.dtMPC + c.place_gain_err * (v[a] - vdw[a])
 *          rel[a] = (double)fminf(fmaxf((float)rel[a], (float)-c.place_max), (float)c.place_max)         (the reference's binary32 narrowing, kept)
 *          st.pf[j] = (Pf[0] + rel[0], Pf[1] + rel[1], +0.0)
 *      6a. First swing update (:134-139).  if swing > 0 and st.first_swing[j]: st.first_swing[j] = 0;  st.p0[j] = pFoot_w
 *   If swing > 0 (else: pDes, vDes, pFoot_b, vFoot_b of the detail row are +0.0 and steps 6b - 7 are skipped):
 *   6b. Trajectory (FootSwingTrajectory.cpp:17-36 over Interpolation.h:53-74), p0 = st.p0[j], pf = st.pf[j], with
 *         bez(y0, yf, x) = y0 + (x * x * x + 3 * (x * x * (1 - x))) * (yf - y0);      dbez(y0, yf, x) = (6 * x * (1 - x)) * (yf - y0)
 *       pDes[k] = bez(p0[k], pf[k], swing),  vDes[k] = dbez(p0[k], pf[k], swing), k = 0, 1;   top = p0[2] + c.height
 *       swing < 0.5:  x = swing * 2;  pDes[2] = bez(p0[2], top, x),  vDes[2] = dbez(p0[2], top, x);    else:  x = swing * 2 - 1;  pDes[2] = bez(top, pf[2], x),  vDes[2] = dbez(top, pf[2], x)
 *       d = pDes - pos;   pFoot_b[k] = (R[3 k] * d[0] + R[3 k + 1] * d[1] + R[3 k + 2] * d[2]) + c.hip_width_offset[j][k]
 *       e[k] = vDes[k] * 0.0 - v[k];   vFoot_b[k] = R[3 k] * e[0] + R[3 k + 1] * e[1] + R[3 k + 2] * e[2]                                    (:141-149)
 *   7.  computeIK (:157-187).  sideK = (j == 0) ? -1.0 : 1.0;   hr = (c.hip_roll[0] - c.ik_hip_x, 0.0, c.hip_yaw[0][2] + c.hip_roll[2] * 2);   f = pFoot_b - hr
 *         d3 = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);   dyz = sqrt(f[1] * f[1] + f[2] * f[2]);   dh = c.ik_horizontal;   L = c.ik_link
 *         m = dyz * dyz - dh * dh;   dv = sqrt((0.00001 < m) ? m : 0.00001);   dxz = sqrt(d3 * d3 - dh * dh)
 *         a1 = clamp1(dxz / (2.0 * L));   a2 = clamp1(dv / dxz);   div = |f[0]|;  if div == 0.0: div = 1e-6
 *         ik[0] = 0.0;    ik[1] = asin(clamp1(f[1] / dyz)) + asin(clamp1(dh * sideK / dyz))
 *         ik[2] = acos(a1) - acos(a2) * f[0] / div;    ik[3] = 2.0 * asin(clamp1(dxz / 2.0 / L)) - PI;    ik[4] = -q3 - q2       (q2, q3 of step 1)
 *         ik[2] = ik[2] - 0.3 * PI;   ik[3] = ik[3] + 0.6 * PI;   ik[4] = ik[4] - 0.3 * PI
 *   8.  setDesiredJointState (:192-219).  swing > 0:  st.q_des[5 j + k] = ik[k];  Kp[5 j + k] = c.kp[k], Kd[5 j + k] = c.kd[k].  Otherwise Kp = Kd = +0.0
 *       and st.q_des is LEFT AS THE LAST UPDATE WROTE IT (zeros before the first swing).  Command of instance i (struct hmpc_motor_cmd), joints 5 j .. 5 j + 4:
 *       q = st.q_des, dq = +0.0, Kp, Kd, tau = device_tau ? device_tau[10 i + 5 j + k] : +0.0.
 *   Detail row [i][j][16], when asked for: swing, pFoot_w[3], pDes[3], vDes[3], pFoot_b[3], vFoot_b[3].
 * Reference oddities KEPT: the timer subtracts the constant dt_update = _dt = 0.001 per update whatever the tick's length; a leg whose sub-phase
 * is exactly 0 is not in swing on that tick; the touchdown heuristic is not the plant's (1.75, 0.1, clamp 0.3, vWorld * swingTimes); the IK does
 * not invert the leg's forward kinematics at the toe (DESIGN.md section 4.25 says by how much); HMPC_TICK_FALLEN is not looked at.
 * DEVIATIONS, both documented in DESIGN.md section 4.25: (1) tau of the command is always the tick's J' f_ff (device_tau).  The reference
 * differs on one tick per leg and cycle, the first tick of the leg's stance step (cur % per == tk.gait_offsets[j] * c.ticks_per_step): step 0
 * of the MPC table already has leg j in stance there and the solve gives it a force, but its swing sub-phase is sd / sd = exactly 1, "in
 * swing", so setDesiredJointState writes feedforwardForce << 0, the swing branch of run() sets nothing and updateCommand commands
 * tau = J' 0 = 0 for that leg -- measured on the executed reference (tests/test_swing_update_reference.py: ticks 0, 25, 50 of a 51-tick
 * walking cycle).  Where the rounding of phase - so puts that tick an ulp past the swing (sub-phase 0, contact sub-phase 0) the leg is
 * neither in swing nor in stance and the reference leaves the feedforwardForce of the tick before, the swing leg's 0: the same command.
 * On every other tick a swing leg has no force in the solve and both give 0; (2) a leg whose stance lasts the whole
 * horizon has sd = 0 and the reference forms 0 / 0 at phase 0: a NaN that only ever meets `> 0`; here it is +0.0, the same "not in swing".
 *
 * struct hmpc_swing_state: one per instance, in HBM, owned by the caller, carried from tick to tick.  All-zero bytes with first_swing = {1, 1}
 * is the reference's initial state: hmpc_swing_state_init_device writes it for `batch` instances on `stream`.
 * hmpc_swing_legs_device: the update alone.  device_ticks = hmpc_tick_inputs[batch] (read only), device_state [batch], device_tau
 * [batch][10] or NULL (= zeros), device_cmd [batch], device_detail double[batch][2][16] or NULL.  It does not replace the handle's batch and
 * reads nothing of a solve.
 * hmpc_tick_command_device: what hmpc_tick_solve_device enqueues (its torques go to a small buffer of the handle's), then the swing launch
 * reading that tick's torques: forces, status, f_ff, wpd and cmd.tau are bit for bit what hmpc_tick_solve_device leaves.  cfg->dtMPC is
 * read as given (the dtMPC argument is the solve's).
 * hmpc_set_rollout_swing: while cfg != NULL is set, every tick of hmpc_rollout_device and hmpc_rollout_sweep_device enqueues the swing launch
 * behind the tick's torque launch (before the plant step), with subtick = (subtick0 + k) % ticks_per_step and ticks_per_step the rollout's own
 * (the two members of cfg are not read; updates and the rest are, and are checked by the rollout); device_state [batch] as above (for a sweep:
 * per EXPANDED instance), device_cmd_log [batch][n_ticks] or NULL: row (i, k) = the command of instance i at tick k.  cfg is copied; the two
 * buffers are the caller's and must outlive the rollouts.  cfg == NULL turns it off (the default): a rollout then enqueues exactly what it
 * did before.  The plant never reads the command (the plant has no legs); struct hmpc_rollout_log is unchanged.
 * HMPC_E_ARG, nothing enqueued: a NULL handle, ticks, cfg, state or cmd; batch < 0 or > max_batch; updates < 1, ticks_per_step < 1, subtick < 0
 * or >= ticks_per_step; a three-contact handle.  hmpc_set_rollout_swing: a NULL handle, cfg != NULL with a NULL state or updates < 1, a
 * three-contact handle.  Device groups: per member, through hmpc_group_member. */
struct hmpc_swing {
  double dt_update;               /* 0.001: what one update takes off the swing timer (the reference's constant _dt) */
  double dtMPC;                   /* 0.04: seconds per horizon step (_dtSwing) */
  int updates;                    /* 2: updates per launch (run() calls updateSwingLeg() once per foot), >= 1 */
  int ticks_per_step;             /* 40: ticks per horizon step (iterationsBetweenMPC), >= 1 */
  int subtick;                    /* 0: this tick's position within its horizon step, 0 .. ticks_per_step - 1 */
  int reserved;                   /* 0 */
  double height;                  /* 0.15: apex of the swing above p0 */
  double place_gain_v;            /* 1.75 */
  double place_gain_err;          /* 0.1 */
  double place_max;               /* 0.3: clamp of the touchdown offset, applied in binary32 */
  double hip_yaw[2][3];           /* Biped.h getHipYawLocation: (-0.005, -0.057, -0.126) for leg 0, y negated for leg 1; body frame */
  double hip_roll[3];             /* Biped.h getHipRollLocation(0): (0.0465, 0.015, -0.0705) */
  double hip_width_offset[2][3];  /* (-0.015, 0.055, 0) for leg 0, y negated for leg 1 (SwingLegController.cpp:145-146) */
  double ik_link;                 /* 0.22: thigh and calf length of the IK */
  double ik_horizontal;           /* 0.0205: distance_horizontal */
  double ik_hip_x;                /* 0.06: taken off hip_roll[0] */
  double kp[5], kd[5];            /* (30, 30, 30, 30, 20), (1, 1, 1, 1, 1): joint gains of a swing leg */
};
struct hmpc_swing_state {
  double p0[2][3], pf[2][3];      /* the trajectory's initial and final position per leg, world frame */
  double swing_time[2];           /* swingTimes */
  double q_des[10];               /* commands[leg].qDes as the last swing update left it */
  int32_t first_swing[2];         /* firstSwing */
};
struct hmpc_motor_cmd {
  double q[10], dq[10], Kp[10], Kd[10], tau[10];   /* left leg 0-4, right leg 5-9 */
};
void hmpc_default_swing(struct hmpc_swing *cfg);
int hmpc_swing_state_init_device(hmpc_handle *h, struct hmpc_swing_state *device_state, int batch, void *stream);
int hmpc_swing_legs_device(hmpc_handle *h, const void *device_ticks, int batch, const struct hmpc_swing *cfg,
                           struct hmpc_swing_state *device_state, const double *device_tau, struct hmpc_motor_cmd *device_cmd,
                           double *device_detail, void *stream);
int hmpc_tick_command_device(hmpc_handle *h, const void *device_ticks, int batch, double dtMPC, const struct hmpc_swing *cfg,
                             struct hmpc_swing_state *device_state, double *device_wpd_out, double *device_f_ff,
                             struct hmpc_motor_cmd *device_cmd, void *stream);
int hmpc_set_rollout_swing(hmpc_handle *h, const struct hmpc_swing *cfg, void *device_state, struct hmpc_motor_cmd *device_cmd_log);
/* copies the current batch's packed records device -> host (parity hook for f1/f2) */
int hmpc_download_records(hmpc_handle *h, void *host_records);

/* Parity hook: runs the ASSEMBLY stage only for instance `index` of the current batch (same device code the
 * solve kernel runs) and returns the reduced QP exactly as the solver sees it: n, m, var_ind[n] (original
 * variable index, SolverMPC.cpp:644-658), H[n*n] (float, row-major, symmetric), g[n], the 16x12 constraint
 * block Fc, lb/ub[16h] (unreduced) and x0[13], Acd[169], Bcd[156].  Any output pointer may be NULL. */
int hmpc_debug_assemble(hmpc_handle *h, int index, int *n, int *m, int *var_ind, float *H, float *g, float *Fc,
                        float *lb, float *ub, float *x0, float *Acd, float *Bcd);
/* Parity hook: double-precision primal solution [batch][12h] and per-instance dual objective of the last solve.
 * hmpc_enable_f64_output (before the solve) makes every later solve write them; without it hmpc_download_f64 enables
 * the copy-out and runs the current batch once more (flagged instances get the safe pass of hmpc_download). */
int hmpc_enable_f64_output(hmpc_handle *h);
/* Parity hook: runs the SOLVER stages of the kernel (inverse, block start, dual active set, scatter) for the current batch
 * on QP data handed in from outside instead of the kernel's own assembly: per instance the reduced Hessian H[ld][ld] and
 * gradient g[ld] in the reference's reduced order (SolverMPC.cpp:644-697; binary32 values -- the reference's H_red / g_red
 * are widened floats; the upper triangle of H is read) and the per-step constraint block Fc[16][12] (fmat,
 * SolverMPC.cpp:466-548; [24][18] with three contacts).  The records of the current batch still supply the gait tables and
 * f_max.  Forces/status are written as by hmpc_solve.  tests/test_reference_source.py feeds it the reference's own data. */
int hmpc_debug_solve_external_qp(hmpc_handle *h, const float *H, const float *g, const float *Fc, int ld);
int hmpc_download_f64(hmpc_handle *h, double *x, double *obj);
/* Test hook: the hand-over slot table of the current batch, slots[batch]: slots[i] == i where the last solve's fast launch
 * left instance i's working set for the continuation pass (its status word HMPC_S_WORKSET) and no pass has consumed it yet,
 * -1 everywhere else.  Never an entry of an earlier solve or batch. */
int hmpc_debug_handover_slots(hmpc_handle *h, int *slots);
/* A/B switch (default on): a solve of a two-contact batch enqueues one small launch ahead of its fast pass that computes the serial
 * scalar front of every instance's assembly -- joint and Euler trigonometry, body algebra, foot rotations, stance prefix counts -- for
 * the whole batch (csrc/hmpc_front.hip), and the fast kernels read the result.  Off: every kernel computes it itself, as the safe and
 * continuation passes, command sweeps, three-contact batches and the derived results always do.  The results are the same bits. */
int hmpc_debug_set_front_prologue(hmpc_handle *h, int on);
/* Test hook: runs that launch on the current batch (two contacts) and copies its blocks to the host, out[batch][320 bytes]; per block:
 * float rpy[3], dt_Rbi[9] (0 + dt Rbi), dt_Iinv[9], dt_blk[2][9] (dt Iinv [r_leg]x), foot[2][12] (per leg t0, t1, flt, flh: the vectors
 * the leg's rows of the constraint block are made of), one float of padding; unsigned char pre_nl[20], pre_nv[20], pre_st[20] (per
 * horizon step: stance leg-steps and reduced variables before it, stance bits; zero beyond the horizon); unsigned short n, nls. */
int hmpc_debug_front_scalars(hmpc_handle *h, void *out);

/* Developer hook (only in builds with -DHMPC_PROFILE, scripts/phase_profile.py): per-phase shader-clock cycles of
 * one more launch of the current batch, [batch][32] (phase ids: hmpc_kernel.h P_*). */
int hmpc_debug_phase_cycles(hmpc_handle *h, long long *cycles);

/* ---- device groups: one process, several GPUs of a node (csrc/hmpc_group.hip) ----
 * Every MPC instance is an independent QP: a batch is cut into contiguous slices [lo, hi), one per member device
 * (hmpc_shard_bounds: the first batch % n members carry one extra instance), each solved by its own handle on its own
 * stream with no data-path collective.  The single exchange step is the gather of what the controller reads,
 * get_solution(0..11) of every instance (ConvexMPCLocomotion.cpp:419-440): the step-0 wrench [F_L F_R M_L M_R] and the
 * status word.  hmpc_group_post_gather packs them on each solve stream and all-gathers the packed slices on each
 * member's communication stream (RCCL: ncclCommInitAll + grouped ncclAllGather, librccl loaded on first use; or
 * hipMemcpyPeerAsync copies), so the exchange of solve k runs under solve k+1; afterwards EVERY member holds the
 * gathered block in HBM (hmpc_group_device_gathered) and hmpc_group_gather_wrench also hands it to the host. */
typedef struct hmpc_group hmpc_group;
enum hmpc_group_deal {
  HMPC_DEAL_CONTIGUOUS = 0, /* member i holds the contiguous slice of hmpc_shard_bounds (default) */
  HMPC_DEAL_STRIPED = 1     /* member i holds instances i, i + G, i + 2 G, ...: an ORDERED sweep's hard instances are spread over all members */
};
enum hmpc_group_transport {
  HMPC_GROUP_AUTO = 0, /* RCCL when all listed devices are distinct, else P2P */
  HMPC_GROUP_RCCL = 1,
  HMPC_GROUP_P2P = 2   /* the only transport that accepts a device listed twice (one-GPU test of the multi-member path) */
};
int hmpc_shard_bounds(int global_batch, int n_shards, int index, int *lo, int *hi);
/* devices == NULL: devices 0 .. n_devices-1.  max_batch is the GLOBAL batch the group can hold. */
int hmpc_group_create(hmpc_group **out, const struct problem_setup *setup, const int *devices, int n_devices,
                      int max_batch, int transport);
/* the same for handles of n_contacts = 2 or 3 (BASELINE config 5 runs the three-contact extension on 4 GPUs): records of
 * hmpc_record_stride_ex(h, n_contacts) bytes, forces [batch][6 n_contacts h], and the exchange carries the step-0 wrench of
 * every contact -- 6 n_contacts values [F_0 .. F_{nc-1}, M_0 .. M_{nc-1}] + the status word per instance. */
int hmpc_group_create_ex(hmpc_group **out, const struct problem_setup *setup, const int *devices, int n_devices,
                         int max_batch, int transport, int n_contacts);
int hmpc_group_contacts(const hmpc_group *g);
int hmpc_group_destroy(hmpc_group *g);
int hmpc_group_size(const hmpc_group *g);
int hmpc_group_transport(const hmpc_group *g);
int hmpc_group_batch(const hmpc_group *g);
/* member's handle (for the per-handle switches), device, slice of the current batch and solve stream; any may be NULL */
int hmpc_group_member(hmpc_group *g, int member, hmpc_handle **handle, int *device, int *lo, int *n, void **solve_stream);
int hmpc_group_upload_records(hmpc_group *g, const void *host_records, int batch);
/* How the next batch is dealt to the members (enum hmpc_group_deal).  Host-facing results (hmpc_group_gather_wrench,
 * hmpc_group_download) are in instance order either way (and the same bits, as long as every member's handle picks the same
 * kernel variant under both deals -- a member that is dealt single-support instances only runs the 60-variable variant, whose
 * answers agree with the 120-variable one's to solver precision); member sizes are the same either way; in striped mode row r of slot s
 * of the device-resident gathered block is instance s + r G, and hmpc_group_member_step returns G (1 for contiguous slices). */
int hmpc_group_set_deal(hmpc_group *g, int deal);
/* the same robot / contact constants on every member (hmpc_set_params) */
int hmpc_group_set_params(hmpc_group *g, const struct hmpc_params *p);
int hmpc_group_deal(const hmpc_group *g);
int hmpc_group_member_step(const hmpc_group *g, int member);
/* device_records[i] = member i's first record, resident on member i's device (slice sizes from hmpc_shard_bounds) */
int hmpc_group_set_device_records(hmpc_group *g, const void *const *device_records, int batch, int max_reduced_vars);
int hmpc_group_solve(hmpc_group *g);       /* asynchronous on every member */
/* hmpc_solve_command_sweep on every member: every member's slice must consist of whole groups (contiguous deal, and
 * slice sizes that are multiples of group_size -- e.g. batch = members x k x group_size), else HMPC_E_ARG and nothing is enqueued */
int hmpc_group_solve_command_sweep(hmpc_group *g, int group_size);
int hmpc_group_post_gather(hmpc_group *g); /* asynchronous: the exchange step for the solves enqueued so far */
int hmpc_group_wait_gather(hmpc_group *g);
/* member's gathered copy in HBM: [group size][slot_rows][6 nc + 1] 32-bit words (13 for two contacts), slot s = member s's
 * slice, row = the 6 nc floats of the step-0 wrench + the status word.  Valid from hmpc_group_wait_gather until the next hmpc_group_post_gather. */
int hmpc_group_device_gathered(hmpc_group *g, int member, const uint32_t **gathered, int *slot_rows);
/* blocking form of the exchange step: collects the exchange hmpc_group_post_gather posted if it has not been collected
 * yet (by hmpc_group_wait_gather or an earlier hmpc_group_gather_wrench) -- the pipelined pattern post(k), solve(k+1),
 * gather_wrench() returns solve k's results -- and otherwise posts one now for the solves enqueued so far; waits, and
 * returns host copies in instance order of the batch the exchange was posted for (its slices are remembered at post
 * time): wrench [batch][6 nc] (12 for two contacts), status [batch] (either may be NULL).
 * The exchange carries REPAIRED rows: every member's solve is followed on its stream, without a host round trip, by the
 * safe variant over the instances the fast variant flagged (hmpc_set_device_repair, on by default for group members).  hmpc_group_set_exchange_repair(g, 0) turns that off: the exchange then carries the fast
 * pass's results as they are (a flagged instance shows in its status word, its wrench is not valid) and only
 * hmpc_group_download repairs.  Instances that defeat even the safe variant (degenerate vertices, < 0.1 % at 6x the
 * nominal input ranges) stay flagged in the status word either way; hmpc_group_download's relaxed passes handle them. */
int hmpc_group_gather_wrench(hmpc_group *g, float *host_wrench, uint32_t *host_status);
int hmpc_group_set_exchange_repair(hmpc_group *g, int on);
/* all 12h forces of every instance to the host (no collective; the members' safe pass included) */
int hmpc_group_download(hmpc_group *g, float *forces, uint32_t *status);
int hmpc_group_synchronize(hmpc_group *g);
const char *hmpc_group_last_error(void);

const char *hmpc_last_hip_error(void);
const char *hmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif
