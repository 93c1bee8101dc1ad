"""Python mirror of the MPC boundary -- same names, argument meaning and error behaviour as the reference's
``ConvexMPC/convexMPC_interface.h:39-43`` (``setup_problem`` / ``update_problem_data`` / ``get_solution`` /
``update_solver_settings``) plus the batched handle API of ``include/hector_mpc.h``.

Everything here is a thin ctypes call into ``libhector_mpc_hip.so``; there is no Python/NumPy/PyTorch compute path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, records

TICK_DTYPE = np.dtype([("position", "f8", 3), ("vWorld", "f8", 3), ("omegaWorld", "f8", 3), ("orientation", "f8", 4),
                       ("rpy", "f8", 3), ("rBody", "f8", 9), ("leg_q", "f8", 10), ("pFoot", "f8", 6),
                       ("v_des_robot", "f8", 2), ("yaw_rate_des", "f8"), ("roll_des", "f8"), ("pitch_des", "f8"),
                       ("world_position_desired", "f8", 2), ("gait_offsets", "i4", 2), ("gait_durations", "i4", 2),
                       ("gait_iteration", "i4"), ("flags", "i4")], align=True)

# struct hmpc_command: the five command fields of a tick, in their order (hmpc_tick_sweep_device)
COMMAND_DTYPE = np.dtype([("v_des_robot", "f8", 2), ("yaw_rate_des", "f8"), ("roll_des", "f8"), ("pitch_des", "f8")], align=True)
SELECT_NONE = 0xFFFFFFFF  # HMPC_SELECT_NONE: the status word of a group without a winner

TICK_LEG_Q_MOTOR, TICK_FALLEN = 1, 2       # HMPC_TICK_* bits of hmpc_tick_inputs.flags
PLANT_GYRO, PLANT_PLACE_FEET = 1, 2        # HMPC_PLANT_* bits of hmpc_plant.flags


def default_plant(**fields):
    """``struct hmpc_plant`` with the defaults of ``hmpc_default_plant``; keyword arguments overwrite scalar fields (dt_tick, dtMPC,
    substeps, advance_gait, flags, mass, gravity, fall_cos) and ``inertia`` (3 values) / ``hip`` (2 x 3)."""
    p = _lib.Plant()
    _lib.load().hmpc_default_plant(C.byref(p))
    for k, v in fields.items():
        if k == "inertia":
            p.inertia[:] = [float(x) for x in v]
        elif k == "hip":
            for leg in range(2):
                p.hip[leg][:] = [float(x) for x in v[leg]]
        else:
            setattr(p, k, v)
    return p


def default_rollout_cost(**fields):
    """``struct hmpc_rollout_cost`` with the defaults of ``hmpc_default_rollout_cost``; keyword arguments overwrite the scalar fields (height,
    dt_tick, fall_penalty, unsolved_penalty) and the weight vectors ``w_state``, ``w_terminal``, ``w_wrench`` (12 values each), ``w_tau`` (10)."""
    c = _lib.RolloutCost()
    _lib.load().hmpc_default_rollout_cost(C.byref(c))
    for k, v in fields.items():
        if k.startswith("w_"):
            getattr(c, k)[:] = [float(x) for x in v]
        else:
            setattr(c, k, float(v))
    return c


# struct hmpc_swing_state and struct hmpc_motor_cmd (swing legs on the device, include/hector_mpc.h)
SWING_STATE_DTYPE = np.dtype([("p0", "f8", (2, 3)), ("pf", "f8", (2, 3)), ("swing_time", "f8", 2), ("q_des", "f8", 10), ("first_swing", "i4", 2)],
                             align=True)
MOTOR_CMD_DTYPE = np.dtype([("q", "f8", 10), ("dq", "f8", 10), ("Kp", "f8", 10), ("Kd", "f8", 10), ("tau", "f8", 10)], align=True)
SWING_DETAIL = ("swing", "pFoot_w", "pDes", "vDes", "pFoot_b", "vFoot_b")  # a detail row [16] of swing_legs: one value, then five vectors of 3


def default_swing(**fields):
    """``struct hmpc_swing`` with the reference's values (``hmpc_default_swing``); keyword arguments overwrite the scalar fields and the
    arrays ``hip_yaw`` / ``hip_width_offset`` (2 x 3), ``hip_roll`` (3), ``kp`` / ``kd`` (5)."""
    c = _lib.Swing()
    _lib.load().hmpc_default_swing(C.byref(c))
    for k, v in fields.items():
        if k in ("hip_yaw", "hip_width_offset"):
            for leg in range(2):
                getattr(c, k)[leg][:] = [float(x) for x in v[leg]]
        elif k in ("hip_roll", "kp", "kd"):
            getattr(c, k)[:] = [float(x) for x in v]
        else:
            setattr(c, k, v)
    return c


def initial_swing_state(batch: int) -> np.ndarray:
    """The reference's initial swing state of ``batch`` instances on the host: all zero, ``first_swing = {1, 1}``."""
    s = np.zeros(int(batch), dtype=SWING_STATE_DTYPE)
    s["first_swing"] = 1
    return s


STATUS_NAMES = {0: "ok", 1: "max_iter", 2: "infeasible", 3: "too_large", 4: "kkt", 5: "working_set_full", 6: "ok_relaxed", 7: "sweep_mismatch", 8: "hessian_not_positive_definite", 9: "regularisation_step"}


class HmpcError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        raise HmpcError(f"{what} failed with {rc}: {_lib.load().hmpc_last_hip_error().decode()}")


# ---------------------------------------------------------------- reference (legacy) interface, process-global
def setup_problem(dt: float, horizon: int, mu: float, f_max: float) -> None:
    _lib.load().setup_problem(float(dt), int(horizon), float(mu), float(f_max))


def update_problem_data(p, v, q, w, r, joint_angles, yaw, weights, state_trajectory, Alpha_K, gait) -> None:
    """Blocking: narrows to float, solves on the GPU, leaves the solution for ``get_solution`` (as the reference does)."""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (p, v, q, w, r, joint_angles)]
    b = [np.ascontiguousarray(x, dtype=np.float64) for x in (weights, state_trajectory, Alpha_K)]
    g = np.ascontiguousarray(gait, dtype=np.int32)
    _lib.load().update_problem_data(*[x.ctypes.data for x in a], float(yaw), *[x.ctypes.data for x in b], g.ctypes.data)


def get_solution(index: int) -> float:
    return float(_lib.load().get_solution(int(index)))


def update_solver_settings(max_iter, rho, sigma, solver_alpha, terminate, use_jcqp) -> None:
    """Stored and read by nothing, exactly as in the reference (convexMPC_interface.cpp:112-118)."""
    _lib.load().update_solver_settings(int(max_iter), float(rho), float(sigma), float(solver_alpha), float(terminate),
                                       float(use_jcqp))


def legacy_set_max_iterations(max_iter: int) -> None:
    """Explicit opt-in: cap on the active-set iterations of the process-global (legacy) solver; 0 = none."""
    _check(_lib.load().hmpc_legacy_set_max_iterations(int(max_iter)), "hmpc_legacy_set_max_iterations")


def legacy_predicted_state(step: int, component: int) -> float:
    """Component (0..12) of the state the process-global solver's model predicts for ``step`` (0..horizon-1) under its last solution
    (include/hector_mpc.h hmpc_legacy_predicted_state); 0 before the first solve and for out-of-range arguments."""
    return float(_lib.load().hmpc_legacy_predicted_state(int(step), int(component)))


def legacy_constraint_slack(step: int, contact: int, j: int) -> float:
    """Slack ``j`` (0..9) of ``contact`` (0, 1) at ``step`` (0..horizon-1) of the process-global solver's last solution
    (include/hector_mpc.h hmpc_legacy_constraint_slack); 0 before the first solve and for out-of-range arguments."""
    return float(_lib.load().hmpc_legacy_constraint_slack(int(step), int(contact), int(j)))


def legacy_multiplier(step: int, contact: int, j: int) -> float:
    """Multiplier ``j`` (0..9) of ``contact`` (0, 1) at ``step`` (0..horizon-1) of the process-global solver's last solution
    (include/hector_mpc.h hmpc_legacy_multiplier); 0 before the first solve and for out-of-range arguments."""
    return float(_lib.load().hmpc_legacy_multiplier(int(step), int(contact), int(j)))


def legacy_stationarity() -> float:
    """The stationarity residual (summary[0] of the KKT certificate) of the process-global solver's last solution; 0 before the first."""
    return float(_lib.load().hmpc_legacy_stationarity())


def legacy_feedback_gain(component: int, state: int) -> float:
    """Entry [component][state] (0..11, 0..12) of K_0 = du_0/dx_0 of the process-global solver's last solution (include/hector_mpc.h
    hmpc_legacy_feedback_gain); 0 before the first solve and for out-of-range arguments."""
    return float(_lib.load().hmpc_legacy_feedback_gain(int(component), int(state)))


def last_status() -> int:
    return int(_lib.load().hmpc_last_status())


# ---------------------------------------------------------------- the results derived from a solve
# THE shape table of the host side: per family -- named by the suffix of its hmpc_set_device_* / hmpc_get_device_* / hmpc_download_*
# entries -- its arrays in the argument order of those entries, each with its dtype and the shape of one row (one instance's; one sweep
# group's for the selection) as a function of (horizon, contacts).  Every host array of a download is allocated from here, and _lib.py
# counts the entries' arguments here.  The library keeps its own copy (csrc/hmpc_results.h); tests/test_result_layout_on_host.py
# compares the two line by line.
def _record_floats(h, c):
    return ((records.N_FIXED3 if c == 3 else records.N_FIXED) + 12 * h,)


_f4, _f8, _i4, _u4 = np.float32, np.float64, np.int32, np.uint32
RESULTS = {
    "prediction": (("states", _f4, lambda h, c: (h, 13)), ("cost", _f8, lambda h, c: (2,))),
    "selection": (("index", _i4, lambda h, c: ()), ("score", _f8, lambda h, c: ()), ("forces", _f4, lambda h, c: (6 * c * h,)),
                  ("status", _u4, lambda h, c: ()), ("states", _f4, lambda h, c: (h, 13))),
    "margins": (("slack", _f8, lambda h, c: (h, c, 10)), ("summary", _f8, lambda h, c: (6,)), ("where", _i4, lambda h, c: (6,))),
    "certificate": (("grad", _f8, lambda h, c: (h, 6 * c)), ("lambda", _f8, lambda h, c: (h, c, 10)), ("resid", _f8, lambda h, c: (h, c, 6)),
                    ("summary", _f8, lambda h, c: (4,)), ("where", _i4, lambda h, c: (2,))),
    "gains": (("gain", _f8, lambda h, c: (6 * c, 13)), ("ref_gain", _f8, lambda h, c: (h, 6 * c, 12)), ("summary", _f8, lambda h, c: (2,)),
              ("free_dims", _i4, lambda h, c: (h,))),
    "first_order": (("wrench", _f4, lambda h, c: (6 * c,)), ("worst_slack", _f8, lambda h, c: ())),
    "adjoint": (("grad_x0", _f8, lambda h, c: (13,)), ("grad_traj", _f8, lambda h, c: (h, 12)), ("grad_weights", _f8, lambda h, c: (12,)),
                ("grad_alpha", _f8, lambda h, c: (6 * c,)), ("dir", _f8, lambda h, c: (h, 6 * c)), ("summary", _f8, lambda h, c: (2,))),
    "adjoint_model": (("grad_A", _f8, lambda h, c: (13, 13)), ("grad_B", _f8, lambda h, c: (13, 6 * c)), ("grad_r", _f8, lambda h, c: (3, c)),
                      ("grad_params", _f8, lambda h, c: (4,)), ("costate", _f8, lambda h, c: (2, 13))),
    "adjoint_limits": (("grad_limits", _f8, lambda h, c: (3 + c,)), ("grad_Fc", _f8, lambda h, c: (8 * c, 6 * c)),
                       ("grad_bound", _f8, lambda h, c: (h, c, 10)), ("lambda", _f8, lambda h, c: (h, c, 10)), ("nu", _f8, lambda h, c: (h, c, 10)),
                       ("summary", _f8, lambda h, c: (3,))),
    "adjoint_record": (("grad_record", _f8, _record_floats), ("grad_frames", _f8, lambda h, c: (1 + c, 3, 3)), ("grad_rpy", _f8, lambda h, c: (3,))),
}
RESULTS["adjoint_multi"] = RESULTS["adjoint"]  # (one row per (seed, instance))


def _row_of(family, name, as_name=None):
    return next((as_name or k, dt, shape) for k, dt, shape in RESULTS[family] if k == name)


# the chain: struct hmpc_adjoint_chain's members, each the record, model or limit row it is (six compact, eight detail)
RESULTS["adjoint_chain_multi"] = (
    tuple(_row_of("adjoint_record", k) for k in ("grad_record", "grad_frames", "grad_rpy")) + (_row_of("adjoint_model", "grad_params"),
    _row_of("adjoint_limits", "grad_limits"), _row_of("adjoint_limits", "summary", "limit_summary"))
    + tuple(_row_of("adjoint_model", k) for k in ("grad_A", "grad_B", "grad_r", "costate"))
    + tuple(_row_of("adjoint_limits", k) for k in ("grad_Fc", "grad_bound", "lambda", "nu")))
assert tuple(k for k, _, _ in RESULTS["adjoint_chain_multi"]) == _lib.CHAIN_COMPACT + _lib.CHAIN_DETAIL


def _result_keys(family):
    return tuple(k for k, _, _ in RESULTS[family])


# ---------------------------------------------------------------- batched handle API
class BatchedMPC:
    """One handle = one GPU, one (dt, f_max, horizon) problem shape, up to ``max_batch`` independent MPC instances.

    ``contacts=3`` selects the hand-contact extension (BASELINE config 5; include/hector_mpc.h ``hmpc_create_ex``)."""

    def __init__(self, dt: float, horizon: int, f_max: float, max_batch: int, mu: float = 0.25, device: int = 0,
                 contacts: int = 2):
        self.L = _lib.load()
        self.horizon, self.max_batch, self.device = int(horizon), int(max_batch), int(device)
        self.contacts = int(contacts)
        self.nvar = 6 * self.contacts * self.horizon  # forces per instance: [step][F of each contact, M of each contact]
        self.setup = _lib.ProblemSetup(np.float32(dt), np.float32(mu), np.float32(f_max), int(horizon))
        self.h = C.c_void_p()
        _check(self.L.hmpc_create_ex(C.byref(self.h), C.byref(self.setup), self.max_batch, self.device, self.contacts),
               "hmpc_create_ex")
        self.stride = int(self.L.hmpc_record_stride_ex(self.horizon, self.contacts))
        self._keep = None
        self._keep_out = None
        self._keepalive = {}  # what the caller's buffers of every derived result keep alive, by family
        self.dt_mpc = float(dt)  # (binary64, as given: what rollout() passes as dtMPC by default)
        self.generation = 0  # counts the calls of this object that replace the batch or its forces (autograd.py compares it)

    def close(self):
        if getattr(self, "h", None):
            self.L.hmpc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def batch(self) -> int:
        return int(self.L.hmpc_batch(self.h))

    def upload(self, recs: np.ndarray) -> None:
        self.generation += 1
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        assert recs.ndim == 2 and recs.shape[1] == self.stride, (recs.shape, self.stride)
        _check(self.L.hmpc_upload_records(self.h, recs.ctypes.data, recs.shape[0]), "hmpc_upload_records")

    def upload_async(self, host_ptr: int, batch: int, stream: int = 0) -> None:
        """Stream-ordered upload from a (pinned) host buffer of ``batch`` packed records."""
        self.generation += 1
        _check(self.L.hmpc_upload_records_async(self.h, C.c_void_p(host_ptr), int(batch), C.c_void_p(stream)),
               "hmpc_upload_records_async")

    def download_async(self, forces_ptr: int, status_ptr: int, stream: int = 0) -> None:
        """Stream-ordered download into (pinned) host buffers; no safe pass (see include/hector_mpc.h)."""
        _check(self.L.hmpc_download_async(self.h, C.c_void_p(forces_ptr), C.c_void_p(status_ptr), C.c_void_p(stream)),
               "hmpc_download_async")

    def upload_fields(self, fields: dict) -> None:
        self.upload(records.pack_records(fields, self.horizon, self.contacts))

    def set_device_records(self, device_ptr: int, batch: int, max_reduced_vars: int = -1, keepalive=None) -> None:
        self.generation += 1
        self._keep = keepalive
        _check(self.L.hmpc_set_device_records(self.h, C.c_void_p(device_ptr), int(batch)), "hmpc_set_device_records")
        _check(self.L.hmpc_set_max_reduced_vars(self.h, int(max_reduced_vars)), "hmpc_set_max_reduced_vars")

    def set_device_outputs(self, forces_ptr: int, status_ptr: int, keepalive=None) -> None:
        self.generation += 1
        self._keep_out = keepalive
        _check(self.L.hmpc_set_device_outputs(self.h, C.c_void_p(forces_ptr), C.c_void_p(status_ptr)),
               "hmpc_set_device_outputs")

    def set_warm_start(self, on: bool) -> None:
        _check(self.L.hmpc_set_warm_start(self.h, 1 if on else 0), "hmpc_set_warm_start")

    def set_tick_warm_start(self, on: bool, horizon_shift: int = 0) -> None:
        """Carry each instance's final working set to the next solve of this handle (off by default: the reference
        cold-starts every tick).  ``horizon_shift`` = steps the gait table advanced since the previous solve."""
        _check(self.L.hmpc_set_tick_warm_start(self.h, 1 if on else 0, int(horizon_shift)), "hmpc_set_tick_warm_start")

    def reset_tick_warm_start(self) -> None:
        _check(self.L.hmpc_reset_tick_warm_start(self.h), "hmpc_reset_tick_warm_start")

    def set_auto_resolve(self, on: bool) -> None:
        _check(self.L.hmpc_set_auto_resolve(self.h, 1 if on else 0), "hmpc_set_auto_resolve")

    def set_params(self, mass=None, inertia=None, mu=None, lt=None, lh=None, gravity=None) -> None:
        """Robot / contact constants (include/hector_mpc.h struct hmpc_params); arguments left out keep the reference's literals
        (mass 9.0, inertia diag (0.5413, 0.5200, 0.0691), mu 2.0, lt 0.09, lh 0.06, gravity 9.81); no arguments = all defaults."""
        p = _lib.Params()
        self.L.hmpc_default_params(C.byref(p))
        if mass is not None:
            p.mass = np.float32(mass)
        if inertia is not None:
            p.inertia[:] = [np.float32(v) for v in inertia]
        if mu is not None:
            p.mu = np.float32(mu)
        if lt is not None:
            p.lt = np.float32(lt)
        if lh is not None:
            p.lh = np.float32(lh)
        if gravity is not None:
            p.gravity = np.float32(gravity)
        _check(self.L.hmpc_set_params(self.h, C.byref(p)), "hmpc_set_params")

    def set_instance_mu(self, device_ptr: int, keepalive=None) -> None:
        """Per-instance friction parameter (float32[batch] in HBM; 0 / None = off): terrain sweeps, also inside a command-sweep group
        (include/hector_mpc.h hmpc_set_instance_mu)."""
        self._keep_mu = keepalive
        _check(self.L.hmpc_set_instance_mu(self.h, C.c_void_p(int(device_ptr or 0))), "hmpc_set_instance_mu")

    def get_params(self) -> dict:
        p = _lib.Params()
        _check(self.L.hmpc_get_params(self.h, C.byref(p)), "hmpc_get_params")
        return dict(mass=float(p.mass), inertia=[float(v) for v in p.inertia], mu=float(p.mu), lt=float(p.lt), lh=float(p.lh),
                    gravity=float(p.gravity))

    def set_handover(self, on: bool) -> None:
        """Continue (default) or re-solve cold the instances whose working set outgrew the fast variant (hmpc_set_handover)."""
        _check(self.L.hmpc_set_handover(self.h, 1 if on else 0), "hmpc_set_handover")

    def set_device_repair(self, on) -> None:
        """Device-side safe pass inside every solve (include/hector_mpc.h hmpc_set_device_repair); 2 = continuation pass only."""
        _check(self.L.hmpc_set_device_repair(self.h, 2 if on == 2 else (1 if on else 0)), "hmpc_set_device_repair")

    def set_max_iterations(self, max_iter: int) -> None:
        """Cap on the active-set iterations (0 = none); the nWSR analogue (include/hector_mpc.h hmpc_set_max_iterations)."""
        _check(self.L.hmpc_set_max_iterations(self.h, int(max_iter)), "hmpc_set_max_iterations")

    def set_dispatch_order(self, mode) -> None:
        """0 / False: natural order; 1 / True (default): longest previous solve first, a cold handle by the cost predicted
        from the records; 2: always by the predictor (include/hector_mpc.h hmpc_set_dispatch_order).  Results do not depend
        on it."""
        _check(self.L.hmpc_set_dispatch_order(self.h, int(mode)), "hmpc_set_dispatch_order")

    def tick_solve_device(self, ticks_ptr: int, batch: int, dt_mpc: float, tau_ptr: int, f_ff_ptr: int = 0, wpd_ptr: int = 0,
                          stream: int = 0) -> None:
        """f1+f2 -> solve -> f3 on one stream, everything device-resident (include/hector_mpc.h hmpc_tick_solve_device)."""
        self.generation += 1
        _check(self.L.hmpc_tick_solve_device(self.h, C.c_void_p(ticks_ptr), int(batch), float(dt_mpc), C.c_void_p(wpd_ptr),
                                             C.c_void_p(f_ff_ptr), C.c_void_p(tau_ptr), C.c_void_p(stream)),
               "hmpc_tick_solve_device")

    def resolve_failed(self) -> int:
        n = C.c_int(0)
        _check(self.L.hmpc_resolve_failed(self.h, C.byref(n)), "hmpc_resolve_failed")
        return int(n.value)

    def solve(self, stream: int = 0) -> None:
        self.generation += 1
        _check(self.L.hmpc_solve(self.h, C.c_void_p(stream)), "hmpc_solve")

    def solve_command_sweep(self, group_size: int, stream: int = 0) -> None:
        """The current batch as groups of ``group_size`` consecutive records that differ in the reference trajectory only: H is
        assembled and inverted once per group, every instance solves with its group's inverse -- bit-identical results
        (include/hector_mpc.h hmpc_solve_command_sweep)."""
        self.generation += 1
        _check(self.L.hmpc_solve_command_sweep(self.h, int(group_size), C.c_void_p(stream)), "hmpc_solve_command_sweep")

    def download(self):
        b = self.batch
        forces = np.zeros((b, self.nvar), dtype=np.float32)
        status = np.zeros(b, dtype=np.uint32)
        _check(self.L.hmpc_download(self.h, forces.ctypes.data, status.ctypes.data), "hmpc_download")
        return forces, status

    def download_f64(self):
        b = self.batch
        x = np.zeros((b, self.nvar), dtype=np.float64)
        obj = np.zeros(b, dtype=np.float64)
        _check(self.L.hmpc_download_f64(self.h, x.ctypes.data, obj.ctypes.data), "hmpc_download_f64")
        return x, obj

    # ---- the results derived from a solve: every public method below is one call of these three helpers over RESULTS
    def result_shapes(self, family: str, lead) -> dict:
        """name -> shape of every array of ``family`` (a key of RESULTS) with the leading axes ``lead`` before one row's."""
        return {k: tuple(lead) + shape(self.horizon, self.contacts) for k, _, shape in RESULTS[family]}

    def _download(self, family: str, lead=None, only=None) -> dict:
        """Host arrays of ``family`` by RESULTS -- ``lead`` rows each (default: one per instance of the batch), ``only`` = the arrays
        wanted (default: all) -- filled by its ``hmpc_download_*`` entry."""
        shapes = self.result_shapes(family, (self.batch,) if lead is None else lead)
        out = {k: np.zeros(shapes[k], dtype=dt) for k, dt, _ in RESULTS[family] if only is None or k in only}
        if family == "adjoint_chain_multi":
            args = [C.byref(_lib.AdjointChain(**{k: v.ctypes.data for k, v in out.items()}))]
        else:
            args = [out[k].ctypes.data for k, _, _ in RESULTS[family]]
        _check(getattr(self.L, "hmpc_download_" + family)(self.h, *args), "hmpc_download_" + family)
        return out

    def _get_device(self, family: str, count: bool = False) -> dict:
        """Device pointers of ``family``'s arrays by name, from its ``hmpc_get_device_*`` entry; ``count``: the entry reports a count first
        (``n_seeds``)."""
        n, ptrs = C.c_int(0), [C.c_void_p() for _ in RESULTS[family]]
        _check(getattr(self.L, "hmpc_get_device_" + family)(self.h, *([C.byref(n)] if count else []), *[C.byref(p) for p in ptrs]),
               "hmpc_get_device_" + family)
        out = {k: int(p.value or 0) for (k, _, _), p in zip(RESULTS[family], ptrs)}
        return dict(out, n_seeds=n.value) if count else out

    def _set_device(self, family: str, ptrs, keepalive, *count) -> None:
        """``family``'s ``hmpc_set_device_*`` entry with the caller's pointers in the order of RESULTS (0 / None = the handle's own), behind
        ``count`` where the entry takes one (``n_seeds``); ``keepalive`` lives as long as the buffers are set."""
        self._keepalive[family] = keepalive
        assert len(ptrs) == len(RESULTS[family])
        _check(getattr(self.L, "hmpc_set_device_" + family)(self.h, *[int(c) for c in count], *[C.c_void_p(int(p or 0)) for p in ptrs]),
               "hmpc_set_device_" + family)

    def predict_states(self, stream: int = 0) -> None:
        """One launch behind the solve on ``stream``: the model's predicted states and tracking cost under the forces in the force buffer
        (include/hector_mpc.h hmpc_predict_states).  Raises when no solve of the current batch has been enqueued."""
        _check(self.L.hmpc_predict_states(self.h, C.c_void_p(stream)), "hmpc_predict_states")

    def download_prediction(self):
        """(states[batch, horizon, 13] float32: row i = the state after step i; cost[batch, 2] float64: tracking, force).  Waits; runs no
        safe pass (``download()`` first, then ``predict_states()`` again, for repaired forces)."""
        out = self._download("prediction")
        return out["states"], out["cost"]

    def set_device_prediction(self, states_ptr: int, cost_ptr: int, keepalive=None) -> None:
        """Caller-owned device buffers for later predictions (float32[max_batch, horizon, 13], float64[max_batch, 2]; 0 / None = the
        handle's own)."""
        self._set_device("prediction", (states_ptr, cost_ptr), keepalive)

    def sweep_select(self, group_size: int, penalty_ptr: int = 0, stream: int = 0) -> None:
        """One launch behind the prediction on ``stream``: the eligible instance of smallest (cost[0] + cost[1]) + penalty in every group of
        ``group_size`` consecutive instances (include/hector_mpc.h hmpc_sweep_select).  ``penalty_ptr``: float64[batch] in HBM, 0 = none.
        Raises when no prediction has been enqueued since the last solve of the current batch."""
        _check(self.L.hmpc_sweep_select(self.h, int(group_size), C.c_void_p(int(penalty_ptr or 0)), C.c_void_p(stream)), "hmpc_sweep_select")

    def download_selection(self) -> dict:
        """The last selection, one row per group: index int32[G] (-1 = no winner), score float64[G] (+inf), forces float32[G, nvar] and
        states float32[G, horizon, 13] (bit copies of the winner's rows, or zeros), status uint32[G] (``SELECT_NONE``).  Waits; runs no
        safe pass."""
        g = C.c_int(0)
        _check(self.L.hmpc_get_device_selection(self.h, None, None, None, None, None, C.byref(g)), "hmpc_get_device_selection")
        return self._download("selection", lead=(int(g.value),))

    def set_device_selection(self, index_ptr: int = 0, score_ptr: int = 0, forces_ptr: int = 0, status_ptr: int = 0, states_ptr: int = 0,
                             keepalive=None) -> None:
        """Caller-owned device buffers for later selections, one row per group (int32[G], float64[G], float32[G, nvar], uint32[G],
        float32[G, horizon, 13]; 0 / None = the handle's own)."""
        self._set_device("selection", (index_ptr, score_ptr, forces_ptr, status_ptr, states_ptr), keepalive)

    def tick_sweep_device(self, ticks_ptr: int, n_ticks: int, commands_ptr: int, group_size: int, dt_mpc: float, tau_ptr: int,
                          f_ff_ptr: int = 0, wpd_ptr: int = 0, penalty_ptr: int = 0, stream: int = 0) -> None:
        """Ticks (``TICK_DTYPE[n_ticks]``) and candidate commands (``COMMAND_DTYPE[n_ticks, group_size]``) in HBM in, the best command's
        torques in HBM out: records, sweep solve, prediction, selection and torques on one stream (include/hector_mpc.h
        hmpc_tick_sweep_device).  Which command won: ``download_selection()``."""
        self.generation += 1
        _check(self.L.hmpc_tick_sweep_device(self.h, C.c_void_p(ticks_ptr), int(n_ticks), C.c_void_p(commands_ptr), int(group_size),
                                             float(dt_mpc), C.c_void_p(int(penalty_ptr or 0)), C.c_void_p(int(wpd_ptr or 0)),
                                             C.c_void_p(int(f_ff_ptr or 0)), C.c_void_p(tau_ptr), C.c_void_p(stream)),
               "hmpc_tick_sweep_device")

    def constraint_margins(self, stream: int = 0) -> None:
        """One launch behind the solve on ``stream``: the slack of every constraint row under the forces in the force buffer and the six
        per-instance minima (include/hector_mpc.h hmpc_constraint_margins).  Raises when no solve of the current batch has been enqueued."""
        _check(self.L.hmpc_constraint_margins(self.h, C.c_void_p(stream)), "hmpc_constraint_margins")

    def download_margins(self) -> dict:
        """slack float64[batch, horizon, contacts, 10] (+inf for swing leg-steps), summary float64[batch, 6] and where int32[batch, 6]
        (-1 = no candidate).  Waits; runs no safe pass."""
        return self._download("margins")

    def set_device_margins(self, slack_ptr: int = 0, summary_ptr: int = 0, where_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later margins (float64[max_batch, horizon, contacts, 10], float64[max_batch, 6],
        int32[max_batch, 6]; 0 / None = the handle's own)."""
        self._set_device("margins", (slack_ptr, summary_ptr, where_ptr), keepalive)

    def margin_penalty(self, floor, out_ptr: int, penalty_in_ptr: int = 0, stream: int = 0) -> None:
        """out[i] = +inf where some summary[i, k] >= floor[k] is false (NaN floor entries are not tested), else penalty_in[i] or 0: a
        ``penalty_ptr`` of ``sweep_select``.  ``out_ptr``, ``penalty_in_ptr``: float64[batch] in HBM (may be the same)."""
        fl = np.ascontiguousarray(floor, dtype=np.float64)
        assert fl.shape == (6,)
        _check(self.L.hmpc_margin_penalty(self.h, fl.ctypes.data, C.c_void_p(int(penalty_in_ptr or 0)), C.c_void_p(int(out_ptr or 0)),
                                          C.c_void_p(stream)), "hmpc_margin_penalty")

    def set_sweep_margin_floor(self, floor=None) -> None:
        """floor[6] for ``tick_sweep_device`` (commands whose margins miss it are masked); None = off, the default."""
        fl = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        assert fl is None or fl.shape == (6,)
        _check(self.L.hmpc_set_sweep_margin_floor(self.h, None if fl is None else fl.ctypes.data), "hmpc_set_sweep_margin_floor")

    def kkt_certificate(self, stream: int = 0) -> None:
        """One launch behind the solve on ``stream``: the gradient of the QP objective at the forces in the force buffer, multipliers >= 0
        on the active limits, the stationarity residual they leave and the per-instance summary (include/hector_mpc.h
        hmpc_kkt_certificate).  Raises when no solve of the current batch has been enqueued."""
        _check(self.L.hmpc_kkt_certificate(self.h, C.c_void_p(stream)), "hmpc_kkt_certificate")

    def download_certificate(self) -> dict:
        """grad float64[batch, horizon, 6 contacts], lambda float64[batch, horizon, contacts, 10], resid float64[batch, horizon, contacts, 6],
        summary float64[batch, 4] and where int32[batch, 2] (-1 = no candidate).  Waits; runs no safe pass."""
        return self._download("certificate")

    def set_device_certificate(self, grad_ptr: int = 0, lambda_ptr: int = 0, resid_ptr: int = 0, summary_ptr: int = 0, where_ptr: int = 0,
                               keepalive=None) -> None:
        """Caller-owned device buffers for later certificates (shapes of ``download_certificate`` with max_batch rows; 0 / None = the
        handle's own)."""
        self._set_device("certificate", (grad_ptr, lambda_ptr, resid_ptr, summary_ptr, where_ptr), keepalive)

    def set_certificate_tolerance(self, act_tol: float) -> None:
        """A slack <= ``act_tol`` makes its limit active for the multipliers (default 1e-3; 0 < act_tol < 0.005)."""
        _check(self.L.hmpc_set_certificate_tolerance(self.h, float(act_tol)), "hmpc_set_certificate_tolerance")

    def certificate_penalty(self, ceil, out_ptr: int, penalty_in_ptr: int = 0, stream: int = 0) -> None:
        """out[i] = +inf where some summary[i, k] <= ceil[k] (k < 3) is false (NaN ceil entries are not tested), else penalty_in[i] or 0: a
        ``penalty_ptr`` of ``sweep_select``.  ``out_ptr``, ``penalty_in_ptr``: float64[batch] in HBM (may be the same)."""
        cl = np.ascontiguousarray(ceil, dtype=np.float64)
        assert cl.shape == (3,)
        _check(self.L.hmpc_certificate_penalty(self.h, cl.ctypes.data, C.c_void_p(int(penalty_in_ptr or 0)), C.c_void_p(int(out_ptr or 0)),
                                               C.c_void_p(stream)), "hmpc_certificate_penalty")

    def set_sweep_certificate_ceiling(self, ceil=None) -> None:
        """ceil[3] for ``tick_sweep_device`` (commands whose certificate exceeds it are masked); None = off, the default."""
        cl = None if ceil is None else np.ascontiguousarray(ceil, dtype=np.float64)
        assert cl is None or cl.shape == (3,)
        _check(self.L.hmpc_set_sweep_certificate_ceiling(self.h, None if cl is None else cl.ctypes.data), "hmpc_set_sweep_certificate_ceiling")

    def feedback_gains(self, stream: int = 0) -> None:
        """One launch behind the solve on ``stream``: K_0 = du_0/dx_0 and du_0/dX_d of the QP that was solved, its linearisation and the
        active set at the forces in the force buffer frozen (include/hector_mpc.h hmpc_feedback_gains).  Raises when no solve of the
        current batch has been enqueued."""
        _check(self.L.hmpc_feedback_gains(self.h, C.c_void_p(stream)), "hmpc_feedback_gains")

    def download_gains(self) -> dict:
        """gain float64[batch, 6 contacts, 13], ref_gain float64[batch, horizon, 6 contacts, 12], summary float64[batch, 2] (smallest
        Cholesky pivot ratio, max |gain|) and free_dims int32[batch, horizon].  Waits; runs no safe pass."""
        return self._download("gains")

    def set_device_gains(self, gain_ptr: int = 0, ref_gain_ptr: int = 0, summary_ptr: int = 0, free_dims_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later gains (shapes of ``download_gains`` with max_batch rows; 0 / None = the handle's own)."""
        self._set_device("gains", (gain_ptr, ref_gain_ptr, summary_ptr, free_dims_ptr), keepalive)

    def first_order_wrench(self, records_ptr: int, stream: int = 0) -> None:
        """One launch: the step-0 wrench of every instance moved to first order to the records at ``records_ptr`` (``batch`` records of
        this handle's stride in HBM: the same robots a moment later), by the gains of the last solve (include/hector_mpc.h
        hmpc_first_order_wrench).  Raises without gains of the last solve."""
        _check(self.L.hmpc_first_order_wrench(self.h, C.c_void_p(int(records_ptr or 0)), C.c_void_p(stream)), "hmpc_first_order_wrench")

    def download_first_order(self) -> dict:
        """wrench float32[batch, 6 contacts] and worst_slack float64[batch] (the least step-0 slack at that wrench; +inf with no stance
        contact).  Waits."""
        return self._download("first_order")

    def set_device_first_order(self, wrench_ptr: int = 0, worst_slack_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later first-order wrenches (float32[max_batch, 6 contacts], float64[max_batch]; 0 / None = the
        handle's own)."""
        self._set_device("first_order", (wrench_ptr, worst_slack_ptr), keepalive)

    ADJOINT_KEYS = _result_keys("adjoint")

    def solve_adjoint(self, seed_ptr: int, stream: int = 0) -> None:
        """One launch behind the solve on ``stream``: from the seed dL/du (float64[batch, horizon, 6 contacts] in HBM) the gradients of L
        in the state, the reference trajectory, the weights and Alpha_K, the active set at the forces in the force buffer frozen
        (include/hector_mpc.h hmpc_solve_adjoint).  Raises for a null seed and when no solve of the current batch has been enqueued."""
        _check(self.L.hmpc_solve_adjoint(self.h, C.c_void_p(int(seed_ptr or 0)), C.c_void_p(stream)), "hmpc_solve_adjoint")

    def download_adjoint(self) -> dict:
        """grad_x0 float64[batch, 13], grad_traj float64[batch, horizon, 12], grad_weights float64[batch, 12], grad_alpha
        float64[batch, 6 contacts], dir float64[batch, horizon, 6 contacts] and summary float64[batch, 2] (smallest Cholesky pivot ratio,
        max |dir|).  Waits; runs no safe pass."""
        return self._download("adjoint")

    def get_device_adjoint(self) -> dict:
        """Device pointers of where the next adjoint goes, by the names of ``download_adjoint`` (the handle's own buffers are allocated
        here if they were not yet)."""
        return self._get_device("adjoint")

    def set_device_adjoint(self, grad_x0_ptr: int = 0, grad_traj_ptr: int = 0, grad_weights_ptr: int = 0, grad_alpha_ptr: int = 0,
                           dir_ptr: int = 0, summary_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later adjoints (shapes of ``download_adjoint`` with max_batch rows; 0 / None = the handle's own)."""
        self._set_device("adjoint", (grad_x0_ptr, grad_traj_ptr, grad_weights_ptr, grad_alpha_ptr, dir_ptr, summary_ptr), keepalive)

    def solve_adjoint_multi(self, seeds_ptr: int, n_seeds: int, stream: int = 0) -> None:
        """``solve_adjoint`` under ``n_seeds`` seeds (float64[n_seeds, batch, horizon, 6 contacts] in HBM) behind ONE matrix backward pass:
        one launch per 6 contacts seeds on ``stream`` (include/hector_mpc.h hmpc_solve_adjoint_multi).  Slice s of every output is bit for
        bit what ``solve_adjoint`` returns under seed s.  Raises for null seeds, a seed count outside 1 .. 240 and when no solve of the
        current batch has been enqueued."""
        _check(self.L.hmpc_solve_adjoint_multi(self.h, C.c_void_p(int(seeds_ptr or 0)), int(n_seeds), C.c_void_p(stream)),
               "hmpc_solve_adjoint_multi")

    def download_adjoint_multi(self) -> dict:
        """The arrays of ``download_adjoint`` with a leading axis over the seeds of the last ``solve_adjoint_multi``.  Waits; runs no safe
        pass."""
        return self._download("adjoint_multi", lead=(self._get_device("adjoint_multi", count=True)["n_seeds"], self.batch))

    def get_device_adjoint_multi(self) -> dict:
        """Device pointers of slice 0 of where the multi-seed adjoint is or goes next, by the names of ``download_adjoint`` (0: one of the
        handle's own that no launch has reserved yet), and ``n_seeds``: the seeds of the one that stands (0: none)."""
        return self._get_device("adjoint_multi", count=True)

    def set_device_adjoint_multi(self, n_seeds: int = 0, grad_x0_ptr: int = 0, grad_traj_ptr: int = 0, grad_weights_ptr: int = 0,
                                 grad_alpha_ptr: int = 0, dir_ptr: int = 0, summary_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later multi-seed adjoints, with room for ``n_seeds`` slices of the current batch (0 / None = the
        handle's own)."""
        self._set_device("adjoint_multi", (grad_x0_ptr, grad_traj_ptr, grad_weights_ptr, grad_alpha_ptr, dir_ptr, summary_ptr), keepalive, n_seeds)

    def select_adjoint_seed(self, s: int) -> None:
        """Makes slice ``s`` of the last ``solve_adjoint_multi`` the current adjoint: ``adjoint_model``, ``adjoint_limits`` (hand it the
        seed's own slice), ``adjoint_record`` and ``download_adjoint`` then behave as after ``solve_adjoint`` under that seed.  No launch, no
        copy.  Raises when ``s`` is out of range or no multi-seed adjoint of the last solve of the current batch stands."""
        _check(self.L.hmpc_select_adjoint_seed(self.h, int(s)), "hmpc_select_adjoint_seed")

    MODEL_ADJOINT_KEYS = _result_keys("adjoint_model")

    def adjoint_model(self, stream: int = 0) -> None:
        """One launch behind ``solve_adjoint`` on ``stream``: from the ``dir`` that adjoint left, the gradients of the same loss in Acd,
        Bcd, the foot positions, the mass and the body inertia (include/hector_mpc.h hmpc_adjoint_model).  Raises when no adjoint of
        the last solve of the current batch has been enqueued."""
        _check(self.L.hmpc_adjoint_model(self.h, C.c_void_p(stream)), "hmpc_adjoint_model")

    def download_adjoint_model(self) -> dict:
        """grad_A float64[batch, 13, 13], grad_B float64[batch, 13, 6 contacts], grad_r float64[batch, 3, contacts] (the record's order:
        axis, then contact), grad_params float64[batch, 4] (mass, inertia 0 .. 2) and costate float64[batch, 2, 13].  Waits; runs no safe
        pass."""
        return self._download("adjoint_model")

    def get_device_adjoint_model(self) -> dict:
        """Device pointers of where the next model gradients go, by the names of ``download_adjoint_model`` (the handle's own buffers are
        allocated here if they were not yet)."""
        return self._get_device("adjoint_model")

    def set_device_adjoint_model(self, grad_A_ptr: int = 0, grad_B_ptr: int = 0, grad_r_ptr: int = 0, grad_params_ptr: int = 0,
                                 costate_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later model gradients (shapes of ``download_adjoint_model`` with max_batch rows; 0 / None = the
        handle's own)."""
        self._set_device("adjoint_model", (grad_A_ptr, grad_B_ptr, grad_r_ptr, grad_params_ptr, costate_ptr), keepalive)

    LIMIT_ADJOINT_KEYS = _result_keys("adjoint_limits")

    def adjoint_limits(self, seed_ptr: int, stream: int = 0) -> None:
        """One launch behind ``solve_adjoint`` on ``stream``: from the ``dir`` that adjoint left and the seed it was given (``seed_ptr``
        again: float64[batch, horizon, 6 contacts] in HBM), the gradients of the same loss in the constraint block, the bounds, mu, lt, lh
        and the Fz caps (include/hector_mpc.h hmpc_adjoint_limits).  Raises when no adjoint of the last solve of the current batch has
        been enqueued."""
        _check(self.L.hmpc_adjoint_limits(self.h, C.c_void_p(int(seed_ptr or 0)), C.c_void_p(stream)), "hmpc_adjoint_limits")

    def download_adjoint_limits(self) -> dict:
        """grad_limits float64[batch, 3 + contacts] (mu, lt, lh, the Fz cap of every contact), grad_Fc float64[batch, 8 contacts,
        6 contacts], grad_bound / lambda / nu float64[batch, horizon, contacts, 10] and summary float64[batch, 3].  Waits; runs no safe
        pass."""
        return self._download("adjoint_limits")

    def get_device_adjoint_limits(self) -> dict:
        """Device pointers of where the next limit gradients go, by the names of ``download_adjoint_limits`` (the handle's own buffers are
        allocated here if they were not yet)."""
        return self._get_device("adjoint_limits")

    def set_device_adjoint_limits(self, grad_limits_ptr: int = 0, grad_Fc_ptr: int = 0, grad_bound_ptr: int = 0, lambda_ptr: int = 0,
                                  nu_ptr: int = 0, summary_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later limit gradients (shapes of ``download_adjoint_limits`` with max_batch rows; 0 / None = the
        handle's own)."""
        self._set_device("adjoint_limits", (grad_limits_ptr, grad_Fc_ptr, grad_bound_ptr, lambda_ptr, nu_ptr, summary_ptr), keepalive)

    RECORD_ADJOINT_KEYS = _result_keys("adjoint_record")

    def adjoint_record(self, stream: int = 0) -> None:
        """One launch behind ``solve_adjoint``, ``adjoint_model`` and ``adjoint_limits`` on ``stream``: their outputs chained through the
        assembly, the gradient of the same loss in every float of the packed record (include/hector_mpc.h hmpc_adjoint_record).  Raises
        unless all three have been enqueued behind the last adjoint of the last solve of the current batch."""
        _check(self.L.hmpc_adjoint_record(self.h, C.c_void_p(stream)), "hmpc_adjoint_record")

    def download_adjoint_record(self) -> dict:
        """grad_record float64[batch, fixed floats + 12 horizon] in the float order of the packed record (``records.OFF`` / ``OFF3``),
        grad_frames float64[batch, 1 + contacts, 3, 3] (the body rotation, then every contact frame) and grad_rpy float64[batch, 3].
        Waits; runs no safe pass."""
        return self._download("adjoint_record")

    def get_device_adjoint_record(self) -> dict:
        """Device pointers of where the next record gradients go, by the names of ``download_adjoint_record`` (the handle's own buffers
        are allocated here if they were not yet)."""
        return self._get_device("adjoint_record")

    def set_device_adjoint_record(self, grad_record_ptr: int = 0, grad_frames_ptr: int = 0, grad_rpy_ptr: int = 0, keepalive=None) -> None:
        """Caller-owned device buffers for later record gradients (shapes of ``download_adjoint_record`` with max_batch rows; 0 / None =
        the handle's own)."""
        self._set_device("adjoint_record", (grad_record_ptr, grad_frames_ptr, grad_rpy_ptr), keepalive)

    CHAIN_KEYS = _result_keys("adjoint_chain_multi")

    def _chain_shapes(self, n_seeds: int) -> dict:
        return self.result_shapes("adjoint_chain_multi", (n_seeds, self.batch))

    def adjoint_chain_multi(self, seeds_ptr: int, stream: int = 0) -> None:
        """Behind ``solve_adjoint_multi``: for every seed of it the chain ``adjoint_model`` -> ``adjoint_limits`` -> ``adjoint_record``,
        one launch per 6 contacts seeds on ``stream`` behind ONE assembly, forward chain and active set (include/hector_mpc.h
        hmpc_adjoint_chain_multi).  ``seeds_ptr``: the seeds that adjoint was given, again.  Slice s of every output is bit for bit what the
        three calls leave behind ``select_adjoint_seed(s)``; neither a selection nor the single-seed results are touched.  Raises for null
        seeds and when no multi-seed adjoint of the last solve of the current batch stands."""
        _check(self.L.hmpc_adjoint_chain_multi(self.h, C.c_void_p(int(seeds_ptr or 0)), C.c_void_p(stream)), "hmpc_adjoint_chain_multi")

    def get_device_adjoint_chain_multi(self) -> dict:
        """Device pointers of slice 0 of where the chain is or goes next, by ``CHAIN_KEYS`` (0: a compact array of the handle's own that
        no launch has reserved yet, or a detail array not given), and ``n_seeds``: the seeds of the chain that stands (0: none)."""
        n, b = C.c_int(0), _lib.AdjointChain()
        _check(self.L.hmpc_get_device_adjoint_chain_multi(self.h, C.byref(n), C.byref(b)), "hmpc_get_device_adjoint_chain_multi")
        return dict({k: int(getattr(b, k) or 0) for k in self.CHAIN_KEYS}, n_seeds=n.value)

    def download_adjoint_chain_multi(self, detail: bool = False) -> dict:
        """The compact arrays of the last ``adjoint_chain_multi`` -- grad_record, grad_frames, grad_rpy (``download_adjoint_record``'s),
        grad_params (``download_adjoint_model``'s), grad_limits and limit_summary (``download_adjoint_limits``') -- with a leading axis
        over the seeds; with ``detail`` the eight detail arrays as well (raises unless buffers were given for all of them).  Waits; runs
        no safe pass."""
        n = C.c_int(0)
        _check(self.L.hmpc_get_device_adjoint_chain_multi(self.h, C.byref(n), None), "hmpc_get_device_adjoint_chain_multi")
        return self._download("adjoint_chain_multi", lead=(n.value, self.batch), only=self.CHAIN_KEYS if detail else _lib.CHAIN_COMPACT)

    def set_device_adjoint_chain_multi(self, n_seeds: int = 0, keepalive=None, **ptrs) -> None:
        """Caller-owned device buffers for later chains, with room for ``n_seeds`` slices of the current batch, by ``CHAIN_KEYS`` with
        ``_ptr`` appended (``grad_record_ptr=...``, ``lambda_ptr=...``).  A compact array left out or 0 is the handle's own; a detail
        array left out or 0 is not written."""
        names = {k + "_ptr": k for k in self.CHAIN_KEYS}
        unknown = [k for k in ptrs if k not in names]
        if unknown:
            raise TypeError(f"set_device_adjoint_chain_multi: unknown buffers {unknown}")
        self._keepalive["adjoint_chain_multi"] = keepalive
        b = _lib.AdjointChain(**{names[k]: int(v or 0) or None for k, v in ptrs.items()})
        _check(self.L.hmpc_set_device_adjoint_chain_multi(self.h, int(n_seeds), C.byref(b)), "hmpc_set_device_adjoint_chain_multi")

    def debug_handover_slots(self) -> np.ndarray:
        """Test hook (hmpc_debug_handover_slots): the hand-over slot table of the current batch, int32[batch]; entry i == i where
        the last solve handed instance i's working set over and nothing has consumed it yet, else -1."""
        out = np.full(self.batch, -2, dtype=np.int32)
        _check(self.L.hmpc_debug_handover_slots(self.h, out.ctypes.data), "hmpc_debug_handover_slots")
        return out

    # one block of hmpc_debug_front_scalars (include/hector_mpc.h; csrc/hmpc_front.h struct FrontScalars), 320 bytes
    FRONT_DTYPE = np.dtype([("rpy", "<f4", 3), ("dt_Rbi", "<f4", 9), ("dt_Iinv", "<f4", 9), ("dt_blk", "<f4", (2, 9)), ("foot", "<f4", (2, 12)),
                            ("pad0", "<f4"), ("pre_nl", "u1", 20), ("pre_nv", "u1", 20), ("pre_st", "u1", 20), ("n", "<u2"), ("nls", "<u2")])

    def debug_set_front_prologue(self, on: bool) -> None:
        """A/B switch (hmpc_debug_set_front_prologue, default on): the batched launch of the assembly's scalar front ahead of the fast pass."""
        _check(self.L.hmpc_debug_set_front_prologue(self.h, int(bool(on))), "hmpc_debug_set_front_prologue")

    def debug_front_scalars(self) -> np.ndarray:
        """Test hook (hmpc_debug_front_scalars): that launch's blocks of the current two-contact batch, a structured array [batch]."""
        out = np.zeros(self.batch, dtype=self.FRONT_DTYPE)
        _check(self.L.hmpc_debug_front_scalars(self.h, out.ctypes.data), "hmpc_debug_front_scalars")
        return out

    def solve_external_qp(self, H: np.ndarray, g: np.ndarray, Fc: np.ndarray) -> None:
        """Parity hook (hmpc_debug_solve_external_qp): solver stages on caller-supplied QP data; H [batch, ld, ld] and
        g [batch, ld] in the reference's reduced order, Fc [batch, 8 nc, 6 nc]."""
        H = np.ascontiguousarray(H, dtype=np.float32)
        g = np.ascontiguousarray(g, dtype=np.float32)
        Fc = np.ascontiguousarray(Fc, dtype=np.float32)
        if not (H.ndim == 3 and H.shape[0] == self.batch and H.shape[1] == H.shape[2] == g.shape[1] and g.shape[0] == self.batch):
            raise ValueError(f"H {H.shape} / g {g.shape}: expected [batch={self.batch}, ld, ld] and [batch, ld]")
        if Fc.shape != (self.batch, 8 * self.contacts, 6 * self.contacts):
            raise ValueError(f"Fc {Fc.shape}: expected {(self.batch, 8 * self.contacts, 6 * self.contacts)}")
        _check(self.L.hmpc_debug_solve_external_qp(self.h, H.ctypes.data, g.ctypes.data, Fc.ctypes.data, H.shape[1]),
               "hmpc_debug_solve_external_qp")

    # ---- rows either side of the solve
    def build_records(self, ticks: np.ndarray, dt_mpc: float):
        """f1+f2 on the device: ticks = structured array with dtype ``TICK_DTYPE``; returns the clamped
        world_position_desired [batch, 2].  The built records become the current batch."""
        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        wpd = np.zeros((ticks.shape[0], 2), dtype=np.float64)
        _check(self.L.hmpc_build_records(self.h, ticks.ctypes.data, ticks.shape[0], float(dt_mpc), wpd.ctypes.data),
               "hmpc_build_records")
        return wpd

    def download_records(self) -> np.ndarray:
        rec = np.zeros((self.batch, self.stride), dtype=np.uint8)
        _check(self.L.hmpc_download_records(self.h, rec.ctypes.data), "hmpc_download_records")
        return rec

    def body_wrench(self, rBody: np.ndarray) -> np.ndarray:
        """f3: f_ff[batch, 2, 6] = -rBody [GRF; GRM] from the last solve's forces."""
        rb = np.ascontiguousarray(rBody, dtype=np.float64).reshape(self.batch, 9)
        out = np.zeros((self.batch, 2, 6), dtype=np.float64)
        _check(self.L.hmpc_body_wrench(self.h, rb.ctypes.data, out.ctypes.data), "hmpc_body_wrench")
        return out

    def leg_torques(self, rBody: np.ndarray, leg_q: np.ndarray):
        """f3 with torques: returns (f_ff[batch,2,6], tau[batch,2,5]) from the last solve's forces."""
        rb = np.ascontiguousarray(rBody, dtype=np.float64).reshape(self.batch, 9)
        lq = np.ascontiguousarray(leg_q, dtype=np.float64).reshape(self.batch, 10)
        fff = np.zeros((self.batch, 2, 6), dtype=np.float64)
        tau = np.zeros((self.batch, 2, 5), dtype=np.float64)
        _check(self.L.hmpc_leg_torques(self.h, rb.ctypes.data, lq.ctypes.data, fff.ctypes.data, tau.ctypes.data),
               "hmpc_leg_torques")
        return fff, tau

    # ---- closed loop on the device (include/hector_mpc.h hmpc_plant_step_device / hmpc_rollout_device)
    def _stage_plant(self, plant, batch: int, instance_mass, ext_wrench):
        """A copy of ``plant`` (default: ``default_plant()``) whose per-instance arrays, given as numpy, live in HBM; + what keeps them alive."""
        import torch

        p = _lib.Plant.from_buffer_copy(plant if plant is not None else default_plant())
        keep = []
        for name, arr, shape in (("device_mass", instance_mass, (batch,)), ("device_ext_wrench", ext_wrench, (batch, 6))):
            if arr is not None:
                t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64).reshape(shape).copy()).cuda(self.device)
                keep.append(t)
                setattr(p, name, t.data_ptr())
        return p, keep

    def plant_step(self, ticks, plant=None, forces=None, status=None, wpd=None, summary=None, device: bool = False, batch: int = 0,
                   force_stride: int = 12, stream: int = 0, instance_mass=None, ext_wrench=None):
        """One plant step: the ticks advanced by one MPC tick under the step-0 forces (include/hector_mpc.h hmpc_plant_step_device).
        ``device=False``: ``ticks`` is a ``TICK_DTYPE`` array, ``forces`` float32[batch, >= 12], ``status`` uint32[batch], ``wpd``
        float64[batch, 2], ``summary`` int32[batch, 4] (``None``: the handle's force / status buffers, the tick's own
        world_position_desired, rows {0, -1, 0, 0}), ``instance_mass`` / ``ext_wrench`` numpy arrays for the plant's per-instance
        pointers; everything is staged through HBM and the call waits: returns (new ticks, new summary).  ``device=True``: ``ticks``,
        ``forces``, ``status``, ``wpd``, ``summary`` are device pointers (0 / None as in C), ``batch`` and ``force_stride`` as in C; the
        launch is enqueued on ``stream`` and nothing is returned."""
        if device:
            p = plant if plant is not None else default_plant()
            _check(self.L.hmpc_plant_step_device(self.h, C.c_void_p(int(ticks)), int(batch), C.byref(p), C.c_void_p(int(forces or 0)),
                                                 int(force_stride), C.c_void_p(int(status or 0)), C.c_void_p(int(wpd or 0)),
                                                 C.c_void_p(int(summary or 0)), C.c_void_p(stream)), "hmpc_plant_step_device")
            return None
        import torch

        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        nb = ticks.shape[0]
        p, keep = self._stage_plant(plant, nb, instance_mass, ext_wrench)
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt).copy()).cuda(self.device)
        d_t = torch.from_numpy(ticks.view(np.uint8).reshape(nb, -1).copy()).cuda(self.device)
        d_f, d_w = dev(forces, np.float32), dev(wpd, np.float64)
        d_s = None if status is None else dev(np.ascontiguousarray(status, dtype=np.uint32).view(np.int32), np.int32)
        if summary is None:
            summary = np.tile(np.array([0, -1, 0, 0], dtype=np.int32), (nb, 1))
        d_sum = dev(summary, np.int32)
        stride = 12 if d_f is None else int(np.asarray(forces).reshape(nb, -1).shape[1])
        ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        torch.cuda.synchronize(self.device)
        _check(self.L.hmpc_plant_step_device(self.h, ptr(d_t), nb, C.byref(p), ptr(d_f), stride, ptr(d_s), ptr(d_w), ptr(d_sum),
                                             C.c_void_p(stream)), "hmpc_plant_step_device")
        torch.cuda.synchronize(self.device)
        del keep
        return d_t.cpu().numpy().reshape(-1).view(TICK_DTYPE).copy(), d_sum.cpu().numpy()

    def download_rollout(self, batch: int, n_ticks: int) -> dict:
        """The log of the last rollout (waits): state float64[batch, n_ticks, 12] (rpy, position, omegaWorld, vWorld after each tick),
        wrench float32[batch, n_ticks, 12], status uint32[batch, n_ticks], tau float64[batch, n_ticks, 10], summary int32[batch, 4]."""
        out = dict(state=np.zeros((batch, n_ticks, 12), dtype=np.float64), wrench=np.zeros((batch, n_ticks, 12), dtype=np.float32),
                   status=np.zeros((batch, n_ticks), dtype=np.uint32), tau=np.zeros((batch, n_ticks, 10), dtype=np.float64),
                   summary=np.zeros((batch, 4), dtype=np.int32))
        _check(self.L.hmpc_download_rollout(self.h, *[out[k].ctypes.data for k in _lib.ROLLOUT_LOG]), "hmpc_download_rollout")
        return out

    # ---- swing legs on the device (include/hector_mpc.h hmpc_swing_legs_device / hmpc_tick_command_device)
    def _to_device(self, a: np.ndarray):
        import torch

        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(self.device)

    def swing_state(self, batch: int, device_ptr: int = 0, stream: int = 0):
        """The reference's initial swing state of ``batch`` instances (all zero, ``first_swing = {1, 1}``): a ``SWING_STATE_DTYPE`` array, or
        with ``device_ptr`` written to that HBM buffer on ``stream`` (hmpc_swing_state_init_device; nothing is returned)."""
        if device_ptr:
            _check(self.L.hmpc_swing_state_init_device(self.h, C.c_void_p(int(device_ptr)), int(batch), C.c_void_p(stream)),
                   "hmpc_swing_state_init_device")
            return None
        return initial_swing_state(batch)

    def swing_legs(self, ticks, state, cfg=None, tau=None, detail=False, device: bool = False, batch: int = 0, cmd=0, stream: int = 0):
        """One swing update per instance (include/hector_mpc.h hmpc_swing_legs_device): ``cfg.updates`` updates of the swing state, then
        the complete motor command.  ``cfg``: a ``default_swing()`` (``None``: the defaults).  ``device=False``: ``ticks`` is a ``TICK_DTYPE``
        array, ``state`` a ``SWING_STATE_DTYPE`` array (``swing_state(batch)`` at the start), ``tau`` float64[batch, 10] or ``None`` (zeros),
        ``detail`` a bool; everything is staged through HBM and the call waits: returns ``dict(cmd=MOTOR_CMD_DTYPE[batch], state=the new
        state)`` plus ``detail`` float64[batch, 2, 16] when asked for (``SWING_DETAIL`` names its columns).  ``device=True``: ``ticks``,
        ``state``, ``tau``, ``cmd``, ``detail`` are device pointers (0 / None as in C), ``batch`` as in C; the launch is only enqueued."""
        c = cfg if cfg is not None else default_swing()
        if device:
            _check(self.L.hmpc_swing_legs_device(self.h, C.c_void_p(int(ticks or 0)), int(batch), C.byref(c), C.c_void_p(int(state or 0)),
                                                 C.c_void_p(int(tau or 0)), C.c_void_p(int(cmd or 0)), C.c_void_p(int(detail or 0)),
                                                 C.c_void_p(stream)), "hmpc_swing_legs_device")
            return None
        import torch

        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        nb = ticks.shape[0]
        d_t, d_s = self._to_device(ticks), self._to_device(np.ascontiguousarray(state, dtype=SWING_STATE_DTYPE).reshape(nb))
        d_tau = None if tau is None else self._to_device(np.ascontiguousarray(tau, dtype=np.float64).reshape(nb, 10))
        d_c = torch.zeros(nb * MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device=d_t.device)
        d_d = torch.zeros((nb, 2, 16), dtype=torch.float64, device=d_t.device) if detail else None
        ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        torch.cuda.synchronize(self.device)
        _check(self.L.hmpc_swing_legs_device(self.h, ptr(d_t), nb, C.byref(c), ptr(d_s), ptr(d_tau), ptr(d_c), ptr(d_d), C.c_void_p(stream)),
               "hmpc_swing_legs_device")
        torch.cuda.synchronize(self.device)
        out = dict(cmd=d_c.cpu().numpy().view(MOTOR_CMD_DTYPE).copy(), state=d_s.cpu().numpy().view(SWING_STATE_DTYPE).copy())
        if detail:
            out["detail"] = d_d.cpu().numpy()
        return out

    def tick_command(self, ticks, state, cfg=None, device: bool = False, batch: int = 0, cmd=0, wpd=0, f_ff=0, dt_mpc: float | None = None,
                     stream: int = 0):
        """Ticks in, complete motor commands out (include/hector_mpc.h hmpc_tick_command_device): what ``tick_solve_device`` enqueues, then
        the swing update reading that tick's torques.  ``device=False``: ``ticks`` a ``TICK_DTYPE`` array, ``state`` a ``SWING_STATE_DTYPE``
        array; the call waits and returns ``dict(cmd, state, f_ff float64[batch, 2, 6], wpd float64[batch, 2], forces, status)``.
        ``device=True``: ``ticks``, ``state``, ``cmd``, ``wpd``, ``f_ff`` are device pointers, ``batch`` as in C; only enqueued."""
        self.generation += 1
        c = cfg if cfg is not None else default_swing()
        dt = self.dt_mpc if dt_mpc is None else float(dt_mpc)
        if device:
            _check(self.L.hmpc_tick_command_device(self.h, C.c_void_p(int(ticks or 0)), int(batch), dt, C.byref(c), C.c_void_p(int(state or 0)),
                                                   C.c_void_p(int(wpd or 0)), C.c_void_p(int(f_ff or 0)), C.c_void_p(int(cmd or 0)),
                                                   C.c_void_p(stream)), "hmpc_tick_command_device")
            return None
        import torch

        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        nb = ticks.shape[0]
        d_t, d_s = self._to_device(ticks), self._to_device(np.ascontiguousarray(state, dtype=SWING_STATE_DTYPE).reshape(nb))
        d_c = torch.zeros(nb * MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device=d_t.device)
        d_w = torch.zeros((nb, 2), dtype=torch.float64, device=d_t.device)
        d_f = torch.zeros((nb, 2, 6), dtype=torch.float64, device=d_t.device)
        torch.cuda.synchronize(self.device)
        _check(self.L.hmpc_tick_command_device(self.h, C.c_void_p(d_t.data_ptr()), nb, dt, C.byref(c), C.c_void_p(d_s.data_ptr()),
                                               C.c_void_p(d_w.data_ptr()), C.c_void_p(d_f.data_ptr()), C.c_void_p(d_c.data_ptr()),
                                               C.c_void_p(stream)), "hmpc_tick_command_device")
        forces, status = self.download()  # (waits for the stream)
        torch.cuda.synchronize(self.device)
        return dict(cmd=d_c.cpu().numpy().view(MOTOR_CMD_DTYPE).copy(), state=d_s.cpu().numpy().view(SWING_STATE_DTYPE).copy(),
                    f_ff=d_f.cpu().numpy(), wpd=d_w.cpu().numpy(), forces=forces, status=status)

    def set_rollout_swing(self, cfg=None, state_ptr: int = 0, cmd_log_ptr: int = 0) -> None:
        """While a ``cfg`` is set, every tick of a rollout or rollout sweep enqueues the swing update behind its torques
        (include/hector_mpc.h hmpc_set_rollout_swing): ``state_ptr`` = ``SWING_STATE_DTYPE[batch]`` in HBM, ``cmd_log_ptr`` =
        ``MOTOR_CMD_DTYPE[batch, n_ticks]`` in HBM or 0.  ``cfg=None`` turns it off (the default)."""
        _check(self.L.hmpc_set_rollout_swing(self.h, C.byref(cfg) if cfg is not None else None, C.c_void_p(int(state_ptr or 0)),
                                             C.c_void_p(int(cmd_log_ptr or 0))), "hmpc_set_rollout_swing")

    def _stage_swing(self, swing, batch: int, n_ticks: int):
        """``swing=`` of ``rollout`` / ``rollout_sweep`` in their host form: ``True`` or a ``_lib.Swing`` (a fresh initial state) or a dict
        ``{"cfg": ..., "state": SWING_STATE_DTYPE[batch]}``; switches the setting on over fresh HBM buffers, which it returns."""
        import torch

        if isinstance(swing, dict):
            cfg, state = swing.get("cfg"), swing.get("state")
        else:
            cfg, state = (None if swing is True else swing), None
        cfg = cfg if cfg is not None else default_swing()
        state = initial_swing_state(batch) if state is None else np.ascontiguousarray(state, dtype=SWING_STATE_DTYPE).reshape(batch)
        d_s = self._to_device(state)
        d_c = torch.zeros(batch * n_ticks * MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device=d_s.device)
        self.set_rollout_swing(cfg, d_s.data_ptr(), d_c.data_ptr())
        return d_s, d_c

    def rollout(self, ticks, n_ticks: int, ticks_per_step: int = 8, subtick0: int = 0, plant=None, device: bool = False, batch: int = 0,
                dt_mpc: float | None = None, stream: int = 0, instance_mass=None, ext_wrench=None, swing=None):
        """``n_ticks`` closed-loop ticks on one stream, nothing leaving the device in between: solve, then plant step, per tick
        (include/hector_mpc.h hmpc_rollout_device).  ``device=False``: ``ticks`` is a ``TICK_DTYPE`` array; the call uploads it, waits and
        returns the log of ``download_rollout`` plus ``ticks`` = the tick structs after the last step.  ``device=True``: ``ticks`` is a
        device pointer to ``batch`` tick structs, advanced in place; the rollout is only enqueued (log: the handle's own buffers, read
        with ``download_rollout``).  ``swing`` (default ``None``: the rollout as it is without it) adds the swing update to every tick
        (``set_rollout_swing``, for this call only): host form ``True``, a ``default_swing()`` or ``{"cfg": ..., "state": ...}`` -- the
        result gains ``cmd`` = ``MOTOR_CMD_DTYPE[batch, n_ticks]`` and ``swing_state``; device form ``{"cfg": ..., "state": pointer,
        "cmd_log": pointer or 0}``."""
        self.generation += 1
        dt = self.dt_mpc if dt_mpc is None else float(dt_mpc)
        if device:
            p = plant if plant is not None else default_plant()
            if swing is not None:
                self.set_rollout_swing(swing.get("cfg") or default_swing(), swing["state"], swing.get("cmd_log", 0))
            try:
                _check(self.L.hmpc_rollout_device(self.h, C.c_void_p(int(ticks)), int(batch), int(n_ticks), dt, int(ticks_per_step),
                                                  int(subtick0), C.byref(p), None, C.c_void_p(stream)), "hmpc_rollout_device")
            finally:
                if swing is not None:
                    self.set_rollout_swing(None)
            return None
        import torch

        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        nb = ticks.shape[0]
        p, keep = self._stage_plant(plant, nb, instance_mass, ext_wrench)
        d_t = torch.from_numpy(ticks.view(np.uint8).reshape(nb, -1).copy()).cuda(self.device)
        sw = self._stage_swing(swing, nb, int(n_ticks)) if swing is not None else None
        torch.cuda.synchronize(self.device)
        try:
            _check(self.L.hmpc_rollout_device(self.h, C.c_void_p(d_t.data_ptr()), nb, int(n_ticks), dt, int(ticks_per_step), int(subtick0),
                                              C.byref(p), None, C.c_void_p(stream)), "hmpc_rollout_device")
        finally:
            if sw is not None:
                self.set_rollout_swing(None)
        out = self.download_rollout(nb, int(n_ticks))
        del keep
        out["ticks"] = d_t.cpu().numpy().reshape(-1).view(TICK_DTYPE).copy()
        if sw is not None:
            out["swing_state"] = sw[0].cpu().numpy().view(SWING_STATE_DTYPE).copy()
            out["cmd"] = sw[1].cpu().numpy().view(MOTOR_CMD_DTYPE).reshape(nb, int(n_ticks)).copy()
        return out

    # ---- closed-loop command sweeps (include/hector_mpc.h hmpc_rollout_score_device / _select_device / _sweep_device)
    def _stage_log(self, log: dict, batch: int, n_ticks: int):
        """``struct hmpc_rollout_log`` over HBM copies of the host arrays of ``log`` (a missing or ``None`` member stays NULL); + the copies."""
        import torch

        lg, keep = _lib.RolloutLog(), {}
        shapes = dict(state=(np.float64, (batch, n_ticks, 12)), wrench=(np.float32, (batch, n_ticks, 12)), status=(np.int32, (batch, n_ticks)),
                      tau=(np.float64, (batch, n_ticks, 10)), summary=(np.int32, (batch, 4)))
        for k, (dt, shape) in shapes.items():
            a = log.get(k)
            if a is None:
                continue
            if k == "status":
                a = np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)
            keep[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape).copy()).cuda(self.device)
            setattr(lg, k, keep[k].data_ptr())
        return lg, keep

    def rollout_score(self, ticks0, log=None, cost=None, device: bool = False, batch: int = 0, n_ticks: int = 0, cost_ptr: int = 0,
                      score_ptr: int = 0, stream: int = 0):
        """The cost of every instance's rollout log (include/hector_mpc.h hmpc_rollout_score_device).  ``ticks0``: the tick structs AS THEY
        WERE BEFORE the rollout; ``cost``: a ``default_rollout_cost()`` (``None``: the defaults).  ``device=False``: ``ticks0`` is a
        ``TICK_DTYPE`` array and ``log`` a dict of host arrays -- ``state`` float64[batch, n_ticks, 12], and optionally ``wrench``, ``tau``,
        ``summary`` as ``download_rollout`` returns them (a missing member is not scored) -- or ``None`` for the log of the handle's last
        rollout (pass its ``n_ticks``); everything is staged through HBM and the call waits: returns ``dict(cost=float64[batch, 4] (tracking,
        effort, terminal, penalty), score=float64[batch])``.  ``device=True``: ``ticks0``, ``cost_ptr``, ``score_ptr`` are device pointers,
        ``log`` a ``_lib.RolloutLog`` or ``None``, ``batch`` and ``n_ticks`` as in C; the launch is only enqueued."""
        c = cost if cost is not None else default_rollout_cost()
        if device:
            _check(self.L.hmpc_rollout_score_device(self.h, C.c_void_p(int(ticks0)), int(batch), int(n_ticks), C.byref(c),
                                                    C.byref(log) if log is not None else None, C.c_void_p(int(cost_ptr or 0)),
                                                    C.c_void_p(int(score_ptr or 0)), C.c_void_p(stream)), "hmpc_rollout_score_device")
            return None
        import torch

        ticks0 = np.ascontiguousarray(ticks0, dtype=TICK_DTYPE)
        nb = ticks0.shape[0]
        keep = None
        if log is not None:
            n_ticks = int(np.asarray(log["state"]).shape[1])
            lg, keep = self._stage_log(log, nb, n_ticks)
        d_t = torch.from_numpy(ticks0.view(np.uint8).reshape(nb, -1).copy()).cuda(self.device)
        d_c = torch.zeros((nb, 4), dtype=torch.float64, device=d_t.device)
        d_s = torch.zeros((nb,), dtype=torch.float64, device=d_t.device)
        torch.cuda.synchronize(self.device)
        _check(self.L.hmpc_rollout_score_device(self.h, C.c_void_p(d_t.data_ptr()), nb, int(n_ticks), C.byref(c),
                                                C.byref(lg) if log is not None else None, C.c_void_p(d_c.data_ptr()),
                                                C.c_void_p(d_s.data_ptr()), C.c_void_p(stream)), "hmpc_rollout_score_device")
        torch.cuda.synchronize(self.device)
        del keep
        return dict(cost=d_c.cpu().numpy(), score=d_s.cpu().numpy())

    def _choice_buffers(self, groups: int, members):
        """``struct hmpc_rollout_choice`` over fresh HBM buffers for the ``members`` asked for; + the buffers."""
        import torch

        shapes = dict(index=(torch.int32, (groups,)), score=(torch.float64, (groups,)), wrench=(torch.float32, (groups, 12)),
                      tau=(torch.float64, (groups, 10)), summary=(torch.int32, (groups, 4)))
        ch, bufs = _lib.RolloutChoice(), {}
        for k in members:
            bufs[k] = torch.zeros(shapes[k][1], dtype=shapes[k][0], device=f"cuda:{self.device}")
            setattr(ch, k, bufs[k].data_ptr())
        return ch, bufs

    def rollout_select(self, score, group_size: int, penalty=None, log=None, device: bool = False, batch: int = 0, choice=None,
                       stream: int = 0):
        """The cheapest instance of every group of ``group_size`` consecutive instances (include/hector_mpc.h hmpc_rollout_select_device):
        ``score + penalty`` where finite, ties to the lowest index.  ``device=False``: ``score`` float64[batch], ``penalty`` float64[batch] or
        ``None``, ``log`` a dict of host arrays as for ``rollout_score`` -- it must be the log the last ``rollout_score`` scored -- or
        ``None`` for the log of the handle's last rollout; the call waits and returns ``dict(index=int32[groups] (-1: no winner),
        score=float64[groups])`` plus, for every member the log has, the winner's ``wrench`` float32[groups, 12] and ``tau``
        float64[groups, 10] of tick 0 and its ``summary`` int32[groups, 4].  ``device=True``: ``score``, ``penalty`` device pointers, ``log``
        a ``_lib.RolloutLog`` or ``None``, ``choice`` a ``_lib.RolloutChoice`` of device pointers; the launch is only enqueued."""
        if device:
            _check(self.L.hmpc_rollout_select_device(self.h, C.c_void_p(int(score)), C.c_void_p(int(penalty or 0)), int(batch), int(group_size),
                                                     C.byref(log) if log is not None else None, C.byref(choice), C.c_void_p(stream)),
                   "hmpc_rollout_select_device")
            return None
        import torch

        score = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
        nb = score.shape[0]
        if group_size < 1 or nb % group_size:
            raise ValueError("group_size must divide the batch")
        keep, members = None, list(_lib.ROLLOUT_CHOICE)
        if log is not None:
            lg, keep = self._stage_log(log, nb, int(np.asarray(log["state"]).shape[1]))
            members = ["index", "score"] + [k for k in ("wrench", "tau", "summary") if k in keep]
        ch, bufs = self._choice_buffers(nb // group_size, members)
        d_s = torch.from_numpy(score.copy()).cuda(self.device)
        d_p = None if penalty is None else torch.from_numpy(np.ascontiguousarray(penalty, dtype=np.float64).reshape(nb).copy()).cuda(self.device)
        torch.cuda.synchronize(self.device)
        _check(self.L.hmpc_rollout_select_device(self.h, C.c_void_p(d_s.data_ptr()), C.c_void_p(0 if d_p is None else d_p.data_ptr()), nb,
                                                 int(group_size), C.byref(lg) if log is not None else None, C.byref(ch), C.c_void_p(stream)),
               "hmpc_rollout_select_device")
        torch.cuda.synchronize(self.device)
        del keep
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    def _device_bytes(self, ptr: int, nbytes: int) -> np.ndarray:
        """``nbytes`` bytes of HBM at ``ptr`` (a buffer of the handle's) as a host array: torch views the pointer and copies it down."""
        import torch

        class _View:
            __cuda_array_interface__ = dict(shape=(int(nbytes),), typestr="|u1", data=(int(ptr), False), strides=None, version=2)

        return torch.as_tensor(_View(), device=f"cuda:{self.device}").cpu().numpy()

    def get_device_rollout_sweep(self) -> dict:
        """Device pointers of the handle's buffers of the last ``rollout_sweep``: ``ticks`` (the expanded tick structs after the rollout),
        ``cost`` [instances, 4], ``score`` [instances]."""
        p = [C.c_void_p() for _ in range(3)]
        _check(self.L.hmpc_get_device_rollout_sweep(self.h, *[C.byref(x) for x in p]), "hmpc_get_device_rollout_sweep")
        return dict(zip(("ticks", "cost", "score"), [x.value for x in p]))

    def rollout_sweep(self, ticks, commands, n_ticks: int, ticks_per_step: int = 8, subtick0: int = 0, plant=None, cost=None, penalty=None,
                      device: bool = False, n_states: int = 0, group_size: int = 0, choice=None, dt_mpc: float | None = None,
                      stream: int = 0, instance_mass=None, ext_wrench=None, swing=None):
        """Every robot state rolled out in closed loop under each of its candidate commands, scored and the best picked, nothing leaving
        the device in between (include/hector_mpc.h hmpc_rollout_sweep_device).  ``device=False``: ``ticks`` is a ``TICK_DTYPE`` array
        [n_states], ``commands`` a ``COMMAND_DTYPE`` array [n_states, K], ``penalty`` float64[n_states * K] or ``None``, ``instance_mass`` /
        ``ext_wrench`` per EXPANDED instance; the call waits and returns the dict of ``rollout_select`` (``index``, ``score``, ``wrench``,
        ``tau``, ``summary`` per state) plus ``cost`` float64[n_states * K, 4], ``all_scores`` float64[n_states * K], ``ticks`` (the expanded
        tick structs after the rollout), ``log`` (``download_rollout``) and ``ticks_in`` (the robot states read back from the device: the
        sweep does not modify them).  ``device=True``: ``ticks``, ``commands``, ``penalty`` are
        device pointers, ``n_states`` and ``group_size`` as in C, ``choice`` a ``_lib.RolloutChoice``; the chain is only enqueued.
        ``swing``: as for ``rollout``, state and command log per EXPANDED instance (the host form returns ``cmd`` [n_states * K, n_ticks] and
        ``swing_state``)."""
        self.generation += 1
        dt = self.dt_mpc if dt_mpc is None else float(dt_mpc)
        c = cost if cost is not None else default_rollout_cost()
        if device:
            p = plant if plant is not None else default_plant()
            if swing is not None:
                self.set_rollout_swing(swing.get("cfg") or default_swing(), swing["state"], swing.get("cmd_log", 0))
            try:
                _check(self.L.hmpc_rollout_sweep_device(self.h, C.c_void_p(int(ticks)), int(n_states), C.c_void_p(int(commands)), int(group_size),
                                                        int(n_ticks), dt, int(ticks_per_step), int(subtick0), C.byref(p), C.byref(c),
                                                        C.c_void_p(int(penalty or 0)), C.byref(choice), C.c_void_p(stream)),
                       "hmpc_rollout_sweep_device")
            finally:
                if swing is not None:
                    self.set_rollout_swing(None)
            return None
        import torch

        ticks = np.ascontiguousarray(ticks, dtype=TICK_DTYPE)
        ns = ticks.shape[0]
        commands = np.ascontiguousarray(commands, dtype=COMMAND_DTYPE).reshape(ns, -1)
        K = commands.shape[1]
        nb = ns * K
        p, keep = self._stage_plant(plant, nb, instance_mass, ext_wrench)
        d_t = torch.from_numpy(ticks.view(np.uint8).reshape(ns, -1).copy()).cuda(self.device)
        d_c = torch.from_numpy(commands.view(np.uint8).reshape(nb, -1).copy()).cuda(self.device)
        d_p = None if penalty is None else torch.from_numpy(np.ascontiguousarray(penalty, dtype=np.float64).reshape(nb).copy()).cuda(self.device)
        ch, bufs = self._choice_buffers(ns, _lib.ROLLOUT_CHOICE)
        sw = self._stage_swing(swing, nb, int(n_ticks)) if swing is not None else None
        torch.cuda.synchronize(self.device)
        try:
            _check(self.L.hmpc_rollout_sweep_device(self.h, C.c_void_p(d_t.data_ptr()), ns, C.c_void_p(d_c.data_ptr()), K, int(n_ticks), dt,
                                                    int(ticks_per_step), int(subtick0), C.byref(p), C.byref(c),
                                                    C.c_void_p(0 if d_p is None else d_p.data_ptr()), C.byref(ch), C.c_void_p(stream)),
                   "hmpc_rollout_sweep_device")
        finally:
            if sw is not None:
                self.set_rollout_swing(None)
        log = self.download_rollout(nb, int(n_ticks))  # (waits for the stream)
        torch.cuda.synchronize(self.device)
        del keep
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
        own = self.get_device_rollout_sweep()
        out["ticks"] = self._device_bytes(own["ticks"], nb * TICK_DTYPE.itemsize).view(TICK_DTYPE).copy()
        out["cost"] = self._device_bytes(own["cost"], nb * 32).view(np.float64).reshape(nb, 4).copy()
        out["all_scores"] = self._device_bytes(own["score"], nb * 8).view(np.float64).copy()
        out["log"] = log
        out["ticks_in"] = d_t.cpu().numpy().reshape(-1).view(TICK_DTYPE).copy()
        if sw is not None:
            out["swing_state"] = sw[0].cpu().numpy().view(SWING_STATE_DTYPE).copy()
            out["cmd"] = sw[1].cpu().numpy().view(MOTOR_CMD_DTYPE).reshape(nb, int(n_ticks)).copy()
        return out

    def time_solve(self, reps: int, stream: int = 0) -> float:
        ms = C.c_float(0)
        _check(self.L.hmpc_time_solve(self.h, C.c_void_p(stream), int(reps), C.byref(ms)), "hmpc_time_solve")
        return float(ms.value)

    def debug_assemble(self, index: int) -> dict:
        """Assembly stage only (same device code the solve kernel runs) -> the reduced QP as the solver sees it."""
        h, nc = self.horizon, self.contacts
        nmax = 180 if nc == 3 else 240  # HMPC_MAX_VARS_3C / HMPC_MAX_VARS_WIDE
        n, m = C.c_int(0), C.c_int(0)
        var_ind = np.zeros(nmax, dtype=np.int32)
        H = np.zeros(nmax * nmax, dtype=np.float32)
        g = np.zeros(nmax, dtype=np.float32)
        Fc = np.zeros(48 * nc * nc, dtype=np.float32)
        lb = np.zeros(8 * nc * h, dtype=np.float32)
        ub = np.zeros(8 * nc * h, dtype=np.float32)
        x0 = np.zeros(13, dtype=np.float32)
        Acd = np.zeros(169, dtype=np.float32)
        Bcd = np.zeros(78 * nc, dtype=np.float32)
        _check(self.L.hmpc_debug_assemble(self.h, int(index), C.byref(n), C.byref(m), var_ind.ctypes.data,
                                          H.ctypes.data, g.ctypes.data, Fc.ctypes.data, lb.ctypes.data,
                                          ub.ctypes.data, x0.ctypes.data, Acd.ctypes.data, Bcd.ctypes.data),
               "hmpc_debug_assemble")
        nn = n.value
        if nn > nmax:
            return dict(n=nn, m=m.value)
        return dict(n=nn, m=m.value, var_ind=var_ind[:nn].copy(), H=H[: nn * nn].reshape(nn, nn).copy(), g=g[:nn].copy(),
                    Fc=Fc.reshape(8 * nc, 6 * nc), lb=lb, ub=ub, x0=x0, Acd=Acd.reshape(13, 13),
                    Bcd=Bcd.reshape(13, 6 * nc))


class DeviceGroup:
    """``hmpc_group_*`` (include/hector_mpc.h, csrc/hmpc_group.hip): one process, several GPUs, contiguous slices, the
    step-0 wrench + status gathered on every member and on the host.  ``devices`` may repeat an index with
    ``transport="p2p"`` (one-GPU exercise of the multi-member path)."""

    TRANSPORT = {"auto": 0, "rccl": 1, "p2p": 2}

    def __init__(self, dt: float, horizon: int, f_max: float, max_batch: int, devices, transport: str = "auto",
                 mu: float = 0.25, contacts: int = 2):
        self.L = _lib.load()
        self.horizon, self.max_batch, self.contacts = int(horizon), int(max_batch), int(contacts)
        self.setup = _lib.ProblemSetup(np.float32(dt), np.float32(mu), np.float32(f_max), int(horizon))
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self.g = C.c_void_p()
        rc = self.L.hmpc_group_create_ex(C.byref(self.g), C.byref(self.setup), devs.ctypes.data, len(devs), self.max_batch,
                                         self.TRANSPORT[transport], self.contacts)
        if rc != 0:
            raise HmpcError(f"hmpc_group_create_ex failed with {rc}: {self.L.hmpc_group_last_error().decode()}")
        self.size = int(self.L.hmpc_group_size(self.g))
        self.stride = int(self.L.hmpc_record_stride_ex(self.horizon, self.contacts))
        self.wrench_width = 6 * self.contacts

    def _check(self, rc, what):
        if rc != 0:
            raise HmpcError(f"{what} failed with {rc}: {self.L.hmpc_group_last_error().decode()}")

    def close(self):
        if getattr(self, "g", None):
            self.L.hmpc_group_destroy(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def transport(self) -> str:
        return {1: "rccl", 2: "p2p"}[int(self.L.hmpc_group_transport(self.g))]

    @property
    def batch(self) -> int:
        return int(self.L.hmpc_group_batch(self.g))

    def member(self, i: int):
        """(handle pointer, device, lo, n, solve stream) of member i."""
        h, st = C.c_void_p(), C.c_void_p()
        dev, lo, n = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.L.hmpc_group_member(self.g, int(i), C.byref(h), C.byref(dev), C.byref(lo), C.byref(n), C.byref(st)),
                    "hmpc_group_member")
        return h, dev.value, lo.value, n.value, st.value

    def upload(self, recs: np.ndarray) -> None:
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        assert recs.ndim == 2 and recs.shape[1] == self.stride
        self._check(self.L.hmpc_group_upload_records(self.g, recs.ctypes.data, recs.shape[0]), "hmpc_group_upload_records")

    def set_device_records(self, member_ptrs, batch: int, max_reduced_vars: int = -1, keepalive=None) -> None:
        """Records already resident on each member's device: member_ptrs[i] = device pointer of member i's first record
        (slice sizes follow ``shard_bounds``)."""
        self._keep = keepalive
        arr = (C.c_void_p * self.size)(*[C.c_void_p(int(p)) for p in member_ptrs])
        self._check(self.L.hmpc_group_set_device_records(self.g, arr, int(batch), int(max_reduced_vars)),
                    "hmpc_group_set_device_records")

    def solve(self) -> None:
        self._check(self.L.hmpc_group_solve(self.g), "hmpc_group_solve")

    def solve_command_sweep(self, group_size: int) -> None:
        """hmpc_solve_command_sweep on every member (slices must consist of whole groups)."""
        self._check(self.L.hmpc_group_solve_command_sweep(self.g, int(group_size)), "hmpc_group_solve_command_sweep")

    def set_deal(self, striped: bool) -> None:
        """Contiguous slices (default) or round-robin: member i holds instances i, i + G, ... (hmpc_group_set_deal)."""
        self._check(self.L.hmpc_group_set_deal(self.g, 1 if striped else 0), "hmpc_group_set_deal")

    def member_step(self, i: int) -> int:
        return int(self.L.hmpc_group_member_step(self.g, int(i)))

    def set_exchange_repair(self, on: bool) -> None:
        self._check(self.L.hmpc_group_set_exchange_repair(self.g, 1 if on else 0), "hmpc_group_set_exchange_repair")

    def post_gather(self) -> None:
        self._check(self.L.hmpc_group_post_gather(self.g), "hmpc_group_post_gather")

    def wait_gather(self) -> None:
        self._check(self.L.hmpc_group_wait_gather(self.g), "hmpc_group_wait_gather")

    def gather_wrench(self):
        b = self.batch
        wrench = np.zeros((b, self.wrench_width), dtype=np.float32)
        status = np.zeros(b, dtype=np.uint32)
        self._check(self.L.hmpc_group_gather_wrench(self.g, wrench.ctypes.data, status.ctypes.data), "hmpc_group_gather_wrench")
        return wrench, status

    def device_gathered(self, member: int):
        """(device pointer of member's gathered block, rows per slot)."""
        p, rows = C.c_void_p(), C.c_int(0)
        self._check(self.L.hmpc_group_device_gathered(self.g, int(member), C.byref(p), C.byref(rows)),
                    "hmpc_group_device_gathered")
        return p.value, rows.value

    def download(self):
        b = self.batch
        forces = np.zeros((b, self.wrench_width * self.horizon), dtype=np.float32)
        status = np.zeros(b, dtype=np.uint32)
        self._check(self.L.hmpc_group_download(self.g, forces.ctypes.data, status.ctypes.data), "hmpc_group_download")
        return forces, status

    def synchronize(self) -> None:
        self._check(self.L.hmpc_group_synchronize(self.g), "hmpc_group_synchronize")


def shard_bounds(global_batch: int, n_shards: int, index: int):
    """``hmpc_shard_bounds`` of the C ABI (pure host arithmetic; works without a GPU)."""
    lo, hi = C.c_int(0), C.c_int(0)
    rc = _lib.load().hmpc_shard_bounds(int(global_batch), int(n_shards), int(index), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise ValueError((global_batch, n_shards, index))
    return lo.value, hi.value


def status_code(status: np.ndarray) -> np.ndarray:
    return (np.asarray(status) & 0xFF).astype(np.int32)


def status_iters(status: np.ndarray) -> np.ndarray:
    return ((np.asarray(status) >> 8) & 0xFFF).astype(np.int32)


def status_nactive(status: np.ndarray) -> np.ndarray:
    return ((np.asarray(status) >> 20) & 0xFFF).astype(np.int32)
