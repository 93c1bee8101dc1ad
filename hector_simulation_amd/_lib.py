"""ctypes loader of libhector_mpc_hip.so.  Fails loudly: there is no CPU / PyTorch fallback for the solve path."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

_lib = None

# every symbol include/hector_mpc.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "setup_problem", "update_problem_data", "get_solution", "update_solver_settings", "hmpc_solve_mpc", "solveDenseMPC",
    "hmpc_get_q_soln", "hmpc_last_status", "hmpc_record_stride", "hmpc_pack_record", "hmpc_create", "hmpc_destroy",
    "hmpc_upload_records", "hmpc_set_device_records", "hmpc_set_max_reduced_vars", "hmpc_set_warm_start", "hmpc_resolve_failed", "hmpc_set_auto_resolve", "hmpc_set_device_outputs",
    "hmpc_solve", "hmpc_download", "hmpc_get_device_outputs", "hmpc_batch", "hmpc_horizon", "hmpc_time_solve",
    "hmpc_build_records", "hmpc_build_records_device", "hmpc_body_wrench", "hmpc_body_wrench_device", "hmpc_leg_torques", "hmpc_leg_torques_device",
    "hmpc_download_records", "hmpc_debug_assemble", "hmpc_debug_phase_cycles", "hmpc_download_f64", "hmpc_last_hip_error", "hmpc_version",
    "hmpc_upload_records_async", "hmpc_download_async", "hmpc_set_tick_warm_start", "hmpc_reset_tick_warm_start", "hmpc_create_ex", "hmpc_contacts", "hmpc_record_stride_ex", "hmpc_pack_record_ex",
    "hmpc_enable_f64_output", "hmpc_debug_solve_external_qp", "hmpc_set_device_repair", "hmpc_group_set_exchange_repair",
    "hmpc_shard_bounds", "hmpc_group_create", "hmpc_group_destroy", "hmpc_group_size", "hmpc_group_transport",
    "hmpc_group_batch", "hmpc_group_member", "hmpc_group_upload_records", "hmpc_group_set_device_records",
    "hmpc_group_solve", "hmpc_group_post_gather", "hmpc_group_wait_gather", "hmpc_group_device_gathered",
    "hmpc_group_gather_wrench", "hmpc_group_download", "hmpc_group_synchronize", "hmpc_group_last_error",
    "hmpc_group_create_ex", "hmpc_group_contacts", "hmpc_group_set_deal", "hmpc_group_deal", "hmpc_group_member_step",
    "hmpc_upload_records_strided_async", "hmpc_set_max_iterations", "hmpc_legacy_set_max_iterations", "hmpc_tick_solve_device", "hmpc_set_dispatch_order",
    "hmpc_set_handover", "hmpc_default_params", "hmpc_set_params", "hmpc_get_params", "hmpc_legacy_set_params", "hmpc_group_set_params",
    "hmpc_solve_command_sweep", "hmpc_set_instance_mu", "hmpc_group_solve_command_sweep", "hmpc_debug_handover_slots",
    "hmpc_debug_set_front_prologue", "hmpc_debug_front_scalars",
    "hmpc_predict_states", "hmpc_set_device_prediction", "hmpc_get_device_prediction", "hmpc_download_prediction",
    "hmpc_legacy_predicted_state",
    "hmpc_sweep_select", "hmpc_set_device_selection", "hmpc_get_device_selection", "hmpc_download_selection", "hmpc_tick_sweep_device",
    "hmpc_constraint_margins", "hmpc_set_device_margins", "hmpc_get_device_margins", "hmpc_download_margins", "hmpc_margin_penalty",
    "hmpc_set_sweep_margin_floor", "hmpc_legacy_constraint_slack",
    "hmpc_kkt_certificate", "hmpc_set_device_certificate", "hmpc_get_device_certificate", "hmpc_download_certificate",
    "hmpc_set_certificate_tolerance", "hmpc_certificate_penalty", "hmpc_set_sweep_certificate_ceiling", "hmpc_legacy_multiplier",
    "hmpc_legacy_stationarity",
    "hmpc_feedback_gains", "hmpc_set_device_gains", "hmpc_get_device_gains", "hmpc_download_gains", "hmpc_first_order_wrench",
    "hmpc_set_device_first_order", "hmpc_download_first_order", "hmpc_legacy_feedback_gain",
    "hmpc_solve_adjoint", "hmpc_set_device_adjoint", "hmpc_get_device_adjoint", "hmpc_download_adjoint",
    "hmpc_solve_adjoint_multi", "hmpc_set_device_adjoint_multi", "hmpc_get_device_adjoint_multi", "hmpc_download_adjoint_multi",
    "hmpc_select_adjoint_seed",
    "hmpc_adjoint_model", "hmpc_set_device_adjoint_model", "hmpc_get_device_adjoint_model", "hmpc_download_adjoint_model",
    "hmpc_adjoint_limits", "hmpc_set_device_adjoint_limits", "hmpc_get_device_adjoint_limits", "hmpc_download_adjoint_limits",
    "hmpc_adjoint_record", "hmpc_set_device_adjoint_record", "hmpc_get_device_adjoint_record", "hmpc_download_adjoint_record",
    "hmpc_adjoint_chain_multi", "hmpc_set_device_adjoint_chain_multi", "hmpc_get_device_adjoint_chain_multi", "hmpc_download_adjoint_chain_multi",
    "hmpc_default_plant", "hmpc_plant_step_device", "hmpc_rollout_device", "hmpc_set_device_rollout", "hmpc_get_device_rollout",
    "hmpc_download_rollout",
    "hmpc_default_rollout_cost", "hmpc_rollout_score_device", "hmpc_rollout_select_device", "hmpc_rollout_sweep_device",
    "hmpc_get_device_rollout_sweep",
    "hmpc_default_swing", "hmpc_swing_state_init_device", "hmpc_swing_legs_device", "hmpc_tick_command_device", "hmpc_set_rollout_swing",
]


class ProblemSetup(C.Structure):
    _fields_ = [("dt", C.c_float), ("mu", C.c_float), ("f_max", C.c_float), ("horizon", C.c_int)]


class Params(C.Structure):
    """include/hector_mpc.h struct hmpc_params (robot / contact constants; defaults = the reference's literals)."""
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float * 3), ("mu", C.c_float), ("lt", C.c_float), ("lh", C.c_float),
                ("gravity", C.c_float)]


CHAIN_COMPACT = ("grad_record", "grad_frames", "grad_rpy", "grad_params", "grad_limits", "limit_summary")
CHAIN_DETAIL = ("grad_A", "grad_B", "grad_r", "costate", "grad_Fc", "grad_bound", "lambda", "nu")


class AdjointChain(C.Structure):
    """include/hector_mpc.h struct hmpc_adjoint_chain (the arrays of hmpc_adjoint_chain_multi: six compact, eight detail)."""
    _fields_ = [(k, C.c_void_p) for k in CHAIN_COMPACT + CHAIN_DETAIL]


class TickInputs(C.Structure):
    """include/hector_mpc.h struct hmpc_tick_inputs (what updateMPCIfNeeded reads for one tick)."""
    _fields_ = [("position", C.c_double * 3), ("vWorld", C.c_double * 3), ("omegaWorld", C.c_double * 3),
                ("orientation", C.c_double * 4), ("rpy", C.c_double * 3), ("rBody", C.c_double * 9),
                ("leg_q", C.c_double * 10), ("pFoot", C.c_double * 6), ("v_des_robot", C.c_double * 2),
                ("yaw_rate_des", C.c_double), ("roll_des", C.c_double), ("pitch_des", C.c_double),
                ("world_position_desired", C.c_double * 2), ("gait_offsets", C.c_int * 2),
                ("gait_durations", C.c_int * 2), ("gait_iteration", C.c_int), ("flags", C.c_int)]


class Plant(C.Structure):
    """include/hector_mpc.h struct hmpc_plant (the plant's own constants; hmpc_default_plant fills the defaults)."""
    _fields_ = [("dt_tick", C.c_double), ("dtMPC", C.c_double), ("substeps", C.c_int), ("advance_gait", C.c_int), ("flags", C.c_int),
                ("reserved", C.c_int), ("mass", C.c_double), ("inertia", C.c_double * 3), ("gravity", C.c_double),
                ("hip", (C.c_double * 3) * 2), ("fall_cos", C.c_double), ("device_mass", C.c_void_p), ("device_ext_wrench", C.c_void_p)]


ROLLOUT_LOG = ("state", "wrench", "status", "tau", "summary")


class RolloutLog(C.Structure):
    """include/hector_mpc.h struct hmpc_rollout_log (device pointers of a rollout's log; each may be NULL)."""
    _fields_ = [(k, C.c_void_p) for k in ROLLOUT_LOG]


class RolloutCost(C.Structure):
    """include/hector_mpc.h struct hmpc_rollout_cost (the weights of hmpc_rollout_score_device; hmpc_default_rollout_cost fills the defaults)."""
    _fields_ = [("w_state", C.c_double * 12), ("w_terminal", C.c_double * 12), ("w_wrench", C.c_double * 12), ("w_tau", C.c_double * 10),
                ("height", C.c_double), ("dt_tick", C.c_double), ("fall_penalty", C.c_double), ("unsolved_penalty", C.c_double)]


ROLLOUT_CHOICE = ("index", "score", "wrench", "tau", "summary")


class RolloutChoice(C.Structure):
    """include/hector_mpc.h struct hmpc_rollout_choice (device pointers of a rollout selection's outputs; each may be NULL)."""
    _fields_ = [(k, C.c_void_p) for k in ROLLOUT_CHOICE]


class Swing(C.Structure):
    """include/hector_mpc.h struct hmpc_swing (the swing update's constants; hmpc_default_swing fills the reference's values)."""
    _fields_ = [("dt_update", C.c_double), ("dtMPC", C.c_double), ("updates", C.c_int), ("ticks_per_step", C.c_int), ("subtick", C.c_int),
                ("reserved", C.c_int), ("height", C.c_double), ("place_gain_v", C.c_double), ("place_gain_err", C.c_double),
                ("place_max", C.c_double), ("hip_yaw", (C.c_double * 3) * 2), ("hip_roll", C.c_double * 3),
                ("hip_width_offset", (C.c_double * 3) * 2), ("ik_link", C.c_double), ("ik_horizontal", C.c_double), ("ik_hip_x", C.c_double),
                ("kp", C.c_double * 5), ("kd", C.c_double * 5)]


class SwingState(C.Structure):
    """include/hector_mpc.h struct hmpc_swing_state (one per instance, carried from tick to tick; all zero with first_swing = {1, 1} at the start)."""
    _fields_ = [("p0", (C.c_double * 3) * 2), ("pf", (C.c_double * 3) * 2), ("swing_time", C.c_double * 2), ("q_des", C.c_double * 10),
                ("first_swing", C.c_int32 * 2)]


class MotorCmd(C.Structure):
    """include/hector_mpc.h struct hmpc_motor_cmd (the complete command of the ten joints)."""
    _fields_ = [(k, C.c_double * 10) for k in ("q", "dq", "Kp", "Kd", "tau")]


class Command(C.Structure):
    """include/hector_mpc.h struct hmpc_command (one candidate command of hmpc_tick_sweep_device)."""
    _fields_ = [("v_des_robot", C.c_double * 2), ("yaw_rate_des", C.c_double), ("roll_des", C.c_double), ("pitch_des", C.c_double)]


class UpdateData(C.Structure):
    _fields_ = [("p", C.c_float * 3), ("v", C.c_float * 3), ("q", C.c_float * 4), ("w", C.c_float * 3),
                ("r", C.c_float * 6), ("joint_angles", C.c_float * 10), ("yaw", C.c_float),
                ("weights", C.c_float * 12), ("traj", C.c_float * (12 * 36)), ("Alpha_K", C.c_float * 12),
                ("gait", C.c_ubyte * 36), ("hack_pad", C.c_ubyte * 1000), ("max_iterations", C.c_int),
                ("rho", C.c_double), ("sigma", C.c_double), ("solver_alpha", C.c_double), ("terminate", C.c_double)]


def lib_path() -> str:
    return _build.LIB


def load():
    """Loads (building first if the sources are newer) the native library; raises if it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build()
    if not os.path.exists(path):
        raise RuntimeError("libhector_mpc_hip.so is missing and could not be built; the solver has no fallback path")
    # ONE HIP runtime per process: PyTorch-ROCm bundles a libamdhip64.so.7 and this library's DT_NEEDED names the same SONAME, so the
    # copy the loader maps first serves both.  torch first = torch's bundled runtime for both (works; bench.py's order); this library
    # first = the system runtime for both, on which torch has been seen to report "no ROCm-capable device".  So if torch is installed,
    # let it come up first.  (A C++ host such as the reference controller has no torch in the process: the system runtime, the one the
    # library was built against, serves it.  tests/test_gpu_runtime.py asserts the single mapping.)
    if os.environ.get("HMPC_NO_TORCH_PRELOAD") != "1":
        try:
            import torch

            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    L = C.CDLL(path)
    vp, ci, cd, cf = C.c_void_p, C.c_int, C.c_double, C.c_float
    L.setup_problem.argtypes = [cd, ci, cd, cd]
    L.setup_problem.restype = None
    L.update_problem_data.argtypes = [vp] * 6 + [cd] + [vp] * 4
    L.update_problem_data.restype = None
    L.get_solution.argtypes = [ci]
    L.get_solution.restype = cd
    L.update_solver_settings.argtypes = [ci, cd, cd, cd, cd, cd]
    L.update_solver_settings.restype = None
    L.hmpc_solve_mpc.argtypes = [C.POINTER(UpdateData), C.POINTER(ProblemSetup)]
    L.hmpc_solve_mpc.restype = None
    L.solveDenseMPC.argtypes = [C.POINTER(UpdateData), C.POINTER(ProblemSetup)]
    L.solveDenseMPC.restype = None
    L.hmpc_get_q_soln.restype = C.POINTER(cd)
    L.hmpc_last_status.restype = C.c_uint32
    L.hmpc_record_stride.argtypes = [ci]
    L.hmpc_record_stride.restype = C.c_size_t
    L.hmpc_pack_record.argtypes = [vp, ci] + [vp] * 6 + [cd] + [vp] * 4
    L.hmpc_create.argtypes = [C.POINTER(vp), C.POINTER(ProblemSetup), ci, ci]
    L.hmpc_create_ex.argtypes = [C.POINTER(vp), C.POINTER(ProblemSetup), ci, ci, ci]
    L.hmpc_contacts.argtypes = [vp]
    L.hmpc_record_stride_ex.argtypes = [ci, ci]
    L.hmpc_record_stride_ex.restype = C.c_size_t
    L.hmpc_pack_record_ex.argtypes = [vp, ci, ci] + [vp] * 6 + [cd] + [vp] * 5 + [cd]
    L.hmpc_destroy.argtypes = [vp]
    L.hmpc_upload_records.argtypes = [vp, vp, ci]
    L.hmpc_set_device_records.argtypes = [vp, vp, ci]
    L.hmpc_set_max_reduced_vars.argtypes = [vp, ci]
    L.hmpc_set_warm_start.argtypes = [vp, ci]
    L.hmpc_upload_records_async.argtypes = [vp, vp, ci, vp]
    L.hmpc_download_async.argtypes = [vp, vp, vp, vp]
    L.hmpc_set_tick_warm_start.argtypes = [vp, ci, ci]
    L.hmpc_reset_tick_warm_start.argtypes = [vp]
    L.hmpc_resolve_failed.argtypes = [vp, C.POINTER(ci)]
    L.hmpc_set_auto_resolve.argtypes = [vp, ci]
    L.hmpc_set_handover.argtypes = [vp, ci]
    L.hmpc_default_params.argtypes = [C.POINTER(Params)]
    L.hmpc_default_params.restype = None
    L.hmpc_set_params.argtypes = [vp, C.POINTER(Params)]
    L.hmpc_get_params.argtypes = [vp, C.POINTER(Params)]
    L.hmpc_legacy_set_params.argtypes = [C.POINTER(Params)]
    L.hmpc_group_set_params.argtypes = [vp, C.POINTER(Params)]
    L.hmpc_set_device_repair.argtypes = [vp, ci]
    L.hmpc_group_set_exchange_repair.argtypes = [vp, ci]
    L.hmpc_set_device_outputs.argtypes = [vp, vp, vp]
    L.hmpc_solve.argtypes = [vp, vp]
    L.hmpc_solve_command_sweep.argtypes = [vp, ci, vp]
    L.hmpc_set_instance_mu.argtypes = [vp, vp]
    L.hmpc_group_solve_command_sweep.argtypes = [vp, ci]
    L.hmpc_download.argtypes = [vp, vp, vp]
    L.hmpc_get_device_outputs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.hmpc_batch.argtypes = [vp]
    L.hmpc_horizon.argtypes = [vp]
    L.hmpc_time_solve.argtypes = [vp, vp, ci, C.POINTER(cf)]
    L.hmpc_debug_assemble.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci)] + [vp] * 9
    L.hmpc_download_f64.argtypes = [vp, vp, vp]
    L.hmpc_build_records.argtypes = [vp, vp, ci, cd, vp]
    L.hmpc_build_records_device.argtypes = [vp, vp, ci, cd, vp, vp]
    L.hmpc_body_wrench.argtypes = [vp, vp, vp]
    L.hmpc_body_wrench_device.argtypes = [vp, vp, vp, vp]
    L.hmpc_download_records.argtypes = [vp, vp]
    L.hmpc_leg_torques.argtypes = [vp, vp, vp, vp, vp]
    L.hmpc_leg_torques_device.argtypes = [vp, vp, vp, vp, vp, vp]
    L.hmpc_enable_f64_output.argtypes = [vp]
    L.hmpc_debug_solve_external_qp.argtypes = [vp, vp, vp, vp, ci]
    L.hmpc_shard_bounds.argtypes = [ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.hmpc_group_create.argtypes = [C.POINTER(vp), C.POINTER(ProblemSetup), vp, ci, ci, ci]
    L.hmpc_group_create_ex.argtypes = [C.POINTER(vp), C.POINTER(ProblemSetup), vp, ci, ci, ci, ci]
    L.hmpc_group_contacts.argtypes = [vp]
    L.hmpc_group_set_deal.argtypes = [vp, ci]
    L.hmpc_group_deal.argtypes = [vp]
    L.hmpc_group_member_step.argtypes = [vp, ci]
    L.hmpc_upload_records_strided_async.argtypes = [vp, vp, ci, C.c_size_t, vp]
    L.hmpc_set_max_iterations.argtypes = [vp, ci]
    L.hmpc_legacy_set_max_iterations.argtypes = [ci]
    L.hmpc_legacy_set_max_iterations.restype = ci
    L.hmpc_set_dispatch_order.argtypes = [vp, ci]
    L.hmpc_tick_solve_device.argtypes = [vp, vp, ci, cd, vp, vp, vp, vp]
    for name in ("hmpc_group_destroy", "hmpc_group_size", "hmpc_group_transport", "hmpc_group_batch", "hmpc_group_solve",
                 "hmpc_group_post_gather", "hmpc_group_wait_gather", "hmpc_group_synchronize"):
        getattr(L, name).argtypes = [vp]
    L.hmpc_group_member.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(vp)]
    L.hmpc_group_upload_records.argtypes = [vp, vp, ci]
    L.hmpc_group_set_device_records.argtypes = [vp, vp, ci, ci]
    L.hmpc_group_device_gathered.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(ci)]
    L.hmpc_group_gather_wrench.argtypes = [vp, vp, vp]
    L.hmpc_group_download.argtypes = [vp, vp, vp]
    L.hmpc_group_last_error.restype = C.c_char_p
    L.hmpc_debug_phase_cycles.argtypes = [vp, vp]
    L.hmpc_debug_handover_slots.argtypes = [vp, vp]
    L.hmpc_debug_set_front_prologue.argtypes = [vp, ci]
    L.hmpc_debug_front_scalars.argtypes = [vp, vp]
    # the set, get and download entries of every derived result: one pointer per array of its family (interface.RESULTS), behind the handle
    # and, for the multi-seed adjoint, the seed count; the selection's get reports its groups last; the chain passes its struct
    from .interface import RESULTS  # (here, not at the top: interface.py imports this module)

    for family, arrays in RESULTS.items():
        if family == "adjoint_chain_multi":
            continue
        count = family == "adjoint_multi"
        getattr(L, "hmpc_set_device_" + family).argtypes = [vp] + [ci] * count + [vp] * len(arrays)
        getattr(L, "hmpc_download_" + family).argtypes = [vp] + [vp] * len(arrays)
        if family != "first_order":  # (the one family without a get)
            getattr(L, "hmpc_get_device_" + family).argtypes = ([vp] + [C.POINTER(ci)] * count + [C.POINTER(vp)] * len(arrays)
                                                                + [C.POINTER(ci)] * (family == "selection"))
    L.hmpc_predict_states.argtypes = [vp, vp]
    L.hmpc_legacy_predicted_state.argtypes = [ci, ci]
    L.hmpc_legacy_predicted_state.restype = cd
    L.hmpc_sweep_select.argtypes = [vp, ci, vp, vp]
    L.hmpc_tick_sweep_device.argtypes = [vp, vp, ci, vp, ci, cd, vp, vp, vp, vp, vp]
    L.hmpc_constraint_margins.argtypes = [vp, vp]
    L.hmpc_margin_penalty.argtypes = [vp, vp, vp, vp, vp]
    L.hmpc_set_sweep_margin_floor.argtypes = [vp, vp]
    L.hmpc_legacy_constraint_slack.argtypes = [ci, ci, ci]
    L.hmpc_legacy_constraint_slack.restype = cd
    L.hmpc_kkt_certificate.argtypes = [vp, vp]
    L.hmpc_set_certificate_tolerance.argtypes = [vp, cd]
    L.hmpc_certificate_penalty.argtypes = [vp, vp, vp, vp, vp]
    L.hmpc_set_sweep_certificate_ceiling.argtypes = [vp, vp]
    L.hmpc_legacy_multiplier.argtypes = [ci, ci, ci]
    L.hmpc_legacy_multiplier.restype = cd
    L.hmpc_legacy_stationarity.argtypes = []
    L.hmpc_legacy_stationarity.restype = cd
    L.hmpc_feedback_gains.argtypes = [vp, vp]
    L.hmpc_first_order_wrench.argtypes = [vp, vp, vp]
    L.hmpc_legacy_feedback_gain.argtypes = [ci, ci]
    L.hmpc_legacy_feedback_gain.restype = cd
    L.hmpc_solve_adjoint.argtypes = [vp, vp, vp]
    L.hmpc_solve_adjoint_multi.argtypes = [vp, vp, ci, vp]
    L.hmpc_select_adjoint_seed.argtypes = [vp, ci]
    L.hmpc_adjoint_model.argtypes = [vp, vp]
    L.hmpc_adjoint_limits.argtypes = [vp, vp, vp]
    L.hmpc_adjoint_record.argtypes = [vp, vp]
    L.hmpc_adjoint_chain_multi.argtypes = [vp, vp, vp]
    L.hmpc_set_device_adjoint_chain_multi.argtypes = [vp, ci, C.POINTER(AdjointChain)]
    L.hmpc_get_device_adjoint_chain_multi.argtypes = [vp, C.POINTER(ci), C.POINTER(AdjointChain)]
    L.hmpc_download_adjoint_chain_multi.argtypes = [vp, C.POINTER(AdjointChain)]
    L.hmpc_default_plant.argtypes = [C.POINTER(Plant)]
    L.hmpc_default_plant.restype = None
    L.hmpc_plant_step_device.argtypes = [vp, vp, ci, C.POINTER(Plant), vp, ci, vp, vp, vp, vp]
    L.hmpc_rollout_device.argtypes = [vp, vp, ci, ci, cd, ci, ci, C.POINTER(Plant), C.POINTER(RolloutLog), vp]
    L.hmpc_set_device_rollout.argtypes = [vp, C.POINTER(RolloutLog)]
    L.hmpc_get_device_rollout.argtypes = [vp, ci, C.POINTER(RolloutLog)]
    L.hmpc_download_rollout.argtypes = [vp, vp, vp, vp, vp, vp]
    L.hmpc_default_rollout_cost.argtypes = [C.POINTER(RolloutCost)]
    L.hmpc_default_rollout_cost.restype = None
    L.hmpc_rollout_score_device.argtypes = [vp, vp, ci, ci, C.POINTER(RolloutCost), C.POINTER(RolloutLog), vp, vp, vp]
    L.hmpc_rollout_select_device.argtypes = [vp, vp, vp, ci, ci, C.POINTER(RolloutLog), C.POINTER(RolloutChoice), vp]
    L.hmpc_rollout_sweep_device.argtypes = [vp, vp, ci, vp, ci, ci, cd, ci, ci, C.POINTER(Plant), C.POINTER(RolloutCost), vp,
                                            C.POINTER(RolloutChoice), vp]
    L.hmpc_get_device_rollout_sweep.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.hmpc_default_swing.argtypes = [C.POINTER(Swing)]
    L.hmpc_default_swing.restype = None
    L.hmpc_swing_state_init_device.argtypes = [vp, vp, ci, vp]
    L.hmpc_swing_legs_device.argtypes = [vp, vp, ci, C.POINTER(Swing), vp, vp, vp, vp, vp]
    L.hmpc_tick_command_device.argtypes = [vp, vp, ci, cd, C.POINTER(Swing), vp, vp, vp, vp, vp]
    L.hmpc_set_rollout_swing.argtypes = [vp, C.POINTER(Swing), vp, vp]
    L.hmpc_last_hip_error.restype = C.c_char_p
    L.hmpc_version.restype = C.c_char_p
    _lib = L
    return L
