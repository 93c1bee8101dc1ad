"""The record-gradient calls of the C ABI: exported with the signatures include/hector_mpc.h declares, the ctypes signatures of the
loader, HMPC_E_ARG for a NULL handle, the contract's items in the header, the Python entry points.  No GPU (the empty batch needs a
handle: tests/test_gpu_pose_adjoint.py has it)."""
import ctypes as C
import inspect
import os
import re

from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
SIGNATURES = {
    "hmpc_adjoint_record": "int hmpc_adjoint_record(hmpc_handle *h, void *stream);",
    "hmpc_set_device_adjoint_record": "int hmpc_set_device_adjoint_record(hmpc_handle *h, double *device_grad_record, double *device_grad_frames, "
                                      "double *device_grad_rpy);",
    "hmpc_get_device_adjoint_record": "int hmpc_get_device_adjoint_record(hmpc_handle *h, double **device_grad_record, double **device_grad_frames, "
                                      "double **device_grad_rpy);",
    "hmpc_download_adjoint_record": "int hmpc_download_adjoint_record(hmpc_handle *h, double *grad_record, double *grad_frames, double *grad_rpy);",
}


def test_the_four_symbols_are_exported_as_declared():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "hector_mpc.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    syms = os.popen(f"nm -D --defined-only {_lib.lib_path()}").read()
    for name, sig in SIGNATURES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(rf"\bT {name}\b", syms), name
        assert re.sub(r"\s+", " ", sig) in flat, name
    vp = C.c_void_p
    assert L.hmpc_adjoint_record.argtypes == [vp, vp]
    assert L.hmpc_set_device_adjoint_record.argtypes == [vp] * 4 and L.hmpc_download_adjoint_record.argtypes == [vp] * 4
    assert L.hmpc_get_device_adjoint_record.argtypes == [vp] + [C.POINTER(vp)] * 3
    assert "hmpc_legacy_adjoint_record" not in flat  # (no accessor on the process-global interface)
    for name in ("adjoint_record", "download_adjoint_record", "set_device_adjoint_record", "get_device_adjoint_record"):
        assert callable(getattr(interface.BatchedMPC, name)), name
    assert interface.BatchedMPC.RECORD_ADJOINT_KEYS == ("grad_record", "grad_frames", "grad_rpy")


def test_the_contract_is_in_the_header():
    text = open(os.path.join(ROOT, "include", "hector_mpc.h")).read()
    joined = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("pose gradients of the solve: orientation, joint angles, the whole record",
                   "Rz(a0) Rx(a1) Ry(a2 + a3 + a4)",
                   "G_Iw = 0 - Y / dt",
                   "exactly 0 where the assembly's clamp !(2 t < 0.99999) holds",
                   "yaw <- +0 (the solve never reads it)",
                   "hmpc_adjoint_record, behind all three, chains them through the assembly",
                   "have not all three been enqueued behind the last adjoint of the last solve of the current batch"):
        assert phrase in joined, phrase


def test_a_null_handle_is_an_argument_error():
    L = _lib.load()
    out = [C.c_void_p() for _ in range(3)]
    assert L.hmpc_adjoint_record(None, None) == E_ARG
    assert L.hmpc_set_device_adjoint_record(None, *[None] * 3) == E_ARG
    assert L.hmpc_get_device_adjoint_record(None, *[C.byref(p) for p in out]) == E_ARG
    assert L.hmpc_download_adjoint_record(None, *[None] * 3) == E_ARG
    assert all(p.value is None for p in out)


def test_differentiable_solve_fields_is_an_entry_point_of_its_own():
    """The older entry points keep their parameter lists."""
    from hector_simulation_amd import autograd

    assert list(inspect.signature(autograd.differentiable_solve_fields).parameters) == ["mpc", "fields"]
    assert list(inspect.signature(autograd.differentiable_solve).parameters) == ["mpc", "fields", "traj", "weights", "alpha_k", "r"]
    assert list(inspect.signature(autograd.differentiable_solve_limits).parameters) == ["mpc", "fields", "traj", "weights", "alpha_k", "r", "mu"]
    assert autograd.FIELD_NAMES == ("p", "v", "q", "w", "r", "joint_angles", "weights", "Alpha_K", "traj", "Rhand", "f_max_hand")
