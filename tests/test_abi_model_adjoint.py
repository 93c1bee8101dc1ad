"""The model-gradient calls of the C ABI: exported with the signatures include/hector_mpc.h declares, the ctypes signatures of the loader,
HMPC_E_ARG for a NULL handle, and a download of an empty batch that copies nothing.  No GPU."""
import ctypes as C
import os
import re

from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
SIGNATURES = {
    "hmpc_adjoint_model": "int hmpc_adjoint_model(hmpc_handle *h, void *stream);",
    "hmpc_set_device_adjoint_model": "int hmpc_set_device_adjoint_model(hmpc_handle *h, double *device_grad_A, double *device_grad_B, "
                                     "double *device_grad_r, double *device_grad_params, double *device_costate);",
    "hmpc_get_device_adjoint_model": "int hmpc_get_device_adjoint_model(hmpc_handle *h, double **device_grad_A, double **device_grad_B, "
                                     "double **device_grad_r, double **device_grad_params, double **device_costate);",
    "hmpc_download_adjoint_model": "int hmpc_download_adjoint_model(hmpc_handle *h, double *grad_A, double *grad_B, double *grad_r, "
                                   "double *grad_params, double *costate);",
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
    assert L.hmpc_adjoint_model.argtypes == [vp, vp]
    assert L.hmpc_set_device_adjoint_model.argtypes == [vp] * 6 and L.hmpc_download_adjoint_model.argtypes == [vp] * 6
    assert L.hmpc_get_device_adjoint_model.argtypes == [vp] + [C.POINTER(vp)] * 5
    assert "hmpc_legacy_adjoint_model" not in flat  # (no accessor on the process-global interface)
    # the adjoint's contract no longer leaves r and hmpc_params to the caller
    assert "left to the caller (r, the orientation, hmpc_params, mu, the caps)" not in text
    assert "left to the caller are the orientation" in re.sub(r"\s*\n \*\s*", " ", text)
    for name in ("adjoint_model", "download_adjoint_model", "set_device_adjoint_model", "get_device_adjoint_model"):
        assert callable(getattr(interface.BatchedMPC, name)), name
    assert interface.BatchedMPC.MODEL_ADJOINT_KEYS == ("grad_A", "grad_B", "grad_r", "grad_params", "costate")


def test_a_null_handle_is_an_argument_error():
    L = _lib.load()
    out = [C.c_void_p() for _ in range(5)]
    assert L.hmpc_adjoint_model(None, None) == E_ARG
    assert L.hmpc_set_device_adjoint_model(None, *[None] * 5) == E_ARG
    assert L.hmpc_get_device_adjoint_model(None, *[C.byref(p) for p in out]) == E_ARG
    assert L.hmpc_download_adjoint_model(None, *[None] * 5) == E_ARG
    assert all(p.value is None for p in out)


def test_differentiable_solve_takes_the_foot_positions():
    import inspect

    from hector_simulation_amd import autograd

    p = inspect.signature(autograd.differentiable_solve).parameters
    assert list(p) == ["mpc", "fields", "traj", "weights", "alpha_k", "r"] and p["r"].default is None
