"""The adjoint calls of the C ABI: exported with the signatures include/hector_mpc.h declares, the ctypes signatures of the loader, and
HMPC_E_ARG for a NULL handle and a NULL seed.  No GPU."""
import ctypes as C
import os
import re

from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
SIGNATURES = {
    "hmpc_solve_adjoint": "int hmpc_solve_adjoint(hmpc_handle *h, const double *device_seed, void *stream);",
    "hmpc_set_device_adjoint": "int hmpc_set_device_adjoint(hmpc_handle *h, double *device_grad_x0, double *device_grad_traj, "
                               "double *device_grad_weights, double *device_grad_alpha, double *device_dir, double *device_summary);",
    "hmpc_get_device_adjoint": "int hmpc_get_device_adjoint(hmpc_handle *h, double **device_grad_x0, double **device_grad_traj, "
                               "double **device_grad_weights, double **device_grad_alpha, double **device_dir, double **device_summary);",
    "hmpc_download_adjoint": "int hmpc_download_adjoint(hmpc_handle *h, double *grad_x0, double *grad_traj, double *grad_weights, "
                             "double *grad_alpha, double *dir, double *summary);",
}


def test_the_four_symbols_are_exported_as_declared():
    L = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hector_mpc.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    syms = os.popen(f"nm -D --defined-only {_lib.lib_path()}").read()
    for name, sig in SIGNATURES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(rf"\bT {name}\b", syms), name
        assert re.sub(r"\s+", " ", sig) in flat, name
    vp = C.c_void_p
    assert L.hmpc_solve_adjoint.argtypes == [vp, vp, vp]
    assert L.hmpc_set_device_adjoint.argtypes == [vp] * 7 and L.hmpc_download_adjoint.argtypes == [vp] * 7
    assert L.hmpc_get_device_adjoint.argtypes == [vp] + [C.POINTER(vp)] * 6
    assert "hmpc_legacy_adjoint" not in flat  # (a seed has no place in the process-global interface: the header says so)
    assert "a seed has no place in that interface" in open(os.path.join(ROOT, "include", "hector_mpc.h")).read()
    for name in ("solve_adjoint", "download_adjoint", "set_device_adjoint"):
        assert callable(getattr(interface.BatchedMPC, name)), name


def test_a_null_handle_and_a_null_seed_are_argument_errors():
    L = _lib.load()
    out = [C.c_void_p() for _ in range(6)]
    seed = (C.c_double * 8)()
    assert L.hmpc_solve_adjoint(None, C.cast(seed, C.c_void_p), None) == E_ARG
    assert L.hmpc_solve_adjoint(None, None, None) == E_ARG
    assert L.hmpc_set_device_adjoint(None, *[None] * 6) == E_ARG
    assert L.hmpc_get_device_adjoint(None, *[C.byref(p) for p in out]) == E_ARG
    assert L.hmpc_download_adjoint(None, *[None] * 6) == E_ARG
    assert all(p.value is None for p in out)


def test_the_autograd_module_offers_differentiable_solve():
    from hector_simulation_amd import autograd

    assert callable(autograd.differentiable_solve)
