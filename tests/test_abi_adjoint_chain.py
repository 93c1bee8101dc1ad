"""The multi-seed chain calls of the C ABI: exported with the signatures include/hector_mpc.h declares, the struct's size and member
order against the header, the ctypes signatures of the loader, and HMPC_E_ARG for a NULL handle.  No GPU."""
import ctypes as C
import os
import re

from hector_simulation_amd import _lib, autograd, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
SIGNATURES = {
    "hmpc_adjoint_chain_multi": "int hmpc_adjoint_chain_multi(hmpc_handle *h, const double *device_seeds, void *stream);",
    "hmpc_set_device_adjoint_chain_multi": "int hmpc_set_device_adjoint_chain_multi(hmpc_handle *h, int n_seeds, "
                                           "const struct hmpc_adjoint_chain *device_buffers);",
    "hmpc_get_device_adjoint_chain_multi": "int hmpc_get_device_adjoint_chain_multi(hmpc_handle *h, int *n_seeds, "
                                           "struct hmpc_adjoint_chain *device_buffers);",
    "hmpc_download_adjoint_chain_multi": "int hmpc_download_adjoint_chain_multi(hmpc_handle *h, const struct hmpc_adjoint_chain *host_buffers);",
}
MEMBERS = ("grad_record", "grad_frames", "grad_rpy", "grad_params", "grad_limits", "limit_summary", "grad_A", "grad_B", "grad_r", "costate",
           "grad_Fc", "grad_bound", "lambda", "nu")


def _header():
    text = open(os.path.join(ROOT, "include", "hector_mpc.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_four_symbols_are_exported_as_declared():
    L = _lib.load()
    flat = _header()
    syms = os.popen(f"nm -D --defined-only {_lib.lib_path()}").read()
    for name, sig in SIGNATURES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(rf"\bT {name}\b", syms), name
        assert re.sub(r"\s+", " ", sig) in flat, name
    vp, ci, st = C.c_void_p, C.c_int, C.POINTER(_lib.AdjointChain)
    assert L.hmpc_adjoint_chain_multi.argtypes == [vp, vp, vp]
    assert L.hmpc_set_device_adjoint_chain_multi.argtypes == [vp, ci, st]
    assert L.hmpc_get_device_adjoint_chain_multi.argtypes == [vp, C.POINTER(ci), st]
    assert L.hmpc_download_adjoint_chain_multi.argtypes == [vp, st]
    assert "hmpc_legacy_adjoint" not in flat and "hmpc_group_adjoint" not in flat  # (nothing on the process-global or the group interface)
    for name in ("adjoint_chain_multi", "download_adjoint_chain_multi", "set_device_adjoint_chain_multi", "get_device_adjoint_chain_multi"):
        assert callable(getattr(interface.BatchedMPC, name)), name
    assert interface.BatchedMPC.CHAIN_KEYS == MEMBERS
    assert callable(autograd.wrench_jacobian)


def test_the_struct_is_fourteen_pointers_in_the_headers_order():
    body = re.search(r"struct hmpc_adjoint_chain \{(.*?)\};", _header()).group(1)
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            assert stmt.startswith("double *"), stmt
            declared += [m.strip().lstrip("*") for m in stmt[len("double "):].split(",")]
    assert tuple(declared) == MEMBERS
    assert tuple(n for n, _ in _lib.AdjointChain._fields_) == MEMBERS
    assert all(t is C.c_void_p for _, t in _lib.AdjointChain._fields_)
    assert C.sizeof(_lib.AdjointChain) == len(MEMBERS) * C.sizeof(C.c_void_p)
    for k, name in enumerate(MEMBERS):
        assert getattr(_lib.AdjointChain, name).offset == k * C.sizeof(C.c_void_p), name


def test_a_null_handle_is_an_argument_error():
    L = _lib.load()
    b = _lib.AdjointChain()
    n = C.c_int(-5)
    seeds = (C.c_double * 8)()
    assert L.hmpc_adjoint_chain_multi(None, C.cast(seeds, C.c_void_p), None) == E_ARG
    assert L.hmpc_set_device_adjoint_chain_multi(None, 1, C.byref(b)) == E_ARG
    assert L.hmpc_get_device_adjoint_chain_multi(None, C.byref(n), C.byref(b)) == E_ARG
    assert L.hmpc_download_adjoint_chain_multi(None, C.byref(b)) == E_ARG
    assert n.value == -5 and all(getattr(b, k) is None for k in MEMBERS)
