"""The feedback-gain calls of the C ABI: exported with the signatures include/hector_mpc.h declares, HMPC_E_ARG for a NULL handle, and
the process-global entry 0 before the first solve and out of range.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

from hector_simulation_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
SIGNATURES = {
    "hmpc_feedback_gains": "int hmpc_feedback_gains(hmpc_handle *h, void *stream);",
    "hmpc_set_device_gains": "int hmpc_set_device_gains(hmpc_handle *h, double *device_gain, double *device_ref_gain, double *device_summary, "
                             "int32_t *device_free_dims);",
    "hmpc_get_device_gains": "int hmpc_get_device_gains(hmpc_handle *h, double **device_gain, double **device_ref_gain, double **device_summary, "
                             "int32_t **device_free_dims);",
    "hmpc_download_gains": "int hmpc_download_gains(hmpc_handle *h, double *gain, double *ref_gain, double *summary, int32_t *free_dims);",
    "hmpc_first_order_wrench": "int hmpc_first_order_wrench(hmpc_handle *h, const void *device_records_new, void *stream);",
    "hmpc_set_device_first_order": "int hmpc_set_device_first_order(hmpc_handle *h, float *device_wrench, double *device_worst_slack);",
    "hmpc_download_first_order": "int hmpc_download_first_order(hmpc_handle *h, float *wrench, double *worst_slack);",
    "hmpc_legacy_feedback_gain": "double hmpc_legacy_feedback_gain(int component, int state);",
}


def test_the_eight_symbols_are_exported_as_declared():
    L = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hector_mpc.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    syms = os.popen(f"nm -D --defined-only {_lib.lib_path()}").read()
    for name, sig in SIGNATURES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(rf"\bT {name}\b", syms), name
        assert re.sub(r"\s+", " ", sig) in flat, name
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert L.hmpc_feedback_gains.argtypes == [vp, vp] and L.hmpc_first_order_wrench.argtypes == [vp, vp, vp]
    assert L.hmpc_set_device_gains.argtypes == [vp] * 5 and L.hmpc_download_gains.argtypes == [vp] * 5
    assert L.hmpc_get_device_gains.argtypes == [vp] + [C.POINTER(vp)] * 4
    assert L.hmpc_set_device_first_order.argtypes == [vp] * 3 and L.hmpc_download_first_order.argtypes == [vp] * 3
    assert L.hmpc_legacy_feedback_gain.argtypes == [ci, ci] and L.hmpc_legacy_feedback_gain.restype == cd


def test_a_null_handle_is_an_argument_error():
    L = _lib.load()
    out = [C.c_void_p() for _ in range(4)]
    assert L.hmpc_feedback_gains(None, None) == E_ARG
    assert L.hmpc_set_device_gains(None, None, None, None, None) == E_ARG
    assert L.hmpc_get_device_gains(None, *[C.byref(p) for p in out]) == E_ARG
    assert L.hmpc_download_gains(None, None, None, None, None) == E_ARG
    assert L.hmpc_first_order_wrench(None, None, None) == E_ARG
    assert L.hmpc_set_device_first_order(None, None, None) == E_ARG
    assert L.hmpc_download_first_order(None, None, None) == E_ARG
    assert all(p.value is None for p in out)


def test_legacy_gain_is_zero_before_the_first_solve():
    """In a process of its own: whatever this session's other tests solved does not count."""
    code = ("from hector_simulation_amd import interface\n"
            "vals = [interface.legacy_feedback_gain(c, s) for c, s in ((0, 0), (11, 12), (-1, 0), (12, 0), (0, 13), (0, -1))]\n"
            "assert all(v == 0.0 for v in vals), vals\n"
            "print('zero before the first solve')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "zero before the first solve" in r.stdout, r.stdout + r.stderr
