"""The two shape tables of the results derived from a solve -- csrc/hmpc_results.h, from which the library allocates and copies, and
``interface.RESULTS``, from which Python allocates the host arrays a download fills -- say the same, array by array: a wrong size in either
is memory written out of bounds.  No GPU needed: tests/src/result_layout_on_host.cpp, a stand-alone program that includes the header alone,
is compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer, run directly, and every line it prints (family, array, element
size, elements per instance) is compared with the Python table.  The two tables stay two (one export per table would be an ABI change);
this test is what ties them together."""
import os
import subprocess

import numpy as np
import pytest

from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(nc, h) for nc in (2, 3) for h in (1, 3, 10)] + [(2, 20)]  # (contacts, horizon)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "result_layout_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "result_layout_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + [str(v) for s in SHAPES for v in s], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 problems", r.stdout + r.stderr
    return [ln.split() for ln in r.stdout.splitlines()[:-1]]


def python_lines(nc, h):
    return [[str(nc), str(h), family, name, str(np.dtype(dt).itemsize), str(int(np.prod(shape(h, nc), dtype=np.int64)))]
            for family, arrays in interface.RESULTS.items() for name, dt, shape in arrays]


def test_both_tables_list_the_same_arrays_with_the_same_sizes(printed):
    want = [ln for nc, h in SHAPES for ln in python_lines(nc, h)]
    assert len(printed) == len(want) and len(want) == len(SHAPES) * 61  # (2 + 5 + 3 + 5 + 4 + 2 + 6 + 5 + 6 + 3 + 6 + 14 arrays)
    for got, exp in zip(printed, want):
        assert got == exp, (got, exp)  # (line by line: the same families and arrays in the same order, the same sizes)


def test_the_chains_rows_are_the_record_model_and_limit_rows():
    R = interface.RESULTS
    chain = {k: (dt, shape) for k, dt, shape in R["adjoint_chain_multi"]}
    assert tuple(chain) == _lib.CHAIN_COMPACT + _lib.CHAIN_DETAIL and len(chain) == 14
    taken = {**{k: ("adjoint_record", k) for k in ("grad_record", "grad_frames", "grad_rpy")},
             **{k: ("adjoint_model", k) for k in ("grad_params", "grad_A", "grad_B", "grad_r", "costate")},
             **{k: ("adjoint_limits", k) for k in ("grad_limits", "grad_Fc", "grad_bound", "lambda", "nu")}, "limit_summary": ("adjoint_limits", "summary")}
    assert set(taken) == set(chain)
    for k, (family, name) in taken.items():
        dt, shape = next((d, s) for n, d, s in R[family] if n == name)
        assert chain[k][0] is dt and chain[k][1] is shape, k  # (the same row, not an equal one)
        for nc, h in SHAPES:
            assert chain[k][1](h, nc) == shape(h, nc)
    assert R["adjoint_multi"] is R["adjoint"]


def test_the_public_key_tuples_come_from_the_table():
    M = interface.BatchedMPC
    for keys, family in ((M.ADJOINT_KEYS, "adjoint"), (M.MODEL_ADJOINT_KEYS, "adjoint_model"), (M.LIMIT_ADJOINT_KEYS, "adjoint_limits"),
                         (M.RECORD_ADJOINT_KEYS, "adjoint_record"), (M.CHAIN_KEYS, "adjoint_chain_multi")):
        assert keys == tuple(k for k, _, _ in interface.RESULTS[family])
