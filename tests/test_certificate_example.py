"""examples/certified_command.c (per tick a command sweep, the prediction, the KKT certificate, then the cheapest command among those the
certificate's ceiling lets through; one candidate's forces spoiled by 1 N in the second tick) compiled against include/hector_mpc.h and
linked to the in-tree library, on the pattern of tests/test_margins_example.py: without a GPU it must fail loudly, with one it must run;
and the new entry points refuse a NULL handle without touching a device."""
import subprocess

import pytest

from hector_simulation_amd import _lib
from test_examples import _compile, _has_gpu

SRC = ("certified_command.c", "gcc", "-std=c11")


def test_certificate_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_certificate_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "certified command of 3 states x 8 commands over 2 ticks: 0 problems" in r.stdout
    assert "tick 0: the ceiling masked 0 of 24 commands" in r.stdout and "tick 1: the ceiling masked 1 of 24 commands" in r.stdout


def test_new_entry_points_refuse_a_null_handle():
    L = _lib.load()
    assert L.hmpc_kkt_certificate(None, None) == -1  # HMPC_E_ARG
    assert L.hmpc_set_device_certificate(None, None, None, None, None, None) == -1
    assert L.hmpc_get_device_certificate(None, None, None, None, None, None) == -1
    assert L.hmpc_download_certificate(None, None, None, None, None, None) == -1
    assert L.hmpc_set_certificate_tolerance(None, 1e-3) == -1
    assert L.hmpc_certificate_penalty(None, None, None, None, None) == -1
    assert L.hmpc_set_sweep_certificate_ceiling(None, None) == -1
    assert L.hmpc_legacy_multiplier(0, 0, 0) == 0.0  # before the first solve
    assert L.hmpc_legacy_stationarity() == 0.0
