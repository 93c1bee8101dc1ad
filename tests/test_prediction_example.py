"""examples/predicted_trajectory.c (a command sweep, then the predicted motion under every command) compiled against
include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_examples.py: without a GPU it must fail loudly,
with one it must run; and the legacy prediction call answers 0 where nothing has been solved."""
import subprocess

import pytest

from hector_simulation_amd import _lib
from test_examples import _compile, _has_gpu

SRC = ("predicted_trajectory.c", "gcc", "-std=c11")


def test_prediction_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_prediction_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prediction of 3 states x 4 commands: 0 problems" in r.stdout
    assert r.stdout.count("predicted vx at step 10") == 12


def test_legacy_prediction_is_zero_for_out_of_range_arguments():
    L = _lib.load()
    for step, comp in ((-1, 0), (0, -1), (0, 13), (10 ** 6, 0)):
        assert L.hmpc_legacy_predicted_state(step, comp) == 0.0  # (as get_solution; also before the first solve)
