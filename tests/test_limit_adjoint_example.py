"""examples/friction_gradient.c (a standing batch pushed sideways solved on slippery ground, the loss "sum of the step-0 lateral forces"
seeded, its gradients in mu, lt, lh and the caps printed, and the predicted change beside re-solves at mu (1 +- 1e-3)) compiled against
include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_model_adjoint_example.py: without a GPU it must fail
loudly, with one it must run."""
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("friction_gradient.c", "gcc", "-std=c11")


def test_friction_gradient_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_friction_gradient_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "friction gradients of 4 pushed standing robots beside re-solves at mu (1 +- 1e-3): 0 problems" in r.stdout
