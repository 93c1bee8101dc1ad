"""examples/foot_placement_gradient.c (a standing batch solved, the loss "step-0 vertical force of the left foot" seeded, its gradients in
the foot positions, the mass and the inertia printed, one foot moved by 1 mm and the mass raised by 1 % and the predicted changes beside
re-solves) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_adjoint_example.py:
without a GPU it must fail loudly, with one it must run."""
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("foot_placement_gradient.c", "gcc", "-std=c11")


def test_foot_placement_gradient_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_foot_placement_gradient_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "foot and payload gradients of 4 standing robots, a foot moved by 1 mm and the mass raised by 1 %: 0 problems" in r.stdout
