"""examples/pose_gradient.c (a pitching standing batch, the loss "step-0 vertical force of the left foot" seeded, its gradients in the
quaternion and the joint angles printed beside re-solves with the body rolled and the hip-yaw joints turned by +-1e-3 rad, each within
the bound of tests/pose_adjoint_mirror.py) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern of
tests/test_limit_adjoint_example.py: without a GPU it must fail loudly, with one it must run."""
import re
import subprocess

import pytest

import pose_adjoint_mirror as pm
from test_examples import _compile, _has_gpu

SRC = ("pose_gradient.c", "gcc", "-std=c11")


def test_the_examples_bounds_are_the_mirrors():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pose_gradient.c")).read()
    assert float(re.search(r"#define BOUND_Q (\S+)", text).group(1)) == pytest.approx(pm.PADJ_FD["q"], rel=1e-12)
    assert float(re.search(r"#define BOUND_JA (\S+)", text).group(1)) == pytest.approx(pm.PADJ_FD["ja"], rel=1e-12)


def test_pose_gradient_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_pose_gradient_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pose gradients of 4 pitching standing robots beside re-solves under a 1e-03 rad tilt: 0 problems" in r.stdout
