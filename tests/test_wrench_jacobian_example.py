"""examples/wrench_jacobian.c (four standing robots solved, the twelve unit seeds of the step-0 wrench in ONE multi-seed adjoint launch,
each slice selected and chained through model, limit and record gradients, the Jacobian's column "left foot's x position" printed and
its vertical-force entry compared with re-solves that have the foot moved by +-1 mm) compiled against include/hector_mpc.h and linked
to the in-tree library, on the pattern of tests/test_model_adjoint_example.py: without a GPU it must fail loudly, with one it must run."""
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("wrench_jacobian.c", "gcc", "-std=c11")


def test_wrench_jacobian_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_wrench_jacobian_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step-0 wrench Jacobian of 4 standing robots from one multi-seed launch, a foot moved by +-1 mm: 0 problems" in r.stdout
