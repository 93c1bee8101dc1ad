"""examples/feedback_gain.c (a standing batch solved, its feedback gains, every robot's velocity nudged by 1 mm/s, the first-order wrench
beside a re-solve) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern of
tests/test_certificate_example.py: without a GPU it must fail loudly, with one it must run."""
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("feedback_gain.c", "gcc", "-std=c11")


def test_feedback_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_feedback_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feedback gains of 4 standing robots, nudged by 1 mm/s: 0 problems" in r.stdout
