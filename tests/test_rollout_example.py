"""examples/rollout.c (64 standing robots, each pushed sideways by its own force for 10 ticks, two rollouts on the device) compiled against
include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_examples.py: without a GPU it must fail loudly, with
one it must run."""
import re
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("rollout.c", "gcc", "-std=c11")


def test_rollout_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_rollout_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rollout example: 0 problems" in r.stdout
    m = re.search(r"(\d+) of 64 robots hold their height", r.stdout)
    assert m and 1 <= int(m.group(1)) <= 64, r.stdout
    assert r.stdout.count("vy after the push") == 9
    print(r.stdout)
