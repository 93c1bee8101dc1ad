"""examples/rollout_sweep.c (16 standing robots pushed sideways, eight candidate commands each, 40 closed-loop ticks, one call of
hmpc_rollout_sweep_device) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern of
tests/test_rollout_example.py: without a GPU it must fail loudly, with one it must run."""
import re
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("rollout_sweep.c", "gcc", "-std=c11")


def test_rollout_sweep_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        return  # (the gpu-marked test below runs it)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_rollout_sweep_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rollout sweep example: 0 problems" in r.stdout
    assert len(re.findall(r"^robot +\d+, push", r.stdout, flags=re.M)) == 16
    assert re.search(r"^robot  0, push   0.0 N: best command", r.stdout, flags=re.M), r.stdout
    print(r.stdout)
