"""examples/motor_command.c (16 walking robots, one gait cycle of ticks: solve, swing update, plant step per tick, the complete motor command
of every joint) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_rollout_example.py:
without a GPU it must fail loudly, with one it must run."""
import re
import subprocess

import pytest

from test_examples import _compile, _has_gpu

SRC = ("motor_command.c", "gcc", "-std=c11")


def test_motor_command_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_motor_command_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "motor command example: 0 problems" in r.stdout
    assert "the left leg swings on 40 of 80 ticks; highest target 0.150 m" in r.stdout
    rows = re.findall(r"tick +\d+: left leg swing phase ([0-9.]+), target height ([0-9.]+) m, qDes", r.stdout)
    # (the cycle's first tick is the last of the left leg's swing, sub-phase 1; then stance until the tick after sub-phase 0)
    assert len(rows) == 20 and rows[0] == ("1.000", "0.000") and rows[15] == ("0.500", "0.150") and all(ph == "0.000" for ph, _ in rows[1:11])
    print(r.stdout)
