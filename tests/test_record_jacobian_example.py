"""examples/record_jacobian.c (four standing robots solved, the twelve unit seeds of the step-0 wrench in ONE multi-seed adjoint launch
and ONE chain launch behind it, the Jacobian's column "left foot's x position" printed and its vertical-force entry compared with
re-solves that have the foot moved by +-1 mm) compiled against include/hector_mpc.h and linked to the in-tree library, on the pattern
of tests/test_wrench_jacobian_example.py, whose inputs, active-set tolerance and bound it shares: the rows are the same bits, so the two
examples must print the same numbers.  Without a GPU it must fail loudly, with one it must run."""
import subprocess

import pytest

from test_examples import _compile, _has_gpu
from test_wrench_jacobian_example import SRC as WRENCH_SRC

SRC = ("record_jacobian.c", "gcc", "-std=c11")


def test_record_jacobian_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_record_jacobian_example_runs_on_gpu_and_prints_the_wrench_examples_numbers(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step-0 record Jacobian of 4 standing robots from two calls, a foot moved by +-1 mm: 0 problems" in r.stdout
    w = subprocess.run([_compile(tmp_path, *WRENCH_SRC)], capture_output=True, text=True, timeout=300)
    assert w.returncode == 0, w.stdout + w.stderr

    def numbers(out):  # every line of the table and the d Fz_left / d x_left-foot comparison, robot by robot
        return [line for line in out.splitlines() if line.startswith("  ")]

    assert len(numbers(r.stdout)) == 4 * 13 and numbers(r.stdout) == numbers(w.stdout)
