"""The limit-gradient kernel's own source behind the assembly (csrc/hmpc_limit_adjoint.h: the passes, the gradient and the adjoint
residual, the two triangular solves per leg-step, the row and bound gradients and the chain rules to mu, lt, lh and the caps) run on the
CPU, no GPU needed: compiled with g++ against a stand-in hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim), checked
bit for bit against a plain sequential loop (tests/src/limit_adjoint_on_host.cpp); a zero seed, a swing contact, ten active limits on a
leg-step, an unloaded foot, a NaN force, a NaN seed and lt = 0 included: the run has to end.  On every leg-step the admitted set is pinned
against free_directions (csrc/hmpc_feedback.h).  The GPU tests (tests/test_gpu_limit_adjoint.py) check the machine code; this one keeps
the source's logic checked where there is no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limit_adjoint_kernel_source_on_the_host(tmp_path):
    exe = str(tmp_path / "limit_adjoint_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "limit_adjoint_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
