"""The feedback-gain kernel's own source behind the assembly (csrc/hmpc_feedback.h: free directions of every leg-step, the Riccati
recursion, the forward chain, the two summaries; and the first-order wrench) run on the CPU, no GPU needed: compiled with g++ against a
stand-in hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim), checked bit for bit against a plain sequential loop
(tests/src/feedback_on_host.cpp); a leg-step with all ten limits active, an unloaded foot and a NaN force included: the run has to end.
The GPU tests (tests/test_gpu_feedback.py) check the machine code; this one keeps the source's logic checked where there is no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feedback_kernel_source_on_the_host(tmp_path):
    exe = str(tmp_path / "feedback_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "feedback_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
