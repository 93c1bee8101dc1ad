"""The pose-gradient kernel's own source behind the assembly (csrc/hmpc_pose_adjoint.h: the staging of the nine upstream buffers, the
chains from the constraint block, the inertia and the Euler-rate map to the body rotation, the foot frames, the joint angles and the
quaternion, and the copies into the record's order) run on the CPU, no GPU needed: compiled with g++ against a stand-in hip_runtime.h
that gives every lane a thread (tests/src/hip_lane_shim), checked bit for bit against a plain sequential loop
(tests/src/pose_adjoint_on_host.cpp); zero upstream gradients, a swing contact, NaN gradients as a NaN force leaves them, a NaN grad_Fc,
the clamped pitch and an un-normalised quaternion included: the run has to end.  The GPU tests (tests/test_gpu_pose_adjoint.py) check the
machine code; this one keeps the source's logic checked where there is no GPU.  profiles/r23/sanitize_host.txt holds one run of the same
program under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_adjoint_kernel_source_on_the_host(tmp_path):
    exe = str(tmp_path / "pose_adjoint_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "pose_adjoint_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
