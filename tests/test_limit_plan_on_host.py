"""The limit-gradient node of the host side's ResultState (csrc/hmpc_plan.h: solve -> adjoint -> limits) on the CPU, no GPU needed: a
stand-alone program (tests/src/limit_plan_on_host.cpp) compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run
directly.  From every reachable state under every transition of the adjoint's branch: valid after on_limit_adjoint; stale after every
batch, solve, on_adjoint, retarget_adjoint and its own retarget; independent of the model gradients."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limit_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "limit_plan_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "limit_plan_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
