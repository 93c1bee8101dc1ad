"""The record-gradient node of the host side's ResultState (csrc/hmpc_plan.h: solve -> adjoint -> (model, limits) -> record) on the CPU, no
GPU needed: a stand-alone program (tests/src/record_plan_on_host.cpp) compiled with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer and run directly.  From every reachable state under every transition of the adjoint's branch: it can be
enqueued only while all three parents stand; valid after on_record_adjoint; stale after every batch, solve, new adjoint, new model or
limit gradients, their retargets and its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "record_plan_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "record_plan_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
