"""The chain's node of the host side's ResultState (csrc/hmpc_plan.h: solve -> multi-seed adjoint -> chain) on the CPU, no GPU needed: a
stand-alone program (tests/src/adjoint_chain_plan_on_host.cpp) compiled with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and
run directly.  From every reachable state under every ordering of batch, solve, single adjoint, multi-seed adjoint, selection, the
single-seed downstream launches, the chain and the retargets: the chain is stale exactly after a batch, a solve, a new multi-seed launch,
the multi-seed adjoint's retarget and its own, and every accessor that existed before the chain answers as it did."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adjoint_chain_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "adjoint_chain_plan_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "adjoint_chain_plan_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
