"""The decisions of the host side (csrc/hmpc_plan.h) on the CPU, no GPU needed: a stand-alone program (tests/src/plan_on_host.cpp) compiled with
g++ under AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  It checks pick_variant and repair_variant over a grid of
(contacts, horizon, widest reduced QP) against the literal expectations and against the search over a variant table built from
HMPC_VARIANT_TABLE's shapes, the size-class launch tables, the repair predicates against the three expressions they replaced, and
ResultState -- which derived results are still valid -- from every reachable state under every transition."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "plan_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "plan_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
