"""The multi-seed chain kernel's own source behind the assembly (csrc/hmpc_adjoint_chain.h: the model, limit and record gradients of a
tile of seeds behind one assembly, one forward chain, one active set and one lambda) run on the CPU, no GPU needed: compiled with g++
against a stand-in hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim) and checked bit for bit, seed by seed, against
the three single-seed sources run one after the other under that seed alone (tests/src/adjoint_chain_on_host.cpp); one, two, one more
than a sub-tile and a whole tile of seeds, a zero seed, a seed on a swing contact, a NaN in one seed only, all ten limits active, an
unloaded foot and the clamped pitch included, with and without the detail arrays.  The GPU tests (tests/test_gpu_adjoint_chain.py) check
the machine code; this one keeps the source's logic checked where there is no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adjoint_chain_kernel_source_on_the_host(tmp_path):
    exe = str(tmp_path / "adjoint_chain_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "adjoint_chain_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
