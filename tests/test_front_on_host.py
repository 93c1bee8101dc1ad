"""The batched prologue's own source (csrc/hmpc_front.hip: front_scalars_kernel and the lane bodies of stages A1 / A2 in csrc/hmpc_front.h)
run on the CPU, no GPU needed: compiled with g++ against the stand-in hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim)
and compared BIT FOR BIT with the oracle's x0, Acd, Bcd and Fc (tests/src/front_on_host.cpp; the cases: tests/front_cases.py).  The GPU
test (tests/test_gpu_front_prologue.py) checks the machine code; this one keeps the source's arithmetic and branches checked where there is
no GPU."""
import os
import struct
import subprocess

import numpy as np

import front_cases as fc
from hector_simulation_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_front_kernel_source_on_the_host(oracle, tmp_path):
    cases = fc.host_cases(oracle)
    path = str(tmp_path / "front_cases.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for name, h, rec, p, exp, wants in cases:
            fh.write(struct.pack("<4i", h, rec.shape[0], rec.shape[1], wants))
            fh.write(np.array([synthetic.DT_MPC, synthetic.F_MAX, *p["Ib"], p["lt"], p["lh"], p["mu"], p["inv_mass"], p["gravity"]],
                              dtype="<f4").tobytes())
            fh.write(np.ascontiguousarray(rec, dtype=np.uint8).tobytes())
            for k in ("x0", "Acd", "Bcd", "Fc"):
                fh.write(np.ascontiguousarray(exp[k], dtype="<f4").tobytes())
    exe = str(tmp_path / "front_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "front_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr
