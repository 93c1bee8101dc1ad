"""The chains of stages A3 / A4 (csrc/hmpc_chains.h: the fourteen power recurrences over the compact table, the Phi and e items) run on the CPU,
no GPU needed: compiled with g++ against tests/src/hip_lane_shim and compared BIT FOR BIT, as uint32 with the sign of zero, with the dense
13-term k-ascending fmaf chains from the identity that tests/src/chains_on_host.cpp writes out itself -- all 169 entries of every power Acd^k,
every entry of Phi_k and of e.  Inputs: the oracle's Acd, Bcd, x0 of the cases of tests/front_cases.py (h = 10, 20), of the smallest horizon
the handle accepts (1) and h = 2, of three contacts at h = 1, 2, 10, and hand-made Acd / Bcd / x0 with -0.0 entries and a zero Rb block.  The
GPU test (tests/test_gpu_chains.py) checks the machine code; this one keeps the source's arithmetic checked where there is no GPU."""
import os
import struct
import subprocess

import numpy as np

import front_cases as fc
from hector_simulation_amd import records, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_case(oracle, f, h, nc):
    rec = records.pack_records(f, h, nc)
    a = [oracle.assemble_record(row, h, synthetic.DT_MPC, synthetic.F_MAX, reduce=False, nc=nc) for row in rec]
    return dict(h=h, nc=nc, Acd=np.stack([x["Acd"].reshape(-1) for x in a]), Bcd=np.stack([x["Bcd"].reshape(-1) for x in a]),
                x0=np.stack([x["x0"] for x in a]), traj=records.unpack_records(rec, h, nc)["traj"])


def _handmade(base):
    """Copies of a case's first instances with signed zeros where the structure has values: the dt Rbi block of Acd all +0, all -0, a
    mix of -0 and values, the dt entries -0; -0 in x0 and in Bcd's live rows."""
    nb = 8
    c = {k: (np.array(v[:nb], dtype=np.float32) if k not in ("h", "nc") else v) for k, v in base.items()}
    A = c["Acd"].reshape(nb, 13, 13)
    nz = np.float32(-0.0)
    A[0, 0:3, 6:9] = 0.0
    A[1, 0:3, 6:9] = nz
    A[2, 0, 6:9] = nz
    A[2, 1:3, 7] = nz
    A[3, 3, 9], A[3, 4, 10], A[3, 5, 11], A[3, 11, 12] = nz, nz, nz, nz
    A[4, 0:3, 6:9] = nz
    A[4, 5, 11], A[4, 11, 12] = nz, nz
    A[5, 0:3, 6:9] = -A[5, 0:3, 6:9]
    c["x0"][4, :] = nz
    c["x0"][5, 6:9] = nz
    c["x0"][6, 12] = nz
    B = c["Bcd"].reshape(nb, 13, -1)
    B[6, 6:9, :] = nz
    B[7, 9:12, :] = -B[7, 9:12, :]
    B[7, 6:9, 0:3] = 0.0
    return c


def test_chains_header_on_the_host(oracle, tmp_path):
    cases = []
    for name, h, rec, p, exp, wants in fc.host_cases(oracle):
        cases.append(dict(h=h, nc=2, Acd=exp["Acd"], Bcd=exp["Bcd"], x0=exp["x0"], traj=records.unpack_records(rec, h, 2)["traj"]))
    for h in (1, 2):
        for gait in ("standing", "walking"):
            cases.append(_oracle_case(oracle, synthetic.make_batch(8, h, gait, seed=370 + h, phase="random", yaw_rate_cmd=True), h, 2))
    for h in (1, 2, 10):
        cases.append(_oracle_case(oracle, synthetic.make_batch3(8, h, "standing", seed=374 + h), h, 3))
    cases.append(_handmade(cases[0]))            # standing, h = 10
    cases.append(_handmade(cases[3]))            # standing, h = 20
    cases.append(_handmade(cases[-3]))           # three contacts, h = 10
    assert (cases[0]["h"], cases[3]["h"], cases[-1]["h"], cases[-1]["nc"]) == (10, 20, 10, 3)
    path = str(tmp_path / "chains_cases.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for c in cases:
            nb, U = len(c["Acd"]), 6 * c["nc"]
            fh.write(struct.pack("<3i", c["h"], c["nc"], nb))
            for k, w in (("Acd", 169), ("Bcd", 13 * U), ("x0", 13), ("traj", 12 * c["h"])):
                a = np.ascontiguousarray(c[k], dtype="<f4").reshape(nb, -1)
                assert a.shape[1] == w, (k, a.shape)
                fh.write(a.tobytes())
    exe = str(tmp_path / "chains_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "chains_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 problems", r.stdout + r.stderr
