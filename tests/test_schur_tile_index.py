"""The index arithmetic of the block start's Schur tiles (csrc/hmpc_schur_tiles.h: offsets into the packed triangle, validity,
scaling-exponent sums, tile liveness -- from lane constants formed once per call) on the CPU, no GPU needed: compiled with g++
and run against the plain per-entry expressions it replaces (tests/src/schur_tiles_on_host.cpp), for NTG = 3 .. 6, four and eight
waves, every wave, lane, tile slot and r, every k0 from 0 to 16 NTG.  A tile is dead exactly when none of its entries is data, and
the ceil(k0 / 4) pivot steps never reach a dead tile row.  The GPU tests (tests/test_gpu_schur_bits.py) check the machine code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schur_tile_index_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "schur_tiles_on_host")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "src", "schur_tiles_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 problems" in r.stdout, r.stdout + r.stderr
