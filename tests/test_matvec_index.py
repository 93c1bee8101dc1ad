"""The lane constants and the coefficient of the solver's gather_w (csrc/hmpc_matvec_index.h: leg-step and position of a variable
by one multiply and one shift, the column of its leg's normals in Cn, the act / slot words, and sgn * cf / its negation / +0.0 from
the packed act byte by bit operations) on the CPU, no GPU needed: compiled with g++ and run against the plain per-use expressions
they replace (tests/src/matvec_index_on_host.cpp).  The coefficient is compared bit for bit for ac in {-1, 0, 1}, sgn in {-1, 1} and
cf over +-0, denormals, +-inf, NaNs and 4000 random bit patterns; the addresses for every thread index below NMAX of every shape.
A second build with -fsanitize=address,undefined runs the same program.  The GPU test (tests/test_gpu_matvec_bits.py) checks the
machine code; the instances it solves are first shown here to be ones qpOASES solves."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_matvec_index_arithmetic_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "matvec_index_on_host")
    cmd = ["g++", "-std=c++17", "-Wall"] + flags + ["-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"),
                                                    os.path.join(ROOT, "tests", "src", "matvec_index_on_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 problems" in r.stdout, r.stdout + r.stderr


def test_qpoases_solves_every_instance_of_the_matvec_bit_cases():
    """What tests/golden/make_matvec_bits.py pins are solves of problems qpOASES solves as well (n_bad == 0): the seeds were picked so."""
    from oracle import oracle_py

    spec = importlib.util.spec_from_file_location("make_matvec_bits", os.path.join(ROOT, "tests", "golden", "make_matvec_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cs = gen.cases()
    gen.check_cases(cs)
    for name, h, nc, first, second in cs:
        for f in (first, second):
            ref = oracle_py.solve_records(gen.pack(f, h, nc), h, gen.DT, gen.FMAX, nc=nc)
            assert ref["n_bad"] == 0, (name, ref["bad"].nonzero())
