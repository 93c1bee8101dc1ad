"""The first-pass variants against their own recorded bits (tests/golden/fast_path_bits.npz, written by
tests/golden/make_fast_path_bits.py with the build of the commit named in the file).

Stage S's tile loader and hand-back and the block start's release loop move data and compute addresses; a change there that
leaves the arithmetic on data alone -- same operations, same operands, same order -- gives the same forces (compared as bit
patterns) and the same status words (code, iteration count, final |W|).  No tolerance: one wrong staging address, one mirror read
of the wrong triangle, one padding row taken for data or one release in another order shows here as different bits.  The shapes are
the generator's (its docstring says what each is the smallest case of); the reference is computed once per session."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_fast_path_bits", os.path.join(HERE, "golden", "make_fast_path_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NAMES = ["standing", "mixed", "single_h20", "sweep120", "sweep60", "walking", "standing_3x"]


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.PATH)


@pytest.fixture(scope="module")
def all_cases():
    cs = gen.cases()
    gen.check_cases(cs)
    assert [c[0] for c in cs] == NAMES
    return {name: (h, fields, k) for name, h, fields, k in cs}


@pytest.mark.parametrize("name", NAMES)
def test_forces_and_status_words_are_the_recorded_bits(golden, all_cases, name):
    from hector_simulation_amd import interface

    h, fields, k = all_cases[name]
    forces, status = gen.solve_case(h, fields, k)
    want_f, want_s = golden[name + "_forces"], golden[name + "_status"]
    got_f = forces.view(np.uint32)
    assert got_f.shape == want_f.shape and status.shape == want_s.shape
    bad_s = np.flatnonzero(status != want_s)
    bad_f = np.flatnonzero((got_f != want_f).any(axis=1))
    print(f"{name}: {len(bad_s)} status words and {len(bad_f)} force vectors of {len(status)} differ from commit {golden['commit']}")
    assert len(bad_s) == 0, (name, bad_s[:8], interface.status_code(status)[bad_s[:8]], interface.status_iters(status)[bad_s[:8]],
                             interface.status_iters(want_s)[bad_s[:8]], interface.status_nactive(status)[bad_s[:8]], interface.status_nactive(want_s)[bad_s[:8]])
    assert len(bad_f) == 0, (name, bad_f[:8], np.abs(forces[bad_f[:8]] - want_f.view(np.float32)[bad_f[:8]]).max(axis=1))
