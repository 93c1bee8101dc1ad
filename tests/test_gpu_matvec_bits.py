"""The solver's mat-vec path against its own recorded bits (tests/golden/matvec_bits.npz, written by
tests/golden/make_matvec_bits.py with the build of the commit named in the file).

gather_w and the reduction at the end of the staged mat-vec compute addresses, masks and selects around a fixed sequence of
multiply-adds and adds; a change there that leaves the arithmetic on data alone -- same operations, same operands, same order --
gives the same forces (compared as bit patterns) and the same status words.  No tolerance: one wrong column of Cn, one act byte of
the neighbouring row, one coefficient with the wrong sign or a -0.0 for an inactive row, one staging row >= ng taken for data shows
here as different bits.  The shapes are the generator's (ng at 1, at every border of a kernel variant or a staging half, and at
"every leg-step in stance"; a second solve on the same handle); the cases are built once per session."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_matvec_bits", os.path.join(HERE, "golden", "make_matvec_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.PATH)


@pytest.fixture(scope="module")
def all_cases():
    cs = gen.cases()
    gen.check_cases(cs)
    assert [c[0] for c in cs] == gen.NAMES
    return {c[0]: c[1:] for c in cs}


@pytest.mark.parametrize("name", gen.NAMES)
def test_forces_and_status_words_are_the_recorded_bits(golden, all_cases, name):
    from hector_simulation_amd import interface

    h, nc, first, second = all_cases[name]
    for tag, (forces, status) in zip(("a", "b"), gen.solve_case(h, nc, first, second)):
        want_f, want_s = golden[f"{name}_{tag}_forces"], golden[f"{name}_{tag}_status"]
        got_f = forces.view(np.uint32)
        assert got_f.shape == want_f.shape and status.shape == want_s.shape
        bad_s = np.flatnonzero(status != want_s)
        bad_f = np.flatnonzero((got_f != want_f).any(axis=1))
        print(f"{name}_{tag}: {len(bad_s)} status words and {len(bad_f)} force vectors of {len(status)} differ from commit {golden['commit']}")
        assert len(bad_s) == 0, (name, tag, bad_s[:8], interface.status_code(status)[bad_s[:8]], interface.status_iters(status)[bad_s[:8]],
                                 interface.status_iters(want_s)[bad_s[:8]])
        assert len(bad_f) == 0, (name, tag, bad_f[:8], np.abs(forces[bad_f[:8]] - want_f.view(np.float32)[bad_f[:8]]).max(axis=1))
