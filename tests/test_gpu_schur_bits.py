"""The variants that invert the block start's Schur matrix on the matrix cores against their own recorded bits
(tests/golden/schur_bits.npz, written by tests/golden/make_schur_bits.py with the build of the commit named in the file).

The tile loader and store of the Schur inversion compute addresses, scaling exponents and validity, and decide which tiles of
the grid take part at all; a change there that leaves the arithmetic on data alone gives the same forces (compared as bit
patterns) and the same status words (code, iteration count, final |W|).  No tolerance.  The cases are the generator's: first-round
row counts k0 on both sides of every tile border of the 3 x 3 grid (1, 15, 16, 17, 31, 32, 33, 47, 48, and more candidates than
the round can take), pinned on the host through a separable QP, and one batch for each of the other tile grids (4 x 4 three
contacts, 5 x 5 wide on eight waves, 6 x 6 continuation, the SWEEP variant's 3 x 3).  Inputs and golden are built once per session."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_schur_bits", os.path.join(HERE, "golden", "make_schur_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NAMES = ["contacts3", "wide_h20", "cont_6x", "sweep_4x8"]


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.PATH)


@pytest.fixture(scope="module")
def all_cases():
    cs = gen.cases()
    assert [c[0] for c in cs] == NAMES
    return {name: (h, nc, fields, k) for name, h, nc, fields, k in cs}


def _same_bits(name, golden, forces, status):
    from hector_simulation_amd import interface

    want_f, want_s = golden[name + "_forces"], golden[name + "_status"]
    got_f = forces.view(np.uint32)
    assert got_f.shape == want_f.shape and status.shape == want_s.shape
    bad_s = np.flatnonzero(status != want_s)
    bad_f = np.flatnonzero((got_f != want_f).any(axis=1))
    print(f"{name}: {len(bad_s)} status words and {len(bad_f)} force vectors of {len(status)} differ from commit {golden['commit']}")
    assert len(bad_s) == 0, (name, bad_s[:8], interface.status_code(status)[bad_s[:8]], interface.status_iters(status)[bad_s[:8]],
                             interface.status_iters(want_s)[bad_s[:8]], interface.status_nactive(status)[bad_s[:8]], interface.status_nactive(want_s)[bad_s[:8]])
    assert len(bad_f) == 0, (name, bad_f[:8], np.abs(forces[bad_f[:8]] - want_f.view(np.float32)[bad_f[:8]]).max(axis=1))


def test_first_round_row_counts_at_the_tile_borders(golden):
    """k0 = 1, 15, 16, 17, 31, 32, 33, 47, 48 and 52 / 54 candidates on the FAST 120-variable variant: the recorded bits, and the
    status words still say what pins k0 (|W| = k0 with no counted iteration; beyond 48 every candidate ends in the working set)."""
    from hector_simulation_amd import interface

    hx, gx, fx, k0 = gen.k0_inputs_from(golden)  # (the generator's random search takes half a minute: its result is in the file)
    assert np.array_equal(k0, np.array(gen.K0_TARGETS)) and golden["k0_edges_proved"].all()
    assert [gen.verify_instance(hx[i], gx[i], fx[i]) for i in range(len(k0))] == k0.tolist()  # host: exactly k0 rows are violated at x_u, and they are the optimal set
    assert set(k0.tolist()) >= {1, 15, 16, 17, 31, 32, 33, 47, 48} and k0.max() > 48
    forces, status = gen.solve_k0_edges(hx, gx, fx)
    _same_bits("k0_edges", golden, forces, status)
    assert (interface.status_code(status) == 0).all() and (interface.status_nactive(status) == k0).all()
    assert (interface.status_iters(status)[k0 <= gen.KB] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_forces_and_status_words_are_the_recorded_bits(golden, all_cases, name):
    h, nc, fields, k = all_cases[name]
    forces, status = gen.solve_case(h, nc, fields, k)
    _same_bits(name, golden, forces, status)
