"""The block-pivot steps of the matrix-core sweeps against their own recorded bits (tests/golden/step_bits.npz, written by
tests/golden/make_step_bits.py with the build of the commit named in the file).

Which step of its tile row a pivot step is decides which accumulator register holds the pivot rows, which quarter of the columns a
tile publishes, which panel buffer is written and whether the next publish belongs to the next tile row; a change that decides any
of it at compile time and leaves the arithmetic on data alone -- same operations, same operands, same order per tile -- gives the
same forces (compared as bit patterns) and the same status words.  No tolerance.  The cases are the generator's: stage S with
ceil(6 ng / 4) steps ending at every place of a tile row (ng = 8, 11, 12, 10, 19, 20) on the FAST variants of h = 10 and h = 20 and on
the SWEEP variant, each with a second solve on the same handle, and the block start's Schur inversion with first-round row counts
that end inside a tile row (9, 10, 12, 21, 24, 41, 44).  The stage-S instances are first shown, on the CPU, to be ones qpOASES solves.
The cases are built once per session."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_step_bits", os.path.join(HERE, "golden", "make_step_bits.py"))
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


def _same_bits(name, golden, forces, status):
    from hector_simulation_amd import interface

    want_f, want_s = golden[name + "_forces"], golden[name + "_status"]
    got_f = forces.view(np.uint32)
    assert got_f.shape == want_f.shape and status.shape == want_s.shape
    bad_s = np.flatnonzero(status != want_s)
    bad_f = np.flatnonzero((got_f != want_f).any(axis=1))
    print(f"{name}: {len(bad_s)} status words and {len(bad_f)} force vectors of {len(status)} differ from commit {golden['commit']}")
    assert len(bad_s) == 0, (name, bad_s[:8], interface.status_code(status)[bad_s[:8]], interface.status_iters(status)[bad_s[:8]],
                             interface.status_iters(want_s)[bad_s[:8]])
    assert len(bad_f) == 0, (name, bad_f[:8], np.abs(forces[bad_f[:8]] - want_f.view(np.float32)[bad_f[:8]]).max(axis=1))


def test_qpoases_solves_every_stage_s_instance(all_cases):
    """What the golden file pins are solves of problems qpOASES solves as well (n_bad == 0): the seeds were picked so."""
    from oracle import oracle_py

    for name, (h, nc, k, first, second) in all_cases.items():
        for f in (first, second):
            ref = oracle_py.solve_records(gen.pack(f, h, nc), h, gen.DT, gen.FMAX, nc=nc)
            assert ref["n_bad"] == 0, (name, ref["bad"].nonzero())


@pytest.mark.gpu
@pytest.mark.parametrize("name", gen.NAMES)
def test_stage_s_steps_ending_at_every_place_of_a_tile_row(golden, all_cases, name):
    h, nc, k, first, second = all_cases[name]
    for tag, (forces, status) in zip(("a", "b"), gen.solve_case(h, nc, k, first, second)):
        _same_bits(f"{name}_{tag}", golden, forces, status)


@pytest.mark.gpu
def test_schur_steps_ending_inside_a_tile_row(golden):
    """k0 = 9, 10, 12, 21, 24, 41, 44 rows in the block start's first round: the recorded bits, and the status words still say what
    pins k0 (|W| = k0 with no counted iteration)."""
    from hector_simulation_amd import interface

    hx, gx, fx, k0 = gen.k0_inputs_from(golden)  # (the generator's random search takes a while: its result is in the file)
    assert np.array_equal(k0, np.array(gen.K0_TARGETS))
    assert {(-(-int(t) // 4)) % 4 for t in k0} | {(-(-t // 4)) % 4 for t in gen.SCHUR_BITS_K0} == {0, 1, 2, 3}  # with the cases of test_gpu_schur_bits.py
    assert [gen.sb.verify_instance(hx[i], gx[i], fx[i]) for i in range(len(k0))] == k0.tolist()  # host: exactly k0 rows are violated at x_u, and they are the optimal set
    forces, status = gen.sb.solve_k0_edges(hx, gx, fx)
    _same_bits("schur_k0", golden, forces, status)
    assert (interface.status_code(status) == 0).all() and (interface.status_nactive(status) == k0).all()
    assert (interface.status_iters(status) == 0).all()
