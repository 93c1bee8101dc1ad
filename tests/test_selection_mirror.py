"""The checker of the GPU selection tests checked on its own (no GPU): tests/selection_mirror.py against cases whose answer is known by
construction -- ties, signed zeros, masks, status codes -- and against an independent vectorised formulation on random data."""
import numpy as np

import selection_mirror as sm


def _case(scores, status=None, k=None):
    s = np.asarray(scores, dtype=np.float64)
    b = s.shape[0]
    cost = np.stack([s, np.full(b, -0.0)], axis=1)  # (x + -0 = x for every x, -0 included)
    status = np.zeros(b, dtype=np.uint32) if status is None else np.asarray(status, dtype=np.uint32)
    forces = np.arange(b * 4, dtype=np.float32).reshape(b, 4) + 1
    states = np.arange(b * 2 * 13, dtype=np.float32).reshape(b, 2, 13) + 1
    return sm.select(cost, states, status, forces, k or b), forces, states


def test_ties_and_signed_zeros_go_to_the_lowest_index():
    out, forces, _ = _case([3.0, 1.0, 1.0, 2.0])
    assert out["index"][0] == 1 and out["score"][0] == 1.0
    np.testing.assert_array_equal(out["forces"][0], forces[1])
    out, _, _ = _case([5.0, 0.0, -0.0, 0.0])
    assert out["index"][0] == 1 and not np.signbit(out["score"][0])  # -0 == +0: the earlier one, bits and all
    out, _, _ = _case([5.0, -0.0, 0.0])
    assert out["index"][0] == 1 and np.signbit(out["score"][0])


def test_masks_and_status_codes():
    out, _, states = _case([np.nan, np.inf, -np.inf, 7.0, 2.0], status=[0, 0, 0, 6 | (3 << 8), 1])
    assert out["index"][0] == 3 and out["status"][0] == (6 | (3 << 8))  # NaN, +-inf and a max-iter instance are out; OK_RELAXED is in
    np.testing.assert_array_equal(out["states"][0], states[3])
    out, _, _ = _case([np.nan, np.inf], k=1)
    assert (out["index"] == -1).all() and (out["score"] == np.inf).all() and (out["status"] == sm.SELECT_NONE).all()
    assert (out["forces"].view(np.uint32) == 0).all() and (out["states"].view(np.uint32) == 0).all()
    for code in (1, 2, 3, 4, 5, 7, 8, 9):
        out, _, _ = _case([1.0, 2.0], status=[code, 0])
        assert out["index"][0] == 1


def test_penalty_is_added_after_the_two_costs():
    cost = np.array([[1e16, 1.0], [1e16, 3.0]])
    pen = np.array([-1e16, -1e16])
    np.testing.assert_array_equal(sm.scores(cost, pen), (cost[:, 0] + cost[:, 1]) + pen)  # (0, 4): not cost[0] + (cost[1] + penalty)
    np.testing.assert_array_equal(sm.scores(cost), cost[:, 0] + cost[:, 1])


def test_against_a_vectorised_formulation_on_random_data():
    rng = np.random.default_rng(3)
    for groups, k in ((7, 1), (5, 3), (4, 64), (3, 130)):
        b = groups * k
        cost = rng.uniform(0, 10, (b, 2)).round(1)  # rounded: ties occur
        pen = rng.choice([0.0, 0.5, np.nan, np.inf, -np.inf], size=b, p=[0.5, 0.3, 0.1, 0.05, 0.05])
        status = rng.choice([0, 6, 1, 7, 3], size=b, p=[0.6, 0.1, 0.1, 0.1, 0.1]).astype(np.uint32) | (rng.integers(0, 50, b).astype(np.uint32) << 8)
        forces = rng.standard_normal((b, 6)).astype(np.float32)
        states = rng.standard_normal((b, 2, 13)).astype(np.float32)
        out = sm.select(cost, states, status, forces, k, pen)
        s = sm.scores(cost, pen)
        ok = np.isin(status & 0xFF, (0, 6)) & np.isfinite(s)
        masked = np.where(ok, s, np.inf).reshape(groups, k)
        idx = masked.argmin(axis=1)  # (first occurrence of the minimum)
        none = ~ok.reshape(groups, k).any(axis=1)
        np.testing.assert_array_equal(out["index"], np.where(none, -1, idx))
        win = np.arange(groups) * k + idx
        np.testing.assert_array_equal(out["score"], np.where(none, np.inf, s[win]))
        np.testing.assert_array_equal(out["forces"], np.where(none[:, None], 0, forces[win]))
        np.testing.assert_array_equal(out["status"], np.where(none, sm.SELECT_NONE, status[win]))
