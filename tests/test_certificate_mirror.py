"""The KKT certificate's definition (tests/certificate_mirror.py) against what is independent of it: the oracle's binary32 H and g, the
reference's qpOASES (its forces and its own dual solution) and scipy's NNLS.  No GPU.  Shapes: the six of prediction_mirror.SHAPES and
hard_batch(16, 10, "standing", seed=17) at 3 x and 6 x, where active sets of dependent normals appear."""
import numpy as np
import pytest

import certificate_mirror as cm
import prediction_mirror as pm
from hector_simulation_amd import records, synthetic

HARD = [("hard_3x", 3.0, 0.10), ("hard_6x", 6.0, 0.25)]  # (name, scale, the share of leg-steps with a non-empty active set item 5 may leave out)
CASES = [(s[0], s) for s in pm.SHAPES] + [(n, (n, "hard", 10, 16, 2, 17, sc)) for n, sc, _ in HARD]
CASE_IDS = [c[0] for c in CASES]
LEFT_OUT_CAP = {**{s[0]: 0.0 for s in pm.SHAPES}, **{n: cap for n, _, cap in HARD}}

_cache = {}


def case_records(case):
    if case[1] == "hard":
        return records.pack_records(synthetic.hard_batch(case[3], case[2], "standing", seed=case[5], scale=case[6]), case[2], case[4])
    return pm.shape_records(case)[1]


def reference_case(oracle, case):
    """Records, qpOASES' forces rounded to binary32, qpOASES' multipliers in one-sided form and the mirror on those forces (with the
    bounds), once per case; shared by the tests here and by tests/test_gpu_certificate.py, left unchanged."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _cache:
        rec = case_records(case)
        u32, y = np.zeros((nb, h, 6 * nc), dtype=np.float32), np.zeros((nb, h, nc, 10))
        for k in range(nb):
            u, y[k] = cm.qpoases_primal_dual(oracle, rec[k], h, nc)
            u32[k] = u.astype(np.float32)
        _cache[name] = dict(rec=rec, u32=u32, y=y, m=cm.certificate_records(oracle, rec, h, nc, u32, with_bounds=True))
    return _cache[name]


def enter_case(name, build, left_out_cap=0.0):
    """A case from outside CASES (tests/derived_irregular.py): build() gives its reference_case dict, once; the multiplier check's cap for
    it is left_out_cap.  From then on reference_case -- and every helper built on it -- takes the case's tuple."""
    assert name not in CASE_IDS
    LEFT_OUT_CAP.setdefault(name, left_out_cap)
    if name not in _cache:
        _cache[name] = build()
    return _cache[name]


def leg_step_bound(G_bound, i, c, nc):
    return float(G_bound[i, cm.cols(c, nc)].max())


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_costate_gradient_is_H_u_plus_g(oracle, case):
    """1: at qpOASES' forces and at random forces in [-50, 150], row by row within G_bound."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    d = reference_case(oracle, case)
    m = d["m"]
    ratio = np.abs(m["grad"] - m["Hu_g"]) / m["G_bound"]
    print(name, "kappa at the optimum", cm.G_FACTOR * ratio.max())
    assert (ratio <= 1.0).all(), ratio.max()
    rng = np.random.default_rng(5)
    ur = rng.uniform(-50.0, 150.0, (2, h, 6 * nc)).astype(np.float32)
    mr = cm.certificate_records(oracle, d["rec"][:2], h, nc, ur, with_bounds=True)
    ratio = np.abs(mr["grad"] - mr["Hu_g"]) / mr["G_bound"]
    print(name, "kappa at random forces", cm.G_FACTOR * ratio.max())
    assert (ratio <= 1.0).all(), ratio.max()


@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_constraint_rows_of_a_contact_touch_its_own_variables_only(oracle, shape):
    """2: rows 8c .. 8c+7 of Fc are zero outside cols(c)."""
    name, gait, h, nb, nc, seed = shape
    _, rec = pm.shape_records(shape)
    for k in range(nb):
        Fc = oracle.assemble_record(rec[k], h, synthetic.DT_MPC, synthetic.F_MAX, reduce=False, nc=nc)["Fc"]
        for c in range(nc):
            outside = np.ones(6 * nc, dtype=bool)
            outside[cm.cols(c, nc)] = False
            assert (Fc[8 * c:8 * c + 8][:, outside] == 0).all()


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_residual_agrees_with_scipy_nnls(oracle, case):
    """3: e of the mirror's Lawson-Hanson against scipy.optimize.nnls on the same columns, to 1e-9 max(1, |r|)."""
    opt = pytest.importorskip("scipy.optimize")
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    m = reference_case(oracle, case)["m"]
    worst = 0.0
    for k in range(nb):
        for i in range(h):
            for c in range(nc):
                if not m["stance"][k, i, c]:
                    continue
                act = cm.active_set(m["slack"][k, i, c])
                r = m["grad"][k, i, cm.cols(c, nc)]
                N = m["N"][k][c][:, act]
                e = r - N @ opt.nnls(N, r)[0] if act else r
                err = np.abs(m["resid"][k, i, c] - e).max() / max(1.0, np.linalg.norm(r))
                worst = max(worst, err)
    print(name, "mirror e against scipy", worst)
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_the_reference_answer_is_stationary_and_feasible(oracle, case):
    """4: |e|_inf <= 2 sqrt(6) max(G_bound over the leg-step's six rows) on every stance leg-step, and summary[2] <= 1e-6."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    m = reference_case(oracle, case)["m"]
    worst = 0.0
    for k in range(nb):
        for i in range(h):
            for c in range(nc):
                if m["stance"][k, i, c]:
                    worst = max(worst, np.abs(m["resid"][k, i, c]).max() / (2.0 * np.sqrt(6.0) * leg_step_bound(m["G_bound"][k], i, c, nc)))
    print(name, "largest |e|_inf / bound", worst, "largest |e|_2", np.sqrt((m["resid"] ** 2).sum(axis=-1)).max(), "summary[2]", m["summary"][:, 2].max())
    assert worst <= 1.0, worst
    assert (m["summary"][:, 2] <= 1e-6).all(), m["summary"][:, 2].max()
    assert (m["lambda"] >= 0).all()


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_multipliers_agree_with_qpoases(oracle, case):
    """5: where the active normals have full column rank (numerical rank at 1e-9 = their number), |lambda - y| <= |N_A^+|_2 sqrt(6)
    max G_bound; the share of leg-steps with a non-empty active set that this leaves out is capped."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    d = reference_case(oracle, case)
    m, y = d["m"], d["y"]
    nonempty = left_out = 0
    worst = worst_abs = 0.0
    for k in range(nb):
        for i in range(h):
            for c in range(nc):
                if not m["stance"][k, i, c]:
                    assert (m["lambda"][k, i, c] == 0).all() and (m["resid"][k, i, c] == 0).all()
                    continue
                act = cm.active_set(m["slack"][k, i, c])
                inactive = [j for j in range(10) if j not in act]
                assert (m["lambda"][k, i, c, inactive] == 0).all()
                if not act:
                    continue
                nonempty += 1
                NA = m["N"][k][c][:, act]
                if np.linalg.matrix_rank(NA, tol=1e-9) < len(act):
                    left_out += 1
                    continue
                bound = np.linalg.norm(np.linalg.pinv(NA), 2) * np.sqrt(6.0) * leg_step_bound(m["G_bound"][k], i, c, nc)
                err = np.abs(m["lambda"][k, i, c] - y[k, i, c]).max()
                worst, worst_abs = max(worst, err / bound), max(worst_abs, err)
    print(name, "leg-steps with an active set", nonempty, "left out", left_out, "largest |lambda - y| / bound", worst, "absolute", worst_abs,
          "largest multiplier", y.max())
    assert nonempty > 0
    assert left_out <= LEFT_OUT_CAP[name] * nonempty, (left_out, nonempty)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_one_newton_moved_is_caught(oracle, shape):
    """6: 1 N moved between the step-0 Fz of the stance feet raises summary[0] of every instance >= 50 x."""
    name, gait, h, nb, nc, seed = shape
    d = reference_case(oracle, shape)
    un = records.unpack_records(d["rec"], h, nc)
    up = np.stack([cm.move_one_newton(d["u32"][k], un["gait"][k], h, nc) for k in range(nb)])
    mp = cm.certificate_records(oracle, d["rec"], h, nc, up)
    ratio = mp["summary"][:, 0] / d["m"]["summary"][:, 0]
    print(name, "summary[0] optimum max", d["m"]["summary"][:, 0].max(), "perturbed min", mp["summary"][:, 0].min(), "ratio min", ratio.min())
    assert (ratio >= 50.0).all(), ratio.min()


def test_nnls_corner_cases():
    """A dependent eight-column active set of rank 5, an empty one, NaN input: lambda >= 0, e = r - N lambda, and the loop ends."""
    rng = np.random.default_rng(3)
    B = rng.normal(size=(6, 5))
    N = np.zeros((6, 10))
    N[:, :8] = B @ rng.normal(size=(5, 8))
    r = N[:, :8] @ np.abs(rng.normal(size=8)) + 0.1 * rng.normal(size=6)
    lam, e = cm.nnls(N, r, list(range(8)))
    assert (lam >= 0).all() and (lam[8:] == 0).all() and np.count_nonzero(lam) <= 5
    np.testing.assert_allclose(e, r - N @ lam, atol=1e-12)
    assert (N[:, :8].T @ e <= 1e-9).all()  # the KKT condition of the projection
    lam, e = cm.nnls(N, r, [])
    assert (lam == 0).all() and (e == r).all()
    rn = r.copy()
    rn[2] = np.nan
    lam, e = cm.nnls(N, rn, list(range(8)))
    assert (lam >= 0).all() and np.isnan(e).any()


def test_penalty_rule():
    nan = np.nan
    summary = np.array([[1e-4, 0.0, 0.0, 9.0], [nan, 0.0, 0.0, 9.0], [1e-2, 1e-6, 2e-7, 9.0], [np.inf, 0.0, 0.0, 9.0]])
    np.testing.assert_array_equal(cm.penalty(summary, [nan] * 3), [0.0] * 4)
    np.testing.assert_array_equal(cm.penalty(summary, [1e-3, nan, nan], [7.0, 8.0, 9.0, 10.0]), [7.0, np.inf, np.inf, np.inf])
    np.testing.assert_array_equal(cm.penalty(summary, [nan, 1e-7, 1e-7]), [0.0, 0.0, np.inf, 0.0])
    np.testing.assert_array_equal(cm.penalty(summary, [0.0, nan, nan]), [np.inf] * 4)
