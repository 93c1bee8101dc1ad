"""The feedback gains' definition (tests/feedback_mirror.py) against what is independent of it: the dense condensed form of the same
equality-constrained problem, the geometry of the active normals, and finite differences of the reference's qpOASES solves.  No GPU.
Shapes: test_certificate_mirror.CASES (the six of prediction_mirror.SHAPES plus hard_3x / hard_6x)."""
import numpy as np
import pytest

import certificate_mirror as cm
import feedback_mirror as fm
from test_certificate_mirror import CASES, CASE_IDS, reference_case

_cache = {}
_fd = {}


def mirror_case(oracle, case):
    """The mirror (and the dense form) on qpOASES' forces rounded to binary32, once per case; shared, left unchanged."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _cache:
        d = reference_case(oracle, case)
        _cache[name] = dict(rec=d["rec"], u32=d["u32"], m=fm.gains_records(oracle, d["rec"], h, nc, d["u32"], with_dense=True))
    return _cache[name]


def fd_case(oracle, case):
    """The perturbed records of a case, qpOASES on both, the kept instances and the first-order error; shared with
    tests/test_gpu_feedback.py, left unchanged.  The trajectory step is halved until at most FD_LEFT_OUT_CAP of the shape is left out."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name in _fd:
        return _fd[name]
    base = mirror_case(oracle, case)
    rec, m = base["rec"], base["m"]
    u0 = fm.qpoases_forces(oracle, rec, h, nc)
    traj_step = fm.FD_STEP
    for _ in range(6):
        rec2 = fm.perturbed_records(rec, h, nc, seed=1000 + case[5], traj_step=traj_step)
        u1 = fm.qpoases_forces(oracle, rec2, h, nc)
        m2 = fm.gains_records(oracle, rec2, h, nc, u1.astype(np.float32))
        keep = fm.same_active_sets(m["active"], m2["active"])
        if (~keep).mean() <= fm.FD_LEFT_OUT_CAP:
            break
        traj_step *= 0.5
    np.testing.assert_array_equal(m["Acd"].view(np.uint32), m2["Acd"].view(np.uint32))
    np.testing.assert_array_equal(m["Bcd"].view(np.uint32), m2["Bcd"].view(np.uint32))
    dx, dt = fm.deltas(oracle, rec, rec2, h, nc)
    lin = np.stack([fm.first_order(m["gain"][k], m["ref_gain"][k], dx[k], dt[k], np.zeros(6 * nc))[1] for k in range(nb)])
    err = np.abs((u1[:, 0] - u0[:, 0]) - lin).max(axis=1) / np.maximum(1.0, np.abs(u0).reshape(nb, -1).max(axis=1))
    _fd[name] = dict(rec=rec, rec2=rec2, keep=keep, err=err, traj_step=traj_step, u0=u0, u1=u1, dx=dx, dt=dt)
    return _fd[name]


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_riccati_gains_are_the_dense_condensed_form(oracle, case):
    name = case[0]
    m = mirror_case(oracle, case)["m"]
    scale = np.maximum(1.0, np.abs(m["dense_gain"]).reshape(len(m["gain"]), -1).max(axis=1))
    eg = np.abs(m["gain"] - m["dense_gain"]).reshape(len(scale), -1).max(axis=1) / scale
    scale_r = np.maximum(1.0, np.abs(m["dense_ref_gain"]).reshape(len(scale), -1).max(axis=1))
    er = np.abs(m["ref_gain"] - m["dense_ref_gain"]).reshape(len(scale), -1).max(axis=1) / scale_r
    print(name, "gain against dense / max|K|", eg.max(), "ref_gain", er.max(), "max|K0|", m["summary"][:, 1].max(), "smallest pivot ratio",
          m["summary"][:, 0].min())
    assert eg.max() <= fm.MIRROR_TOL and er.max() <= fm.MIRROR_TOL, (eg.max(), er.max())
    np.testing.assert_array_equal(m["summary"][:, 1], np.abs(m["gain"]).reshape(len(scale), -1).max(axis=1))


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_gains_stay_on_the_active_limits(oracle, case):
    """N_A' K_0 = 0 and N_A' ref_gain = 0 on every stance leg-step of step 0; swing rows exactly 0; free_dims = 6 - rank, summed."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    m = mirror_case(oracle, case)["m"]
    worst = 0.0
    for k in range(nb):
        bound = fm.MIRROR_TOL * max(1.0, np.abs(m["gain"][k]).max())
        bound_r = fm.MIRROR_TOL * max(1.0, np.abs(m["ref_gain"][k]).max())
        for i in range(h):
            want = 0
            for c in range(nc):
                if not m["stance"][k, i, c]:
                    if i == 0:
                        assert (m["gain"][k][cm.cols(c, nc)] == 0).all() and (m["ref_gain"][k][:, cm.cols(c, nc)] == 0).all()
                    continue
                NA = m["N"][k][c][:, m["active"][k][(i, c)]]
                want += 6 - (np.linalg.matrix_rank(NA, tol=1e-9) if NA.shape[1] else 0)
                if i == 0 and NA.shape[1]:
                    NAu = NA / np.linalg.norm(NA, axis=0)
                    e0 = np.abs(NAu.T @ m["gain"][k][cm.cols(c, nc)]).max()
                    e1 = max(np.abs(NAu.T @ m["ref_gain"][k][j][cm.cols(c, nc)]).max() for j in range(h))
                    worst = max(worst, e0 / bound, e1 / bound_r)
            assert m["free_dims"][k, i] == want, (name, k, i, m["free_dims"][k, i], want)
    print(name, "largest |N_A' gain| over its bound", worst)
    assert worst <= 1.0, worst


def test_first_order_update_follows_the_reference(oracle):
    """Finite differences of qpOASES against K_0 dx + sum ref_gain dt over the kept instances of all shapes."""
    worst = 0.0
    for name, case in CASES:
        d = fd_case(oracle, case)
        left = float((~d["keep"]).mean())
        e = float(d["err"][d["keep"]].max()) if d["keep"].any() else 0.0
        print(name, "left out", left, "trajectory step", d["traj_step"], "E", e, "E of the instances left out",
              float(d["err"][~d["keep"]].max()) if (~d["keep"]).any() else 0.0)
        assert left <= fm.FD_LEFT_OUT_CAP, (name, left)
        assert d["keep"].any(), name
        worst = max(worst, e)
    print("E over all shapes", worst, "FD_FORCE", fm.FD_FORCE)
    assert worst <= fm.FD_FORCE, worst


def test_free_directions_corner_cases():
    """Ten active limits of rank 6 leave nothing; an eight-row set of rank 5 leaves one direction orthogonal to all; none leaves R^6."""
    rng = np.random.default_rng(4)
    N = rng.normal(size=(6, 10))
    m, V = fm.free_directions(N, list(range(10)))
    assert m == 6
    B = rng.normal(size=(6, 5))
    N5 = np.zeros((6, 10))
    N5[:, :8] = B @ rng.normal(size=(5, 8))
    m, V = fm.free_directions(N5, list(range(8)))
    assert m == 5 and np.abs(N5[:, :8].T @ V[:, 5:]).max() <= 1e-12 * np.abs(N5).max()
    np.testing.assert_allclose(V.T @ V, np.eye(6), atol=1e-14)
    m, V = fm.free_directions(N, [])
    assert m == 0
    np.testing.assert_array_equal(V, np.eye(6))
