"""The adjoint's definition (tests/adjoint_mirror.py) against what is independent of it: the dense frozen-set QP, the feedback gains'
mirror, and finite differences of the reference's qpOASES solves in the state, the reference trajectory, the weights and Alpha_K.  No GPU.
Shapes: test_certificate_mirror.CASES."""
import numpy as np
import pytest

import adjoint_mirror as am
import feedback_mirror as fm
from hector_simulation_amd import records
from test_certificate_mirror import CASES, CASE_IDS
from test_feedback_mirror import fd_case, mirror_case

_adj = {}


def adjoint_case(oracle, case):
    """The adjoint's mirror at qpOASES' forces rounded to binary32 under the seeds of the finite-difference tests, once per case."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _adj:
        base = mirror_case(oracle, case)
        ell = am.seeds(nb, h, 6 * nc)
        _adj[name] = dict(ell=ell, a=am.adjoint_records(oracle, base["rec"], h, nc, base["u32"], ell, gains=base["m"]))
    return _adj[name]


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_adjoint_is_the_dense_frozen_set_qp(oracle, case):
    """dir against -Zf (Zf' H Zf)^-1 Zf' l within MIRROR_TOL; the four gradients against central differences of l.u* within DENSE_FD."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    base, d = mirror_case(oracle, case), adjoint_case(oracle, case)
    m, a, ell = base["m"], d["a"], d["ell"]
    un = records.unpack_records(base["rec"], h, nc)
    e_dir, e_fd = 0.0, {}
    for k in range(nb):
        w, al = np.asarray(un["weights"][k], dtype=np.float64), np.asarray(un["Alpha_K"][k], dtype=np.float64)
        dm = am.DenseModel(m["Acd"][k], m["Bcd"][k], m["Z"][k], base["u32"][k]).anchor(m["x0"][k], un["traj"][k], w, al)
        dd = dm.direction(w, al, ell[k])
        e_dir = max(e_dir, np.abs(a["dir"][k] - dd).max() / max(1.0, np.abs(dd).max()))
        fd = dm.central_differences(m["x0"][k], un["traj"][k], w, al, ell[k])
        for key, want in zip(("grad_x0", "grad_traj", "grad_weights", "grad_alpha"), fd):
            e_fd[key] = max(e_fd.get(key, 0.0), np.abs(a[key][k] - want).max() / max(1.0, np.abs(want).max()))
    print(name, "dir against the dense form / max|dir|", e_dir, "central differences", e_fd, "DENSE_FD", am.DENSE_FD)
    assert e_dir <= am.MIRROR_TOL, e_dir
    assert max(e_fd.values()) <= am.DENSE_FD, e_fd
    np.testing.assert_array_equal(a["summary"][:, 0], m["summary"][:, 0])
    np.testing.assert_array_equal(a["summary"][:, 1], np.abs(a["dir"]).reshape(nb, -1).max(axis=1))
    for k in range(nb):  # rows of dir on swing contacts are exactly 0
        for i in range(h):
            for c in range(nc):
                if not m["stance"][k, i, c]:
                    assert (a["dir"][k, i, am.cm.cols(c, nc)] == 0).all(), (name, k, i, c)


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_unit_seeds_return_the_gains(oracle, case):
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    U = 6 * nc
    base = mirror_case(oracle, case)
    m = base["m"]
    a = am.adjoint_records(oracle, base["rec"], h, nc, base["u32"], am.unit_seeds(nb, h, U), gains=m)
    worst = 0.0
    for k in range(nb):
        c = k % U
        bound = fm.MIRROR_TOL * max(1.0, np.abs(m["gain"][k]).max())
        worst = max(worst, np.abs(a["grad_x0"][k] - m["gain"][k][c]).max() / bound, np.abs(a["grad_traj"][k] - m["ref_gain"][k][:, c, :]).max() / bound)
    print(name, "unit seeds against the gains / (MIRROR_TOL max(1, max|K0|))", worst)
    assert worst <= 1.0, worst
    z = am.adjoint_records(oracle, base["rec"], h, nc, base["u32"], np.zeros((nb, h, U)), gains=m)
    for key in am.KEYS[:5]:
        assert (z[key] == 0).all(), key


def test_state_and_reference_gradients_follow_the_reference(oracle):
    """Finite differences of qpOASES on the records of fd_case: E = |grad_x0.dx + sum grad_traj.dt - l.(u1 - u0)| / max(1, max|u0|)."""
    worst = 0.0
    for name, case in CASES:
        nb = case[3]
        d, a = fd_case(oracle, case), adjoint_case(oracle, case)
        pred = am.predicted_change(a["a"], dx=d["dx"], dt=d["dt"])
        act = (a["ell"] * (d["u1"] - d["u0"])).reshape(nb, -1).sum(axis=1)
        e = np.abs(pred - act) / np.maximum(1.0, np.abs(d["u0"]).reshape(nb, -1).max(axis=1))
        keep = d["keep"]
        print(name, "kept", int(keep.sum()), "of", nb, "E", float(e[keep].max()), "l.u moved by", float(np.abs(act[keep]).max()),
              "E of the instances left out", float(e[~keep].max()) if (~keep).any() else 0.0)
        assert (~keep).mean() <= fm.FD_LEFT_OUT_CAP and keep.any(), name
        worst = max(worst, float(e[keep].max()))
    print("E over all shapes", worst, "ADJ_FD", am.ADJ_FD)
    assert worst <= am.ADJ_FD, worst


def test_weight_and_alpha_gradients_follow_the_reference(oracle):
    worst, num, den = 0.0, 0.0, 0.0
    for name, case in CASES:
        nb = case[3]
        d, a = am.fd_weights_case(oracle, case, mirror_case(oracle, case)), adjoint_case(oracle, case)
        pred = am.predicted_change(a["a"], dw=d["dw"], da=d["da"])
        act = (a["ell"] * (d["u1"] - d["u0"])).reshape(nb, -1).sum(axis=1)
        e = np.abs(pred - act) / np.maximum(1.0, np.abs(d["u0"]).reshape(nb, -1).max(axis=1))
        keep = d["keep"]
        assert (~keep).mean() <= fm.FD_LEFT_OUT_CAP and keep.any(), name
        ratio = float(np.abs(pred - act)[keep].sum() / np.abs(act)[keep].sum())
        print(name, "s", d["s"], "kept", int(keep.sum()), "of", nb, "E", float(e[keep].max()), "sum|pred - act| / sum|act|", ratio)
        worst = max(worst, float(e[keep].max()))
        num, den = num + float(np.abs(pred - act)[keep].sum()), den + float(np.abs(act)[keep].sum())
    print("E over all shapes", worst, "ADJ_FD_W", am.ADJ_FD_W, "pooled sum|pred - act| / sum|act|", num / den)
    assert worst <= am.ADJ_FD_W, worst
    assert num / den < am.FD_W_POOLED, num / den
