"""The model gradients' definition (tests/model_adjoint_mirror.py) against what is independent of it: central differences of l.u* in the
dense frozen-set QP under random moves of Acd and Bcd and under moves of r, mass and inertia pushed through a float64 restatement of
stage A2's B; the adjoint mirror's grad_x0.  No GPU.  Shapes: test_certificate_mirror.CASES."""
import numpy as np
import pytest

import adjoint_mirror as am
import model_adjoint_mirror as mam
from hector_simulation_amd import records, synthetic
from test_adjoint_mirror import adjoint_case
from test_certificate_mirror import CASES, CASE_IDS
from test_feedback_mirror import mirror_case

_madj = {}


def model_case(oracle, case):
    """The model gradients' mirror at qpOASES' forces rounded to binary32 and the adjoint mirror's dir, once per case; left unchanged."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _madj:
        base, d = mirror_case(oracle, case), adjoint_case(oracle, case)
        _madj[name] = mam.model_adjoint_records(oracle, base["rec"], h, nc, base["u32"], d["a"]["dir"], gains=base["m"])
    return _madj[name]


def moved_model(base, un, k):
    m = base["m"]
    w, al = np.asarray(un["weights"][k], dtype=np.float64), np.asarray(un["Alpha_K"][k], dtype=np.float64)
    return mam.MovedModel(m["Acd"][k], m["Bcd"][k], m["Z"][k], base["u32"][k], m["x0"][k], un["traj"][k], w, al)


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_grad_A_and_grad_B_are_the_dense_models_derivatives(oracle, case, step=mam.FD_DENSE_STEP):
    """Central differences of l.u* under random dA, dB against <G_A, dA> + <G_B, dB>, within DENSE_AB of max(1, |value|); dA alone and dB
    alone as well, so that neither hides behind the other.  (step: the central difference's; the irregular gait tables of
    tests/derived_irregular.py need a smaller one, see model_adjoint_mirror.FD_DENSE_STEP_IRREGULAR.)"""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    base, d, g = mirror_case(oracle, case), adjoint_case(oracle, case), model_case(oracle, case)
    un = records.unpack_records(base["rec"], h, nc)
    rng = np.random.default_rng(77)
    worst = 0.0
    for k in range(nb):
        mm = moved_model(base, un, k)
        # (dB in units of Bcd[9][0] = dt / mass ~ 3e-3, the smallest structural entry of B: l.u* is strongly curved in B -- Z'HZ is held by
        #  Alpha_K ~ 1e-6 in some directions --, and a step of 1e-6 in entries of size 1 would be 3e-4 of that entry: a truncation error
        #  of 1e-4 was measured there, which falls with the square of the step)
        dA, dB = rng.uniform(-1.0, 1.0, (13, 13)), rng.uniform(-1.0, 1.0, (13, 6 * nc)) * float(base["m"]["Bcd"][k][9, 0])
        for a, b in ((dA, dB), (dA, None), (None, dB)):
            want = mm.central(d["ell"][k], a, b, step=step)
            got = (0.0 if a is None else (g["grad_A"][k] * a).sum()) + (0.0 if b is None else (g["grad_B"][k] * b).sum())
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
    print(name, "directional derivatives in Acd, Bcd against central differences / max(1, |value|)", worst, "DENSE_AB", mam.DENSE_AB)
    assert worst <= mam.DENSE_AB, worst


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_grad_r_and_grad_params_are_the_dense_models_derivatives(oracle, case):
    """Central differences of l.u* under moves of every foot coordinate, the mass and every inertia entry, pushed through stage_a2_B
    (float64) and added to the binary32 Bcd, against grad_r / grad_params within DENSE_P of max(1, max|output|)."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    base, d, g = mirror_case(oracle, case), adjoint_case(oracle, case), model_case(oracle, case)
    un = records.unpack_records(base["rec"], h, nc)
    step = mam.FD_DENSE_STEP
    worst = {}
    for k in range(nb):
        mm = moved_model(base, un, k)
        R = mam.quat_to_R32(un["q"][k]).astype(np.float64)
        r0 = np.asarray(un["r"][k], dtype=np.float64).reshape(-1)
        theta0 = dict(r=r0, mass=np.array([mam.MASS]), inertia=np.asarray(mam.INERTIA, dtype=np.float64))

        def Bof(th):
            return mam.stage_a2_B(th["r"], R, nc, float(np.float32(synthetic.DT_MPC)), mass=float(th["mass"][0]), inertia=th["inertia"])

        fd = {}
        for key in ("r", "mass", "inertia"):
            fd[key] = np.zeros(theta0[key].size)
            for j in range(theta0[key].size):
                dl = step * max(1.0, abs(theta0[key][j])) if key != "inertia" else step * theta0[key][j]
                vals = []
                for sg in (1.0, -1.0):
                    th = {kk: v.copy() for kk, v in theta0.items()}
                    th[key][j] += sg * dl
                    vals.append(mm.value(d["ell"][k], None, Bof(th) - Bof(theta0)))
                fd[key][j] = (vals[0] - vals[1]) / (2.0 * dl)
        for key, got, want in (("grad_r", g["grad_r"][k].reshape(-1), fd["r"]), ("grad_mass", g["grad_params"][k][:1], fd["mass"]),
                               ("grad_inertia", g["grad_params"][k][1:], fd["inertia"])):
            worst[key] = max(worst.get(key, 0.0), np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    print(name, "grad_r, grad_mass, grad_inertia against central differences / max(1, max|output|)", worst, "DENSE_P", mam.DENSE_P)
    assert max(worst.values()) <= mam.DENSE_P, worst


@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_costate_zero_seed_and_swing_columns(oracle, case):
    """A' d_1 against the adjoint mirror's grad_x0 within MIRROR_TOL of its scale; a zero seed (dir = 0) gives zeros in everything but c_1; columns of G_B on a contact that is swing at every step are exactly 0."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    base, d, g = mirror_case(oracle, case), adjoint_case(oracle, case), model_case(oracle, case)
    m = base["m"]
    worst = 0.0
    for k in range(nb):
        gx0 = d["a"]["grad_x0"][k]
        worst = max(worst, np.abs(m["Acd"][k].astype(np.float64).T @ g["costate"][k, 1] - gx0).max() / max(1.0, np.abs(gx0).max()))
    print(name, "A' d_1 against grad_x0 / max(1, max|grad_x0|)", worst)
    assert worst <= mam.MIRROR_TOL, worst
    z = mam.model_adjoint_records(oracle, base["rec"], h, nc, base["u32"], np.zeros((nb, h, 6 * nc)), gains=m)
    for key in ("grad_A", "grad_B", "grad_r", "grad_params"):
        assert (z[key] == 0).all(), key
    assert (z["costate"][:, 1] == 0).all()
    for k in range(nb):
        for c in range(nc):
            if not m["stance"][k, :, c].any():
                assert (g["grad_B"][k][:, am.cm.cols(c, nc)] == 0).all(), (name, k, c)


@pytest.mark.parametrize("group", ["r", "params"])
def test_foot_and_payload_gradients_follow_the_reference(oracle, group):
    """Finite differences of qpOASES under moved feet (the record) and a moved mass and inertia (orc_set_params):
    E = |pred - l.(u1 - u0)| / max(1, max|u0|) on the kept instances within 2 x the measured E of the group, pooled ratio below FD_POOLED."""
    worst, num, den = 0.0, 0.0, 0.0
    bound = mam.MADJ_FD_R if group == "r" else mam.MADJ_FD_P
    for name, case in CASES:
        nb = case[3]
        fd, a, g = mam.fd_model_case(oracle, case, mirror_case(oracle, case)), adjoint_case(oracle, case), model_case(oracle, case)
        d = fd[group]
        pred = mam.predicted_change(g, dr=d["dr"]) if group == "r" else mam.predicted_change(g, dtheta=d["dtheta"])
        act = (a["ell"] * (d["u1"] - fd["u0"])).reshape(nb, -1).sum(axis=1)
        e = np.abs(pred - act) / np.maximum(1.0, np.abs(fd["u0"]).reshape(nb, -1).max(axis=1))
        keep = d["keep"]
        assert (~keep).mean() <= mam.fm.FD_LEFT_OUT_CAP and keep.any(), name
        ratio = float(np.abs(pred - act)[keep].sum() / np.abs(act)[keep].sum())
        print(name, group, "s", d["s"], "kept", int(keep.sum()), "of", nb, "E", float(e[keep].max()), "l.u moved by", float(np.abs(act[keep]).max()),
              "sum|pred - act| / sum|act|", ratio)
        worst = max(worst, float(e[keep].max()))
        num, den = num + float(np.abs(pred - act)[keep].sum()), den + float(np.abs(act)[keep].sum())
    print(group, "E over all shapes", worst, "bound", bound, "pooled sum|pred - act| / sum|act|", num / den)
    assert worst <= bound, worst
    assert num / den < mam.FD_POOLED, num / den
