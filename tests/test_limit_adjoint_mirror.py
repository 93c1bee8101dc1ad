"""The limit gradients' definition (tests/limit_adjoint_mirror.py) against what is independent of it: central differences of l.u* in the
dense frozen-set QP with its admitted rows as equalities, under random moves of the constraint block and the bounds and under moves of
mu, lt, lh and the caps pushed through a float64 restatement of the block; its structure; the certificate mirror's multipliers.  No GPU.
Shapes: test_certificate_mirror.CASES, and standing, walking and standing_3c once more at f_max = 40, where the Fz cap is active."""
import numpy as np
import pytest

import adjoint_mirror as am
import certificate_mirror as cm
import feedback_mirror as fm
import limit_adjoint_mirror as lam
from hector_simulation_amd import records, synthetic
from test_adjoint_mirror import adjoint_case
from test_certificate_mirror import CASES, case_records
from test_feedback_mirror import mirror_case

ALL_CASES = lam.all_cases(CASES)
ALL_IDS = [c[0] for c in ALL_CASES]
_cache = {}


def limit_case(oracle, entry):
    """Records, qpOASES' forces rounded to binary32 under the entry's f_max, the seeds of the finite-difference tests, the adjoint mirror's
    dir and the limit gradients' mirror on them, once per entry; shared with tests/test_gpu_limit_adjoint.py, left unchanged."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    if name not in _cache:
        if f_max == synthetic.F_MAX:
            base, d = mirror_case(oracle, case), adjoint_case(oracle, case)
            rec, u32, ell, dirs = base["rec"], base["u32"], d["ell"], d["a"]["dir"]
        else:
            rec = case_records(case)
            u32, ell = lam.reference_forces(oracle, rec, h, nc, f_max), am.seeds(nb, h, 6 * nc)
            dirs = lam.adjoint_dirs(oracle, rec, h, nc, u32, ell, f_max)
        _cache[name] = dict(rec=rec, u32=u32, ell=ell, dir=dirs, g=lam.limit_adjoint_records(oracle, rec, h, nc, u32, dirs, ell, f_max=f_max))
    return _cache[name]


def dense_limits(oracle, d, un, k, h, nc):
    """The dense frozen-set QP of instance k of a limit_case, on the oracle's assembly and the mirror's admitted rows."""
    if "asm" not in d:
        d["asm"] = [lam.mm.assemble(oracle, d["rec"][i], h, nc) for i in range(d["rec"].shape[0])]
    o, g = d["asm"][k], d["g"]
    return lam.DenseLimits(o["Acd"], o["Bcd"], o["x0"], un["traj"][k], np.asarray(un["weights"][k], dtype=np.float64),
                           np.asarray(un["Alpha_K"][k], dtype=np.float64), g["Fc"][k], d["u32"][k], g["rows"][k], nc, g["stance"][k])


@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_grad_Fc_and_grad_bound_are_the_dense_models_derivatives(oracle, entry, step=lam.FD_DENSE_STEP):
    """Central differences of l.u* under random dFc (inside each row's cols(c)) and random dbeta against <grad_Fc, dFc> + <grad_bound,
    dbeta>, within DENSE_FC of max(1, |value|); dFc alone and dbeta alone as well, so that neither hides behind the other.  (step: the central difference's; the irregular gait tables of
    tests/derived_irregular.py need a larger one, see limit_adjoint_mirror.FD_DENSE_STEP_IRREGULAR.)"""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = limit_case(oracle, entry)
    g = d["g"]
    lam.assert_covered(g["rows"], lam.groups_of(name, f_max), name)
    un = records.unpack_records(d["rec"], h, nc)
    rng = np.random.default_rng(91)
    worst = 0.0
    for k in range(nb):
        dl = dense_limits(oracle, d, un, k, h, nc)
        dFc, dbeta = lam.random_dFc(rng, nc), rng.uniform(-1.0, 1.0, (h, nc, 10))
        for a, b in ((dFc, dbeta), (dFc, None), (None, dbeta)):
            want = dl.central(d["ell"][k], a, b, step=step)
            got = (0.0 if a is None else (g["grad_Fc"][k] * a).sum()) + (0.0 if b is None else (g["grad_bound"][k] * b).sum())
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
    print(name, "directional derivatives in Fc, beta against central differences / max(1, |value|)", worst, "DENSE_FC", lam.DENSE_FC)
    assert worst <= lam.DENSE_FC, worst


@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_grad_limits_are_the_dense_models_derivatives(oracle, entry):
    """Central differences of l.u* under moves of mu, lt, lh (through constraint_block, float64) and of every cap (ub7 = cap x gait)
    against grad_limits, within DENSE_L of max(1, |value|)."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = limit_case(oracle, entry)
    g = d["g"]
    lam.assert_covered(g["rows"], lam.groups_of(name, f_max), name)
    un = records.unpack_records(d["rec"], h, nc)
    step = lam.FD_DENSE_STEP
    worst = {}
    for k in range(nb):
        dl = dense_limits(oracle, d, un, k, h, nc)
        F0 = np.asarray(g["Fc"][k], dtype=np.float64)
        gait = np.asarray(un["gait"][k]).reshape(h, nc).astype(np.float64)
        base = dict(mu=lam.MU, lt=lam.LT, lh=lam.LH)
        # (constraint_block at the base point is the binary32 block itself but for the rounding of mu = 2, which is exact)
        assert np.array_equal(lam.constraint_block(F0, nc, **base), F0)
        for idx, key in enumerate(("mu", "lt", "lh")):
            dth = step * base[key]
            vals = [dl.value(d["ell"][k], lam.constraint_block(F0, nc, **{**base, key: base[key] + sg * dth}) - F0) for sg in (1.0, -1.0)]
            want = (vals[0] - vals[1]) / (2.0 * dth)
            worst[key] = max(worst.get(key, 0.0), abs(g["grad_limits"][k, idx] - want) / max(1.0, abs(want)))
        for c in range(nc):
            dth = step * float(lam.caps_row(un, k, nc, f_max)[c])
            vals = []
            for sg in (1.0, -1.0):
                db = np.zeros((h, nc, 10))
                db[:, c, 9] = sg * dth * gait[:, c]
                vals.append(dl.value(d["ell"][k], None, db))
            want = (vals[0] - vals[1]) / (2.0 * dth)
            worst["cap"] = max(worst.get("cap", 0.0), abs(g["grad_limits"][k, 3 + c] - want) / max(1.0, abs(want)))
    print(name, "grad_limits against central differences / max(1, |value|)", worst, "DENSE_L", lam.DENSE_L)
    assert max(worst.values()) <= lam.DENSE_L, worst


def test_lone_cap_row_gives_one_half():
    """One stance leg-step with only the Fz cap active, dir = 0 and the seed e_Fz: nu_9 = -0.5 and dL/dub7 = +0.5 exactly."""
    h, nc = 1, 2
    U = 6 * nc
    Fc = np.zeros((8 * nc, U), dtype=np.float32)
    for c in range(nc):
        Fc[8 * c + 0, [3 * c, 3 * c + 2]] = (-2.0, 1.0)
        Fc[8 * c + 1, [3 * c, 3 * c + 2]] = (2.0, 1.0)
        Fc[8 * c + 2, [3 * c + 1, 3 * c + 2]] = (-2.0, 1.0)
        Fc[8 * c + 3, [3 * c + 1, 3 * c + 2]] = (2.0, 1.0)
        Fc[8 * c + 4, 3 * nc + 3 * c] = 1.0
        Fc[8 * c + 5, [3 * c + 2, 3 * nc + 3 * c + 1]] = (-0.09, 1.0)
        Fc[8 * c + 6, [3 * c + 2, 3 * nc + 3 * c + 1]] = (-0.06, -1.0)
        Fc[8 * c + 7, 3 * c + 2] = 2.0
    u = np.zeros((h, U), dtype=np.float32)
    u[0, 2], u[0, 6 + 0] = 20.0, 0.005  # contact 0: Fz at its cap of 20 (row 7 = 2 Fz = ub7 = 40), Mx inside its window
    seed = np.zeros((h, U))
    seed[0, 2] = 1.0
    gait = np.array([1, 0], dtype=np.uint8)  # contact 1 swings
    out = lam.limit_adjoint(np.eye(13), np.zeros((13, U)), np.zeros(13), np.ones(12), np.zeros(12 * h), np.ones(U), Fc, u, np.zeros((h, U)), seed,
                            gait, [np.float32(40.0)] * 2, nc)
    assert out["rows"] == {(0, 0): [9]}
    assert out["nu"][0, 0, 9] == -0.5 and out["grad_bound"][0, 0, 9] == 0.5 and out["grad_limits"][3] == 0.5
    assert (out["nu"][0, 1] == 0).all() and (out["lambda"][0, 1] == 0).all() and out["grad_limits"][4] == 0.0


@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_structure(oracle, entry):
    """A zero seed (dir = 0 with it) gives zero nu, grad_bound and the nu half of grad_Fc (all of it: the lambda half multiplies dir);
    swing leg-steps and rows not admitted are exact zeros; the admitted rows are free_directions' own; summary[1] is round-off on the
    adjoint mirror's own dir and large under another seed; summary[0] is the certificate's stationarity where its set is the admitted one."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = limit_case(oracle, entry)
    g = d["g"]
    lam.assert_covered(g["rows"], lam.groups_of(name, f_max), name)
    z = lam.limit_adjoint_records(oracle, d["rec"][:2], h, nc, d["u32"][:2], np.zeros((2, h, 6 * nc)), np.zeros((2, h, 6 * nc)), f_max=f_max)
    for key in ("nu", "grad_bound", "grad_Fc", "grad_limits"):
        assert (z[key] == 0).all(), key
    np.testing.assert_array_equal(z["lambda"], g["lambda"][:2])
    worst = 0.0
    for k in range(nb):
        N = [cm.normals(g["Fc"][k], c, nc) for c in range(nc)]
        for i in range(h):
            for c in range(nc):
                if not g["stance"][k, i, c]:
                    assert (g["lambda"][k, i, c] == 0).all() and (g["nu"][k, i, c] == 0).all() and (g["grad_bound"][k, i, c] == 0).all()
                    continue
                rows = g["rows"][k][(i, c)]
                out = [j for j in range(10) if j not in rows]
                assert (g["lambda"][k, i, c, out] == 0).all() and (g["nu"][k, i, c, out] == 0).all()
                active = cm.active_set(g["slack"][k, i, c], lam.ACT_TOL)
                m, V = fm.free_directions(N[c], active)
                rj, Q = lam.admitted(N[c], active)
                assert m == len(rj) and all(np.array_equal(V[:, a], Q[a]) for a in range(m)), (name, k, i, c)
        scale = max(1.0, np.abs(g["rho"][k]).max())
        worst = max(worst, g["summary"][k, 1] / scale)
        outside = np.ones(6 * nc, dtype=bool)
        for c in range(nc):
            outside[:] = True
            outside[cm.cols(c, nc)] = False
            assert (g["grad_Fc"][k][8 * c:8 * c + 8][:, outside] == 0).all()
    print(name, "summary[1] / max(1, max|rho|) on the adjoint mirror's own dir", worst, "MIRROR_TOL", lam.MIRROR_TOL)
    assert worst <= lam.MIRROR_TOL, worst
    other = lam.limit_adjoint_records(oracle, d["rec"][:2], h, nc, d["u32"][:2], d["dir"][:2], d["ell"][:2][::-1] * 2.0, f_max=f_max)
    assert (other["summary"][:, 1] > 1e3 * lam.MIRROR_TOL * np.maximum(1.0, np.abs(other["rho"]).reshape(2, -1).max(axis=1))).all()


@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_lambda_is_the_certificates_where_its_set_is_the_admitted_one(oracle, entry):
    """lambda against the certificate mirror's NNLS lambda on every stance leg-step where that one is positive on exactly the admitted
    rows: two solutions of the same least-squares problem, within MIRROR_TOL of max(1, max|lambda|)."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = limit_case(oracle, entry)
    g = d["g"]
    worst, compared = 0.0, 0
    for k in range(nb):
        for (i, c), rows in g["rows"][k].items():
            N = cm.normals(g["Fc"][k], c, nc)
            ln, _ = cm.nnls(N, g["grad"][k, i, cm.cols(c, nc)], cm.active_set(g["slack"][k, i, c], lam.ACT_TOL))
            if rows and [j for j in range(10) if ln[j] > 0.0] == rows:
                compared += 1
                worst = max(worst, np.abs(ln - g["lambda"][k, i, c]).max() / max(1.0, np.abs(ln).max()))
    print(name, "leg-steps compared", compared, "lambda against the certificate's NNLS / max(1, max|lambda|)", worst)
    assert compared > 0 and worst <= lam.MIRROR_TOL, (compared, worst)


@pytest.mark.parametrize("group", lam.GROUPS)
def test_limit_gradients_follow_the_reference(oracle, group):
    """Finite differences of qpOASES under a moved mu, lt, lh (orc_set_params) and a moved f_max, on the batches that cover the group:
    E = |pred - l.(u1 - u0)| / max(1, max|u0|) on the kept instances within 2 x the measured E of the group, pooled ratio below FD_POOLED."""
    worst, num, den, ran = 0.0, 0.0, 0.0, 0
    for entry in ALL_CASES:
        name, case, f_max = entry
        nb = case[3]
        if group not in lam.groups_of(name, f_max):
            continue
        d = limit_case(oracle, entry)
        lam.assert_covered(d["g"]["rows"], (group,), name)
        fd = lam.fd_limits_entry(oracle, entry, d)
        m = fd[group]
        pred = lam.predicted_change(d["g"], group, m["dtheta"])
        act = (d["ell"] * (m["u1"] - fd["u0"])).reshape(nb, -1).sum(axis=1)
        e = np.abs(pred - act) / np.maximum(1.0, np.abs(fd["u0"]).reshape(nb, -1).max(axis=1))
        keep = m["keep"]
        assert (~keep).mean() <= fm.FD_LEFT_OUT_CAP and keep.any(), (name, group, float((~keep).mean()))
        ratio = float(np.abs(pred - act)[keep].sum() / np.abs(act)[keep].sum())
        print(name, group, "s", m["s"], "kept", int(keep.sum()), "of", nb, "E", float(e[keep].max()), "l.u moved by", float(np.abs(act[keep]).max()),
              "sum|pred - act| / sum|act|", ratio)
        worst = max(worst, float(e[keep].max()))
        num, den, ran = num + float(np.abs(pred - act)[keep].sum()), den + float(np.abs(act)[keep].sum()), ran + 1
    print(group, "batches", ran, "E over all batches", worst, "bound", lam.LADJ_FD[group], "pooled sum|pred - act| / sum|act|", num / den)
    assert ran >= 3 and worst <= lam.LADJ_FD[group], worst
    assert num / den < lam.FD_POOLED, num / den
