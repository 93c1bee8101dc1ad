"""The adjoint of the solve (hmpc_solve_adjoint, csrc/hmpc_adjoint.hip) and ``loss.backward()`` through a solve
(hector_simulation_amd/autograd.py).

The reference is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/adjoint_mirror.py), fed with the ORACLE's
binary32 assembly of each record, THE GPU'S OWN downloaded float32 forces and the same seed: no solver tolerance enters the comparison.
The GPU and the mirror run the same algorithm, so they must agree well inside the 1e-9 max(1, max|mirror|) that separates the mirror
from the dense frozen-set QP (tests/test_adjoint_mirror.py); the ratio is printed.  What the gradients are worth is then measured against
re-solves of perturbed records, within the bounds the CPU test derives from the reference's qpOASES."""
import ctypes as C

import numpy as np
import pytest

import adjoint_mirror as am
import certificate_mirror as cm
import feedback_mirror as fm
import prediction_mirror as pm
from hector_simulation_amd import interface, records, synthetic
from test_certificate_mirror import CASES, CASE_IDS, reference_case
from test_feedback_mirror import fd_case, mirror_case
from test_margins_mirror import PARAM_SET_0

pytestmark = pytest.mark.gpu
E_ARG = -1
GRADS = ("grad_x0", "grad_traj", "grad_weights", "grad_alpha", "dir")
# the gains' three small shapes, beside those of CASES (which hold h = 20 single support, three contacts at h = 10 and a walking gait);
# what the gait TABLE indexes (flight steps, swinging first contacts, a swinging hand, n = 0, the wide shape): tests/test_gpu_derived_irregular.py
SMALL = [("h1", "standing", 1, 8, 2, 201), ("h3", "walking", 3, 8, 2, 202), ("h11", "walking", 11, 8, 2, 203)]

_cache = {}


def _torch():
    import torch

    return torch


def _device(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def assert_same_bits(a, b, what=""):
    for key in am.KEYS:
        np.testing.assert_array_equal(a[key].view(np.uint64), b[key].view(np.uint64), err_msg=f"{what} {key}")


def adjoint_with(mpc, seed):
    """One adjoint launch of a solved handle under seed[b, h, U] (float64), downloaded."""
    t = _device(np.asarray(seed, dtype=np.float64))
    mpc.solve_adjoint(t.data_ptr())
    return mpc.download_adjoint()


def solved(rec, h, nc=2, prepare=None):
    """A handle with `rec` solved and downloaded (the safe pass has run): (mpc, forces, status)."""
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, rec.shape[0], contacts=nc)
    if prepare:
        prepare(mpc)
    mpc.upload(rec)
    mpc.solve()
    forces, status = mpc.download()
    return mpc, forces, status


def case_records(oracle, case):
    return reference_case(oracle, case)["rec"] if case in [c[1] for c in CASES] else pm.shape_records(case)[1]


def solved_case(oracle, case):
    """One solve + gains + adjoint (the seeds of the finite-difference tests) per case, and the numpy definition on the downloaded forces;
    shared by the tests, left unchanged."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _cache:
        rec = case_records(oracle, case)
        ell = am.seeds(nb, h, 6 * nc)
        mpc, forces, status = solved(rec, h, nc)
        mpc.feedback_gains()
        gains = mpc.download_gains()
        a = adjoint_with(mpc, ell)
        mpc.close()
        _cache[name] = dict(rec=rec, forces=forces, status=status, gains=gains, a=a, ell=ell, ref=am.adjoint_records(oracle, rec, h, nc, forces, ell))
    return _cache[name]


def mirror_error(a, ref, what=""):
    """The largest error of the five arrays against the mirror over MIRROR_TOL max(1, max|mirror|) per instance and output."""
    nb = a["dir"].shape[0]
    worst = 0.0
    for key in GRADS:
        assert a[key].shape == ref[key].shape, (what, key, a[key].shape, ref[key].shape)
        scale = np.maximum(1.0, np.abs(ref[key]).reshape(nb, -1).max(axis=1))
        worst = max(worst, float((np.abs(a[key] - ref[key]).reshape(nb, -1).max(axis=1) / scale).max()))
    return worst / am.MIRROR_TOL


def assert_is_the_definition(a, ref, h, nc, what=""):
    nb, U = a["dir"].shape[0], 6 * nc
    assert a["grad_x0"].shape == (nb, 13) and a["grad_traj"].shape == (nb, h, 12) and a["grad_weights"].shape == (nb, 12)
    assert a["grad_alpha"].shape == (nb, U) and a["dir"].shape == (nb, h, U) and a["summary"].shape == (nb, 2)
    ratio = mirror_error(a, ref, what)
    print(what, "largest error against the mirror / (1e-9 max(1, max|mirror|))", ratio, "max|dir|", a["summary"][:, 1].max(),
          "smallest pivot ratio", a["summary"][:, 0].min())
    assert ratio <= 1.0, (what, ratio)
    np.testing.assert_array_equal(a["summary"][:, 1].view(np.uint64), np.abs(a["dir"]).reshape(nb, -1).max(axis=1).view(np.uint64), err_msg=what)
    stance = ref["gains"]["stance"]
    for k in range(nb):
        for i in range(h):
            for c in range(nc):
                if not stance[k, i, c]:
                    assert (a["dir"][k, i, cm.cols(c, nc)] == 0).all(), (what, k, i, c)


# ------------------------------------------------------------------------------------------------ 1. the kernel is the definition
@pytest.mark.parametrize("case", [c[1] for c in CASES] + SMALL, ids=CASE_IDS + [s[0] for s in SMALL])
def test_adjoint_is_the_definition(oracle, case):
    name, h, nc = case[0], case[2], case[4]
    d = solved_case(oracle, case)
    assert_is_the_definition(d["a"], d["ref"], h, nc, name)
    np.testing.assert_array_equal(d["a"]["summary"][:, 0].view(np.uint64), d["gains"]["summary"][:, 0].view(np.uint64))
    if name in ("walking", "h3", "h11"):
        assert (~d["ref"]["gains"]["stance"][:, 0, :]).any()  # (a swing leg at step 0: its rows of dir were checked to be zeros)
    if name == "h1":
        assert d["a"]["grad_traj"].shape[1] == 1
    assert np.abs(d["a"]["dir"]).max() > 0.0 and np.abs(d["a"]["grad_x0"]).max() > 0.0


# ------------------------------------------------------------------------------------------------ 2. structure
def test_structure_zero_swing_additivity_and_a_nan_seed(oracle):
    case = CASES[1][1]  # walking
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    U = 6 * nc
    d = solved_case(oracle, case)
    stance = d["ref"]["gains"]["stance"]
    assert (~stance[:, 0, :]).any()
    mpc, forces, _ = solved(d["rec"], h, nc)
    np.testing.assert_array_equal(forces.view(np.uint32), d["forces"].view(np.uint32))
    z = adjoint_with(mpc, np.zeros((nb, h, U)))
    for key in GRADS:
        assert (z[key] == 0).all(), key
    assert (z["summary"][:, 1] == 0).all()
    np.testing.assert_array_equal(z["summary"][:, 0].view(np.uint64), d["a"]["summary"][:, 0].view(np.uint64))
    a = adjoint_with(mpc, d["ell"])
    assert_same_bits(a, d["a"], "the same seed on a second handle")
    # finite seed entries on swing contacts change no output bit
    rng = np.random.default_rng(7)
    moved = d["ell"].copy()
    n_swing = 0
    for k in range(nb):
        for i in range(h):
            for c in range(nc):
                if not stance[k, i, c]:
                    moved[k, i, cm.cols(c, nc)] = rng.uniform(-3.0, 3.0, 6)
                    n_swing += 1
    assert n_swing > 0
    assert_same_bits(adjoint_with(mpc, moved), d["a"], "seed entries on swing contacts")
    # the adjoints of a, b and a + b add up
    sa, sb = am.seeds(nb, h, U, rng_seed=11), am.seeds(nb, h, U, rng_seed=12)
    ga, gb, gab = adjoint_with(mpc, sa), adjoint_with(mpc, sb), adjoint_with(mpc, sa + sb)
    worst = 0.0
    for key in GRADS:
        scale = np.maximum(1.0, np.abs(gab[key]).reshape(nb, -1).max(axis=1))
        worst = max(worst, float((np.abs(ga[key] + gb[key] - gab[key]).reshape(nb, -1).max(axis=1) / scale).max()))
    print("additivity: largest |adj(a) + adj(b) - adj(a + b)| / (1e-9 max(1, max|value|))", worst / am.MIRROR_TOL)
    assert worst <= am.MIRROR_TOL, worst
    # a NaN in one instance's seed: the launch returns, every other instance keeps its bits
    bad = d["ell"].copy()
    stance_cols = [c for c in range(nc) if stance[3, 0, c]]
    bad[3, 0, cm.cols(stance_cols[0], nc)[2]] = np.nan
    n = adjoint_with(mpc, bad)
    mpc.close()
    others = np.arange(nb) != 3
    for key in am.KEYS:
        np.testing.assert_array_equal(n[key][others].view(np.uint64), d["a"][key][others].view(np.uint64), err_msg=key)
    assert np.isnan(n["dir"][3]).any() and n["summary"][3, 1] == np.inf


# ------------------------------------------------------------------------------------------------ 3. unit seeds, crafted forces
@pytest.mark.parametrize("case", [CASES[0][1], CASES[1][1], CASES[5][1], SMALL[2]], ids=["standing", "walking", "standing_3c", "h11"])
def test_unit_seeds_return_the_gpus_own_gains(oracle, case):
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    U = 6 * nc
    d = solved_case(oracle, case)
    mpc, _, _ = solved(d["rec"], h, nc)
    a = adjoint_with(mpc, am.unit_seeds(nb, h, U))
    mpc.close()
    g = d["gains"]
    worst = 0.0
    for k in range(nb):
        c = k % U
        bound = fm.MIRROR_TOL * max(1.0, np.abs(g["gain"][k]).max())
        worst = max(worst, np.abs(a["grad_x0"][k] - g["gain"][k][c]).max() / bound, np.abs(a["grad_traj"][k] - g["ref_gain"][k][:, c, :]).max() / bound)
    print(name, "unit seeds against the GPU's gains / (1e-9 max(1, max|K0|))", worst)
    assert worst <= 1.0, worst


def test_crafted_forces_an_unloaded_foot_and_an_interior_point(oracle):
    torch = _torch()
    shape = pm.SHAPES[0]
    name, gait, h, nb, nc, seed = shape
    rec = reference_case(oracle, shape)["rec"]
    U = 6 * nc
    ell = am.seeds(nb, h, U)
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.upload(rec)
    mpc.solve()
    forces, _ = mpc.download()
    # an unloaded stance foot at step 0: all six of contact 0 are 0, so rows 0-4, 6, 7, 8 are active, of rank 5
    unloaded = forces.copy().reshape(nb, h, U)
    unloaded[:, 0, cm.cols(0, nc)] = 0.0
    t_f.copy_(torch.from_numpy(unloaded.reshape(nb, -1)))
    torch.cuda.synchronize()
    a = adjoint_with(mpc, ell)
    ref = am.adjoint_records(oracle, rec, h, nc, unloaded.reshape(nb, -1), ell)
    for k in range(nb):
        assert sorted(ref["gains"]["active"][k][(0, 0)]) == [0, 1, 2, 3, 4, 6, 7, 8]
    assert_is_the_definition(a, ref, h, nc, "unloaded foot")
    # strictly inside every limit: 100 N of Fz on every contact, and the moment that puts row 4 in the middle of its window
    inside = np.zeros((nb, h, U), dtype=np.float32)
    for k in range(nb):
        Fc = ref["gains"]["Fc"][k].astype(np.float64)
        for c in range(nc):
            n4 = Fc[8 * c + 4, cm.cols(c, nc)]
            uc = np.array([0.0, 0.0, 100.0, 0.0, 0.0, 0.0])
            uc[3:] = n4[3:] * (0.005 - n4[:3] @ uc[:3]) / (n4[3:] @ n4[3:])
            inside[k, :, cm.cols(c, nc)] = uc.astype(np.float32)[:, None]
    t_f.copy_(torch.from_numpy(inside.reshape(nb, -1)))
    torch.cuda.synchronize()
    mpc.feedback_gains()
    g = mpc.download_gains()
    a = adjoint_with(mpc, ell)
    mpc.close()
    ref = am.adjoint_records(oracle, rec, h, nc, inside.reshape(nb, -1), ell)
    assert (ref["gains"]["slack"] > fm.ACT_TOL).all()
    assert (g["free_dims"] == U).all()
    assert_is_the_definition(a, ref, h, nc, "interior point")
    un = records.unpack_records(rec, h, nc)
    for k in range(nb):
        free = am.adjoint(ref["gains"]["Acd"][k], ref["gains"]["Bcd"][k], ref["gains"]["x0"][k], un["weights"][k], un["traj"][k], un["Alpha_K"][k],
                          inside[k], [np.eye(U)] * h, ell[k])["dir"]
        assert np.abs(a["dir"][k] - free).max() <= fm.MIRROR_TOL * max(1.0, np.abs(free).max()), k


# ------------------------------------------------------------------------------------------------ 4. a re-solve
@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_gradients_follow_a_re_solve(oracle, case):
    """fd_case's rec and rec2 (state and reference moved) and the weights / Alpha_K pair of the CPU test, solved on the GPU: on the kept
    instances the predicted change of l.u is within ADJ_FD (ADJ_FD_W) max(1, max|u|) of the re-solve's."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    d = solved_case(oracle, case)
    np.testing.assert_array_equal(d["rec"], mirror_case(oracle, case)["rec"])
    u1 = d["forces"].astype(np.float64).reshape(nb, h, -1)
    scale = np.maximum(1.0, np.abs(u1).reshape(nb, -1).max(axis=1))
    fd, fdw = fd_case(oracle, case), am.fd_weights_case(oracle, case, mirror_case(oracle, case))
    for what, pair, pred, bound in (("state and reference", fd, am.predicted_change(d["a"], dx=fd["dx"], dt=fd["dt"]), am.ADJ_FD),
                                    ("weights and Alpha_K", fdw, am.predicted_change(d["a"], dw=fdw["dw"], da=fdw["da"]), am.ADJ_FD_W)):
        mpc, f2, st2 = solved(pair["rec2"], h, nc)
        mpc.close()
        assert np.isin(interface.status_code(d["status"]), (0, 6)).all() and np.isin(interface.status_code(st2), (0, 6)).all()
        act = (d["ell"] * (f2.astype(np.float64).reshape(nb, h, -1) - u1)).reshape(nb, -1).sum(axis=1)
        err = np.abs(pred - act) / scale
        keep = pair["keep"]
        print(name, what, "kept", int(keep.sum()), "of", nb, "largest error / scale", float(err[keep].max()), "bound", bound, "l.u itself moved by",
              float(np.abs(act[keep]).max()), "error of the instances left out", float(err[~keep].max()) if (~keep).any() else 0.0)
        assert (err[keep] <= bound).all(), (name, what, err[keep].max())


# ------------------------------------------------------------------------------------------------ 5. constants
def test_params_and_instance_mu_reach_the_adjoint(oracle):
    shape = ("params", "walking", 10, 8, 2, 107)
    _, rec = pm.shape_records(shape)
    h, nc, nb = 10, 2, 8
    ell = am.seeds(nb, h, 6 * nc)

    def run(r, prepare=None):
        mpc, forces, status = solved(r, h, nc, prepare)
        a = adjoint_with(mpc, ell)
        mpc.close()
        return forces, status, a

    forces1, status1, a1 = run(rec, lambda mpc: mpc.set_params(**PARAM_SET_0))
    assert (interface.status_code(status1) == 0).all()
    try:
        oracle.set_params(**PARAM_SET_0)
        assert_is_the_definition(a1, am.adjoint_records(oracle, rec, h, nc, forces1, ell), h, nc, "params")
    finally:
        oracle.set_params()
    _, _, a0 = run(rec)
    assert np.abs(a1["grad_x0"] - a0["grad_x0"]).max() > 1e-3
    rec6 = reference_case(oracle, CASES[7][1])["rec"][:nb]
    mu = np.linspace(0.3, 1.4, nb).astype(np.float32)
    d_mu = _device(mu)
    forces, status, a = run(rec6, lambda mpc: mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu))
    assert np.isin(interface.status_code(status), (0, 6)).all(), status
    assert_is_the_definition(a, am.adjoint_records(oracle, rec6, h, nc, forces, ell, mu=mu), h, nc, "instance mu")
    _, _, a6 = run(rec6)
    assert np.abs(a["grad_x0"] - a6["grad_x0"]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 6. pure function
def test_pure_function_of_record_force_buffer_and_seed(oracle):
    torch = _torch()
    h, nb, nc, k = 10, 16, 2, 4
    U = 6 * nc
    base = reference_case(oracle, CASES[1][1])["rec"]
    rec = np.repeat(base[:nb // k], k, axis=0)  # groups of four records that share everything: a command sweep may solve them
    ell = am.seeds(nb, h, U)
    t_seed = _device(ell)
    mpc0, _, _ = solved(rec, h, nc)
    own = adjoint_with(mpc0, ell)
    mpc0.close()
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    shapes = dict(grad_x0=(nb, 13), grad_traj=(nb, h, 12), grad_weights=(nb, 12), grad_alpha=(nb, U), dir=(nb, h, U), summary=(nb, 2))
    mine = {key: torch.zeros(s, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_adjoint(*[mine[key].data_ptr() for key in am.KEYS], keepalive=mine)
    assert mpc.get_device_adjoint() == {key: mine[key].data_ptr() for key in am.KEYS}
    mpc.upload(rec)
    for order in (0, 1):
        mpc.set_dispatch_order(order)
        mpc.solve()
        mpc.solve_adjoint(t_seed.data_ptr())
        torch.cuda.synchronize()
        assert_same_bits({key: mine[key].cpu().numpy() for key in am.KEYS}, own, f"caller-owned buffers, dispatch order {order}")
        assert_same_bits(mpc.download_adjoint(), own, f"downloaded from the caller's buffers, dispatch order {order}")
    f_solve = t_f.cpu().numpy().copy()
    mpc.solve_command_sweep(k)
    mpc.solve_adjoint(t_seed.data_ptr())
    swept = mpc.download_adjoint()
    np.testing.assert_array_equal(t_f.cpu().numpy().view(np.uint32), f_solve.view(np.uint32))  # (same forces in ...)
    assert_same_bits(swept, own, "after a command sweep")  # (... same adjoint out)
    mpc.solve_adjoint(t_seed.data_ptr())
    assert_same_bits(mpc.download_adjoint(), own, "twice")
    mpc.close()
    # a device group's member against the plain handle
    grp = interface.DeviceGroup(synthetic.DT_MPC, h, synthetic.F_MAX, nb, [0, 0], transport="p2p")
    grp.upload(rec)
    grp.solve()
    grp.download()
    L = grp.L
    for i in range(grp.size):
        hd, _, lo, n, st = grp.member(i)
        t_part = _device(ell[lo:lo + n])
        assert L.hmpc_solve_adjoint(hd, C.c_void_p(t_part.data_ptr()), C.c_void_p(st)) == 0
        got = {key: np.zeros((n,) + shapes[key][1:]) for key in am.KEYS}
        assert L.hmpc_download_adjoint(hd, *[got[key].ctypes.data for key in am.KEYS]) == 0
        assert_same_bits(got, {key: own[key][lo:lo + n] for key in am.KEYS}, f"group member {i}")
    grp.close()


# ------------------------------------------------------------------------------------------------ 7. ordering
def test_ordering_errors_enqueue_nothing_and_leave_the_buffers_alone():
    torch = _torch()
    h, U = 10, 12
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    shapes = dict(grad_x0=(16, 13), grad_traj=(16, h, 12), grad_weights=(16, 12), grad_alpha=(16, U), dir=(16, h, U), summary=(16, 2))
    mine = {key: torch.full(s, -7.0, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    t_seed = _device(am.seeds(16, h, U))
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    ptrs = [mine[key].data_ptr() for key in am.KEYS]
    mpc.set_device_adjoint(*ptrs, keepalive=mine)
    host = [np.full(shapes[key], -9.0) for key in am.KEYS]
    seed_p = C.c_void_p(t_seed.data_ptr())

    def snapshot():
        torch.cuda.synchronize()
        return [mine[key].cpu().numpy().copy() for key in am.KEYS]

    def refused(what, before, solve_too, download_too=True):
        """download (and, where no solve of the batch exists, the launch) answers HMPC_E_ARG; nothing on the device or in the host moved"""
        if download_too:
            assert L.hmpc_download_adjoint(hd, *[a.ctypes.data for a in host]) == E_ARG, what
        if solve_too:
            assert L.hmpc_solve_adjoint(hd, seed_p, None) == E_ARG, what
        assert L.hmpc_solve_adjoint(hd, None, None) == E_ARG, what
        assert all((a == -9).all() for a in host), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    s0 = snapshot()
    refused("before a batch", s0, True, download_too=False)  # (a download of the empty batch copies nothing and is no error, as for the gains)
    assert L.hmpc_download_adjoint(hd, *[a.ctypes.data for a in host]) == 0 and all((a == -9).all() for a in host)
    mpc.upload(rec_a)
    refused("before a solve of the batch", s0, True)
    mpc.solve()
    refused("a solve, no adjoint from it", s0, False)
    forces_before, _ = mpc.download()
    mpc.feedback_gains()
    mpc.constraint_margins()
    gains_before, margins_before = mpc.download_gains(), mpc.download_margins()
    mpc.solve_adjoint(t_seed.data_ptr())
    first = mpc.download_adjoint()
    s1 = snapshot()
    assert (s1[0] != -7.0).all() and (s1[4] != -7.0).any()
    # an adjoint leaves the gains', the margins' and the force buffers' bits alone (and their results valid)
    g2, m2 = mpc.download_gains(), mpc.download_margins()
    for key in ("gain", "ref_gain", "summary"):
        np.testing.assert_array_equal(g2[key].view(np.uint64), gains_before[key].view(np.uint64))
    np.testing.assert_array_equal(m2["slack"].view(np.uint64), margins_before["slack"].view(np.uint64))
    np.testing.assert_array_equal(mpc.download()[0].view(np.uint32), forces_before.view(np.uint32))
    assert_same_bits(mpc.download_adjoint(), first, "after the other downloads")
    mpc.feedback_gains()  # (new gains: the adjoint is independent of them)
    assert_same_bits(mpc.download_adjoint(), first, "after new gains")
    mpc.set_device_adjoint(*ptrs, keepalive=mine)  # a retarget: whatever was computed went elsewhere
    refused("after a retarget", s1, False)
    mpc.solve_adjoint(t_seed.data_ptr())
    assert_same_bits(mpc.download_adjoint(), first, "after the retarget")
    mpc.upload(rec_b)
    refused("after a new upload", s1, True)
    mpc.solve()
    refused("after a solve of the new batch", s1, False)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.download_adjoint()
    mpc.solve()
    refused("after a second solve", snapshot(), False)
    mpc.solve_adjoint(t_seed.data_ptr())
    second = mpc.download_adjoint()
    mpc.close()
    mpc2, _, _ = solved(rec_b, h)
    fresh = adjoint_with(mpc2, am.seeds(16, h, U)[:8])
    mpc2.close()
    assert second["dir"].shape == (8, h, U)
    assert_same_bits(second, fresh, "against a fresh handle")


# ------------------------------------------------------------------------------------------------ 8. autograd
def test_backward_through_a_solve_is_the_adjoint():
    torch = _torch()
    from hector_simulation_amd.autograd import differentiable_solve

    h, nb, nc = 10, 8, 2
    U = 6 * nc
    fields = synthetic.make_batch(nb, h, "walking", seed=401, phase="random")
    rng = np.random.default_rng(9)
    c = torch.from_numpy(rng.uniform(-1.0, 1.0, (nb, h * U)).astype(np.float32)).cuda()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)

    def leaves(scale):
        return [torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1) * scale, requires_grad=True) for key in ("traj", "weights", "Alpha_K")]

    for scale in (1.0, 1.05):  # the second forward: another batch on the same handle, whose backward must not return the first one's gradients
        traj, weights, alpha_k = leaves(np.float32(scale) if scale != 1.0 else np.float32(1.0))
        forces = differentiable_solve(mpc, fields, traj, weights, alpha_k)
        assert forces.is_cuda and forces.dtype == torch.float32 and tuple(forces.shape) == (nb, h * U)
        np.testing.assert_array_equal(forces.detach().cpu().numpy().view(np.uint32), mpc.download()[0].view(np.uint32))
        loss = (forces * c).sum()
        loss.backward()
        torch.cuda.synchronize()
        got = mpc.download_adjoint()
        want = adjoint_with(mpc, c.cpu().numpy().astype(np.float64).reshape(nb, h, U))
        assert_same_bits(got, want, f"the adjoint behind backward, scale {scale}")
        np.testing.assert_array_equal(traj.grad.numpy().view(np.uint32), want["grad_traj"].reshape(nb, -1).astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(weights.grad.numpy().view(np.uint32), want["grad_weights"].astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(alpha_k.grad.numpy().view(np.uint32), want["grad_alpha"].astype(np.float32).view(np.uint32))
        assert np.abs(want["grad_traj"]).max() > 0.0
        if scale == 1.0:
            first = {key: v.copy() for key, v in want.items()}
            stale = forces
    assert np.abs(first["grad_traj"] - want["grad_traj"]).max() > 0.0  # (the second backward saw the second solve)
    # the first graph's forces are gone from the handle: its backward is refused, not answered with the second solve's; so is one behind
    # a solve made on the object directly
    old = differentiable_solve(mpc, fields, *leaves(np.float32(1.0)))
    differentiable_solve(mpc, fields, *leaves(np.float32(1.05)))
    with pytest.raises(RuntimeError, match="has solved another batch since this forward"):
        (old * c).sum().backward()
    old = differentiable_solve(mpc, fields, *leaves(np.float32(1.0)))
    mpc.solve()
    with pytest.raises(RuntimeError, match="has solved another batch since this forward"):
        (old * c).sum().backward()
    # float64 leaves on the handle's own device: the gradients are copies, not views of the handle's buffers -- two backwards without
    # zeroing accumulate to g1 + g2, and a set_device_adjoint of the user's in between does not leave backward reading dead buffers
    leaves64 = [torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1), dtype=torch.float64, device="cuda", requires_grad=True)
                for key in ("traj", "weights", "Alpha_K")]
    keys = ("grad_traj", "grad_weights", "grad_alpha")
    total = None
    for n, cn in enumerate((c, 0.5 * c + 0.25)):
        if n == 1:
            mpc.set_device_adjoint()  # back to the handle's own buffers, behind autograd's back
        (differentiable_solve(mpc, fields, *leaves64) * cn).sum().backward()
        torch.cuda.synchronize()
        g = adjoint_with(mpc, cn.cpu().numpy().astype(np.float64).reshape(nb, h, U))
        total = {key: (total[key] + g[key].reshape(nb, -1)) if total else g[key].reshape(nb, -1).copy() for key in keys}
        buffers = {t.data_ptr() for t in mpc._autograd_buffers.values()}
        for leaf, key in zip(leaves64, keys):
            assert leaf.grad.dtype == torch.float64 and leaf.grad.data_ptr() not in buffers, key
            np.testing.assert_array_equal(leaf.grad.cpu().numpy().view(np.uint64), total[key].view(np.uint64), err_msg=f"{key} after backward {n + 1}")
    assert np.abs(total["grad_traj"] - g["grad_traj"].reshape(nb, -1)).max() > 0.0  # (g1 + g2, not 2 g2)
    del stale
    mpc.close()
