"""The model gradients of the solve (hmpc_adjoint_model, csrc/hmpc_model_adjoint.hip) and ``loss.backward()`` into the foot positions
(hector_simulation_amd/autograd.py).

The reference is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/model_adjoint_mirror.py), fed with the
ORACLE's binary32 assembly of each record, THE GPU'S OWN downloaded float32 forces and THE GPU'S OWN dir: no solver tolerance enters the
comparison.  The GPU and the mirror run the same algorithm and differ by binary64 round-off alone, so they must agree within the
MIRROR_TOL = 1e-9 max(1, max|mirror|) that the adjoint's test uses -- two orders below DENSE_AB, which separates the mirror from the dense
model's central differences (tests/test_model_adjoint_mirror.py); the ratio is printed.  What the gradients are worth is then measured
against re-solves with moved feet, mass and inertia, within the bounds the CPU test derives from the reference's qpOASES."""
import ctypes as C

import numpy as np
import pytest

import adjoint_mirror as am
import certificate_mirror as cm
import model_adjoint_mirror as mam
import prediction_mirror as pm
from hector_simulation_amd import interface, records, synthetic
from test_certificate_mirror import CASES, CASE_IDS, reference_case
from test_feedback_mirror import mirror_case
from test_gpu_adjoint import SMALL, _device, _torch, case_records, solved
from test_margins_mirror import PARAM_SET_0

pytestmark = pytest.mark.gpu
E_ARG = -1
PARAM_SET_B = dict(mass=7.3, inertia=(0.45, 0.48, 0.11), mu=1.1, lt=0.09, lh=0.06, gravity=9.81)

_cache = {}


def same_bits(a, b, what=""):
    for key in mam.KEYS:
        np.testing.assert_array_equal(a[key].view(np.uint64), b[key].view(np.uint64), err_msg=f"{what} {key}")


def gradients_with(mpc, seed):
    """One adjoint and one model launch of a solved handle under seed[b, h, U] (float64), both downloaded: (adjoint, model)."""
    t = _device(np.asarray(seed, dtype=np.float64))
    mpc.solve_adjoint(t.data_ptr())
    mpc.adjoint_model()
    return mpc.download_adjoint(), mpc.download_adjoint_model()


def solved_case(oracle, case):
    """One solve + adjoint + model gradients per case (the seeds of the finite-difference tests) and the numpy definition on the downloaded
    forces and dir; shared by the tests, left unchanged."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name not in _cache:
        rec = case_records(oracle, case)
        ell = am.seeds(nb, h, 6 * nc)
        mpc, forces, status = solved(rec, h, nc)
        a, g = gradients_with(mpc, ell)
        mpc.close()
        gains = mam.fm.gains_records(oracle, rec, h, nc, forces)
        _cache[name] = dict(rec=rec, forces=forces, status=status, a=a, g=g, ell=ell, gains=gains,
                            ref=mam.model_adjoint_records(oracle, rec, h, nc, forces, a["dir"], gains=gains))
    return _cache[name]


def mirror_error(g, ref):
    nb = g["grad_A"].shape[0]
    worst = 0.0
    for key in mam.KEYS:
        assert g[key].shape == ref[key].shape, (key, g[key].shape, ref[key].shape)
        scale = np.maximum(1.0, np.abs(ref[key]).reshape(nb, -1).max(axis=1))
        worst = max(worst, float((np.abs(g[key] - ref[key]).reshape(nb, -1).max(axis=1) / scale).max()))
    return worst / mam.MIRROR_TOL


def assert_is_the_definition(g, ref, a, gains, h, nc, what=""):
    nb, U = g["grad_A"].shape[0], 6 * nc
    assert g["grad_A"].shape == (nb, 13, 13) and g["grad_B"].shape == (nb, 13, U) and g["grad_r"].shape == (nb, 3, nc)
    assert g["grad_params"].shape == (nb, 4) and g["costate"].shape == (nb, 2, 13)
    ratio = mirror_error(g, ref)
    worst = 0.0
    for k in range(nb):  # A' d_1 is the GPU's own grad_x0
        gx0 = a["grad_x0"][k]
        worst = max(worst, np.abs(gains["Acd"][k].astype(np.float64).T @ g["costate"][k, 1] - gx0).max() / max(1.0, np.abs(gx0).max()))
    print(what, "largest error against the mirror / (1e-9 max(1, max|mirror|))", ratio, "A' d_1 against grad_x0 / (1e-9 max(1, max|grad_x0|))",
          worst / mam.MIRROR_TOL, "max|grad_r|", np.abs(g["grad_r"]).max(), "max|grad_params|", np.abs(g["grad_params"]).max())
    assert ratio <= 1.0, (what, ratio)
    assert worst <= mam.MIRROR_TOL, (what, worst)
    stance = gains["stance"]
    for k in range(nb):
        for c in range(nc):
            if not stance[k, :, c].any():
                assert (g["grad_B"][k][:, cm.cols(c, nc)] == 0).all(), (what, k, c)


# ------------------------------------------------------------------------------------------------ 1. the kernel is the definition
@pytest.mark.parametrize("case", [c[1] for c in CASES] + SMALL, ids=CASE_IDS + [s[0] for s in SMALL])
def test_model_adjoint_is_the_definition(oracle, case):
    name, h, nc = case[0], case[2], case[4]
    d = solved_case(oracle, case)
    assert_is_the_definition(d["g"], d["ref"], d["a"], d["gains"], h, nc, name)
    assert np.abs(d["g"]["grad_r"]).max() > 0.0 and np.abs(d["g"]["grad_params"]).min(axis=0).max() > 0.0


def test_a_zero_seed_gives_zeros(oracle):
    case = CASES[1][1]
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    d = solved_case(oracle, case)
    mpc, _, _ = solved(d["rec"], h, nc)
    _, z = gradients_with(mpc, np.zeros((nb, h, 6 * nc)))
    _, again = gradients_with(mpc, d["ell"])
    mpc.close()
    for key in ("grad_A", "grad_B", "grad_r", "grad_params"):
        assert (z[key] == 0).all(), key
    assert (z["costate"][:, 1] == 0).all()
    np.testing.assert_array_equal(z["costate"][:, 0].view(np.uint64), d["g"]["costate"][:, 0].view(np.uint64))  # (c_1 knows no seed)
    same_bits(again, d["g"], "the same seed on a second handle")


# ------------------------------------------------------------------------------------------------ 2. constants
def test_params_and_instance_mu_reach_the_model_gradients(oracle):
    shape = ("params", "walking", 10, 8, 2, 107)
    _, rec = pm.shape_records(shape)
    h, nc, nb = 10, 2, 8
    ell = am.seeds(nb, h, 6 * nc)

    def run(r, prepare=None):
        mpc, forces, status = solved(r, h, nc, prepare)
        a, g = gradients_with(mpc, ell)
        mpc.close()
        return forces, status, a, g

    _, _, _, g0 = run(rec)
    for ps in (PARAM_SET_0, PARAM_SET_B):
        forces1, status1, a1, g1 = run(rec, lambda mpc: mpc.set_params(**ps))
        assert np.isin(interface.status_code(status1), (0, 6)).all(), status1
        try:
            oracle.set_params(**ps)
            gains = mam.fm.gains_records(oracle, rec, h, nc, forces1)
            ref = mam.model_adjoint_records(oracle, rec, h, nc, forces1, a1["dir"], gains=gains, mass=float(np.float32(ps["mass"])))
        finally:
            oracle.set_params()
        assert_is_the_definition(g1, ref, a1, gains, h, nc, f"params mass {ps['mass']}")
        assert np.abs(g1["grad_params"] - g0["grad_params"]).max() > 1e-6
    rec6 = reference_case(oracle, CASES[7][1])["rec"][:nb]
    mu = np.linspace(0.3, 1.4, nb).astype(np.float32)
    d_mu = _device(mu)
    forces, status, a, g = run(rec6, lambda mpc: mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu))
    assert np.isin(interface.status_code(status), (0, 6)).all(), status
    gains = mam.fm.gains_records(oracle, rec6, h, nc, forces, mu=mu)
    assert_is_the_definition(g, mam.model_adjoint_records(oracle, rec6, h, nc, forces, a["dir"], gains=gains), a, gains, h, nc, "instance mu")
    _, _, _, g6 = run(rec6)
    assert np.abs(g["grad_r"] - g6["grad_r"]).max() > 0.0


# ------------------------------------------------------------------------------------------------ 3. pure function
def test_pure_function_of_record_force_buffer_and_dir(oracle):
    torch = _torch()
    h, nb, nc, k = 10, 16, 2, 4
    U = 6 * nc
    base = reference_case(oracle, CASES[1][1])["rec"]
    rec = np.repeat(base[:nb // k], k, axis=0)  # groups of four records that share everything: a command sweep may solve them
    ell = am.seeds(nb, h, U)
    t_seed = _device(ell)
    mpc0, _, _ = solved(rec, h, nc)
    _, own = gradients_with(mpc0, ell)
    assert all(v != 0 for v in mpc0.get_device_adjoint_model().values())
    mpc0.close()
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    shapes = dict(grad_A=(nb, 13, 13), grad_B=(nb, 13, U), grad_r=(nb, 3, nc), grad_params=(nb, 4), costate=(nb, 2, 13))
    mine = {key: torch.zeros(s, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_adjoint_model(*[mine[key].data_ptr() for key in mam.KEYS], keepalive=mine)
    assert mpc.get_device_adjoint_model() == {key: mine[key].data_ptr() for key in mam.KEYS}
    mpc.upload(rec)
    for order in (0, 1):
        mpc.set_dispatch_order(order)
        mpc.solve()
        mpc.solve_adjoint(t_seed.data_ptr())
        mpc.adjoint_model()
        torch.cuda.synchronize()
        same_bits({key: mine[key].cpu().numpy() for key in mam.KEYS}, own, f"caller-owned buffers, dispatch order {order}")
        same_bits(mpc.download_adjoint_model(), own, f"downloaded from the caller's buffers, dispatch order {order}")
    mpc.solve_command_sweep(k)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_model()
    same_bits(mpc.download_adjoint_model(), own, "after a command sweep")
    mpc.adjoint_model()
    same_bits(mpc.download_adjoint_model(), own, "twice")
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
        assert L.hmpc_adjoint_model(hd, C.c_void_p(st)) == E_ARG  # (no adjoint yet)
        assert L.hmpc_solve_adjoint(hd, C.c_void_p(t_part.data_ptr()), C.c_void_p(st)) == 0
        assert L.hmpc_adjoint_model(hd, C.c_void_p(st)) == 0
        got = {key: np.zeros((n,) + shapes[key][1:]) for key in mam.KEYS}
        assert L.hmpc_download_adjoint_model(hd, *[got[key].ctypes.data for key in mam.KEYS]) == 0
        same_bits(got, {key: own[key][lo:lo + n] for key in mam.KEYS}, f"group member {i}")
    grp.close()


# ------------------------------------------------------------------------------------------------ 4. ordering
def test_ordering_errors_enqueue_nothing_and_leave_the_buffers_alone():
    torch = _torch()
    h, U, nc = 10, 12, 2
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    shapes = dict(grad_A=(16, 13, 13), grad_B=(16, 13, U), grad_r=(16, 3, nc), grad_params=(16, 4), costate=(16, 2, 13))
    mine = {key: torch.full(s, -7.0, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    t_seed = _device(am.seeds(16, h, U))
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    ptrs = [mine[key].data_ptr() for key in mam.KEYS]
    mpc.set_device_adjoint_model(*ptrs, keepalive=mine)
    host = [np.full(shapes[key], -9.0) for key in mam.KEYS]

    def snapshot():
        torch.cuda.synchronize()
        return [mine[key].cpu().numpy().copy() for key in mam.KEYS]

    def refused(what, before, launch_too, download_too=True):
        """the download (and, where no adjoint of the last solve exists, the launch) answers HMPC_E_ARG; nothing on the device or in the host moved"""
        if download_too:
            assert L.hmpc_download_adjoint_model(hd, *[a.ctypes.data for a in host]) == E_ARG, what
        if launch_too:
            assert L.hmpc_adjoint_model(hd, None) == E_ARG, what
        assert all((a == -9).all() for a in host), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    s0 = snapshot()
    refused("before a batch", s0, True, download_too=False)  # (a download of the empty batch copies nothing and is no error, as for the adjoint)
    assert L.hmpc_download_adjoint_model(hd, *[a.ctypes.data for a in host]) == 0 and all((a == -9).all() for a in host)
    mpc.upload(rec_a)
    refused("before a solve of the batch", s0, True)
    mpc.solve()
    refused("a solve, no adjoint from it", s0, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    adj_before = mpc.download_adjoint()
    refused("an adjoint, no model gradients from it", s0, False)
    mpc.adjoint_model()
    first = mpc.download_adjoint_model()
    s1 = snapshot()
    assert (s1[0] != -7.0).all()
    after = mpc.download_adjoint()  # the model launch leaves the adjoint's bits alone (and its results valid)
    for key in am.KEYS:
        np.testing.assert_array_equal(after[key].view(np.uint64), adj_before[key].view(np.uint64), err_msg=key)
    same_bits(mpc.download_adjoint_model(), first, "after the other download")
    mpc.solve_adjoint(t_seed.data_ptr())  # a new adjoint (a new seed, for all the handle knows)
    refused("after a new adjoint", s1, False)
    mpc.adjoint_model()
    same_bits(mpc.download_adjoint_model(), first, "after the new adjoint")
    mpc.set_device_adjoint_model(*ptrs, keepalive=mine)  # its own retarget: whatever was computed went elsewhere
    refused("after a retarget", s1, False)
    mpc.adjoint_model()
    same_bits(mpc.download_adjoint_model(), first, "after the retarget")
    mpc.set_device_adjoint()  # the adjoint's retarget: dir is no longer where the launch would read it
    refused("after the adjoint's retarget", s1, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_model()
    same_bits(mpc.download_adjoint_model(), first, "after the adjoint's retarget and a new adjoint")
    mpc.upload(rec_b)
    refused("after a new upload", s1, True)
    mpc.solve()
    refused("after a solve of the new batch", s1, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_model()
    mpc.download_adjoint_model()
    mpc.solve()
    refused("after a second solve", snapshot(), True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_model()
    second = mpc.download_adjoint_model()
    mpc.close()
    mpc2, _, _ = solved(rec_b, h)
    _, fresh = gradients_with(mpc2, am.seeds(16, h, U)[:8])
    mpc2.close()
    assert second["grad_r"].shape == (8, 3, nc)
    same_bits(second, fresh, "against a fresh handle")


# ------------------------------------------------------------------------------------------------ 5. autograd
def test_backward_returns_grad_r_and_leaves_the_old_gradients_alone():
    torch = _torch()
    from hector_simulation_amd.autograd import differentiable_solve

    h, nb, nc = 10, 8, 2
    U = 6 * nc
    fields = synthetic.make_batch(nb, h, "walking", seed=401, phase="random")
    rng = np.random.default_rng(9)
    c = torch.from_numpy(rng.uniform(-1.0, 1.0, (nb, h * U)).astype(np.float32)).cuda()
    seed = c.cpu().numpy().astype(np.float64).reshape(nb, h, U)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)

    def leaves():
        return [torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1), requires_grad=True) for key in ("traj", "weights", "Alpha_K")]

    # r = None: the three old gradients, bit for bit the adjoint's; no model launch (nothing to download)
    old = leaves()
    (differentiable_solve(mpc, fields, *old) * c).sum().backward()
    torch.cuda.synchronize()
    assert mpc.L.hmpc_download_adjoint_model(mpc.h, *[None] * 5) == E_ARG
    want_a, want_g = gradients_with(mpc, seed)
    for leaf, key in zip(old, ("grad_traj", "grad_weights", "grad_alpha")):
        np.testing.assert_array_equal(leaf.grad.numpy().view(np.uint32), want_a[key].reshape(nb, -1).astype(np.float32).view(np.uint32), err_msg=key)
    # r given as the fields' own values: the same forces, the same three gradients, and grad_r
    new = leaves()
    r = torch.tensor(np.asarray(fields["r"], dtype=np.float32).reshape(nb, -1), requires_grad=True)
    forces = differentiable_solve(mpc, fields, *new, r)
    np.testing.assert_array_equal(forces.detach().cpu().numpy().view(np.uint32), mpc.download()[0].view(np.uint32))
    (forces * c).sum().backward()
    torch.cuda.synchronize()
    same_bits(mpc.download_adjoint_model(), want_g, "the model gradients behind backward")
    for a, b in zip(old, new):
        np.testing.assert_array_equal(a.grad.numpy().view(np.uint32), b.grad.numpy().view(np.uint32))
    assert tuple(r.grad.shape) == (nb, 3 * nc)
    np.testing.assert_array_equal(r.grad.numpy().view(np.uint32), want_g["grad_r"].reshape(nb, -1).astype(np.float32).view(np.uint32))
    assert np.abs(want_g["grad_r"]).max() > 0.0
    # moved feet are substituted into the records
    moved = torch.tensor(np.asarray(fields["r"], dtype=np.float32).reshape(nb, -1) + np.float32(0.01), requires_grad=True)
    f2 = differentiable_solve(mpc, fields, *leaves(), moved)
    assert np.abs(f2.detach().cpu().numpy() - forces.detach().cpu().numpy()).max() > 0.0
    # float64 r on the handle's own device: the gradient is a copy, not a view of the handle's buffer; the generation guard stays
    r64 = torch.tensor(np.asarray(fields["r"], dtype=np.float32).reshape(nb, -1), dtype=torch.float64, device="cuda", requires_grad=True)
    (differentiable_solve(mpc, fields, *leaves(), r64) * c).sum().backward()
    torch.cuda.synchronize()
    assert r64.grad.data_ptr() not in {t.data_ptr() for t in mpc._autograd_model_buffers.values()}
    np.testing.assert_array_equal(r64.grad.cpu().numpy().view(np.uint64), want_g["grad_r"].reshape(nb, -1).view(np.uint64))
    stale = differentiable_solve(mpc, fields, *leaves(), r64)
    mpc.solve()
    with pytest.raises(RuntimeError, match="has solved another batch since this forward"):
        (stale * c).sum().backward()
    mpc.close()


# ------------------------------------------------------------------------------------------------ 6. a re-solve
@pytest.mark.parametrize("case", [c[1] for c in CASES], ids=CASE_IDS)
def test_gradients_follow_a_re_solve(oracle, case):
    """fd_model_case's moved feet and moved mass / inertia of the CPU test, solved on the GPU: on the kept instances the predicted change
    of l.u is within MADJ_FD_R (MADJ_FD_P) max(1, max|u|) of the re-solve's."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    d = solved_case(oracle, case)
    np.testing.assert_array_equal(d["rec"], mirror_case(oracle, case)["rec"])
    u1 = d["forces"].astype(np.float64).reshape(nb, h, -1)
    scale = np.maximum(1.0, np.abs(u1).reshape(nb, -1).max(axis=1))
    fd = mam.fd_model_case(oracle, case, mirror_case(oracle, case))
    for what, pair, rec2, prepare, pred, bound in (
            ("feet", fd["r"], fd["r"]["rec2"], None, mam.predicted_change(d["g"], dr=fd["r"]["dr"]), mam.MADJ_FD_R),
            ("mass and inertia", fd["params"], d["rec"], lambda mpc: mpc.set_params(**fd["params"]["kw"]),
             mam.predicted_change(d["g"], dtheta=fd["params"]["dtheta"]), mam.MADJ_FD_P)):
        mpc, f2, st2 = solved(rec2, h, nc, prepare)
        mpc.close()
        assert np.isin(interface.status_code(d["status"]), (0, 6)).all() and np.isin(interface.status_code(st2), (0, 6)).all()
        act = (d["ell"] * (f2.astype(np.float64).reshape(nb, h, -1) - u1)).reshape(nb, -1).sum(axis=1)
        err = np.abs(pred - act) / scale
        keep = pair["keep"]
        print(name, what, "kept", int(keep.sum()), "of", nb, "largest error / scale", float(err[keep].max()), "bound", bound, "l.u itself moved by",
              float(np.abs(act[keep]).max()), "error of the instances left out", float(err[~keep].max()) if (~keep).any() else 0.0)
        assert (err[keep] <= bound).all(), (name, what, err[keep].max())
