"""The limit gradients of the solve (hmpc_adjoint_limits, csrc/hmpc_limit_adjoint.hip) and ``loss.backward()`` into the instances' friction
parameter (hector_simulation_amd/autograd.py).

The reference is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/limit_adjoint_mirror.py), fed with the
ORACLE's binary32 assembly of each record, THE GPU'S OWN downloaded float32 forces, THE GPU'S OWN dir and the seed: no solver tolerance
enters the comparison.  The GPU and the mirror run the same algorithm and differ by binary64 round-off alone, so they must agree within
MIRROR_TOL = 1e-9 max(1, max|mirror output|), the project's bound for this class of arithmetic; the ratio is printed.  Shapes:
test_certificate_mirror.CASES, and standing, walking and standing_3c once more at f_max = 40, where the Fz cap is active; every test
asserts first that its batch holds admitted active rows of the parameter groups it speaks of (limit_adjoint_mirror.groups_of)."""
import ctypes as C

import numpy as np
import pytest

import adjoint_mirror as am
import limit_adjoint_mirror as lam
from hector_simulation_amd import interface, records, synthetic
from test_certificate_mirror import CASES, case_records
from test_gpu_adjoint import _device, _torch

pytestmark = pytest.mark.gpu
E_ARG = -1
ALL_CASES = lam.all_cases(CASES)
ALL_IDS = [c[0] for c in ALL_CASES]
PARAM_SETS = (dict(mu=1.1, lt=0.07, lh=0.05), dict(mu=0.6, lt=0.12, lh=0.03), dict(mu=3.0, lt=0.05, lh=0.08))

_cache = {}


def same_bits(a, b, what=""):
    for key in lam.KEYS:
        np.testing.assert_array_equal(a[key].view(np.uint64), b[key].view(np.uint64), err_msg=f"{what} {key}")


def solved(rec, h, nc=2, f_max=synthetic.F_MAX, prepare=None):
    """A handle with `rec` solved under the feet's cap f_max and downloaded (the safe pass has run): (mpc, forces, status)."""
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, f_max, rec.shape[0], contacts=nc)
    if prepare:
        prepare(mpc)
    mpc.upload(rec)
    mpc.solve()
    forces, status = mpc.download()
    return mpc, forces, status


def gradients_with(mpc, seed):
    """One adjoint and one limit launch of a solved handle under seed[b, h, U] (float64), both downloaded: (adjoint, limits)."""
    t = _device(np.asarray(seed, dtype=np.float64))
    mpc.solve_adjoint(t.data_ptr())
    mpc.adjoint_limits(t.data_ptr())
    return mpc.download_adjoint(), mpc.download_adjoint_limits()


def solved_entry(oracle, entry):
    """One solve + adjoint + limit gradients per entry (the seeds of the finite-difference tests) and the numpy definition on the
    downloaded forces and dir; shared by the tests, left unchanged."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    if name not in _cache:
        rec = case_records(case)
        ell = am.seeds(nb, h, 6 * nc)
        mpc, forces, status = solved(rec, h, nc, f_max)
        a, g = gradients_with(mpc, ell)
        mpc.close()
        _cache[name] = dict(rec=rec, forces=forces, status=status, a=a, g=g, ell=ell,
                            ref=lam.limit_adjoint_records(oracle, rec, h, nc, forces, a["dir"], ell, f_max=f_max))
    return _cache[name]


def mirror_error(g, ref):
    nb = g["grad_limits"].shape[0]
    worst = {}
    for key in lam.KEYS:
        assert g[key].shape == ref[key].shape, (key, g[key].shape, ref[key].shape)
        scale = np.maximum(1.0, np.abs(ref[key]).reshape(nb, -1).max(axis=1))
        worst[key] = float((np.abs(g[key] - ref[key]).reshape(nb, -1).max(axis=1) / scale).max()) / lam.MIRROR_TOL
    return worst


def assert_is_the_definition(g, ref, h, nc, groups, what=""):
    nb, U = g["grad_limits"].shape[0], 6 * nc
    lam.assert_covered(ref["rows"], groups, what)
    assert g["grad_limits"].shape == (nb, 3 + nc) and g["grad_Fc"].shape == (nb, 8 * nc, U) and g["summary"].shape == (nb, 3)
    assert g["grad_bound"].shape == g["lambda"].shape == g["nu"].shape == (nb, h, nc, 10)
    worst = mirror_error(g, ref)
    print(what, "largest error against the mirror / (1e-9 max(1, max|mirror|))", worst, "max|grad_limits|", np.abs(g["grad_limits"]).max(axis=0))
    assert max(worst.values()) <= 1.0, (what, worst)
    for k in range(nb):  # exact zeros: swing leg-steps, rows not admitted, entries outside a row's own columns
        for i in range(h):
            for c in range(nc):
                rows = ref["rows"][k].get((i, c), [])
                out = [j for j in range(10) if j not in rows]
                assert (g["lambda"][k, i, c, out] == 0).all() and (g["nu"][k, i, c, out] == 0).all() and (g["grad_bound"][k, i, c, out] == 0).all()
        for c in range(nc):
            outside = np.ones(U, dtype=bool)
            outside[lam.cm.cols(c, nc)] = False
            assert (g["grad_Fc"][k][8 * c:8 * c + 8][:, outside] == 0).all()


# ------------------------------------------------------------------------------------------------ 1. the kernel is the definition
@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_limit_adjoint_is_the_definition(oracle, entry):
    name, case, f_max = entry
    h, nc = case[2], case[4]
    d = solved_entry(oracle, entry)
    assert np.isin(interface.status_code(d["status"]), (0, 6)).all(), d["status"]
    assert_is_the_definition(d["g"], d["ref"], h, nc, lam.groups_of(name, f_max), name)
    np.testing.assert_array_equal(d["g"]["grad_bound"], 0.0 - d["g"]["nu"])


@pytest.mark.parametrize("entry", [ALL_CASES[0], ALL_CASES[-2]], ids=[ALL_IDS[0], ALL_IDS[-2]])
def test_summary_tells_the_seed(oracle, entry):
    """summary[1] is round-off with the seed the adjoint was given and large with another; a zero seed gives zero nu, grad_bound, grad_Fc
    and grad_limits, and the lambda of any seed."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = solved_entry(oracle, entry)
    lam.assert_covered(d["ref"]["rows"], lam.groups_of(name, f_max), name)
    scale = np.maximum(1.0, np.abs(d["ref"]["rho"]).reshape(nb, -1).max(axis=1))
    print(name, "summary[1] / (1e-9 max(1, max|rho|)) with the right seed", (d["g"]["summary"][:, 1] / scale).max() / lam.MIRROR_TOL)
    assert (d["g"]["summary"][:, 1] <= lam.MIRROR_TOL * scale).all()
    mpc, _, _ = solved(d["rec"], h, nc, f_max)
    t_right, t_other = _device(d["ell"]), _device(d["ell"][::-1] * 2.0)
    mpc.solve_adjoint(t_right.data_ptr())
    mpc.adjoint_limits(t_other.data_ptr())
    other = mpc.download_adjoint_limits()
    print(name, "summary[1] with another seed", other["summary"][:, 1].min())
    assert (other["summary"][:, 1] > 1e3 * lam.MIRROR_TOL * scale).all()
    _, z = gradients_with(mpc, np.zeros((nb, h, 6 * nc)))
    _, again = gradients_with(mpc, d["ell"])
    mpc.close()
    for key in ("nu", "grad_bound", "grad_Fc", "grad_limits"):
        assert (z[key] == 0).all(), key
    np.testing.assert_array_equal(z["lambda"].view(np.uint64), d["g"]["lambda"].view(np.uint64))  # (lambda knows no seed)
    same_bits(again, d["g"], "the same seed on a second handle")


# ------------------------------------------------------------------------------------------------ 2. constants
def test_params_and_instance_mu_reach_the_limit_gradients(oracle):
    name, case, f_max = ALL_CASES[-3]  # standing at f_max = 40: all four groups
    h, nb, nc = case[2], case[3], case[4]
    rec = case_records(case)
    ell = am.seeds(nb, h, 6 * nc)

    def run(prepare=None):
        mpc, forces, status = solved(rec, h, nc, f_max, prepare)
        a, g = gradients_with(mpc, ell)
        mpc.close()
        assert np.isin(interface.status_code(status), (0, 6)).all(), status
        return forces, a, g

    _, _, g0 = run()
    for ps in PARAM_SETS:
        forces1, a1, g1 = run(lambda mpc: mpc.set_params(**ps))
        try:
            oracle.set_params(**ps)
            ref = lam.limit_adjoint_records(oracle, rec, h, nc, forces1, a1["dir"], ell, f_max=f_max, lt=float(np.float32(ps["lt"])),
                                            lh=float(np.float32(ps["lh"])))
        finally:
            oracle.set_params()
        assert_is_the_definition(g1, ref, h, nc, lam.GROUPS, f"params {ps}")
        assert np.abs(g1["grad_limits"] - g0["grad_limits"]).max() > 1e-6
    mu = np.linspace(0.4, 1.6, nb).astype(np.float32)
    d_mu = _device(mu)
    forces, a, g = run(lambda mpc: mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu))
    ref = lam.limit_adjoint_records(oracle, rec, h, nc, forces, a["dir"], ell, f_max=f_max, mu=mu)
    assert_is_the_definition(g, ref, h, nc, lam.GROUPS, "instance mu")
    assert np.abs(g["grad_limits"][:, 0] - g0["grad_limits"][:, 0]).max() > 0.0


# ------------------------------------------------------------------------------------------------ 3. pure function
def test_pure_function_of_record_force_buffer_dir_and_seed(oracle):
    torch = _torch()
    h, nb, nc, k = 10, 16, 2, 4
    U = 6 * nc
    rec = np.repeat(case_records(CASES[0][1])[:nb // k], k, axis=0)  # groups of four records that share everything: a command sweep may solve them
    ell = am.seeds(nb, h, U)
    t_seed = _device(ell)
    mpc0, forces0, _ = solved(rec, h, nc, lam.LOW_CAP)
    a0, own = gradients_with(mpc0, ell)
    assert all(v != 0 for v in mpc0.get_device_adjoint_limits().values())
    mpc0.close()
    lam.assert_covered(lam.limit_adjoint_records(oracle, rec[::k], h, nc, forces0[::k], a0["dir"][::k], ell[::k], f_max=lam.LOW_CAP)["rows"], lam.GROUPS,
                       "pure function")
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    shapes = dict(grad_limits=(nb, 3 + nc), grad_Fc=(nb, 8 * nc, U), grad_bound=(nb, h, nc, 10), nu=(nb, h, nc, 10), summary=(nb, 3))
    shapes["lambda"] = (nb, h, nc, 10)
    mine = {key: torch.zeros(s, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, lam.LOW_CAP, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_adjoint_limits(*[mine[key].data_ptr() for key in lam.KEYS], keepalive=mine)
    assert mpc.get_device_adjoint_limits() == {key: mine[key].data_ptr() for key in lam.KEYS}
    mpc.upload(rec)
    for order in (0, 1):
        mpc.set_dispatch_order(order)
        mpc.solve()
        mpc.download()  # (the safe pass, as on the first handle)
        mpc.solve_adjoint(t_seed.data_ptr())
        mpc.adjoint_limits(t_seed.data_ptr())
        torch.cuda.synchronize()
        same_bits({key: mine[key].cpu().numpy() for key in lam.KEYS}, own, f"caller-owned buffers, dispatch order {order}")
        same_bits(mpc.download_adjoint_limits(), own, f"downloaded from the caller's buffers, dispatch order {order}")
    mpc.solve_command_sweep(k)
    mpc.download()
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_limits(t_seed.data_ptr())
    same_bits(mpc.download_adjoint_limits(), own, "after a command sweep")
    mpc.adjoint_limits(t_seed.data_ptr())
    same_bits(mpc.download_adjoint_limits(), own, "twice")
    mpc.close()
    # a device group's member against the plain handle
    grp = interface.DeviceGroup(synthetic.DT_MPC, h, lam.LOW_CAP, nb, [0, 0], transport="p2p")
    grp.upload(rec)
    grp.solve()
    grp.download()
    L = grp.L
    for i in range(grp.size):
        hd, _, lo, n, st = grp.member(i)
        t_part = _device(ell[lo:lo + n])
        assert L.hmpc_adjoint_limits(hd, C.c_void_p(t_part.data_ptr()), C.c_void_p(st)) == E_ARG  # (no adjoint yet)
        assert L.hmpc_solve_adjoint(hd, C.c_void_p(t_part.data_ptr()), C.c_void_p(st)) == 0
        assert L.hmpc_adjoint_limits(hd, C.c_void_p(t_part.data_ptr()), C.c_void_p(st)) == 0
        got = {key: np.zeros((n,) + shapes[key][1:]) for key in lam.KEYS}
        assert L.hmpc_download_adjoint_limits(hd, *[got[key].ctypes.data for key in lam.KEYS]) == 0
        same_bits(got, {key: own[key][lo:lo + n] for key in lam.KEYS}, f"group member {i}")
    grp.close()


# ------------------------------------------------------------------------------------------------ 4. ordering
def test_ordering_errors_enqueue_nothing_and_leave_the_buffers_alone():
    torch = _torch()
    h, U, nc = 10, 12, 2
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    shapes = dict(grad_limits=(16, 3 + nc), grad_Fc=(16, 8 * nc, U), grad_bound=(16, h, nc, 10), nu=(16, h, nc, 10), summary=(16, 3))
    shapes["lambda"] = (16, h, nc, 10)
    mine = {key: torch.full(s, -7.0, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    t_seed = _device(am.seeds(16, h, U))
    sp = C.c_void_p(t_seed.data_ptr())
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    ptrs = [mine[key].data_ptr() for key in lam.KEYS]
    mpc.set_device_adjoint_limits(*ptrs, keepalive=mine)
    host = [np.full(shapes[key], -9.0) for key in lam.KEYS]

    def snapshot():
        torch.cuda.synchronize()
        return [mine[key].cpu().numpy().copy() for key in lam.KEYS]

    def refused(what, before, launch_too, download_too=True):
        """the download (and, where no adjoint of the last solve exists, the launch) answers HMPC_E_ARG; nothing on the device or in the host moved"""
        if download_too:
            assert L.hmpc_download_adjoint_limits(hd, *[a.ctypes.data for a in host]) == E_ARG, what
        if launch_too:
            assert L.hmpc_adjoint_limits(hd, sp, None) == E_ARG, what
        assert all((a == -9).all() for a in host), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    s0 = snapshot()
    refused("before a batch", s0, True, download_too=False)  # (a download of the empty batch copies nothing and is no error, as for the adjoint)
    assert L.hmpc_download_adjoint_limits(hd, *[a.ctypes.data for a in host]) == 0 and all((a == -9).all() for a in host)
    mpc.upload(rec_a)
    refused("before a solve of the batch", s0, True)
    mpc.solve()
    refused("a solve, no adjoint from it", s0, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    adj_before = mpc.download_adjoint()
    refused("an adjoint, no limit gradients from it", s0, False)
    assert L.hmpc_adjoint_limits(hd, None, None) == E_ARG  # a NULL seed
    refused("a NULL seed", s0, False)
    mpc.adjoint_limits(t_seed.data_ptr())
    first = mpc.download_adjoint_limits()
    s1 = snapshot()
    assert (s1[0] != -7.0).all()
    after = mpc.download_adjoint()  # the limit launch leaves the adjoint's bits alone (and its results valid)
    for key in am.KEYS:
        np.testing.assert_array_equal(after[key].view(np.uint64), adj_before[key].view(np.uint64), err_msg=key)
    mpc.adjoint_model()  # the model gradients are a node of their own: nothing of the limits goes stale
    same_bits(mpc.download_adjoint_limits(), first, "after the model gradients")
    mpc.solve_adjoint(t_seed.data_ptr())  # a new adjoint (a new seed, for all the handle knows)
    refused("after a new adjoint", s1, False)
    mpc.adjoint_limits(t_seed.data_ptr())
    same_bits(mpc.download_adjoint_limits(), first, "after the new adjoint")
    mpc.set_device_adjoint_limits(*ptrs, keepalive=mine)  # its own retarget: whatever was computed went elsewhere
    refused("after a retarget", s1, False)
    mpc.adjoint_limits(t_seed.data_ptr())
    same_bits(mpc.download_adjoint_limits(), first, "after the retarget")
    mpc.set_device_adjoint()  # the adjoint's retarget: dir is no longer where the launch would read it
    refused("after the adjoint's retarget", s1, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_limits(t_seed.data_ptr())
    same_bits(mpc.download_adjoint_limits(), first, "after the adjoint's retarget and a new adjoint")
    mpc.upload(rec_b)
    refused("after a new upload", s1, True)
    mpc.solve()
    refused("after a solve of the new batch", s1, True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_limits(t_seed.data_ptr())
    mpc.download_adjoint_limits()
    mpc.solve()
    refused("after a second solve", snapshot(), True)
    mpc.solve_adjoint(t_seed.data_ptr())
    mpc.adjoint_limits(t_seed.data_ptr())
    second = mpc.download_adjoint_limits()
    mpc.close()
    mpc2, _, _ = solved(rec_b, h)
    _, fresh = gradients_with(mpc2, am.seeds(16, h, U)[:8])
    mpc2.close()
    assert second["grad_limits"].shape == (8, 3 + nc)
    same_bits(second, fresh, "against a fresh handle")


# ------------------------------------------------------------------------------------------------ 5. autograd
def test_backward_returns_grad_mu_and_leaves_the_old_gradients_alone(oracle):
    torch = _torch()
    from hector_simulation_amd.autograd import differentiable_solve_limits

    h, nb, nc = 10, 8, 2
    U = 6 * nc
    fields = synthetic.hard_batch(nb, h, "standing", seed=17, scale=3.0)  # (friction rows are active here)
    rng = np.random.default_rng(9)
    c = torch.from_numpy(rng.uniform(-1.0, 1.0, (nb, h * U)).astype(np.float32)).cuda()
    seed = c.cpu().numpy().astype(np.float64).reshape(nb, h, U)
    mu_np = np.linspace(0.5, 1.5, nb).astype(np.float32)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)

    def leaves():
        return [torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1), requires_grad=True) for key in ("traj", "weights", "Alpha_K")]

    # mu = None: the three old gradients and r.grad, bit for bit the older launches'; no limit launch (nothing to download)
    old = leaves()
    r_old = torch.tensor(np.asarray(fields["r"], dtype=np.float32).reshape(nb, -1), requires_grad=True)
    (differentiable_solve_limits(mpc, fields, *old, r_old, mu=None) * c).sum().backward()
    torch.cuda.synchronize()
    assert mpc.L.hmpc_download_adjoint_limits(mpc.h, *[None] * 6) == E_ARG
    t = _device(seed)
    mpc.solve_adjoint(t.data_ptr())
    mpc.adjoint_model()
    want_a, want_m = mpc.download_adjoint(), mpc.download_adjoint_model()
    for leaf, key in zip(old, ("grad_traj", "grad_weights", "grad_alpha")):
        np.testing.assert_array_equal(leaf.grad.numpy().view(np.uint32), want_a[key].reshape(nb, -1).astype(np.float32).view(np.uint32), err_msg=key)
    np.testing.assert_array_equal(r_old.grad.numpy().view(np.uint32), want_m["grad_r"].reshape(nb, -1).astype(np.float32).view(np.uint32))
    # mu given: the C calls under the same per-instance mu, bit for bit
    new = leaves()
    mu = torch.tensor(mu_np, requires_grad=True)
    forces = differentiable_solve_limits(mpc, fields, *new, mu=mu)
    np.testing.assert_array_equal(forces.detach().cpu().numpy().view(np.uint32), mpc.download()[0].view(np.uint32))
    (forces * c).sum().backward()
    torch.cuda.synchronize()
    got = mpc.download_adjoint_limits()
    d_mu = _device(mu_np)
    mpc2, forces2, _ = solved(records.pack_records(fields, h, nc), h, nc, prepare=lambda m: m.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu))
    np.testing.assert_array_equal(forces2.view(np.uint32), forces.detach().cpu().numpy().view(np.uint32))
    a2, want_g = gradients_with(mpc2, seed)
    mpc2.close()
    same_bits(got, want_g, "the limit gradients behind backward")
    ref = lam.limit_adjoint_records(oracle, records.pack_records(fields, h, nc), h, nc, forces2, a2["dir"], seed, mu=mu_np)
    lam.assert_covered(ref["rows"], ("mu",), "backward")
    assert tuple(mu.grad.shape) == (nb,)
    np.testing.assert_array_equal(mu.grad.numpy().view(np.uint32), want_g["grad_limits"][:, 0].astype(np.float32).view(np.uint32))
    assert np.abs(want_g["grad_limits"][:, 0]).max() > 0.0
    for leaf, key in zip(new, ("grad_traj", "grad_weights", "grad_alpha")):
        np.testing.assert_array_equal(leaf.grad.numpy().view(np.uint32), a2[key].reshape(nb, -1).astype(np.float32).view(np.uint32), err_msg=key)
    # float64 mu on the handle's own device: the gradient is a copy, not a view of the handle's buffer; the generation guard stays
    mu64 = torch.tensor(mu_np, dtype=torch.float64, device="cuda", requires_grad=True)
    (differentiable_solve_limits(mpc, fields, *leaves(), mu=mu64) * c).sum().backward()
    torch.cuda.synchronize()
    assert mu64.grad.data_ptr() not in {t.data_ptr() for t in mpc._autograd_limit_buffers.values()}
    np.testing.assert_array_equal(mu64.grad.cpu().numpy().view(np.uint64), want_g["grad_limits"][:, 0].view(np.uint64))
    stale = differentiable_solve_limits(mpc, fields, *leaves(), mu=mu64)
    mpc.solve()
    with pytest.raises(RuntimeError, match="has solved another batch since this forward"):
        (stale * c).sum().backward()
    mpc.close()


# ------------------------------------------------------------------------------------------------ 6. a re-solve
@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_gradients_follow_a_re_solve(oracle, entry):
    """fd_limits_entry's moved mu, lt, lh and f_max of the CPU test, solved on the GPU: on the kept instances the predicted change of l.u is
    within LADJ_FD[group] max(1, max|u|) of the re-solve's, for every group the batch covers."""
    from test_limit_adjoint_mirror import limit_case

    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = solved_entry(oracle, entry)
    base = limit_case(oracle, entry)
    np.testing.assert_array_equal(d["rec"], base["rec"])
    groups = lam.groups_of(name, f_max)
    lam.assert_covered(d["ref"]["rows"], groups, name)
    u1 = d["forces"].astype(np.float64).reshape(nb, h, -1)
    scale = np.maximum(1.0, np.abs(u1).reshape(nb, -1).max(axis=1))
    fd = lam.fd_limits_entry(oracle, entry, base)
    failed = []
    for group in groups:
        m = fd[group]
        mpc, f2, st2 = solved(d["rec"], h, nc, m["f_max"], (lambda mpc: mpc.set_params(**m["kw"])) if m["kw"] else None)
        mpc.close()
        assert np.isin(interface.status_code(d["status"]), (0, 6)).all() and np.isin(interface.status_code(st2), (0, 6)).all()
        pred = lam.predicted_change(d["g"], group, m["dtheta"])
        act = (d["ell"] * (f2.astype(np.float64).reshape(nb, h, -1) - u1)).reshape(nb, -1).sum(axis=1)
        err = np.abs(pred - act) / scale
        keep = m["keep"]
        print(name, group, "kept", int(keep.sum()), "of", nb, "largest error / scale", float(err[keep].max()), "bound", lam.LADJ_FD[group],
              "l.u itself moved by", float(np.abs(act[keep]).max()), "error of the instances left out", float(err[~keep].max()) if (~keep).any() else 0.0)
        if not (err[keep] <= lam.LADJ_FD[group]).all():
            failed.append((group, float(err[keep].max())))
    assert not failed, (name, failed)
