"""The pose gradients of the solve (hmpc_adjoint_record, csrc/hmpc_pose_adjoint.hip) and ``loss.backward()`` into any field of the record
(hector_simulation_amd/autograd.py differentiable_solve_fields).

The reference is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/pose_adjoint_mirror.py), fed with the
ORACLE's binary32 assembly of each record and THE GPU'S OWN downloaded upstream buffers (the adjoint's, the model gradients', the limit
gradients'): no solver tolerance enters the comparison.  The GPU and the mirror run the same algorithm and differ by binary64 round-off
alone, so they must agree within MIRROR_TOL = 1e-9 max(1, max|mirror output|); the fraction of that bound is printed per batch.  Shapes:
limit_adjoint_mirror.all_cases(CASES); every test asserts first that its batch holds admitted active rows among the rows the foot frames
enter and a non-zero grad_B[6:9] (pose_adjoint_mirror.assert_pose_covered)."""
import ctypes as C

import numpy as np
import pytest

import adjoint_mirror as am
import limit_adjoint_mirror as lam
import pose_adjoint_mirror as pm
from hector_simulation_amd import interface, records, synthetic
from test_certificate_mirror import CASES, case_records
from test_gpu_adjoint import _device, _torch
from test_gpu_limit_adjoint import solved

pytestmark = pytest.mark.gpu
E_ARG = -1
ALL_CASES = lam.all_cases(CASES)
ALL_IDS = [c[0] for c in ALL_CASES]
PARAM_SETS = (dict(mu=1.1, lt=0.07, lh=0.05, mass=11.0, inertia=(0.61, 0.48, 0.09)), dict(mu=0.6, lt=0.12, lh=0.03, inertia=(0.4, 0.7, 0.05)),
              dict(mu=3.0, lt=0.05, lh=0.08, mass=7.5))

_cache = {}


def same_bits(a, b, what=""):
    for key in pm.KEYS:
        np.testing.assert_array_equal(a[key].view(np.uint64), b[key].view(np.uint64), err_msg=f"{what} {key}")


def chain_with(mpc, seed):
    """Adjoint -> model gradients -> limit gradients -> record gradients of a solved handle under seed[b, h, U] (float64), all four
    downloaded: (adjoint, model, limits, record)."""
    t = _device(np.asarray(seed, dtype=np.float64))
    mpc.solve_adjoint(t.data_ptr())
    mpc.adjoint_model()
    mpc.adjoint_limits(t.data_ptr())
    mpc.adjoint_record()
    return mpc.download_adjoint(), mpc.download_adjoint_model(), mpc.download_adjoint_limits(), mpc.download_adjoint_record()


def solved_entry(oracle, entry):
    """One solve and one chain per entry (the seeds of the finite-difference tests), the numpy definition on the downloaded upstream
    buffers and the limit mirror's admitted rows on the downloaded forces; shared by the tests, left unchanged."""
    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    if name not in _cache:
        rec = case_records(case)
        ell = am.seeds(nb, h, 6 * nc)
        mpc, forces, status = solved(rec, h, nc, f_max)
        a, m, l, g = chain_with(mpc, ell)
        mpc.close()
        up = pm.upstream_of(a, m, l)
        rows = lam.limit_adjoint_records(oracle, rec, h, nc, forces, a["dir"], ell, f_max=f_max)["rows"]
        _cache[name] = dict(rec=rec, forces=forces, status=status, a=a, m=m, l=l, g=g, ell=ell, up=up, rows=rows,
                            ref=pm.pose_adjoint_records(oracle, rec, h, nc, up))
    return _cache[name]


def mirror_error(g, ref):
    nb = g["grad_record"].shape[0]
    worst = {}
    for key in pm.KEYS:
        assert g[key].shape == ref[key].shape, (key, g[key].shape, ref[key].shape)
        scale = np.maximum(1.0, np.abs(ref[key]).reshape(nb, -1).max(axis=1))
        worst[key] = float((np.abs(g[key] - ref[key]).reshape(nb, -1).max(axis=1) / scale).max()) / pm.MIRROR_TOL
    return worst


def assert_is_the_definition(g, ref, up, h, nc, what=""):
    nb = g["grad_record"].shape[0]
    sl = pm.slices(nc, h)
    assert g["grad_record"].shape == (nb, (records.N_FIXED3 if nc == 3 else records.N_FIXED) + 12 * h)
    assert g["grad_frames"].shape == (nb, 1 + nc, 3, 3) and g["grad_rpy"].shape == (nb, 3)
    worst = mirror_error(g, ref)
    print(what, "largest error against the mirror / (1e-9 max(1, max|mirror|))", worst, "max|grad q|", float(np.abs(g["grad_record"][:, sl["q"]]).max()),
          "max|grad ja|", float(np.abs(g["grad_record"][:, sl["joint_angles"]]).max()))
    assert max(worst.values()) <= 1.0, (what, worst)
    # the copies are copies, the yaw word is +0, the three sagittal joints of a leg get one number
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    r = g["grad_record"]
    for field, src in (("p", up["grad_x0"][:, 3:6]), ("w", up["grad_x0"][:, 6:9]), ("v", up["grad_x0"][:, 9:12]), ("r", up["grad_r"].reshape(nb, -1)),
                       ("weights", up["grad_weights"]), ("Alpha_K", up["grad_alpha"]), ("traj", up["grad_traj"].reshape(nb, -1))):
        np.testing.assert_array_equal(bits(r[:, sl[field]]), bits(src), err_msg=f"{what} {field}")
    assert (bits(r[:, sl["yaw"]]) == 0).all()
    ja = r[:, sl["joint_angles"]].reshape(nb, 2, 5)
    assert np.array_equal(bits(ja[:, :, 2]), bits(ja[:, :, 3])) and np.array_equal(bits(ja[:, :, 2]), bits(ja[:, :, 4]))
    np.testing.assert_array_equal(bits(g["grad_rpy"][:, 0]), bits(up["grad_x0"][:, 0]))
    if nc == 3:
        np.testing.assert_array_equal(bits(r[:, sl["f_max_hand"]][:, 0]), bits(up["grad_limits"][:, 5]))
        np.testing.assert_array_equal(bits(r[:, sl["Rhand"]]), bits(g["grad_frames"][:, 3].reshape(nb, 9)))


# ------------------------------------------------------------------------------------------------ 1. the kernel is the definition
@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_pose_adjoint_is_the_definition(oracle, entry):
    name, case, f_max = entry
    h, nc = case[2], case[4]
    d = solved_entry(oracle, entry)
    assert np.isin(interface.status_code(d["status"]), (0, 6)).all(), d["status"]
    pm.assert_pose_covered(d["rows"], d["m"]["grad_B"], name)
    assert_is_the_definition(d["g"], d["ref"], d["up"], h, nc, name)


def test_a_zero_seed_gives_zeros(oracle):
    name, case, f_max = ALL_CASES[0]
    h, nb, nc = case[2], case[3], case[4]
    mpc, _, _ = solved(case_records(case), h, nc, f_max)
    _, _, _, z = chain_with(mpc, np.zeros((nb, h, 6 * nc)))
    mpc.close()
    for key in pm.KEYS:
        assert (z[key] == 0).all(), key


# ------------------------------------------------------------------------------------------------ 2. constants
def test_params_and_instance_mu_reach_the_pose_gradients(oracle):
    name, case, f_max = ALL_CASES[-3]  # standing at f_max = 40
    h, nb, nc = case[2], case[3], case[4]
    rec = case_records(case)
    ell = am.seeds(nb, h, 6 * nc)

    def run(prepare=None):
        mpc, forces, status = solved(rec, h, nc, f_max, prepare)
        a, m, l, g = chain_with(mpc, ell)
        mpc.close()
        assert np.isin(interface.status_code(status), (0, 6)).all(), status
        return forces, a, m, l, g

    g0 = run()[4]
    sl = pm.slices(nc, h)
    for ps in PARAM_SETS:
        forces1, a1, m1, l1, g1 = run(lambda mpc: mpc.set_params(**ps))
        try:
            oracle.set_params(**ps)
            rows = lam.limit_adjoint_records(oracle, rec, h, nc, forces1, a1["dir"], ell, f_max=f_max, lt=float(np.float32(ps["lt"])),
                                             lh=float(np.float32(ps["lh"])))["rows"]
            up = pm.upstream_of(a1, m1, l1)
            ref = pm.pose_adjoint_records(oracle, rec, h, nc, up, lt=float(np.float32(ps["lt"])), lh=float(np.float32(ps["lh"])),
                                          inertia=tuple(float(np.float32(v)) for v in ps.get("inertia", pm.INERTIA)))
        finally:
            oracle.set_params()
        pm.assert_pose_covered(rows, m1["grad_B"], f"params {ps}")
        assert_is_the_definition(g1, ref, up, h, nc, f"params {ps}")
        assert np.abs(g1["grad_record"][:, sl["q"]] - g0["grad_record"][:, sl["q"]]).max() > 1e-6
    mu = np.linspace(0.4, 1.6, nb).astype(np.float32)
    d_mu = _device(mu)
    forces, a, m, l, g = run(lambda mpc: mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu))
    up = pm.upstream_of(a, m, l)
    assert_is_the_definition(g, pm.pose_adjoint_records(oracle, rec, h, nc, up, mu=mu), up, h, nc, "instance mu")
    assert np.abs(g["grad_record"][:, sl["joint_angles"]] - g0["grad_record"][:, sl["joint_angles"]]).max() > 0.0


# ------------------------------------------------------------------------------------------------ 3. pure function
def test_pure_function_of_record_and_upstream_buffers(oracle):
    torch = _torch()
    h, nb, nc, k = 10, 16, 2, 4
    U = 6 * nc
    rec = np.repeat(case_records(CASES[0][1])[:nb // k], k, axis=0)  # groups of four records that share everything: a command sweep may solve them
    ell = am.seeds(nb, h, U)
    t_seed = _device(ell)
    mpc0, forces0, _ = solved(rec, h, nc, lam.LOW_CAP)
    a0, m0, _, own = chain_with(mpc0, ell)
    assert all(v != 0 for v in mpc0.get_device_adjoint_record().values())
    mpc0.close()
    pm.assert_pose_covered(lam.limit_adjoint_records(oracle, rec[::k], h, nc, forces0[::k], a0["dir"][::k], ell[::k], f_max=lam.LOW_CAP)["rows"],
                           m0["grad_B"], "pure function")
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    shapes = dict(grad_record=(nb, records.N_FIXED + 12 * h), grad_frames=(nb, 1 + nc, 3, 3), grad_rpy=(nb, 3))
    mine = {key: torch.zeros(s, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, lam.LOW_CAP, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_adjoint_record(*[mine[key].data_ptr() for key in pm.KEYS], keepalive=mine)
    assert mpc.get_device_adjoint_record() == {key: mine[key].data_ptr() for key in pm.KEYS}
    mpc.upload(rec)

    def chain():
        mpc.solve_adjoint(t_seed.data_ptr())
        mpc.adjoint_model()
        mpc.adjoint_limits(t_seed.data_ptr())
        mpc.adjoint_record()

    for order in (0, 1):
        mpc.set_dispatch_order(order)
        mpc.solve()
        mpc.download()  # (the safe pass, as on the first handle)
        chain()
        torch.cuda.synchronize()
        same_bits({key: mine[key].cpu().numpy() for key in pm.KEYS}, own, f"caller-owned buffers, dispatch order {order}")
        same_bits(mpc.download_adjoint_record(), own, f"downloaded from the caller's buffers, dispatch order {order}")
    mpc.solve_command_sweep(k)
    mpc.download()
    chain()
    same_bits(mpc.download_adjoint_record(), own, "after a command sweep")
    mpc.adjoint_record()
    same_bits(mpc.download_adjoint_record(), own, "twice")
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
        sp, stp = C.c_void_p(t_part.data_ptr()), C.c_void_p(st)
        assert L.hmpc_solve_adjoint(hd, sp, stp) == 0 and L.hmpc_adjoint_model(hd, stp) == 0
        assert L.hmpc_adjoint_record(hd, stp) == E_ARG  # (no limit gradients yet)
        assert L.hmpc_adjoint_limits(hd, sp, stp) == 0 and L.hmpc_adjoint_record(hd, stp) == 0
        got = {key: np.zeros((n,) + shapes[key][1:]) for key in pm.KEYS}
        assert L.hmpc_download_adjoint_record(hd, *[got[key].ctypes.data for key in pm.KEYS]) == 0
        same_bits(got, {key: own[key][lo:lo + n] for key in pm.KEYS}, f"group member {i}")
    grp.close()


# ------------------------------------------------------------------------------------------------ 4. ordering
def test_ordering_errors_enqueue_nothing_and_leave_the_buffers_alone():
    torch = _torch()
    h, U, nc = 10, 12, 2
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    shapes = dict(grad_record=(16, records.N_FIXED + 12 * h), grad_frames=(16, 1 + nc, 3, 3), grad_rpy=(16, 3))
    mine = {key: torch.full(s, -7.0, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    t_seed = _device(am.seeds(16, h, U))
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    ptrs = [mine[key].data_ptr() for key in pm.KEYS]
    mpc.set_device_adjoint_record(*ptrs, keepalive=mine)
    host = [np.full(shapes[key], -9.0) for key in pm.KEYS]

    def snapshot():
        torch.cuda.synchronize()
        return [mine[key].cpu().numpy().copy() for key in pm.KEYS]

    def refused(what, before, launch_too, download_too=True):
        """the download (and, where one of the three inputs is missing, the launch) answers HMPC_E_ARG; nothing on the device or in the host moved"""
        if download_too:
            assert L.hmpc_download_adjoint_record(hd, *[a.ctypes.data for a in host]) == E_ARG, what
        if launch_too:
            assert L.hmpc_adjoint_record(hd, None) == E_ARG, what
        assert all((a == -9).all() for a in host), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    def parents(model=True, limits=True):
        mpc.solve_adjoint(t_seed.data_ptr())
        if model:
            mpc.adjoint_model()
        if limits:
            mpc.adjoint_limits(t_seed.data_ptr())

    s0 = snapshot()
    refused("before a batch", s0, True, download_too=False)  # (a download of the empty batch copies nothing and is no error)
    assert L.hmpc_download_adjoint_record(hd, *[a.ctypes.data for a in host]) == 0 and all((a == -9).all() for a in host)
    mpc.upload(rec_a)
    refused("before a solve of the batch", s0, True)
    mpc.solve()
    refused("a solve, no adjoint from it", s0, True)
    parents(model=False, limits=False)
    refused("an adjoint alone", s0, True)
    mpc.adjoint_model()
    refused("missing limit gradients", s0, True)
    parents(model=False)
    refused("missing model gradients", s0, True)
    mpc.adjoint_model()
    refused("all three, no record gradients from them", s0, False)
    before = (mpc.download_adjoint(), mpc.download_adjoint_model(), mpc.download_adjoint_limits())
    mpc.adjoint_record()
    first = mpc.download_adjoint_record()
    s1 = snapshot()
    assert (s1[2] != -7.0).all()
    after = (mpc.download_adjoint(), mpc.download_adjoint_model(), mpc.download_adjoint_limits())  # the launch leaves its inputs' bits alone (and valid)
    for b, a in zip(before, after):
        for key in b:
            np.testing.assert_array_equal(a[key].view(np.uint64), b[key].view(np.uint64), err_msg=key)
    mpc.set_device_adjoint_record(*ptrs, keepalive=mine)  # its own retarget: whatever was computed went elsewhere
    refused("after a retarget", s1, False)
    mpc.adjoint_record()
    same_bits(mpc.download_adjoint_record(), first, "after the retarget")
    mpc.set_device_adjoint_model()  # a parent's retarget: grad_B is no longer where the launch would read it
    refused("after the model gradients' retarget", s1, True)
    mpc.adjoint_model()
    mpc.adjoint_record()
    same_bits(mpc.download_adjoint_record(), first, "after the model gradients' retarget and new model gradients")
    mpc.set_device_adjoint_limits()
    refused("after the limit gradients' retarget", s1, True)
    mpc.adjoint_limits(t_seed.data_ptr())
    mpc.adjoint_record()
    same_bits(mpc.download_adjoint_record(), first, "after the limit gradients' retarget and new limit gradients")
    mpc.set_device_adjoint()
    refused("after the adjoint's retarget", s1, True)
    parents()
    mpc.adjoint_record()
    same_bits(mpc.download_adjoint_record(), first, "after the adjoint's retarget and a new chain")
    mpc.solve_adjoint(t_seed.data_ptr())  # a new adjoint (a new seed, for all the handle knows)
    refused("after a new adjoint", s1, True)
    mpc.upload(rec_b)
    refused("after a new upload", s1, True)
    mpc.solve()
    refused("after a solve of the new batch", s1, True)
    parents()
    mpc.adjoint_record()
    mpc.download_adjoint_record()
    mpc.solve()
    refused("after a second solve", snapshot(), True)
    parents()
    mpc.adjoint_record()
    second = mpc.download_adjoint_record()
    mpc.close()
    mpc2, _, _ = solved(rec_b, h)
    fresh = chain_with(mpc2, am.seeds(16, h, U)[:8])[3]
    mpc2.close()
    assert second["grad_record"].shape == (8, records.N_FIXED + 12 * h)
    same_bits(second, fresh, "against a fresh handle")


# ------------------------------------------------------------------------------------------------ 5. autograd
def test_backward_through_any_field_is_the_c_calls(oracle):
    torch = _torch()
    from hector_simulation_amd.autograd import differentiable_solve, differentiable_solve_fields

    h, nb, nc = 10, 8, 2
    U = 6 * nc
    fields = synthetic.hard_batch(nb, h, "standing", seed=17, scale=3.0)
    rng = np.random.default_rng(9)
    c = torch.from_numpy(rng.uniform(-1.0, 1.0, (nb, h * U)).astype(np.float32)).cuda()
    seed = c.cpu().numpy().astype(np.float64).reshape(nb, h, U)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    sl = pm.slices(nc, h)
    leaf = lambda key, **kw: torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1), requires_grad=True, **kw)
    # every field a tensor: each .grad is its slice of the C calls' grad_record, bit for bit
    names = ("p", "v", "q", "w", "r", "joint_angles", "weights", "Alpha_K", "traj")
    leaves = {key: leaf(key) for key in names}
    forces = differentiable_solve_fields(mpc, {**fields, **leaves})
    np.testing.assert_array_equal(forces.detach().cpu().numpy().view(np.uint32), mpc.download()[0].view(np.uint32))
    (forces * c).sum().backward()
    torch.cuda.synchronize()
    got = mpc.download_adjoint_record()
    mpc2, forces2, _ = solved(records.pack_records(fields, h, nc), h, nc)
    np.testing.assert_array_equal(forces2.view(np.uint32), forces.detach().cpu().numpy().view(np.uint32))
    a2, m2, l2, want = chain_with(mpc2, seed)
    mpc2.close()
    same_bits(got, want, "the record gradients behind backward")
    rows = lam.limit_adjoint_records(oracle, records.pack_records(fields, h, nc), h, nc, forces2, a2["dir"], seed)["rows"]
    pm.assert_pose_covered(rows, m2["grad_B"], "backward")
    for key in names:
        assert tuple(leaves[key].grad.shape) == tuple(leaves[key].shape), key
        np.testing.assert_array_equal(leaves[key].grad.numpy().view(np.uint32), want["grad_record"][:, sl[key]].astype(np.float32).view(np.uint32), err_msg=key)
    assert np.abs(want["grad_record"][:, sl["q"]]).max() > 0.0 and np.abs(want["grad_record"][:, sl["joint_angles"]]).max() > 0.0
    # only traj / weights / Alpha_K / r as tensors: differentiable_solve, bit for bit
    some = {key: leaf(key) for key in ("traj", "weights", "Alpha_K", "r")}
    (differentiable_solve_fields(mpc, {**fields, **some}) * c).sum().backward()
    old = {key: leaf(key) for key in ("traj", "weights", "Alpha_K", "r")}
    (differentiable_solve(mpc, fields, old["traj"], old["weights"], old["Alpha_K"], old["r"]) * c).sum().backward()
    torch.cuda.synchronize()
    for key in some:
        np.testing.assert_array_equal(some[key].grad.numpy().view(np.uint32), old[key].grad.numpy().view(np.uint32), err_msg=key)
    # a float64 q on the handle's own device: the gradient is a copy, not a view of the handle's buffer; the generation guard stays
    q64 = leaf("q", dtype=torch.float64, device="cuda")
    (differentiable_solve_fields(mpc, {**fields, "q": q64}) * c).sum().backward()
    torch.cuda.synchronize()
    lo, hi = mpc._autograd_record_buffers["grad_record"].data_ptr(), mpc._autograd_record_buffers["grad_record"].data_ptr() + mpc._autograd_record_buffers["grad_record"].numel() * 8
    assert not (lo <= q64.grad.data_ptr() < hi)
    np.testing.assert_array_equal(q64.grad.cpu().numpy().view(np.uint64), want["grad_record"][:, sl["q"]].view(np.uint64))
    with pytest.raises(ValueError, match="no gradient is defined"):
        differentiable_solve_fields(mpc, {**fields, "gait": torch.zeros(nb, 2 * h)})
    stale = differentiable_solve_fields(mpc, {**fields, "q": q64})
    mpc.solve()
    with pytest.raises(RuntimeError, match="has solved another batch since this forward"):
        (stale * c).sum().backward()
    mpc.close()


# ------------------------------------------------------------------------------------------------ 6. a re-solve
@pytest.mark.parametrize("entry", ALL_CASES, ids=ALL_IDS)
def test_gradients_follow_a_re_solve(oracle, entry):
    """fd_pose_entry's moved quaternions and joint angles of the CPU test, solved on the GPU: on the kept instances the predicted change
    of l.u is within PADJ_FD[group] max(1, max|u|) of the re-solve's."""
    from test_limit_adjoint_mirror import limit_case

    name, case, f_max = entry
    h, nb, nc = case[2], case[3], case[4]
    d = solved_entry(oracle, entry)
    base = limit_case(oracle, entry)
    np.testing.assert_array_equal(d["rec"], base["rec"])
    pm.assert_pose_covered(d["rows"], d["m"]["grad_B"], name)
    u1 = d["forces"].astype(np.float64).reshape(nb, h, -1)
    scale = np.maximum(1.0, np.abs(u1).reshape(nb, -1).max(axis=1))
    fd = pm.fd_pose_entry(oracle, entry, base)
    failed = []
    for group in pm.FD_GROUPS:
        m = fd[group]
        mpc, f2, st2 = solved(m["rec2"], h, nc, f_max)
        mpc.close()
        assert np.isin(interface.status_code(d["status"]), (0, 6)).all() and np.isin(interface.status_code(st2), (0, 6)).all()
        pred = pm.predicted_change(d["g"], group, m["delta"], nc, h)
        act = (d["ell"] * (f2.astype(np.float64).reshape(nb, h, -1) - u1)).reshape(nb, -1).sum(axis=1)
        err = np.abs(pred - act) / scale
        keep = m["keep"]
        print(name, group, "s", m["s"], "kept", int(keep.sum()), "of", nb, "largest error / scale", float(err[keep].max()), "bound", pm.PADJ_FD[group],
              "l.u itself moved by", float(np.abs(act[keep]).max()), "error of the instances left out", float(err[~keep].max()) if (~keep).any() else 0.0)
        if not (err[keep] <= pm.PADJ_FD[group]).all():
            failed.append((group, float(err[keep].max())))
    assert not failed, (name, failed)
