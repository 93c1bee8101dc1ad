"""The multi-seed adjoint (hmpc_solve_adjoint_multi, csrc/hmpc_adjoint_multi.hip), the selection of one of its slices as the current
adjoint (hmpc_select_adjoint_seed) and ``autograd.wrench_jacobian``.

The reference is hmpc_solve_adjoint itself, seed by seed, on the same handle behind the same solve: every output of slice s must be bit
for bit what the single-seed launch returns under seed s (tests/test_gpu_adjoint.py pins that launch to the numpy definition), so no
tolerance enters but the two the single-seed tests already use against the gains."""
import ctypes as C

import numpy as np
import pytest

import adjoint_mirror as am
import feedback_mirror as fm
import limit_adjoint_mirror as lam
import model_adjoint_mirror as mm
import pose_adjoint_mirror as pm
from hector_simulation_amd import interface, records, synthetic
from test_certificate_mirror import CASES, case_records
from test_gpu_adjoint import SMALL, _device, _torch, adjoint_with, assert_same_bits, solved

pytestmark = pytest.mark.gpu
E_ARG = -1
BY_NAME = {**{c[0]: c[1] for c in CASES}, **{s[0]: s for s in SMALL}}
BIT_CASES = ["standing", "walking", "single_h20", "standing_3c", "h1", "h11", "hard_6x"]


def seed_set(S, nb, h, U):
    """S different seeds[nb, h, U] of the finite-difference tests' kind."""
    return np.stack([am.seeds(nb, h, U, rng_seed=40 + s) for s in range(S)])


def multi_with(mpc, seeds):
    """One multi-seed adjoint of a solved handle under seeds[S, b, h, U] (float64), downloaded."""
    t = _device(np.asarray(seeds, dtype=np.float64))
    mpc.solve_adjoint_multi(t.data_ptr(), seeds.shape[0])
    return mpc.download_adjoint_multi()


def slice_of(m, s):
    return {key: m[key][s] for key in am.KEYS}


def shape_of(case):
    return case[2], case[3], case[4]  # h, nb, nc


def chain_behind(mpc, seed_ptr):
    """model -> limits -> record behind the current adjoint, and the current adjoint itself, downloaded"""
    mpc.adjoint_model()
    mpc.adjoint_limits(seed_ptr)
    mpc.adjoint_record()
    return mpc.download_adjoint(), mpc.download_adjoint_model(), mpc.download_adjoint_limits(), mpc.download_adjoint_record()


def assert_chain_bits(got, want, what):
    for g, w, keys in zip(got, want, (am.KEYS, mm.KEYS, lam.KEYS, pm.KEYS)):
        for key in keys:
            np.testing.assert_array_equal(g[key].view(np.uint64), w[key].view(np.uint64), err_msg=f"{what} {key}")


# ------------------------------------------------------------------------------------------------ 1. bits, seed by seed
@pytest.mark.parametrize("name", BIT_CASES)
def test_every_slice_is_the_single_seed_adjoint(name):
    case = BY_NAME[name]
    h, nb, nc = shape_of(case)
    U = 6 * nc
    mpc, _, _ = solved(case_records(case), h, nc)
    seeds = seed_set(U + 1, nb, h, U)
    single = [adjoint_with(mpc, seeds[s]) for s in range(U + 1)]
    assert np.abs(single[0]["dir"]).max() > 0.0
    for S in (1, 2, U, U + 1):  # (U + 1: a ragged second launch)
        m = multi_with(mpc, seeds[:S])
        assert m["grad_x0"].shape == (S, nb, 13) and m["grad_traj"].shape == (S, nb, h, 12) and m["dir"].shape == (S, nb, h, U)
        assert mpc.get_device_adjoint_multi()["n_seeds"] == S
        for s in range(S):
            assert_same_bits(slice_of(m, s), single[s], f"{name} S {S} seed {s}")
            np.testing.assert_array_equal(m["summary"][s, :, 0].view(np.uint64), m["summary"][0, :, 0].view(np.uint64))
    assert_same_bits(mpc.download_adjoint(), single[U], "the single-seed adjoint stands beside the multi-seed one")
    mpc.close()


# ------------------------------------------------------------------------------------------------ 2. unit seeds
@pytest.mark.parametrize("name", ["standing", "walking", "standing_3c", "h11"])
def test_unit_seeds_return_the_gpus_own_gains(name):
    case = BY_NAME[name]
    h, nb, nc = shape_of(case)
    U = 6 * nc
    mpc, _, _ = solved(case_records(case), h, nc)
    mpc.feedback_gains()
    g = mpc.download_gains()
    seeds = np.zeros((U, nb, h, U))
    seeds[np.arange(U), :, 0, np.arange(U)] = 1.0
    m = multi_with(mpc, seeds)
    mpc.close()
    worst = 0.0
    for k in range(nb):
        bound = fm.MIRROR_TOL * max(1.0, np.abs(g["gain"][k]).max())
        worst = max(worst, np.abs(m["grad_x0"][:, k] - g["gain"][k]).max() / bound,
                    np.abs(m["grad_traj"][:, k] - g["ref_gain"][k].transpose(1, 0, 2)).max() / bound)
    print(name, "unit seeds of one launch against the GPU's gains / (1e-9 max(1, max|K0|))", worst)
    assert worst <= 1.0, worst
    np.testing.assert_array_equal(m["summary"][0, :, 0].view(np.uint64), g["summary"][:, 0].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 3. selection
@pytest.mark.parametrize("name", ["walking", "standing_3c"])
def test_a_selected_slice_is_the_current_adjoint(name):
    case = BY_NAME[name]
    h, nb, nc = shape_of(case)
    U = 6 * nc
    S = 3
    mpc, _, _ = solved(case_records(case), h, nc)
    seeds = seed_set(S, nb, h, U)
    t = _device(seeds)
    want = []
    for s in range(S):
        mpc.solve_adjoint(t[s].data_ptr())
        want.append(chain_behind(mpc, t[s].data_ptr()))
    mpc.solve_adjoint_multi(t.data_ptr(), S)
    for s in (2, 0, 1):
        mpc.select_adjoint_seed(s)
        L, hd = mpc.L, mpc.h
        # a selection is a new adjoint: what stood behind the last one is stale
        assert L.hmpc_download_adjoint_model(hd, *[None] * 5) == E_ARG and L.hmpc_download_adjoint_limits(hd, *[None] * 6) == E_ARG
        assert L.hmpc_adjoint_record(hd, None) == E_ARG
        assert_chain_bits(chain_behind(mpc, t[s].data_ptr()), want[s], f"{name} selected seed {s}")
    # whichever came last: a single launch replaces the selection, a selection the single launch
    mpc.solve_adjoint(t[1].data_ptr())
    assert_same_bits(mpc.download_adjoint(), want[1][0], "a single launch behind a selection")
    mpc.select_adjoint_seed(2)
    assert_same_bits(mpc.download_adjoint(), want[2][0], "a selection behind a single launch")
    # a new multi-seed launch overwrites the slice: the selection falls with it, the multi-seed adjoint stands
    mpc.solve_adjoint_multi(t.data_ptr(), 2)
    assert mpc.L.hmpc_download_adjoint(mpc.h, *[None] * 6) == E_ARG and mpc.L.hmpc_adjoint_model(mpc.h, None) == E_ARG
    assert mpc.L.hmpc_select_adjoint_seed(mpc.h, 2) == E_ARG  # (two seeds now)
    mpc.select_adjoint_seed(1)
    assert_same_bits(mpc.download_adjoint(), want[1][0], "after a second multi-seed launch")
    mpc.close()


# ------------------------------------------------------------------------------------------------ 4. buffers, orders, sweeps, groups
def test_pure_function_of_record_force_buffer_and_seeds():
    torch = _torch()
    case = BY_NAME["walking"]
    h, nb, nc, k = 10, 16, 2, 4
    U, S = 6 * nc, 3
    rec = np.repeat(case_records(case)[:nb // k], k, axis=0)  # groups of four records that share everything: a command sweep may solve them
    seeds = seed_set(S, nb, h, U)
    t_seeds = _device(seeds)
    mpc0, _, _ = solved(rec, h, nc)
    own = multi_with(mpc0, seeds)  # (handle-owned buffers)
    for s in range(S):
        assert_same_bits(slice_of(own, s), adjoint_with(mpc0, seeds[s]), f"handle-owned, seed {s}")
    more = multi_with(mpc0, seed_set(S + 2, nb, h, U))  # (the handle's own buffers grow)
    for s in range(S):
        assert_same_bits(slice_of(more, s), slice_of(own, s), f"after the buffers grew, seed {s}")
    mpc0.close()
    t_f = torch.zeros((nb, U * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    shapes = dict(grad_x0=(S, nb, 13), grad_traj=(S, nb, h, 12), grad_weights=(S, nb, 12), grad_alpha=(S, nb, U), dir=(S, nb, h, U), summary=(S, nb, 2))
    mine = {key: torch.zeros(s, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_adjoint_multi(S, *[mine[key].data_ptr() for key in am.KEYS], keepalive=mine)
    assert mpc.get_device_adjoint_multi() == dict({key: mine[key].data_ptr() for key in am.KEYS}, n_seeds=0)
    mpc.upload(rec)
    for order in (0, 1):
        mpc.set_dispatch_order(order)
        mpc.solve()
        mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
        torch.cuda.synchronize()
        assert_same_bits({key: mine[key].cpu().numpy() for key in am.KEYS}, own, f"caller-owned buffers, dispatch order {order}")
        assert_same_bits(mpc.download_adjoint_multi(), own, f"downloaded from the caller's buffers, dispatch order {order}")
    assert mpc.L.hmpc_solve_adjoint_multi(mpc.h, C.c_void_p(t_seeds.data_ptr()), S + 1, None) == E_ARG  # (the caller's buffers hold S slices)
    f_solve = t_f.cpu().numpy().copy()
    mpc.solve_command_sweep(k)
    mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
    swept = mpc.download_adjoint_multi()
    np.testing.assert_array_equal(t_f.cpu().numpy().view(np.uint32), f_solve.view(np.uint32))  # (same forces in ...)
    assert_same_bits(swept, own, "after a command sweep")  # (... same adjoints out)
    mpc.close()
    # a device group's members against the plain handle
    grp = interface.DeviceGroup(synthetic.DT_MPC, h, synthetic.F_MAX, nb, [0, 0], transport="p2p")
    grp.upload(rec)
    grp.solve()
    grp.download()
    L = grp.L
    for i in range(grp.size):
        hd, _, lo, n, st = grp.member(i)
        t_part = _device(seeds[:, lo:lo + n])
        assert L.hmpc_solve_adjoint_multi(hd, C.c_void_p(t_part.data_ptr()), S, C.c_void_p(st)) == 0
        got = {key: np.zeros((S, n) + shapes[key][2:]) for key in am.KEYS}
        assert L.hmpc_download_adjoint_multi(hd, *[got[key].ctypes.data for key in am.KEYS]) == 0
        assert_same_bits(got, {key: own[key][:, lo:lo + n] for key in am.KEYS}, f"group member {i}")
        assert L.hmpc_select_adjoint_seed(hd, 1) == 0
        one = {key: np.zeros((n,) + shapes[key][2:]) for key in am.KEYS}
        assert L.hmpc_download_adjoint(hd, *[one[key].ctypes.data for key in am.KEYS]) == 0
        assert_same_bits(one, {key: own[key][1, lo:lo + n] for key in am.KEYS}, f"group member {i}, seed 1 selected")
    grp.close()


# ------------------------------------------------------------------------------------------------ 5. errors and staleness
def test_errors_enqueue_nothing_and_a_multi_seed_adjoint_goes_stale():
    torch = _torch()
    h, U, S = 10, 12, 3
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    shapes = dict(grad_x0=(S, 16, 13), grad_traj=(S, 16, h, 12), grad_weights=(S, 16, 12), grad_alpha=(S, 16, U), dir=(S, 16, h, U), summary=(S, 16, 2))
    mine = {key: torch.full(s, -7.0, dtype=torch.float64, device="cuda") for key, s in shapes.items()}
    t_seeds = _device(seed_set(S, 16, h, U))
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    ptrs = [mine[key].data_ptr() for key in am.KEYS]
    mpc.set_device_adjoint_multi(S, *ptrs, keepalive=mine)
    host = [np.full(shapes[key], -9.0) for key in am.KEYS]
    seed_p = C.c_void_p(t_seeds.data_ptr())

    def snapshot():
        torch.cuda.synchronize()
        return [mine[key].cpu().numpy().copy() for key in am.KEYS]

    def refused(what, before, solve_too, download_too=True):
        """download, selection (and, where no solve of the batch exists, the launch) answer HMPC_E_ARG; nothing on the device or in the
        host moved"""
        if download_too:
            assert L.hmpc_download_adjoint_multi(hd, *[a.ctypes.data for a in host]) == E_ARG, what
        assert L.hmpc_select_adjoint_seed(hd, 0) == E_ARG, what
        if solve_too:
            assert L.hmpc_solve_adjoint_multi(hd, seed_p, S, None) == E_ARG, what
        assert L.hmpc_solve_adjoint_multi(hd, None, S, None) == E_ARG, what
        for n in (0, -1, S + 1, interface_max_seeds() + 1):  # (S + 1: more than the caller's buffers hold)
            assert L.hmpc_solve_adjoint_multi(hd, seed_p, n, None) == E_ARG, (what, n)
        assert all((a == -9).all() for a in host), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    assert L.hmpc_solve_adjoint_multi(None, seed_p, S, None) == E_ARG and L.hmpc_select_adjoint_seed(None, 0) == E_ARG
    assert L.hmpc_set_device_adjoint_multi(hd, 0, *[C.c_void_p(p) for p in ptrs]) == E_ARG  # (buffers for no seed)
    assert L.hmpc_set_device_adjoint_multi(hd, interface_max_seeds() + 1, *[C.c_void_p(p) for p in ptrs]) == E_ARG
    s0 = snapshot()
    refused("before a batch", s0, True, download_too=False)  # (a download of the empty batch copies nothing and is no error)
    assert L.hmpc_download_adjoint_multi(hd, *[a.ctypes.data for a in host]) == 0 and all((a == -9).all() for a in host)
    mpc.upload(rec_a)
    refused("before a solve of the batch", s0, True)
    mpc.solve()
    refused("a solve, no multi-seed adjoint from it", s0, False)
    mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
    first = mpc.download_adjoint_multi()
    s1 = snapshot()
    assert (s1[0] != -7.0).all() and (s1[4] != -7.0).any()
    assert L.hmpc_select_adjoint_seed(hd, S) == E_ARG and L.hmpc_select_adjoint_seed(hd, -1) == E_ARG
    assert L.hmpc_download_adjoint(hd, *[None] * 6) == E_ARG  # (no selection, no single launch: no current adjoint)
    mpc.select_adjoint_seed(S - 1)
    assert_same_bits(mpc.download_adjoint(), slice_of(first, S - 1), "the selected slice")
    mpc.set_device_adjoint_multi(S, *ptrs, keepalive=mine)  # a retarget: whatever was computed went elsewhere, the selection with it
    refused("after a retarget", s1, False)
    assert L.hmpc_download_adjoint(hd, *[None] * 6) == E_ARG and L.hmpc_adjoint_model(hd, None) == E_ARG
    mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
    assert_same_bits(mpc.download_adjoint_multi(), first, "after the retarget")
    mpc.select_adjoint_seed(0)
    mpc.solve()
    refused("after a second solve", s1, False)
    assert L.hmpc_download_adjoint(hd, *[None] * 6) == E_ARG
    mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
    mpc.upload(rec_b)
    s2 = snapshot()
    refused("after a new upload", s2, True)
    mpc.solve()
    refused("after a solve of the new batch", s2, False)
    t_b = _device(seed_set(S, 8, h, U))
    mpc.solve_adjoint_multi(t_b.data_ptr(), S)
    second = mpc.download_adjoint_multi()
    assert second["dir"].shape == (S, 8, h, U)
    for s in range(S):  # (seed-major over the CURRENT batch of 8, in buffers with room for 16)
        assert_same_bits(slice_of(second, s), adjoint_with(mpc, seed_set(S, 8, h, U)[s]), f"the smaller batch, seed {s}")
    mpc.close()


def interface_max_seeds():
    import re
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define HMPC_ADJOINT_MAX_SEEDS (\d+)", open(os.path.join(root, "include", "hector_mpc.h")).read()).group(1))


# ------------------------------------------------------------------------------------------------ 6. the wrench Jacobian
def test_wrench_jacobian_rows_are_backward_under_unit_grad_outputs():
    torch = _torch()
    from hector_simulation_amd.autograd import differentiable_solve_fields, wrench_jacobian

    h, nb, nc = 10, 8, 2
    U = 6 * nc
    fields = synthetic.hard_batch(nb, h, "standing", seed=17, scale=3.0)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    sl = pm.slices(nc, h)
    names = ("p", "v", "q", "w", "r", "joint_angles", "weights", "Alpha_K", "traj")
    leaves = {key: torch.tensor(np.asarray(fields[key], dtype=np.float32).reshape(nb, -1), dtype=torch.float64, requires_grad=True) for key in names}
    forces = differentiable_solve_fields(mpc, {**fields, **leaves})
    generation = mpc.generation
    jac, grad_params, grad_limits = wrench_jacobian(mpc, 0, generation=generation)
    assert jac.is_cuda and jac.dtype == torch.float64 and tuple(jac.shape) == (nb, U, sl["traj"].stop)
    assert tuple(grad_params.shape) == (nb, U, 4) and tuple(grad_limits.shape) == (nb, U, 3 + nc)
    torch.cuda.synchronize()
    J = jac.cpu().numpy()
    mpc.feedback_gains()
    g = mpc.download_gains()
    for c in range(U):
        for t in leaves.values():
            t.grad = None
        e = torch.zeros((nb, h * U), dtype=torch.float32, device="cuda")
        e[:, c] = 1.0  # (step 0, component c)
        forces.backward(gradient=e, retain_graph=True)
        torch.cuda.synchronize()
        for key in names:
            np.testing.assert_array_equal(leaves[key].grad.numpy().view(np.uint64), J[:, c, sl[key]].view(np.uint64), err_msg=f"row {c}, {key}")
        np.testing.assert_array_equal(mpc.download_adjoint_model()["grad_params"].view(np.uint64), grad_params[:, c].cpu().numpy().view(np.uint64))
        np.testing.assert_array_equal(mpc.download_adjoint_limits()["grad_limits"].view(np.uint64), grad_limits[:, c].cpu().numpy().view(np.uint64))
    # the state's columns that enter x0 alone: position (x0[3:6]) and velocity (x0[9:12]) are the gains' columns
    worst = 0.0
    for k in range(nb):
        bound = fm.MIRROR_TOL * max(1.0, np.abs(g["gain"][k]).max())
        worst = max(worst, np.abs(J[k][:, sl["p"]] - g["gain"][k][:, 3:6]).max() / bound, np.abs(J[k][:, sl["v"]] - g["gain"][k][:, 9:12]).max() / bound)
    print("wrench_jacobian's p and v columns against the GPU's gains / (1e-9 max(1, max|K0|))", worst)
    assert worst <= 1.0, worst
    assert np.abs(J[:, :, sl["q"]]).max() > 0.0 and np.abs(J[:, :, sl["r"]]).max() > 0.0
    J1, _, _ = wrench_jacobian(mpc, 1)
    assert (J1.cpu().numpy() != J).any()
    with pytest.raises(ValueError, match="outside the horizon"):
        wrench_jacobian(mpc, h)
    mpc.solve()
    with pytest.raises(RuntimeError, match="has solved another batch since"):
        wrench_jacobian(mpc, 0, generation=generation)
    mpc.close()
