"""Where a handle's outputs go (csrc/hmpc_device_buffer.h OutputBuffer, as the handle of csrc/hmpc_handle.h uses it): its own buffers, the caller's, and its
own again after the caller's were reset to NULL -- the same bits every time, in the buffers hmpc_get_device_* names.

One batch: 8 instances of the standing case at h = 10 (the 120-variable shape) as 2 groups of 4 commands, device repair on; every run is
solve -> command sweep -> prediction -> selection."""
import ctypes as C

import numpy as np
import pytest

from hector_simulation_amd import interface, records, synthetic
from test_gpu_command_sweep import sweep_fields

pytestmark = pytest.mark.gpu
H, GROUPS, K = 10, 2, 4
B = GROUPS * K
NAMES = ("forces", "status", "states", "cost", "index", "score", "sel_forces", "sel_status", "sel_states")


def _pointers(mpc):
    """what hmpc_get_device_outputs / _prediction / _selection name, as integers, in the order of NAMES"""
    p = [C.c_void_p() for _ in NAMES]
    L, r = mpc.L, C.byref
    interface._check(L.hmpc_get_device_outputs(mpc.h, r(p[0]), r(p[1])), "hmpc_get_device_outputs")
    interface._check(L.hmpc_get_device_prediction(mpc.h, r(p[2]), r(p[3])), "hmpc_get_device_prediction")
    interface._check(L.hmpc_get_device_selection(mpc.h, r(p[4]), r(p[5]), r(p[6]), r(p[7]), r(p[8]), None), "hmpc_get_device_selection")
    return dict(zip(NAMES, [int(x.value or 0) for x in p]))


def _run(mpc, rec):
    mpc.upload(rec)
    mpc.solve()
    mpc.solve_command_sweep(K)
    mpc.predict_states()
    mpc.sweep_select(K)
    forces, status = mpc.download()
    states, cost = mpc.download_prediction()
    sel = mpc.download_selection()
    return dict(forces=forces, status=status, states=states, cost=cost, index=sel["index"], score=sel["score"], sel_forces=sel["forces"],
                sel_status=sel["status"], sel_states=sel["states"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_same_bits(got, want, what):
    for n in NAMES:
        assert got[n].shape == want[n].shape, (what, n)
        np.testing.assert_array_equal(_bits(got[n]), _bits(want[n]), err_msg=f"{what}: {n}")


def test_own_buffers_caller_buffers_and_own_again_give_the_same_bits():
    import torch

    rec = records.pack_records(sweep_fields(GROUPS, K, H, "standing", seed=301), H)

    # 1. a fresh handle, its own buffers
    m1 = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, B)
    m1.set_device_repair(1)
    want = _run(m1, rec)
    p1 = _pointers(m1)
    m1.close()
    assert (interface.status_code(want["status"]) == 0).all(), want["status"]
    assert (want["index"] >= 0).all() and (want["index"] < K).all()
    assert all(p1.values()) and len(set(p1.values())) == len(NAMES), p1

    # 2. a second handle, caller-supplied tensors for outputs, prediction and selection
    def fresh():
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        t = dict(forces=torch.full((B, 12 * H), 7.0, dtype=f32, device="cuda"), status=torch.full((B,), 77, dtype=i32, device="cuda"),
                 states=torch.full((B, H, 13), 7.0, dtype=f32, device="cuda"), cost=torch.full((B, 2), 7.0, dtype=f64, device="cuda"),
                 index=torch.full((GROUPS,), 77, dtype=i32, device="cuda"), score=torch.full((GROUPS,), 7.0, dtype=f64, device="cuda"),
                 sel_forces=torch.full((GROUPS, 12 * H), 7.0, dtype=f32, device="cuda"),
                 sel_status=torch.full((GROUPS,), 77, dtype=i32, device="cuda"),
                 sel_states=torch.full((GROUPS, H, 13), 7.0, dtype=f32, device="cuda"))
        torch.cuda.synchronize()
        return t

    t = fresh()
    sentinel = {n: t[n].cpu().numpy() for n in NAMES}
    m2 = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, B)
    m2.set_device_repair(1)
    m2.set_device_outputs(t["forces"].data_ptr(), t["status"].data_ptr(), keepalive=t)
    m2.set_device_prediction(t["states"].data_ptr(), t["cost"].data_ptr())
    m2.set_device_selection(*[t[n].data_ptr() for n in ("index", "score", "sel_forces", "sel_status", "sel_states")])
    got2 = _run(m2, rec)
    p2 = _pointers(m2)
    torch.cuda.synchronize()
    assert p2 == {n: t[n].data_ptr() for n in NAMES}
    _assert_same_bits(got2, want, "caller's buffers, downloaded")
    _assert_same_bits({n: t[n].cpu().numpy() for n in NAMES}, want, "caller's buffers, read directly")

    # 3. the same handle after each of them was reset to NULL: its own buffers, allocated now, and the caller's left alone
    for n in NAMES:
        t[n].copy_(torch.from_numpy(sentinel[n]).cuda())
    torch.cuda.synchronize()
    m2.set_device_outputs(0, 0, keepalive=t)
    m2.set_device_prediction(0, 0)
    m2.set_device_selection(0, 0, 0, 0, 0)
    got3 = _run(m2, rec)
    p3 = _pointers(m2)
    torch.cuda.synchronize()
    m2.close()
    assert all(p3.values()) and len(set(p3.values())) == len(NAMES), p3
    assert not set(p3.values()) & set(p2.values()), (p2, p3)
    _assert_same_bits(got3, want, "own buffers after the reset")
    _assert_same_bits({n: t[n].cpu().numpy() for n in NAMES}, sentinel, "caller's buffers after the reset")
