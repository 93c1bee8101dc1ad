"""Constraint margins of every solved instance (hmpc_constraint_margins, csrc/hmpc_margins.hip), the penalty built from them
(hmpc_margin_penalty) and the planning tick that respects a floor (hmpc_set_sweep_margin_floor).

The reference is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/margins_mirror.py), fed with the ORACLE's
binary32 constraint block of each record and THE GPU'S OWN downloaded float32 forces: no solver tolerance enters the slacks, what is left
is binary64 round-off (numpy has no fused multiply-add), bounded per row by 64 * 2^-53 * sum |Fc u|.  The minima, the penalty and the
selection are compared as bit patterns."""
import numpy as np
import pytest

import margins_mirror as mm
import prediction_mirror as pm
import selection_mirror as sm
from hector_simulation_amd import interface, records, synthetic
from test_margins_mirror import FEAS_MARGIN, FEAS_MEASURED, PARAM_SET_0

pytestmark = pytest.mark.gpu
H = 10
NAN = float("nan")
E_ARG = -1
LEG_OFFSET = np.tile([0.0, 0.0, 0.3 * 3.14159, -0.6 * 3.14159, 0.3 * 3.14159], 2)  # LegController.cpp:111-113

_cache = {}


def _torch():
    import torch

    return torch


def _device(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def margins_of(rec, h, nc=2, prepare=None, keep=False):
    """(forces, status, margins) of a fresh handle: solve, download, margins, download."""
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, rec.shape[0], contacts=nc)
    if prepare:
        prepare(mpc)
    mpc.upload(rec)
    mpc.solve()
    forces, status = mpc.download()
    mpc.constraint_margins()
    m = mpc.download_margins()
    if keep:
        return mpc, forces, status, m
    mpc.close()
    return forces, status, m


def solved_shape(oracle, shape):
    """One solve + margins per shape, and the numpy definition on the downloaded forces; shared by the tests, left unchanged."""
    name, gait, h, nb, nc, seed = shape
    if name not in _cache:
        _, rec = pm.shape_records(shape)
        forces, status, m = margins_of(rec, h, nc)
        _cache[name] = dict(rec=rec, forces=forces, status=status, m=m, ref=mm.margins_records(oracle, rec, h, nc, forces))
    return _cache[name]


def assert_is_the_definition(m, ref, rec, h, nc, what=""):
    """Slacks within the derived bound of the mirror's, +inf patterns identical; summary and where bit for bit the lexicographic minima
    of the GPU's OWN slacks."""
    got, want = m["slack"], ref["slack"]
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=f"{what} +inf pattern")
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    print(what, "largest slack error / bound", float((err / np.maximum(ref["bound"][fin], 1e-300)).max()) if fin.any() else 0.0)
    assert (err <= ref["bound"][fin]).all(), (what, err.max())
    gaits, caps = mm.batch_caps(rec, h, nc)
    summary, where = mm.lexmin_of_slacks(got, gaits, caps)
    np.testing.assert_array_equal(m["where"], where, err_msg=f"{what} where")
    np.testing.assert_array_equal(m["summary"].view(np.uint64), summary.view(np.uint64), err_msg=f"{what} summary")


# ------------------------------------------------------------------------------------------------ 1. definition
@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_slacks_and_minima_are_the_definition(oracle, shape):
    name, gait, h, nb, nc, seed = shape
    d = solved_shape(oracle, shape)
    assert d["m"]["slack"].shape == (nb, h, nc, 10) and d["m"]["summary"].shape == (nb, 6) and d["m"]["where"].shape == (nb, 6)
    assert_is_the_definition(d["m"], d["ref"], d["rec"], h, nc, name)
    if gait != "standing":
        assert np.isinf(d["m"]["slack"]).any()  # (the shape has swing leg-steps)


# ------------------------------------------------------------------------------------------------ 2. meaning
@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_solved_instances_respect_every_limit(oracle, shape):
    """Every HMPC_S_OK instance has all six class minima >= -4 x the figure measured on the CPU for qpOASES' own forces
    (tests/test_margins_mirror.py FEAS_MEASURED); on the standing shape an active friction or line-contact row is seen as active."""
    name = shape[0]
    d = solved_shape(oracle, shape)
    ok = interface.status_code(d["status"]) == 0
    assert ok.all(), d["status"]
    s = d["m"]["summary"]
    print(name, "class minima over the shape", s[ok].min(axis=0), "bound", -FEAS_MARGIN * FEAS_MEASURED[name])
    assert (s[ok] >= -FEAS_MARGIN * FEAS_MEASURED[name]).all(), s[ok].min(axis=0)
    if name == "standing":
        active = np.minimum(s[:, 0], s[:, 2])
        print(name, "smallest friction / line-contact minimum", active.min())
        assert (active < FEAS_MARGIN * FEAS_MEASURED[name]).any(), active


# ------------------------------------------------------------------------------------------------ 3. constants
def test_params_and_instance_mu_reach_the_margins(oracle):
    shape = ("params", "walking", 10, 8, 2, 107)
    _, rec = pm.shape_records(shape)
    h, nc, nb = 10, 2, 8
    mu = np.linspace(0.3, 1.4, nb).astype(np.float32)
    d_mu = _device(mu)

    def prepare(mpc):
        mpc.set_params(**PARAM_SET_0)
        mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu)

    forces, status, m = margins_of(rec, h, nc, prepare=prepare)
    forces1, status1, m1 = margins_of(rec, h, nc, prepare=lambda mpc: mpc.set_params(**PARAM_SET_0))
    assert (interface.status_code(status) == 0).all() and (interface.status_code(status1) == 0).all()
    try:
        oracle.set_params(**PARAM_SET_0)
        assert_is_the_definition(m, mm.margins_records(oracle, rec, h, nc, forces, mu=mu), rec, h, nc, "params + instance mu")
        assert_is_the_definition(m1, mm.margins_records(oracle, rec, h, nc, forces1), rec, h, nc, "params")
    finally:
        oracle.set_params()
    _, _, m0 = margins_of(rec, h, nc)
    fin = np.isfinite(m0["slack"])
    assert np.abs(m1["slack"][fin] - m0["slack"][fin]).max() > 1e-3 and np.abs(m["slack"][fin] - m1["slack"][fin]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 4. pure function of the force buffer
def test_pure_function_of_the_force_buffer(oracle):
    """Off-nominal batch with the device-side repair chain: fast, continuation and safe passes write the force buffer; the margins behind
    them on the same stream are the definition on what they left -- with the handle's buffers and with the caller's; twice: same bits."""
    torch = _torch()
    h, nb = 10, 64
    rec = records.pack_records(synthetic.hard_batch(nb, h, "standing", scale=3), h)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_repair(1)
    mpc.upload(rec)
    mpc.solve()
    mpc.constraint_margins()
    m = mpc.download_margins()
    forces, status = mpc.download()
    assert np.isin(interface.status_code(status), (0, 6)).all(), status
    assert_is_the_definition(m, mm.margins_records(oracle, rec, h, 2, forces), rec, h, 2, "hard batch")
    mpc.constraint_margins()
    again = mpc.download_margins()
    for key in ("slack", "summary"):
        np.testing.assert_array_equal(again[key].view(np.uint64), m[key].view(np.uint64), err_msg=key)
    np.testing.assert_array_equal(again["where"], m["where"])
    # caller-owned force, status and margin buffers
    t_f = torch.zeros((nb, 12 * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    t_sl = torch.zeros((nb, h, 2, 10), dtype=torch.float64, device="cuda")
    t_su = torch.zeros((nb, 6), dtype=torch.float64, device="cuda")
    t_w = torch.zeros((nb, 6), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_margins(t_sl.data_ptr(), t_su.data_ptr(), t_w.data_ptr(), keepalive=(t_sl, t_su, t_w))
    mpc.solve()
    mpc.constraint_margins()
    torch.cuda.synchronize()
    via_download = mpc.download_margins()
    mpc.close()
    np.testing.assert_array_equal(t_f.cpu().numpy().view(np.uint32), forces.view(np.uint32))
    mine = dict(slack=t_sl.cpu().numpy(), summary=t_su.cpu().numpy(), where=t_w.cpu().numpy())
    for got in (mine, via_download):
        for key in ("slack", "summary"):
            np.testing.assert_array_equal(got[key].view(np.uint64), m[key].view(np.uint64), err_msg=key)
        np.testing.assert_array_equal(got["where"], m["where"])


# ------------------------------------------------------------------------------------------------ 5. ordering errors
def test_ordering_errors_enqueue_nothing_and_leave_the_buffers_alone():
    torch = _torch()
    h = 10
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=311), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=312, phase="random"), h)
    t_sl = torch.full((16, h, 2, 10), -7.0, dtype=torch.float64, device="cuda")
    t_su = torch.full((16, 6), -7.0, dtype=torch.float64, device="cuda")
    t_w = torch.full((16, 6), -7, dtype=torch.int32, device="cuda")
    t_pen = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    L, hd = mpc.L, mpc.h
    mpc.set_device_margins(t_sl.data_ptr(), t_su.data_ptr(), t_w.data_ptr(), keepalive=(t_sl, t_su, t_w))
    floor = np.array([0.0, NAN, NAN, NAN, NAN, NAN])
    host = dict(slack=np.full((16, h, 2, 10), -9.0), summary=np.full((16, 6), -9.0), where=np.full((16, 6), -9, dtype=np.int32))

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (t_sl, t_su, t_w, t_pen)]

    def refused(what, before):
        """margins, download and penalty all answer HMPC_E_ARG; nothing on the device or in the host arrays moved"""
        assert L.hmpc_download_margins(hd, host["slack"].ctypes.data, host["summary"].ctypes.data, host["where"].ctypes.data) == E_ARG, what
        assert L.hmpc_margin_penalty(hd, floor.ctypes.data, None, t_pen.data_ptr(), None) == E_ARG, what
        assert (host["slack"] == -9.0).all() and (host["summary"] == -9.0).all() and (host["where"] == -9).all(), what
        for a, b in zip(snapshot(), before):
            np.testing.assert_array_equal(a, b, err_msg=what)

    s0 = snapshot()
    assert L.hmpc_constraint_margins(hd, None) == E_ARG  # no batch, no solve
    mpc.upload(rec_a)
    assert L.hmpc_constraint_margins(hd, None) == E_ARG  # a batch, no solve of it
    refused("before any solve", s0)
    mpc.solve()
    refused("a solve, no margins from it", s0)
    mpc.constraint_margins()
    first = mpc.download_margins()
    mpc.margin_penalty(floor, t_pen.data_ptr())
    s1 = snapshot()
    assert (s1[0] != -7.0).all() and (s1[3] != -7.0).all()
    mpc.upload(rec_b)
    assert L.hmpc_constraint_margins(hd, None) == E_ARG  # batch A's solve does not count for batch B
    refused("after a new upload", s1)
    mpc.solve()
    refused("after a solve of the new batch", s1)
    mpc.constraint_margins()
    mpc.download_margins()
    mpc.solve()
    refused("after a second solve", snapshot())
    mpc.constraint_margins()
    second = mpc.download_margins()
    mpc.close()
    _, _, fresh = margins_of(rec_b, h)
    assert second["slack"].shape == (8, h, 2, 10)
    np.testing.assert_array_equal(second["slack"].view(np.uint64), fresh["slack"].view(np.uint64))
    np.testing.assert_array_equal(second["summary"].view(np.uint64), fresh["summary"].view(np.uint64))
    assert not np.array_equal(first["summary"][:8], second["summary"])


# ------------------------------------------------------------------------------------------------ 6. penalty
def test_penalty_is_the_rule_on_the_summary_bit_for_bit(oracle):
    torch = _torch()
    shape = pm.SHAPES[0]
    name, gait, h, nb, nc, seed = shape
    rec = solved_shape(oracle, shape)["rec"]
    t_f = torch.zeros((nb, 12 * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    t_su = torch.zeros((nb, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_margins(0, t_su.data_ptr(), 0, keepalive=(t_su,))
    mpc.upload(rec)
    mpc.solve()
    torch.cuda.synchronize()
    t_f[3, :] = NAN  # a poisoned slot: no value of it enters a minimum (+inf, -1 by the definition)
    t_f[5, 2] = float("inf")
    torch.cuda.synchronize()
    mpc.constraint_margins()
    m = mpc.download_margins()
    assert (m["where"][3] == -1).all() and np.isinf(m["summary"][3]).all() and not np.isnan(m["summary"]).any()
    forces = t_f.cpu().numpy()
    gaits, caps = mm.batch_caps(rec, h, nc)
    summary, where = mm.lexmin_of_slacks(m["slack"], gaits, caps)
    np.testing.assert_array_equal(m["summary"].view(np.uint64), summary.view(np.uint64))
    np.testing.assert_array_equal(m["where"], where)
    ref = mm.margins_records(oracle, rec, h, nc, forces)
    np.testing.assert_array_equal(np.isnan(m["slack"]), np.isnan(ref["slack"]))
    pen = np.random.default_rng(6).uniform(0.0, 20.0, nb)
    d_pen = _device(pen)
    d_out = torch.full((nb,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def run(floor, with_pen, in_place=False, summ=None):
        src = _device(pen) if in_place else d_pen
        dst = src if in_place else d_out
        mpc.margin_penalty(floor, dst.data_ptr(), src.data_ptr() if with_pen else 0)
        torch.cuda.synchronize()
        want = mm.penalty(m["summary"] if summ is None else summ, floor, pen if with_pen else None)
        np.testing.assert_array_equal(dst.cpu().numpy().view(np.uint64), want.view(np.uint64), err_msg=str(floor))
        return want

    assert np.array_equal(run([NAN] * 6, True), pen)  # all-NaN floor: pass-through
    assert (run([NAN] * 6, False).view(np.uint64) == 0).all()  # ... or +0.0
    f5 = float(np.median(m["summary"][:, 5]))
    masked = run([NAN] * 5 + [f5], True)
    assert np.isinf(masked).any() and np.isfinite(masked).any()
    run([NAN] * 5 + [f5], True, in_place=True)
    run([0.0, 0.0, -1e-6, 0.0, 0.0, NAN], False)
    # a NaN in the summary masks (the margins kernel never writes one: the caller's buffer is poked)
    t_su[7, 1] = NAN
    torch.cuda.synchronize()
    poked = m["summary"].copy()
    poked[7, 1] = NAN
    got = run([NAN, -1e30, NAN, NAN, NAN, NAN], True, summ=poked)
    assert np.isinf(got[7]) and np.isfinite(np.delete(got, 7)).all()
    mpc.close()


# ------------------------------------------------------------------------------------------------ 7. the chain
def _ticks_and_commands(groups, k, seed):
    rng = np.random.default_rng(seed)
    t = synthetic.make_ticks(groups, H, "walking", seed=seed)
    t["gait_offsets"][1::2] = (0, 0)
    t["gait_durations"][1::2] = (H, H)
    motor = t["leg_q"] - LEG_OFFSET
    t["leg_q"], t["flags"] = motor, 1  # raw motor angles (HMPC_TICK_LEG_Q_MOTOR)
    cmd = np.zeros((groups, k), dtype=interface.COMMAND_DTYPE)
    cmd["v_des_robot"] = rng.uniform(-0.5, 0.5, (groups, k, 2))
    cmd["yaw_rate_des"] = rng.uniform(-0.3, 0.3, (groups, k))
    cmd["roll_des"], cmd["pitch_des"] = rng.uniform(-0.02, 0.02, (groups, k)), rng.uniform(-0.02, 0.02, (groups, k))
    return t, motor, cmd, rng.uniform(0.0, 5.0, groups * k)


def test_tick_sweep_device_with_a_margin_floor_equals_the_separate_calls():
    torch = _torch()
    groups, k = 8, 16
    b = groups * k
    t, motor, cmd, pen = _ticks_and_commands(groups, k, 331)
    d_t = _device(t.view(np.uint8).reshape(groups, -1).copy())
    d_c = _device(cmd.view(np.uint8).reshape(b, -1).copy())
    d_p = _device(pen)
    outs = [torch.zeros((groups, n), dtype=torch.float64, device="cuda") for n in (10, 12, 2)]
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, b)

    def tick():
        mpc.tick_sweep_device(d_t.data_ptr(), groups, d_c.data_ptr(), k, synthetic.DT_MPC, outs[0].data_ptr(), outs[1].data_ptr(),
                              outs[2].data_ptr(), d_p.data_ptr())
        sel = mpc.download_selection()
        return sel, [o.cpu().numpy().copy() for o in outs]

    sel0, out0 = tick()  # no floor: the launches of the parent
    assert sel0["index"][0] >= 0
    mpc.constraint_margins()
    v = mpc.download_margins()["summary"][sel0["index"][0], 5]
    assert np.isfinite(v)
    floor = np.array([NAN] * 5 + [np.nextafter(v, np.inf)])
    mpc.set_sweep_margin_floor(floor)
    sel1, out1 = tick()
    mpc.set_sweep_margin_floor(None)
    sel2, out2 = tick()
    mpc.close()
    sm.assert_equal(sel2, sel0, "floor cleared")
    for a, c in zip(out2, out0):
        np.testing.assert_array_equal(a.view(np.uint64), c.view(np.uint64))
    assert sel1["index"][0] != sel0["index"][0]  # group 0's unmasked winner is masked: another one, or -1
    # the separate calls: expand, build, sweep, predict, margins, penalty, select, torques
    te = sm.expand_ticks(t, cmd)
    sep = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, b)
    wpd = sep.build_records(te, synthetic.DT_MPC)
    sep.solve_command_sweep(k)
    forces, status = sep.download()
    assert (interface.status_code(status) == 0).all(), status
    sep.predict_states()
    states, cost = sep.download_prediction()
    sep.constraint_margins()
    m = sep.download_margins()
    d_out = torch.zeros(b, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sep.margin_penalty(floor, d_out.data_ptr(), d_p.data_ptr())
    sep.sweep_select(k, d_out.data_ptr())
    sel_sep = sep.download_selection()
    f_ff, tau = sep.leg_torques(te["rBody"], np.repeat(motor, k, axis=0))
    sep.close()
    sm.assert_equal(sel1, sel_sep, "tick with a floor against the separate calls")
    want_pen = mm.penalty(m["summary"], floor, pen)
    np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint64), want_pen.view(np.uint64))
    sm.assert_equal(sel1, sm.select(cost, states, status, forces, k, want_pen), "tick with a floor against the mirrors")
    won = sel1["index"] >= 0
    assert won.any()
    win = (np.arange(groups) * k + sel1["index"])[won]
    np.testing.assert_array_equal(out1[0][won].view(np.uint64), tau.reshape(b, 10)[win].view(np.uint64), err_msg="tau")
    np.testing.assert_array_equal(out1[1][won].view(np.uint64), f_ff.reshape(b, 12)[win].view(np.uint64), err_msg="f_ff")
    np.testing.assert_array_equal(out1[2].view(np.uint64), wpd[::k].view(np.uint64), err_msg="wpd")


# ------------------------------------------------------------------------------------------------ 8. legacy
def test_legacy_surface_is_the_batched_margins():
    h = 10
    f = synthetic.make_batch(1, h, "walking", seed=115, phase="random")
    rec = records.pack_records(f, h)
    _, status, m = margins_of(rec, h)
    assert interface.status_code(status)[0] == 0
    interface.setup_problem(synthetic.DT_MPC, h, 0.25, synthetic.F_MAX)
    interface.update_problem_data(f["p"][0], f["v"][0], f["q"][0], f["w"][0], f["r"][0], f["joint_angles"][0], f["yaw"][0], f["weights"][0],
                                  f["traj"][0], f["Alpha_K"][0], f["gait"][0])
    got = np.array([[[interface.legacy_constraint_slack(i, c, j) for j in range(10)] for c in range(2)] for i in range(h)])
    np.testing.assert_array_equal(got.view(np.uint64), m["slack"][0].view(np.uint64))
    assert np.isinf(got).any() and np.isfinite(got).any()
    for i, c, j in ((-1, 0, 0), (h, 0, 0), (0, -1, 0), (0, 2, 0), (0, 0, -1), (0, 0, 10), (h + 5, 7, 20)):
        assert interface.legacy_constraint_slack(i, c, j) == 0.0
