"""Predicted state trajectory and tracking cost (hmpc_predict_states, csrc/hmpc_predict.hip).

The reference for every comparison is the definition itself (include/hector_mpc.h) restated in numpy float64 (tests/prediction_mirror.py),
fed with the ORACLE's binary32 Acd / Bcd / x0 of each record and with THE GPU'S OWN downloaded float32 forces: no solver tolerance
enters, what is left is binary64 round-off (numpy has no fused multiply-add), which can flip one float32 rounding and nothing more."""
import numpy as np
import pytest

import prediction_mirror as pm
from hector_simulation_amd import interface, records, synthetic

pytestmark = pytest.mark.gpu

# Cost identity  cost[0] + cost[1] - ||e||^2_S = 0.5 u'Hu + g'u  against qpOASES' objective: the expression of the test below, evaluated
# on the CPU with qpOASES' own forces (binary64, and rounded to binary32: the same figures) for these shapes and seeds -- the binary32
# round-off of the reference's H and g.  Asserted at 4x: the margin covers the GPU forces' <= 6e-8 distance from qpOASES'.
IDENTITY_MEASURED = {"standing": 5.203e-07, "walking": 5.596e-07, "mixed": 5.846e-07, "single_h20": 3.715e-07, "walking_h5": 3.205e-07,
                     "standing_3c": 3.266e-06}
IDENTITY_MARGIN = 4.0

_cache = {}


def solved_shape(oracle, shape):
    """One solve + prediction per shape, and the numpy definition on the downloaded forces; shared by the tests, left unchanged."""
    name, gait, h, nb, nc, seed = shape
    if name not in _cache:
        f, rec = pm.shape_records(shape)
        mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
        mpc.upload(rec)
        mpc.solve()
        forces, status = mpc.download()
        mpc.predict_states()
        states, cost = mpc.download_prediction()
        mpc.close()
        ref_states, ref_cost = pm.predict_records(oracle, rec, h, nc, forces)
        _cache[name] = dict(rec=rec, forces=forces, status=status, states=states, cost=cost, ref_states=ref_states, ref_cost=ref_cost)
    return _cache[name]


def x0_gravity(oracle, rec, h, nc):
    return np.array([oracle.assemble_record(r, h, synthetic.DT_MPC, synthetic.F_MAX, reduce=False, nc=nc)["x0"][12] for r in rec], dtype=np.float32)


def predict_batch(rec, h, nc=2, sweep=0, **params):
    """(forces, status, states, cost) of a fresh handle."""
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, rec.shape[0], contacts=nc)
    if params:
        mpc.set_params(**params)
    mpc.upload(rec)
    if sweep:
        mpc.solve_command_sweep(sweep)
    else:
        mpc.solve()
    forces, status = mpc.download()
    mpc.predict_states()
    states, cost = mpc.download_prediction()
    mpc.close()
    return forces, status, states, cost


@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_states_and_cost_are_the_definition(oracle, shape):
    name, gait, h, nb, nc, seed = shape
    d = solved_shape(oracle, shape)
    assert (interface.status_code(d["status"]) == 0).all(), d["status"]
    assert d["states"].shape == (nb, h, 13) and d["cost"].shape == (nb, 2)
    pm.assert_matches_definition(d["states"], d["cost"], d["ref_states"], d["ref_cost"], x0_gravity(oracle, d["rec"], h, nc))
    assert (d["cost"] > 0).all()


@pytest.mark.parametrize("shape", pm.SHAPES, ids=pm.SHAPE_IDS)
def test_cost_identity_against_the_reference_solver(oracle, shape):
    """J - ||e||^2_S is the QP objective: the GPU's cost, less the cost of applying no force (from the oracle's binary32 powers), against
    the objective qpOASES reports for the same record."""
    name, gait, h, nb, nc, seed = shape
    d = solved_shape(oracle, shape)
    ref = oracle.solve_records(d["rec"], h, synthetic.DT_MPC, synthetic.F_MAX, nc=nc)
    assert ref["n_bad"] == 0
    gaps = []
    for k in range(nb):
        e2 = pm.free_response_cost(oracle, d["rec"][k], h, nc)
        obj = ref["obj"][k]
        gaps.append(abs(d["cost"][k, 0] + d["cost"][k, 1] - e2 - obj) / max(1.0, abs(obj)))
    print(name, "cost identity gap max", max(gaps), "bound", IDENTITY_MARGIN * IDENTITY_MEASURED[name])
    assert max(gaps) <= IDENTITY_MARGIN * IDENTITY_MEASURED[name], max(gaps)


def test_params_are_honoured(oracle):
    from test_gpu_assembly import PARAM_SETS

    prm = PARAM_SETS[0]  # the +35 % payload set
    shape = ("params", "walking", 10, 8, 2, 107)
    _, rec = pm.shape_records(shape)
    h, nc = 10, 2
    try:
        oracle.set_params(**prm)
        forces, status, states, cost = predict_batch(rec, h, **prm)
        assert (interface.status_code(status) == 0).all()
        ref_states, ref_cost = pm.predict_records(oracle, rec, h, nc, forces)
        pm.assert_matches_definition(states, cost, ref_states, ref_cost, x0_gravity(oracle, rec, h, nc))
    finally:
        oracle.set_params()
    _, _, states0, _ = predict_batch(rec, h)
    assert np.abs(states - states0).max() > 1e-4  # (the constants really reach the model)


def test_pure_function_of_the_force_buffer(oracle):
    """Off-nominal batch with the device-side repair chain: fast, continuation and safe passes write the force buffer; the prediction
    behind them on the same stream is the definition on what they left -- with the handle's buffers and with the caller's."""
    import torch

    h, nb = 10, 32
    rec = records.pack_records(synthetic.hard_batch(nb, h, "standing", scale=6), h)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb)
    mpc.set_device_repair(1)
    mpc.upload(rec)
    mpc.solve()
    mpc.predict_states()
    forces, status = mpc.download()
    states, cost = mpc.download_prediction()
    assert np.isin(interface.status_code(status), (0, 6)).all(), status
    ref_states, ref_cost = pm.predict_records(oracle, rec, h, 2, forces)
    g = x0_gravity(oracle, rec, h, 2)
    pm.assert_matches_definition(states, cost, ref_states, ref_cost, g)
    # caller-owned force, status and prediction buffers
    t_f = torch.zeros((nb, 12 * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(nb, dtype=torch.int32, device="cuda")
    t_x = torch.zeros((nb, h, 13), dtype=torch.float32, device="cuda")
    t_c = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.set_device_prediction(t_x.data_ptr(), t_c.data_ptr(), keepalive=(t_x, t_c))
    mpc.solve()
    mpc.predict_states()
    torch.cuda.synchronize()
    f2, x2, c2 = t_f.cpu().numpy(), t_x.cpu().numpy(), t_c.cpu().numpy()
    mpc.close()
    np.testing.assert_array_equal(f2.view(np.uint32), forces.view(np.uint32))
    rs2, rc2 = pm.predict_records(oracle, rec, h, 2, f2)
    pm.assert_matches_definition(x2, c2, rs2, rc2, g)
    np.testing.assert_array_equal(x2.view(np.uint32), states.view(np.uint32))
    np.testing.assert_array_equal(c2.view(np.uint64), cost.view(np.uint64))


def test_prediction_after_a_command_sweep_is_bitwise_that_after_a_solve():
    from test_gpu_command_sweep import sweep_fields

    h, groups, k = 10, 4, 4
    rec = records.pack_records(sweep_fields(groups, k, h, "standing", seed=47), h)
    f0, s0, x0, c0 = predict_batch(rec, h)
    f1, s1, x1, c1 = predict_batch(rec, h, sweep=k)
    assert (interface.status_code(s0) == 0).all()
    np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32))
    np.testing.assert_array_equal(x1.view(np.uint32), x0.view(np.uint32))
    np.testing.assert_array_equal(c1.view(np.uint64), c0.view(np.uint64))
    xs = x1.reshape(groups, k, h, 13)
    assert np.abs(xs[:, 0] - xs[:, 1]).max() > 1e-4  # the commands of a group lead to different motions


def test_no_stale_state():
    h = 10
    rec_a = records.pack_records(synthetic.make_batch(16, h, "standing", seed=111), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "walking", seed=112, phase="random"), h)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    with pytest.raises(interface.HmpcError):
        mpc.predict_states()  # no batch, no solve
    mpc.upload(rec_a)
    with pytest.raises(interface.HmpcError):
        mpc.predict_states()  # a batch, no solve of it
    mpc.solve()
    with pytest.raises(interface.HmpcError):
        mpc.download_prediction()  # a solve, no prediction from it
    mpc.predict_states()
    xa, ca = mpc.download_prediction()
    mpc.upload(rec_b)
    with pytest.raises(interface.HmpcError):
        mpc.predict_states()  # batch A's solve does not count for batch B
    mpc.solve()
    mpc.predict_states()
    xb, cb = mpc.download_prediction()
    mpc.close()
    _, _, xf, cf = predict_batch(rec_b, h)
    assert xb.shape == (8, h, 13)
    np.testing.assert_array_equal(xb.view(np.uint32), xf.view(np.uint32))
    np.testing.assert_array_equal(cb.view(np.uint64), cf.view(np.uint64))
    assert not np.array_equal(xa[:8], xb)


def test_solves_are_unchanged_by_predictions_between_them():
    h = 10
    rec_a = records.pack_records(synthetic.make_batch(16, h, "mixed", seed=113, phase="random"), h)
    rec_b = records.pack_records(synthetic.make_batch(8, h, "standing", seed=114), h)
    outs = []
    for predict in (False, True):
        mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
        got = []
        for rec in (rec_a, rec_b):
            mpc.upload(rec)
            mpc.solve()
            if predict:
                mpc.predict_states()
            got.append(mpc.download())
            if predict:
                mpc.download_prediction()
        mpc.close()
        outs.append(got)
    for (f0, s0), (f1, s1) in zip(*outs):
        np.testing.assert_array_equal(s1, s0)
        np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32))


def test_legacy_surface_is_the_batched_prediction():
    h = 10
    f = synthetic.make_batch(1, h, "walking", seed=115, phase="random")
    rec = records.pack_records(f, h)
    _, status, states, _ = predict_batch(rec, h)
    assert interface.status_code(status)[0] == 0
    interface.setup_problem(synthetic.DT_MPC, h, 0.25, synthetic.F_MAX)
    interface.update_problem_data(f["p"][0], f["v"][0], f["q"][0], f["w"][0], f["r"][0], f["joint_angles"][0], f["yaw"][0], f["weights"][0],
                                  f["traj"][0], f["Alpha_K"][0], f["gait"][0])
    got = np.array([[interface.legacy_predicted_state(i, s) for s in range(13)] for i in range(h)])
    assert np.array_equal(got, states[0].astype(np.float64))  # (binary32 values widened: bit for bit)
    for i, s in ((-1, 0), (h, 0), (0, -1), (0, 13), (h + 5, 20)):
        assert interface.legacy_predicted_state(i, s) == 0.0
