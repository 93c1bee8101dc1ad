"""Command sweeps (hmpc_solve_command_sweep, round 6): groups of records that share state and gait and differ in the reference
trajectory only are solved on ONE inverse per group -- the results must be the bits of independent solves (hmpc_solve), whose
parity against qpOASES the rest of the suite establishes; records that do not belong to their group are reported, never solved
with another record's Hessian.

What changes inside a group is what ConvexMPCLocomotion.cpp:351-406 builds from the commands (the reference trajectory);
A_qp, B_qp, H and the constraint block come from the state and the gait alone (SolverMPC.cpp:398-447, 488-570)."""
import numpy as np
import pytest

from hector_simulation_amd import interface, records, synthetic
from sweep_cases import sweep_fields  # noqa: F401  (other test modules import it from here)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gait,h,groups,k", [("standing", 10, 24, 16), ("walking", 10, 16, 8), ("mixed", 10, 12, 5), ("standing", 7, 6, 3),
                                             ("standing", 10, 3, 64)])
def test_sweep_is_bitwise_the_independent_solve(oracle, gait, h, groups, k):
    f = sweep_fields(groups, k, h, gait, seed=41)
    rec = records.pack_records(f, h)
    b = groups * k
    ind = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
    ind.upload(rec)
    ind.solve()
    f0, s0 = ind.download()
    ind.close()
    sw = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
    sw.upload(rec)
    sw.solve_command_sweep(k)
    f1, s1 = sw.download()
    sw.close()
    assert (interface.status_code(s0) == 0).all()
    np.testing.assert_array_equal(s1, s0)  # status words: code, iteration count and final |W| of every instance
    np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32))
    # (and the independent solve is what qpOASES gives: a few instances of the sweep against the oracle)
    idx = np.arange(0, b, max(1, b // 12))
    ref = oracle.solve_records(np.ascontiguousarray(rec[idx]), h, synthetic.DT_MPC, synthetic.F_MAX)
    q = ref["q_soln"]
    err = np.abs(f1[idx] - q).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
    assert ref["n_bad"] == 0 and err.max() < 1e-4  # north_star's tolerance
    # the commands really differ inside a group
    assert np.abs(f1.reshape(groups, k, -1)[:, 0] - f1.reshape(groups, k, -1)[:, 1]).max() > 1e-3


def test_sweep_reports_records_that_do_not_belong_to_their_group():
    h, groups, k = 10, 8, 8
    f = sweep_fields(groups, k, h, "standing", seed=43)
    rec = records.pack_records(f, h)
    bad_state, bad_gait, bad_weight = 3 * k + 5, 5 * k + 1, 6 * k + 7
    f2 = {key: np.array(v, copy=True) for key, v in f.items()}
    f2["v"][bad_state, 0] += 1e-3                     # another body velocity: another x0 (g would differ, H would not -- still refused)
    f2["gait"][bad_gait, 4] = 0                       # another gait table: another reduced QP altogether
    f2["weights"][bad_weight, 2] *= 1.5               # another weight: another H
    rec2 = records.pack_records(f2, h)
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, groups * k)
    m.set_auto_resolve(False)
    m.upload(rec2)
    m.solve_command_sweep(k)
    forces, st = m.download()
    code = interface.status_code(st)
    bad = np.zeros(groups * k, dtype=bool)
    bad[[bad_state, bad_gait, bad_weight]] = True
    assert (code[bad] == 7).all() and (code[~bad] == 0).all()
    assert (forces[bad] == 0).all()
    # the other instances are the independent solves of THEIR records, bit for bit
    m.upload(rec2)
    m.solve()
    f_ind, st_ind = m.download()
    m.close()
    np.testing.assert_array_equal(forces[~bad].view(np.uint32), f_ind[~bad].view(np.uint32))
    np.testing.assert_array_equal(st[~bad], st_ind[~bad])


@pytest.mark.parametrize("h", [5, 7, 9, 10])
def test_sweep_ignores_the_padding_bytes_after_the_gait_table(h):
    """The group check compares the gait table, not the bytes that pad the record after it: at odd horizons 2 h % 4 = 2, so the
    table's last word holds two padding bytes (h = 10: none, the control).  Records whose padding differs from record to record --
    caller-built ones, uploaded or handed in by device pointer -- are solved, bit for bit as the independent solves of the same
    records.  (h = 5: 60 reduced variables; device records carry no size hint and must still reach the 60-variable sweep variant,
    the one hmpc_solve's size-class launch gives them.)"""
    import torch

    groups, k = 8, 4
    b = groups * k
    rec = records.pack_records(sweep_fields(groups, k, h, "standing", seed=53), h)
    goff = 4 * (54 + 12 * h) + 2 * h        # first byte after the gait table
    assert rec.shape[1] - goff >= 2
    rec[:, goff:] = np.random.default_rng(h).integers(1, 256, (b, rec.shape[1] - goff), dtype=np.uint8)
    assert (rec[0::k, goff] != rec[1::k, goff]).any()
    ind = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
    ind.upload(rec)
    ind.solve()
    f0, s0 = ind.download()
    ind.close()
    assert (interface.status_code(s0) == 0).all()
    d_rec = torch.from_numpy(rec).cuda()
    for device in (False, True):
        sw = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
        sw.set_auto_resolve(False)
        if device:
            sw.set_device_records(d_rec.data_ptr(), b, keepalive=d_rec)
        else:
            sw.upload(rec)
        sw.solve_command_sweep(k)
        f1, s1 = sw.download()
        sw.close()
        assert (interface.status_code(s1) != 7).all(), (device, np.flatnonzero(interface.status_code(s1) == 7))
        np.testing.assert_array_equal(s1, s0)
        np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32))


def test_a_mismatched_sweep_record_leaves_no_tick_warm_row_behind():
    """HMPC_S_SWEEP_MISMATCH is terminal and carries nothing to the next tick: with the tick-to-tick warm start on, the next ordinary
    solve of the mismatched instance starts from an empty working set -- its status word and forces are those of a handle whose
    rows were just reset (hmpc_reset_tick_warm_start), not of one warm-started from what the instance solved before the sweep."""
    h, groups, k = 10, 8, 8
    b = groups * k
    f = sweep_fields(groups, k, h, "standing", seed=43)
    rec = records.pack_records(f, h)
    j = 3 * k + 5
    f2 = {key: np.array(v, copy=True) for key, v in f.items()}
    f2["weights"][j, 2] *= 1.5
    rec2 = records.pack_records(f2, h)
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
    m.set_tick_warm_start(True)
    m.upload(rec)
    m.solve()
    _, s_first = m.download()                      # every instance leaves its final working set for the next tick
    m.upload(rec2)
    m.solve_command_sweep(k)
    _, s_sw = m.download()
    assert interface.status_code(s_sw)[j] == 7 and (np.delete(interface.status_code(s_sw), j) == 0).all()
    m.upload(rec)
    m.solve()
    f_after, s_after = m.download()
    m.reset_tick_warm_start()
    m.solve()
    f_reset, s_reset = m.download()
    m.upload(rec)                                  # (the control: a row carried over does change instance j's solve)
    m.solve()
    _, s_warm = m.download()
    m.close()
    assert s_warm[j] != s_reset[j] and interface.status_iters(s_reset)[j] > interface.status_iters(s_warm)[j], (s_warm[j], s_reset[j])
    assert interface.status_code(s_first)[j] == 0 and interface.status_code(s_after)[j] == 0
    assert s_after[j] == s_reset[j], (s_after[j], s_reset[j])
    np.testing.assert_array_equal(f_after[j].view(np.uint32), f_reset[j].view(np.uint32))


def test_sweep_argument_errors_and_the_group_of_one():
    h = 10
    rec = records.pack_records(sweep_fields(4, 4, h, "standing", seed=44), h)
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 16)
    m.upload(rec)
    with pytest.raises(interface.HmpcError):
        m.solve_command_sweep(5)   # 16 % 5 != 0
    with pytest.raises(interface.HmpcError):
        m.solve_command_sweep(0)
    m.solve_command_sweep(1)       # = hmpc_solve
    f1, s1 = m.download()
    m.solve()
    f0, s0 = m.download()
    m.close()
    np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32))
    m3 = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 4, contacts=3)
    m3.upload(records.pack_records(synthetic.make_batch3(4, h, "standing", seed=5), h, 3))
    with pytest.raises(interface.HmpcError):
        m3.solve_command_sweep(2)  # two-contact handles only
    m3.close()


def test_sweep_flagged_instances_are_repaired_as_independent_ones(oracle):
    """A sweep at 6x the nominal ranges: instances whose working set outgrows the fast variant are flagged by the sweep kernel and
    repaired by the safe pass (no hand-over inside a sweep), on the device or by hmpc_download -- every instance ends ok and equals
    qpOASES."""
    h, groups, k = 10, 16, 8
    base = synthetic.hard_batch(groups, h, "standing", 17, 6)
    f = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in base.items()}
    rng = np.random.default_rng(5)
    tr = f["traj"].reshape(groups * k, h, 12).copy()
    tr[:, :, 9] += rng.uniform(-0.5, 0.5, groups * k)[:, None]
    f["traj"] = tr.reshape(groups * k, -1)
    rec = records.pack_records(f, h)
    ref = oracle.solve_records(rec, h, synthetic.DT_MPC, synthetic.F_MAX)
    q = ref["q_soln"]
    for device_side in (False, True):
        m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, groups * k)
        m.set_device_repair(device_side)
        m.upload(rec)
        m.solve_command_sweep(k)
        forces, st = m.download()
        m.close()
        assert (interface.status_code(st) == 0).all()
        assert (interface.status_nactive(st) > 64).any()   # the regime really leaves the fast variant's capacity
        err = np.abs(forces - q).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
        assert err.max() < 2e-6, err.max()


def test_terrain_sweep_per_instance_friction_on_a_shared_inverse(oracle):
    """hmpc_set_instance_mu: one friction parameter per instance.  (1) It is the hmpc_params path per instance: the instances that
    share a value come out bit for bit as a handle whose hmpc_params.mu is that value gives them (and that path is checked against
    the oracle in tests/test_gpu_assembly.py); spot-checked against qpOASES with the oracle's parameters set accordingly.  (2) H does
    not depend on mu, so a command-sweep group may mix floors: states x (commands x floors) on one inverse per state, bit-identical
    to the independent solves."""
    import torch

    h, groups, k = 10, 12, 12
    f = sweep_fields(groups, k, h, "standing", seed=47)
    rec = records.pack_records(f, h)
    b = groups * k
    mus = np.array([0.8, 1.25, 2.0, 3.0], dtype=np.float32)
    mu_i = mus[np.arange(b) % 4]                       # inside every group: four floors x three commands
    d_mu = torch.from_numpy(mu_i).cuda()
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, b)
    m.upload(rec)
    m.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu)
    m.solve()
    f_ind, s_ind = m.download()
    m.solve_command_sweep(k)
    f_sw, s_sw = m.download()
    assert (interface.status_code(s_ind) == 0).all()
    np.testing.assert_array_equal(f_sw.view(np.uint32), f_ind.view(np.uint32))
    np.testing.assert_array_equal(s_sw, s_ind)
    m.set_instance_mu(0)
    for j, mu in enumerate(mus):
        m.set_params(mu=float(mu))
        m.solve()
        f_p, s_p = m.download()
        sel = (np.arange(b) % 4) == j
        np.testing.assert_array_equal(f_p[sel].view(np.uint32), f_ind[sel].view(np.uint32))
        np.testing.assert_array_equal(s_p[sel], s_ind[sel])
        try:                                            # ... and what qpOASES gives for that floor
            oracle.set_params(mu=float(mu))
            idx = np.flatnonzero(sel)[:6]
            ref = oracle.solve_records(np.ascontiguousarray(rec[idx]), h, synthetic.DT_MPC, synthetic.F_MAX)
        finally:
            oracle.set_params()
        q = ref["q_soln"]
        err = np.abs(f_ind[idx] - q).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
        assert ref["n_bad"] == 0 and err.max() < 1e-4, (mu, err.max())
    m.close()
    # the floors really matter
    assert np.abs(f_ind[0::4] - f_ind[3::4]).max() > 1e-3
