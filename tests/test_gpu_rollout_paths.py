"""Paths of ``hmpc_rollout_device`` that tests/test_gpu_rollout.py does not run: every plant option inside a rollout,
more than one plant workgroup, the log's own consistency, ticks that are not solved, the device repair, two rollouts on one handle, log
buffers that grow and shrink, caller-owned and partial logs.  Host-driven loops are built as tests/test_gpu_rollout.py builds them: tick
solve, synchronisation, download, plant step, per tick.  Every rollout here has at most 17 ticks and at most 257 instances."""
import ctypes as C

import numpy as np
import pytest

import rollout_mirror as rm
from hector_simulation_amd import _lib, interface, synthetic
from test_gpu_rollout import START, _bits, _commanded, _plant, _rollout_and_loop, _rollout_ticks, _ticks_back, _to_device, _torch
from test_reference_source import E2E_FORCE

pytestmark = pytest.mark.gpu
H = rm.H
NB = 24
DT = synthetic.DT_MPC
LOG_KEYS = ("state", "wrench", "status", "tau", "summary", "ticks")


def _handle(nb, warm=False, max_iter=None, repair=False, auto_resolve=True):
    m = interface.BatchedMPC(DT, H, synthetic.F_MAX, nb)
    m.set_tick_warm_start(warm, 0)
    if max_iter is not None:
        m.set_max_iterations(max_iter)
    m.set_device_repair(repair)
    m.set_auto_resolve(auto_resolve)
    return m


def _rollout(m, t, n_ticks, plant, tps=8, sub0=0, mass=None, ext=None):
    return m.rollout(t, n_ticks, tps, sub0, plant=_plant(plant), dt_mpc=DT, instance_mass=mass, ext_wrench=ext)


def _loop(t, n_ticks, plant, tps=8, sub0=0, mass=None, ext=None, warm=False, max_iter=None, repair=False, mirror=False):
    """n_ticks host-driven rounds of tick solve + plant step on a fresh handle (the download between them repairs nothing).  ``mirror``: the
    plant step is tests/rollout_mirror.py on the host instead of the kernel."""
    torch = _torch()
    nb = len(t)
    b = _handle(nb, warm, max_iter, repair, auto_resolve=False)
    d_t = _to_device(t)
    d_tau = torch.zeros((nb, 10), dtype=torch.float64, device="cuda")
    d_wpd = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
    d_sum = torch.from_numpy(np.tile(START, (nb, 1))).cuda()
    staged, keep = b._stage_plant(_plant(plant), nb, mass, ext)
    loop = dict(state=np.zeros((nb, n_ticks, 12)), wrench=np.zeros((nb, n_ticks, 12), dtype=np.float32),
                status=np.zeros((nb, n_ticks), dtype=np.uint32), tau=np.zeros((nb, n_ticks, 10)), ticks_in=[])
    shift, now, summary = 0, t.copy(), None
    for k in range(n_ticks):
        b.set_tick_warm_start(warm, shift)
        if mirror:
            d_t = _to_device(now)
        loop["ticks_in"].append(_ticks_back(d_t))
        b.tick_solve_device(d_t.data_ptr(), nb, DT, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)
        torch.cuda.synchronize()
        forces, status = b.download()
        staged.advance_gait = 1 if (sub0 + k + 1) % tps == 0 else 0
        if mirror:
            now, summary = rm.plant_step(now, dict(plant, advance_gait=staged.advance_gait), H, forces, status, d_wpd.cpu().numpy(), summary,
                                         instance_mass=mass, ext_wrench=ext)
        else:
            b.plant_step(d_t.data_ptr(), staged, wpd=d_wpd.data_ptr(), summary=d_sum.data_ptr(), device=True, batch=nb)
            torch.cuda.synchronize()
            now = _ticks_back(d_t)
        shift = staged.advance_gait
        loop["state"][:, k] = rm.state_row(now)
        loop["wrench"][:, k], loop["status"][:, k], loop["tau"][:, k] = forces[:, :12], status, d_tau.cpu().numpy()
    loop["summary"], loop["ticks"] = (summary if mirror else d_sum.cpu().numpy()), now
    b.close()
    del keep
    return loop


def _assert_same(roll, loop, what, keys=LOG_KEYS):
    for k in keys:
        np.testing.assert_array_equal(_bits(roll[k]), _bits(loop[k]), err_msg=f"{what}: {k}")


# ---------------------------------------------------------------------------------------------- a. every plant option inside the rollout
def test_rollout_with_every_plant_option_is_the_loop_and_the_mirror():
    """substeps 3, GYRO + PLACE_FEET, masses 9 / 12 alternating, a push ~ N(0, 20) on the odd instances, walking, 9 ticks (the gait advances
    after tick 7): the log and the final ticks are the host-driven loop's bit for bit, and the mirror-driven loop's within the bound that
    test_gpu_rollout.test_walking_rollout_equals_the_mirror_driven_loop derives (its docstring; with the lightest mass here)."""
    n = 9
    t = _commanded("walking", 0.2)
    plant = rm.default_plant(flags=rm.PLANT_GYRO | rm.PLANT_PLACE_FEET, substeps=3, dtMPC=DT)
    mass = np.where(np.arange(NB) % 2 == 0, 9.0, 12.0)
    ext = np.random.default_rng(3).normal(0.0, 20.0, (NB, 6))
    ext[::2] = 0.0
    a = _handle(NB)
    roll = _rollout(a, t, n, plant, mass=mass, ext=ext)
    a.close()
    _assert_same(roll, _loop(t, n, plant, mass=mass, ext=ext), "every plant option")
    plain = _handle(NB)
    other = _rollout(plain, t, n, rm.default_plant(flags=rm.PLANT_PLACE_FEET, dtMPC=DT))
    plain.close()
    assert (other["state"][:, 0] != roll["state"][:, 0]).any(axis=1).all()  # (the options reached every instance)
    assert (roll["ticks"]["gait_iteration"] == 1).all() and (roll["ticks"]["pFoot"] != t["pFoot"]).any()
    mir = _loop(t, n, plant, mass=mass, ext=ext, mirror=True)
    E = E2E_FORCE["walking"][0]
    Fs = max(1.0, float(np.abs(roll["wrench"]).max()))
    worst = np.zeros(4)
    for k in range(n):
        tin = mir["ticks_in"][k]
        r = np.abs(tin["pFoot"].reshape(NB, 2, 3) - tin["position"][:, None, :]).max()
        dv = 0.005 * 2 * E * Fs / mass.min()
        dw = 0.005 * 2 * (2 * r * E * Fs + E * Fs) / min(plant["inertia"])
        tol = np.concatenate([np.full(3, 2 * 0.005 * dw + rm.RPY_TOL), np.full(3, 0.005 * dv), np.full(3, dw), np.full(3, dv)])
        diff = np.abs(mir["state"][:, k] - roll["state"][:, k])
        worst = np.maximum(worst, diff.reshape(NB, 4, 3).max(axis=(0, 2)))
        assert (diff <= tol[None, :]).all(), (k, diff.max(axis=0), tol)
    np.testing.assert_array_equal(roll["summary"], mir["summary"])
    for k in ("gait_iteration", "flags", "leg_q"):
        np.testing.assert_array_equal(roll["ticks"][k], mir["ticks"][k], err_msg=k)
    print(f"every plant option, 9 ticks: largest state difference to the mirror-driven loop (rpy, p, omega, v) {worst}")


# ---------------------------------------------------------------------------------------------- b. more than one plant workgroup
def test_rollout_of_257_instances_is_the_loop():
    nb, n = 257, 3
    t = synthetic.make_ticks(nb, H, "standing", seed=91)
    plant = rm.default_plant(dtMPC=DT)
    a = _handle(nb)
    roll = _rollout(a, t, n, plant)
    a.close()
    _assert_same(roll, _loop(t, n, plant), "257 instances")
    # the instance alone in the second plant workgroup: its rows are written, and they are its own
    for k in ("state", "wrench", "tau"):
        last = roll[k][256]
        assert (last != 0).any(axis=-1).all(), k
        assert (roll[k][:256] != last[None]).any(axis=(1, 2)).all(), k
    assert tuple(roll["summary"][256, :2]) == (n, -1)
    np.testing.assert_array_equal(_bits(rm.state_row(roll["ticks"][256:])), _bits(roll["state"][256:, n - 1]))


# ---------------------------------------------------------------------------------------------- c. the log is self-consistent
@pytest.mark.parametrize("gait", rm.GAITS)
def test_logged_velocity_follows_from_the_logged_wrench(gait):
    """substeps 1: the vWorld of row (i, k) is v_prev + d (F / m - g) with F from the wrench of row (i, k), in the contract's operation order,
    bit for bit -- a row index or a stride that the rollout and the loop shared would break this chain"""
    roll, _ = _rollout_and_loop(gait, False)
    d = rm.default_plant()
    assert (roll["summary"][:, 1] == -1).all()  # (nobody fell: nobody was frozen)
    v = _rollout_ticks(gait)["vWorld"]
    for k in range(roll["state"].shape[1]):
        u = roll["wrench"][:, k].astype(np.float64)
        F = (u[:, 0:3] + u[:, 3:6]) + 0.0
        v = v + (d["dt_tick"] / 1.0) * (F / d["mass"] + np.array([0.0, 0.0, -d["gravity"]]))
        np.testing.assert_array_equal(_bits(roll["state"][:, k, 9:12]), _bits(v), err_msg=f"{gait} tick {k}")
    assert (np.abs(roll["wrench"][:, :, [2, 5]]).sum(axis=2) > 1).all()


# ---------------------------------------------------------------------------------------------- d. ticks that are not solved
def test_rollout_with_unsolved_ticks_is_the_loop_and_counts_them():
    """two iterations at most: the forces are applied as they stand, the status words are logged, summary[2] counts them"""
    n = 5
    t = _rollout_ticks("standing")
    plant = rm.default_plant(dtMPC=DT)
    a = _handle(NB, max_iter=2)
    roll = _rollout(a, t, n, plant)
    a.close()
    _assert_same(roll, _loop(t, n, plant, max_iter=2), "max_iterations 2")
    code = interface.status_code(roll["status"])
    unsolved = ((code != rm.S_OK) & (code != rm.S_OK_RELAXED)).sum(axis=1)
    np.testing.assert_array_equal(roll["summary"][:, 2], unsolved)
    print(f"max_iterations 2, {n} ticks: unsolved ticks per instance {unsolved.tolist()}, codes {sorted(set(code.reshape(-1).tolist()))}")
    assert unsolved.sum() > 0
    # (the block start's rounds always complete and count as iterations: the cap bounds the single-row iterations only)
    assert (roll["summary"][:, 3] == interface.status_iters(roll["status"]).max(axis=1)).all() and (roll["summary"][:, 0] == n).all()


# ---------------------------------------------------------------------------------------------- e. device repair
REPAIR_SCALE = 6.0
QCAP_FAST = 64  # HMPC_QCAP_FAST: the rows the fast variant's working set holds


def _scaled_ticks(scale):
    """make_ticks("standing", seed 90) with its random attitude, velocity, angular velocity, joint-angle and command fields (about their
    nominal values) multiplied by ``scale``"""
    t = synthetic.make_ticks(NB, H, "standing", seed=90)
    rpy = t["rpy"] * np.array([scale, scale, 1.0])
    t["rpy"] = rpy
    t["orientation"] = synthetic.quat_from_rpy(rpy[:, 0], rpy[:, 1], rpy[:, 2])
    t["rBody"] = synthetic.rotation_world_to_body(t["orientation"]).reshape(NB, 9)
    nominal = synthetic.make_ticks(NB, H, "standing", seed=90, randomize=False)["leg_q"]
    t["leg_q"] = nominal + scale * (t["leg_q"] - nominal)
    for k in ("vWorld", "omegaWorld", "v_des_robot", "yaw_rate_des"):
        t[k] = t[k] * scale
    return t


def _active_rows_at_the_optimum(oracle, t):
    """per instance: the constraint rows with a nonzero multiplier at qpOASES's optimum of the reduced QP"""
    rec, _ = oracle.build_records(t, H, DT)
    counts = []
    for row in rec:
        qp = oracle.assemble_record(row, H, DT, synthetic.F_MAX)
        x, y, _, _, st = oracle.qpoases_solve(qp["H_red"], qp["g_red"], qp["A_red"], qp["lb_red"], qp["ub_red"])
        assert st == 0
        counts.append(int((np.abs(y[qp["n"]:]) > 1e-9).sum()))
    return np.array(counts)


def test_rollout_with_device_repair_is_the_loop_and_solves(oracle):
    """The scale was chosen on the CPU with the oracle, by the rows with a nonzero multiplier at qpOASES's optimum of tick 0 (recomputed and
    asserted below).  Instances with more than 64 rows (the fast variant's capacity): none of 24 at scale 3 (largest 61), 4 at scale 4,
    6 at scale 5, 8 at scale 6, 16 at scale 8.  At scale 6, per instance:
    55 67 54 57 78 64 59 64 74 52 56 41 67 76 76 75 74 47 54 49 63 49 63 54.
    With the repair off those instances end working_set_full, so the rest of the test cannot pass vacuously; with it on the rollout is the
    host-driven loop of the same setting bit for bit, every tick-0 status is OK and the tick-0 wrench is qpOASES's within 1e-4."""
    t = _scaled_ticks(REPAIR_SCALE)
    counts = _active_rows_at_the_optimum(oracle, t)
    big = counts > QCAP_FAST
    print(f"scale {REPAIR_SCALE}: active rows at the optimum of tick 0 {counts.tolist()}")
    assert big.sum() >= 2
    torch = _torch()
    plain = _handle(NB, auto_resolve=False)
    d_t = _to_device(t)
    d_tau = torch.zeros((NB, 10), dtype=torch.float64, device="cuda")
    plain.tick_solve_device(d_t.data_ptr(), NB, DT, d_tau.data_ptr(), 0, 0, 0)
    torch.cuda.synchronize()
    _, st = plain.download()
    plain.close()
    assert (interface.status_code(st)[big] == 5).all(), interface.status_code(st)  # working_set_full: there is something to repair
    n = 3
    plant = rm.default_plant(dtMPC=DT)
    a = _handle(NB, repair=True, auto_resolve=False)
    roll = _rollout(a, t, n, plant)
    a.close()
    _assert_same(roll, _loop(t, n, plant, repair=True), "device repair")
    assert (interface.status_code(roll["status"][:, 0]) == 0).all(), interface.status_code(roll["status"][:, 0])
    assert (interface.status_nactive(roll["status"][:, 0]) > QCAP_FAST).sum() >= 2
    rec, _ = oracle.build_records(t, H, DT)
    ref = oracle.solve_records(rec, H, DT, synthetic.F_MAX)
    q = ref["q_soln"]
    err = np.abs(roll["wrench"][:, 0] - q[:, :12]).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
    print(f"device repair: tick-0 wrench vs qpOASES {err.max():.2e}")
    assert ref["n_bad"] == 0 and err.max() < 1e-4


# ---------------------------------------------------------------------------------------------- f. history
@pytest.mark.parametrize("warm,reset", [(False, False), (True, True), (True, False)])
def test_second_rollout_on_a_handle(oracle, warm, reset):
    """a walking rollout, then a standing one on other ticks, on one handle: the second is a fresh handle's bit for bit with the warm start
    off, and with the warm start on after hmpc_reset_tick_warm_start; without the reset its first tick starts from the other rollout's last
    solution and must still be solved: every status OK, the wrench within 1e-4 of qpOASES"""
    n = 5
    walk, stand = _commanded("walking", 0.2), synthetic.make_ticks(NB, H, "standing", seed=92)
    p_walk, p_stand = rm.default_plant(flags=rm.PLANT_PLACE_FEET, dtMPC=DT), rm.default_plant(dtMPC=DT)
    m = _handle(NB, warm)
    _rollout(m, walk, 9, p_walk)
    if reset:
        m.reset_tick_warm_start()
    second = _rollout(m, stand, n, p_stand)
    m.close()
    if not warm or reset:
        fresh = _handle(NB, warm)
        want = _rollout(fresh, stand, n, p_stand)
        fresh.close()
        _assert_same(second, want, f"second rollout, warm {warm}")
        return
    code = interface.status_code(second["status"][:, 0])
    rec, _ = oracle.build_records(stand, H, DT)
    ref = oracle.solve_records(rec, H, DT, synthetic.F_MAX)
    q = ref["q_soln"]
    err = np.abs(second["wrench"][:, 0] - q[:, :12]).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
    print(f"second rollout warm-started from another rollout: tick-0 codes {sorted(set(code.tolist()))}, wrench vs qpOASES {err.max():.2e}")
    assert (code == 0).all(), code
    assert ref["n_bad"] == 0 and err.max() < 1e-4


# ---------------------------------------------------------------------------------------------- g. buffers
def _fresh(t, n, plant):
    m = _handle(len(t))
    out = _rollout(m, t, n, plant)
    m.close()
    return out


def test_own_log_buffers_grow_and_shrink():
    """5, then 9, then 3 ticks on one handle through hmpc_get_device_rollout / hmpc_download_rollout: each is its own fresh-handle result; the
    buffers are kept when they already hold as many ticks"""
    t = _rollout_ticks("standing")
    plant = rm.default_plant(dtMPC=DT)
    m = _handle(NB)
    ptrs = []
    for n in (5, 9, 3):
        log = _lib.RolloutLog()
        interface._check(m.L.hmpc_get_device_rollout(m.h, n, C.byref(log)), "hmpc_get_device_rollout")
        ptrs.append(tuple(getattr(log, k) for k in _lib.ROLLOUT_LOG))
        assert all(ptrs[-1])
        _assert_same(_rollout(m, t, n, plant), _fresh(t, n, plant), f"{n} ticks")
    assert ptrs[2] == ptrs[1]  # (3 ticks fit into the buffers of 9)
    m.close()


def test_caller_owned_and_partial_logs():
    """hmpc_set_device_rollout with tau and status NULL: state, wrench and summary go to the caller's buffers, tau and status to the handle's
    own (a NULL member of that call is the handle's own, include/hector_mpc.h).  A log passed to hmpc_rollout_device itself with tau and
    status NULL does not log them: hmpc_download_rollout refuses both.  Either way nothing is written outside the caller's arrays (poisoned
    guards on both sides of each)."""
    torch = _torch()
    n = 4
    t = _rollout_ticks("standing")
    plant = rm.default_plant(dtMPC=DT)
    want = _fresh(t, n, plant)
    POISON, G = 0x5A, 4096
    sizes = dict(state=NB * n * 12 * 8, wrench=NB * n * 12 * 4, summary=NB * 4 * 4)
    for through_argument in (False, True):
        buf = torch.full((4 * G + sum(sizes.values()),), POISON, dtype=torch.uint8, device="cuda")
        log, off, where = _lib.RolloutLog(), G, {}
        for k, size in sizes.items():
            setattr(log, k, buf.data_ptr() + off)
            where[k] = (off, size)
            off += size + G
        m = _handle(NB)
        d_t = _to_device(t)
        if through_argument:
            p = _plant(plant)
            interface._check(m.L.hmpc_rollout_device(m.h, C.c_void_p(d_t.data_ptr()), NB, n, DT, 8, 0, C.byref(p), C.byref(log), None), "rollout")
        else:
            interface._check(m.L.hmpc_set_device_rollout(m.h, C.byref(log)), "hmpc_set_device_rollout")
            m.rollout(d_t.data_ptr(), n, 8, 0, plant=_plant(plant), device=True, batch=NB, dt_mpc=DT)
        got = dict(state=np.zeros((NB, n, 12)), wrench=np.zeros((NB, n, 12), dtype=np.float32), summary=np.zeros((NB, 4), dtype=np.int32),
                   status=np.zeros((NB, n), dtype=np.uint32), tau=np.zeros((NB, n, 10)))
        ptr = lambda *names: [got[k].ctypes.data if k in names else None for k in _lib.ROLLOUT_LOG]
        interface._check(m.L.hmpc_download_rollout(m.h, *ptr("state", "wrench", "summary")), "hmpc_download_rollout")
        if through_argument:
            for k in ("tau", "status"):
                with pytest.raises(interface.HmpcError):
                    interface._check(m.L.hmpc_download_rollout(m.h, *ptr(k)), "hmpc_download_rollout")
        else:
            interface._check(m.L.hmpc_download_rollout(m.h, *ptr("tau", "status")), "hmpc_download_rollout")
            _assert_same(got, want, "the handle's own tau and status", keys=("tau", "status"))
        _assert_same(got, want, "downloaded", keys=tuple(sizes))
        got["ticks"] = _ticks_back(d_t)
        _assert_same(got, want, "final ticks", keys=("ticks",))
        host = buf.cpu().numpy()
        m.close()
        inside = np.zeros(len(host), dtype=bool)
        for k, (o, size) in where.items():
            inside[o:o + size] = True
            np.testing.assert_array_equal(host[o:o + size], _bits(want[k]).reshape(-1), err_msg=f"caller's {k}")
        assert (host[~inside] == POISON).all()
