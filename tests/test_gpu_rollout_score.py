"""Closed-loop command sweeps on the device: ``hmpc_rollout_score_device`` and ``hmpc_rollout_select_device`` against
the numpy mirror written from the header comment (tests/rollout_score_mirror.py) BIT FOR BIT -- the contract has no libm call -- on the
cases the CPU test of the kernels' source runs (synthetic logs: no solve needed); ``hmpc_rollout_sweep_device`` against its parts driven from
the host, bit for bit; and what it is for: a pushed-over candidate never wins."""
import ctypes as C

import numpy as np
import pytest

import rollout_mirror as rm
import rollout_score_mirror as sm
from hector_simulation_amd import _lib, interface, synthetic
from test_rollout_score_kernel_on_host import cost_struct

pytestmark = pytest.mark.gpu
H = sm.H
DT = synthetic.DT_MPC


def _torch():
    import torch

    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def mpc():
    m = interface.BatchedMPC(DT, H, synthetic.F_MAX, 32)
    yield m
    m.close()


# ---------------------------------------------------------------------------------------------- 1. the score against the mirror
def test_score_is_the_mirror_bit_for_bit(mpc):
    """n_ticks 1, 63, 64, 65, 130 x batch 1, 5, 257; a yaw error beyond +-pi, NaN and inf entries, fallen rows under an infinite and a finite
    penalty, an infinite unsolved penalty with nothing unsolved, every NULL member of the log"""
    seen = set()
    for name, t, log, cost in sm.score_cases():
        got = mpc.rollout_score(t, log, cost_struct(cost))
        want_cost, want_score = sm.score(t, log, cost)
        np.testing.assert_array_equal(_bits(got["cost"]), _bits(want_cost), err_msg=name)
        np.testing.assert_array_equal(_bits(got["score"]), _bits(want_score), err_msg=name)
        seen.add(log["state"].shape[:2])
        if name == "nan":
            assert np.isnan(got["score"][2])
        if name == "unsolved-inf":
            assert np.isfinite(got["score"]).all()
        if name == "fallen-inf":
            assert np.isposinf(got["score"][[1, 3]]).all()
    assert {(b, n) for b in sm.SCORE_BATCHES for n in sm.SCORE_TICKS} <= seen


def test_score_outputs_are_optional_and_guarded(mpc):
    """cost alone, score alone: the other is not written, and nothing lands outside either array (poisoned guards on both sides)"""
    torch = _torch()
    name, t, log, cost = next(c for c in sm.score_cases() if c[0] == "shape-b5-n65")
    nb, n = log["state"].shape[:2]
    want_cost, want_score = sm.score(t, log, cost)
    lg, keep = mpc._stage_log(log, nb, n)
    d_t = torch.from_numpy(t.view(np.uint8).reshape(nb, -1).copy()).cuda()
    G = 64
    for which in ("cost", "score", "both"):
        arena = torch.full((3 * G + nb * 5,), -7.0, dtype=torch.float64, device="cuda")
        cp, sp = arena.data_ptr() + 8 * G, arena.data_ptr() + 8 * (2 * G + 4 * nb)
        mpc.rollout_score(d_t.data_ptr(), lg, cost_struct(cost), device=True, batch=nb, n_ticks=n, cost_ptr=cp if which != "score" else 0,
                          score_ptr=sp if which != "cost" else 0)
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        inside = np.zeros(len(host), dtype=bool)
        if which != "score":
            inside[G:G + 4 * nb] = True
            np.testing.assert_array_equal(_bits(host[G:G + 4 * nb]), _bits(want_cost).reshape(-1), err_msg=name)
        if which != "cost":
            inside[2 * G + 4 * nb:2 * G + 5 * nb] = True
            np.testing.assert_array_equal(_bits(host[2 * G + 4 * nb:2 * G + 5 * nb]), _bits(want_score), err_msg=name)
        assert (host[~inside] == -7.0).all(), which
    del keep


# ---------------------------------------------------------------------------------------------- 2. the selection against the mirror
SELECT_OUT = (("index", np.int32, 1), ("score", np.float64, 1), ("wrench", np.float32, 12), ("tau", np.float64, 10), ("summary", np.int32, 4))


def test_select_is_the_mirror_bit_for_bit_and_writes_nothing_else(mpc):
    """group sizes 1, 3, 64, 300; exact ties, -0.0 against +0.0, NaN and -inf penalties, a wholly masked group (-1, +inf, +0 rows,
    {0, -1, 0, 0}); poisoned guard words around every output"""
    torch = _torch()
    POISON, G = 0x5A, 256
    for name, sc, pen, K, log, n in sm.select_cases():
        nb, groups = len(sc), len(sc) // K
        want = sm.select(sc, pen, K, log)
        t, _ = sm.synthetic_log(nb, 1, seed=1)
        lg, keep = mpc._stage_log(log, nb, n)
        d_t = torch.from_numpy(t.view(np.uint8).reshape(nb, -1).copy()).cuda()
        # the shape of a caller's log is the one last scored
        mpc.rollout_score(d_t.data_ptr(), lg, None, device=True, batch=nb, n_ticks=n)
        sizes = {k: groups * per * np.dtype(dt).itemsize for k, dt, per in SELECT_OUT if k in want}
        arena = torch.full((G * (len(sizes) + 1) + sum(sizes.values()),), POISON, dtype=torch.uint8, device="cuda")
        ch, off, where = _lib.RolloutChoice(), G, {}
        for k, size in sizes.items():
            setattr(ch, k, arena.data_ptr() + off)
            where[k] = (off, size)
            off += size + G
        d_s = torch.from_numpy(sc.copy()).cuda()
        d_p = None if pen is None else torch.from_numpy(pen.copy()).cuda()
        mpc.rollout_select(d_s.data_ptr(), K, 0 if d_p is None else d_p.data_ptr(), lg, device=True, batch=nb, choice=ch)
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        inside = np.zeros(len(host), dtype=bool)
        for k, (o, size) in where.items():
            inside[o:o + size] = True
            np.testing.assert_array_equal(host[o:o + size], _bits(want[k]).reshape(-1), err_msg=f"{name}: {k}")
        assert (host[~inside] == POISON).all(), name
        if K > 1 and "wrench" in want:
            assert want["index"][1] == -1  # (the wholly masked group: the mirror's no-winner row was compared above)
        # the host-array path returns the same
        if K == 3:
            again = mpc.rollout_select(sc, K, pen, log=log)
            assert sorted(again) == sorted(want)
            for k in want:
                np.testing.assert_array_equal(_bits(again[k]), _bits(want[k]), err_msg=f"{name}: host path {k}")
        del keep


# ---------------------------------------------------------------------------------------------- 3. the chain is its parts
def test_sweep_is_expansion_rollout_score_select():
    """6 states x 4 commands, 17 ticks, ticks_per_step 8, subtick0 6 (the gait advances after ticks 1 and 9), walking with placed feet, a
    finite fall penalty, terminal and torque weights and a penalty per expanded instance: hmpc_rollout_sweep_device against the expansion on
    the host -> rollout -> rollout_score -> rollout_select on another handle, bit for bit in cost, score, choice, log and final ticks; the
    score is the mirror's of the downloaded log; device_ticks is unchanged"""
    ns, K, n, tps, sub0 = 6, 4, 17, 8, 6
    nb = ns * K
    t = synthetic.make_ticks(ns, H, "walking", seed=93)
    rng = np.random.default_rng(94)
    cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
    cmd["v_des_robot"] = rng.uniform(-0.3, 0.3, (ns, K, 2))
    cmd["yaw_rate_des"] = rng.uniform(-0.4, 0.4, (ns, K))
    cmd["roll_des"], cmd["pitch_des"] = rng.uniform(-0.03, 0.03, (ns, K)), rng.uniform(-0.03, 0.03, (ns, K))
    pen = rng.integers(0, 3, nb) * 0.25
    pen[5] = np.nan
    mass = np.where(np.arange(nb) % 2 == 0, 9.0, 10.0)
    plant = rm.default_plant(flags=rm.PLANT_GYRO | rm.PLANT_PLACE_FEET, dtMPC=DT)
    cost_d = sm.default_cost(fall_penalty=1e6, unsolved_penalty=10.0, w_terminal=[10.0] * 12, w_tau=[1e-3] * 10)
    a = interface.BatchedMPC(DT, H, synthetic.F_MAX, nb)
    got = a.rollout_sweep(t, cmd, n, tps, sub0, plant=interface.default_plant(**plant), cost=cost_struct(cost_d), penalty=pen, dt_mpc=DT,
                          instance_mass=mass)
    a.close()
    np.testing.assert_array_equal(_bits(got["ticks_in"]), _bits(t))
    ex = sm.expand(t, cmd)
    b = interface.BatchedMPC(DT, H, synthetic.F_MAX, nb)
    roll = b.rollout(ex, n, tps, sub0, plant=interface.default_plant(**plant), dt_mpc=DT, instance_mass=mass)
    log = {k: roll[k] for k in _lib.ROLLOUT_LOG}
    scored = b.rollout_score(ex, log, cost_struct(cost_d))
    chosen = b.rollout_select(scored["score"], K, pen, log=log)
    last = b.rollout_select(scored["score"], K, pen)  # (log NULL: the last rollout's, the route the chain takes)
    b.close()
    for k in _lib.ROLLOUT_LOG:
        np.testing.assert_array_equal(_bits(got["log"][k]), _bits(roll[k]), err_msg=f"log {k}")
    np.testing.assert_array_equal(_bits(got["ticks"]), _bits(roll["ticks"]))
    np.testing.assert_array_equal(_bits(got["cost"]), _bits(scored["cost"]))
    np.testing.assert_array_equal(_bits(got["all_scores"]), _bits(scored["score"]))
    for k in _lib.ROLLOUT_CHOICE:
        np.testing.assert_array_equal(_bits(got[k]), _bits(chosen[k]), err_msg=f"choice {k}")
        np.testing.assert_array_equal(_bits(got[k]), _bits(last[k]), err_msg=f"choice {k}, last rollout's log")
    want_cost, want_score = sm.score(ex, log, cost_d)
    np.testing.assert_array_equal(_bits(got["cost"]), _bits(want_cost))
    np.testing.assert_array_equal(_bits(got["all_scores"]), _bits(want_score))
    want = sm.select(want_score, pen, K, log)
    for k in _lib.ROLLOUT_CHOICE:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"mirror {k}")
    assert (got["ticks"]["gait_iteration"] == (np.repeat(t["gait_iteration"], K) + 2) % H).all()
    assert (got["index"] >= 0).all() and got["index"][1] != 1  # (instance 5 = state 1, command 1 carries the NaN penalty)
    print(f"sweep 6 x 4 x 17: winners {got['index'].tolist()}, scores {np.round(got['score'], 3).tolist()}")


# ---------------------------------------------------------------------------------------------- 4. what it is for
def test_a_felled_candidate_never_wins():
    """4 standing robots x 4 candidates, 24 ticks, the default cost (fall_penalty +inf).  Known candidates are felled through
    plant.device_ext_wrench with a roll torque of 300 N m about the centre of mass.  (tests/test_gpu_rollout.py's fall test fells by a
    starting tilt, which cannot differ between the candidates of one state; a push can.)  Why 300 N m fells: it turns the body at
    300 / 0.5413 = 554 rad/s^2; the feet stand 0.06 m beside the centre of mass and carry at most f_max = 500 N each, so the controller
    resists with well under 100 N m; at 200 N m net the roll passes 1.8 rad within 0.1 s = 20 ticks, and the plant flags a fall at 60 degrees
    = 1.05 rad.  Asserted: the felled candidates fell and the others did not (so nothing below is vacuous), no winner has summary[1] >= 0,
    and the group made only of felled candidates has no winner.  No other behavioural figure is asserted."""
    ns, K, n = 4, 4, 24
    nb = ns * K
    t = synthetic.make_ticks(ns, H, "standing", seed=90, randomize=False)
    cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
    cmd["yaw_rate_des"] = np.array([0.0, 0.1, -0.1, 0.2])[None, :]
    felled = np.zeros((ns, K), dtype=bool)
    felled[0, [0, 2]] = True
    felled[1, [1, 2, 3]] = True
    felled[2, 3] = True
    felled[3, :] = True
    ext = np.zeros((nb, 6))
    ext[felled.reshape(-1), 3] = 300.0
    m = interface.BatchedMPC(DT, H, synthetic.F_MAX, nb)
    out = m.rollout_sweep(t, cmd, n, 8, 0, plant=interface.default_plant(flags=interface.PLANT_GYRO), dt_mpc=DT, ext_wrench=ext)
    m.close()
    fell = out["log"]["summary"][:, 1].reshape(ns, K) >= 0
    print(f"first fall tick per candidate:\n{out['log']['summary'][:, 1].reshape(ns, K)}\nwinners {out['index'].tolist()}, scores {out['score'].tolist()}")
    np.testing.assert_array_equal(fell, felled)
    assert np.isposinf(out["all_scores"].reshape(ns, K)[felled]).all() and np.isfinite(out["all_scores"].reshape(ns, K)[~felled]).all()
    assert (out["summary"][:, 1] < 0).all()
    assert out["index"][3] == -1 and np.isposinf(out["score"][3]) and (out["summary"][3] == sm.NO_WINNER_SUMMARY).all()
    assert not out["tau"][3].any() and not out["wrench"][3].any()
    for g in range(3):
        assert out["index"][g] >= 0 and not felled[g, out["index"][g]]
        i = g * K + out["index"][g]
        np.testing.assert_array_equal(_bits(out["tau"][g]), _bits(out["log"]["tau"][i, 0]))  # the torques to apply now: the winner's tick 0
        np.testing.assert_array_equal(_bits(out["wrench"][g]), _bits(out["log"]["wrench"][i, 0]))
        np.testing.assert_array_equal(out["summary"][g], out["log"]["summary"][i])
