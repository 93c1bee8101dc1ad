"""What a handle carries from one closed-loop call to the next (DESIGN.md sections 4.22 and 4.23): ``hmpc_rollout_sweep_device``,
``hmpc_rollout_score_device`` and ``hmpc_rollout_select_device`` are called every tick on ONE handle, and the handle's fields decide which
memory a later call reads and with which row stride.  Here: the own log that grows between a rollout and its readers (the handle forgets
the rollout instead of reading freed memory), sweeps of different shapes, a plain solve and a caller-logged rollout in between on one handle
against fresh handles, candidates moved around the batch, a sweep on a caller's stream, sweeps with unsolved ticks and with the device
repair.  Every comparison is on bits; the largest shape is 48 instances x 13 ticks."""
import ctypes as C
import functools

import numpy as np
import pytest

import rollout_mirror as rm
import rollout_score_mirror as sm
from hector_simulation_amd import _lib, interface, records, synthetic
from test_gpu_rollout import _plant, _ticks_back, _to_device
from test_gpu_rollout_paths import _assert_same, _handle, _rollout, _scaled_ticks
from test_rollout_score_kernel_on_host import cost_struct

pytestmark = pytest.mark.gpu
H = sm.H
DT = synthetic.DT_MPC
QCAP_FAST = 64  # HMPC_QCAP_FAST: the rows the fast variant's working set holds
E_ARG = r"failed with -1:"  # HMPC_E_ARG in interface._check's message
SWEEP_KEYS = _lib.ROLLOUT_CHOICE + ("cost", "all_scores", "ticks")
CHOICE_SHAPES = dict(index=(np.int32, ()), score=(np.float64, ()), wrench=(np.float32, (12,)), tau=(np.float64, (10,)), summary=(np.int32, (4,)))
COST_FULL = dict(fall_penalty=1e6, unsolved_penalty=10.0, w_terminal=[10.0] * 12, w_tau=[1e-3] * 10)


def _torch():
    import torch

    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------------------------------------- scenarios and their fresh-handle results
def _scenario(ns, K, n, gait, seed, flags=0, tps=8, sub0=0, cost=None, per_instance=False, nan_penalty=None):
    """ns states x K commands: ticks, commands, plant and cost dicts and, with ``per_instance``, a mass, a push and a penalty per expanded
    instance (``nan_penalty``: the instance whose penalty is NaN)"""
    nb = ns * K
    rng = np.random.default_rng(seed)
    cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
    cmd["v_des_robot"] = rng.uniform(-0.3, 0.3, (ns, K, 2))
    cmd["yaw_rate_des"] = rng.uniform(-0.4, 0.4, (ns, K))
    cmd["roll_des"], cmd["pitch_des"] = rng.uniform(-0.03, 0.03, (ns, K)), rng.uniform(-0.03, 0.03, (ns, K))
    s = dict(t=synthetic.make_ticks(ns, H, gait, seed=seed), cmd=cmd, n=n, tps=tps, sub0=sub0, plant=rm.default_plant(flags=flags, dtMPC=DT),
             cost=sm.default_cost(**(cost or {})), mass=None, ext=None, pen=None)
    if per_instance:
        s["mass"], s["ext"] = rng.uniform(8.0, 11.0, nb), rng.normal(0.0, 5.0, (nb, 6))
        s["pen"] = rng.integers(0, 3, nb) * 0.25
        if nan_penalty is not None:
            s["pen"][nan_penalty] = np.nan
    return s


@functools.lru_cache(maxsize=None)
def _named(name):
    """the scenarios more than one test runs; every array is left unchanged by its users"""
    if name == "S1":
        return _scenario(4, 8, 9, "walking", 101, flags=rm.PLANT_GYRO | rm.PLANT_PLACE_FEET, sub0=6, cost=COST_FULL, per_instance=True,
                         nan_penalty=13)
    if name == "S2":
        return _scenario(5, 3, 13, "standing", 102)
    if name == "S3":
        return _scenario(2, 5, 3, "walking", 103, flags=rm.PLANT_PLACE_FEET, sub0=7)
    if name == "S1-longer":
        return dict(_named("S1"), n=12)
    raise KeyError(name)


def _sweep(m, s):
    return m.rollout_sweep(s["t"], s["cmd"], s["n"], s["tps"], s["sub0"], plant=_plant(s["plant"]), cost=cost_struct(s["cost"]), penalty=s["pen"],
                           dt_mpc=DT, instance_mass=s["mass"], ext_wrench=s["ext"])


@functools.lru_cache(maxsize=None)
def _fresh_sweep(name, warm=False):
    m = _handle(32, warm)
    out = _sweep(m, _named(name))
    m.close()
    return out


def _assert_same_sweep(got, want, what):
    _assert_same(got, want, what, keys=SWEEP_KEYS)
    _assert_same(got["log"], want["log"], f"{what}: log", keys=_lib.ROLLOUT_LOG)


def _parts(b, s):
    """expansion on the host -> rollout -> score -> selection over the last rollout's log, on handle ``b``: the dict of ``rollout_sweep``"""
    K = s["cmd"].shape[1]
    ex = sm.expand(s["t"], s["cmd"])
    roll = b.rollout(ex, s["n"], s["tps"], s["sub0"], plant=_plant(s["plant"]), dt_mpc=DT, instance_mass=s["mass"], ext_wrench=s["ext"])
    log = {k: roll[k] for k in _lib.ROLLOUT_LOG}
    scored = b.rollout_score(ex, None, cost_struct(s["cost"]), n_ticks=s["n"])
    out = b.rollout_select(scored["score"], K, s["pen"])
    out.update(cost=scored["cost"], all_scores=scored["score"], ticks=roll["ticks"], log=log)
    return out


def _assert_is_the_mirror(got, s, what):
    """cost, score and choice of a sweep's result against the mirror of its own downloaded log"""
    ex = sm.expand(s["t"], s["cmd"])
    want_cost, want_score = sm.score(ex, got["log"], s["cost"])
    np.testing.assert_array_equal(_bits(got["cost"]), _bits(want_cost), err_msg=f"{what}: cost")
    np.testing.assert_array_equal(_bits(got["all_scores"]), _bits(want_score), err_msg=f"{what}: score")
    want = sm.select(want_score, s["pen"], s["cmd"].shape[1], got["log"])
    for k in _lib.ROLLOUT_CHOICE:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: mirror {k}")


def _caller_log(nb, n, members=_lib.ROLLOUT_LOG):
    """``struct hmpc_rollout_log`` over torch buffers for ``members`` (the others NULL); + the buffers"""
    torch = _torch()
    shapes = dict(state=(torch.float64, (nb, n, 12)), wrench=(torch.float32, (nb, n, 12)), status=(torch.int32, (nb, n)),
                  tau=(torch.float64, (nb, n, 10)), summary=(torch.int32, (nb, 4)))
    lg, bufs = _lib.RolloutLog(), {}
    for k in members:
        bufs[k] = torch.zeros(shapes[k][1], dtype=shapes[k][0], device="cuda")
        setattr(lg, k, bufs[k].data_ptr())
    return lg, bufs


def _own_log(m, n):
    log = _lib.RolloutLog()
    interface._check(m.L.hmpc_get_device_rollout(m.h, n, C.byref(log)), "hmpc_get_device_rollout")
    ptrs = tuple(getattr(log, k) for k in _lib.ROLLOUT_LOG)
    assert all(ptrs)
    return ptrs


# ---------------------------------------------------------------------------------------------- 1. the own log grows under the last rollout
NB1, K1 = 6, 3


@functools.lru_cache(maxsize=None)
def _standing6(n):
    """(ticks, plant dict, a fresh handle's rollout of n ticks)"""
    t = synthetic.make_ticks(NB1, H, "standing", seed=95)
    plant = rm.default_plant(dtMPC=DT)
    m = _handle(NB1)
    out = _rollout(m, t, n, plant)
    m.close()
    return t, plant, out


def _score_and_select_last(m, t, n, log, cost_d, what):
    """score(log = NULL) and select(log = NULL) over the handle's last rollout run and are the mirror of ``log``, its downloaded rows"""
    scored = m.rollout_score(t, None, cost_struct(cost_d), n_ticks=n)
    want_cost, want_score = sm.score(t, log, cost_d)
    np.testing.assert_array_equal(_bits(scored["cost"]), _bits(want_cost), err_msg=f"{what}: cost")
    np.testing.assert_array_equal(_bits(scored["score"]), _bits(want_score), err_msg=f"{what}: score")
    chosen = m.rollout_select(scored["score"], K1)
    want = sm.select(want_score, None, K1, log)
    for k in _lib.ROLLOUT_CHOICE:
        np.testing.assert_array_equal(_bits(chosen[k]), _bits(want[k]), err_msg=f"{what}: choice {k}")


def _assert_forgotten(m, t, n):
    """download, score(log = NULL) and select(log = NULL) return HMPC_E_ARG and write nothing, as before the first rollout"""
    torch = _torch()
    with pytest.raises(interface.HmpcError, match=E_ARG):
        m.download_rollout(NB1, n)
    d_t = _to_device(t)
    d_cost = torch.full((NB1, 4), -7.0, dtype=torch.float64, device="cuda")
    d_score = torch.full((NB1,), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(interface.HmpcError, match=E_ARG):
        m.rollout_score(d_t.data_ptr(), None, None, device=True, batch=NB1, n_ticks=n, cost_ptr=d_cost.data_ptr(), score_ptr=d_score.data_ptr())
    ch, bufs = _lib.RolloutChoice(), {}
    for k, (dt, shape) in CHOICE_SHAPES.items():
        bufs[k] = torch.full((NB1 // K1 * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        setattr(ch, k, bufs[k].data_ptr())
    with pytest.raises(interface.HmpcError, match=E_ARG):
        m.rollout_select(d_score.data_ptr(), K1, 0, None, device=True, batch=NB1, choice=ch)
    torch.cuda.synchronize()
    assert (d_cost.cpu().numpy() == -7.0).all() and (d_score.cpu().numpy() == -7.0).all()
    for k, b in bufs.items():
        assert (b.cpu().numpy() == 0x5A).all(), k


@pytest.mark.parametrize("where", ["own", "callers-argument", "callers-and-own"])
def test_growing_the_own_log_forgets_the_last_rollout(where):
    """6 standing instances, 3 ticks, then ``hmpc_get_device_rollout(h, 7)`` frees and reallocates the handle's own log buffers.
    ``own``: the rollout logged into them (log == NULL); asking for 3 ticks again changes nothing, the growth makes the handle forget the
    rollout -- ``hmpc_download_rollout`` and the score and selection with log == NULL return HMPC_E_ARG and write nothing, while both
    still work on a caller's log -- and a rollout of 7 ticks brings all three back.  ``callers-argument``: the rollout logged wholly into
    the caller's ``log`` argument and survives the growth.  ``callers-and-own``: ``hmpc_set_device_rollout`` with tau and status NULL sends
    those two into the handle's own buffers, so the growth forgets that rollout as well."""
    n, grown = 3, 7
    t, plant, want = _standing6(n)
    cost_d = sm.default_cost(**COST_FULL)
    m = _handle(NB1)
    if where == "own":
        roll = _rollout(m, t, n, plant)
        _assert_same(roll, want, "3 ticks")
        log = {k: roll[k] for k in _lib.ROLLOUT_LOG}
        ptrs = _own_log(m, n)
        assert _own_log(m, n) == ptrs and _own_log(m, n - 1) == ptrs  # (no growth: the same buffers)
        _assert_same(m.download_rollout(NB1, n), want, "second download", keys=_lib.ROLLOUT_LOG)
        _score_and_select_last(m, t, n, log, cost_d, "after hmpc_get_device_rollout without growth")
        _own_log(m, grown)
        _assert_forgotten(m, t, n)
        # a caller's log goes on working
        scored = m.rollout_score(t, log, cost_struct(cost_d))
        want_cost, want_score = sm.score(t, log, cost_d)
        np.testing.assert_array_equal(_bits(scored["cost"]), _bits(want_cost))
        np.testing.assert_array_equal(_bits(scored["score"]), _bits(want_score))
        chosen = m.rollout_select(scored["score"], K1, None, log=log)
        for k, v in sm.select(want_score, None, K1, log).items():
            np.testing.assert_array_equal(_bits(chosen[k]), _bits(v), err_msg=f"caller's log: choice {k}")
        _assert_forgotten(m, t, n)  # (neither remembered anything)
        again = _rollout(m, t, grown, plant)
        _assert_same(again, _standing6(grown)[2], "7 ticks after the growth")
        _score_and_select_last(m, t, grown, {k: again[k] for k in _lib.ROLLOUT_LOG}, cost_d, "7 ticks after the growth")
    elif where == "callers-argument":
        _own_log(m, n)  # (the handle has own buffers to free)
        lg, bufs = _caller_log(NB1, n)
        d_t = _to_device(t)
        p = _plant(plant)
        interface._check(m.L.hmpc_rollout_device(m.h, C.c_void_p(d_t.data_ptr()), NB1, n, DT, 8, 0, C.byref(p), C.byref(lg), None), "rollout")
        _own_log(m, grown)
        got = m.download_rollout(NB1, n)
        got["ticks"] = _ticks_back(d_t)
        _assert_same(got, want, "caller's log after the growth")
        _score_and_select_last(m, t, n, {k: got[k] for k in _lib.ROLLOUT_LOG}, cost_d, "caller's log after the growth")
        del bufs
    else:
        lg, bufs = _caller_log(NB1, n, members=("state", "wrench", "summary"))
        interface._check(m.L.hmpc_set_device_rollout(m.h, C.byref(lg)), "hmpc_set_device_rollout")
        d_t = _to_device(t)
        m.rollout(d_t.data_ptr(), n, 8, 0, plant=_plant(plant), device=True, batch=NB1, dt_mpc=DT)
        _assert_same(m.download_rollout(NB1, n), want, "caller's state, wrench, summary; own tau, status", keys=_lib.ROLLOUT_LOG)
        _own_log(m, grown)
        _assert_forgotten(m, t, n)
        del bufs
    m.close()


# ---------------------------------------------------------------------------------------------- 2. sweeps on a used handle
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "tick-warm-start-reset"])
def test_sweeps_on_a_used_handle_are_a_fresh_handles(warm):
    """One handle of 32 instances runs, in order: S1 = 4 x 8 walking, GYRO + PLACE_FEET, 9 ticks, per-instance mass, push and penalty
    (one NaN), finite fall penalty, terminal and torque weights; a plain solve of 20 unrelated standing instances uploaded from the host;
    S2 = 5 x 3 standing, 13 ticks (the own log grows), default cost, NO mass, push or penalty (a device pointer kept from S1's plant would
    show); a rollout of 7 instances x 4 ticks into a caller's ``log`` argument, scored and selected with log == NULL; S3 = 2 x 5, 3 ticks,
    logged into buffers that hold 13 ticks per row.  Every sweep's choice, cost, scores, log and final ticks are a fresh handle's bit for
    bit, the plain solve's forces and status words too, the rollout's score and selection are the mirror's, and the sweep's own buffers
    are allocated once.  With the tick warm start on, every solve starts from the working sets the handle's previous solve left, by design
    (include/hector_mpc.h), so ``reset_tick_warm_start`` comes before each unrelated batch: the sweeps, the plain solve and the rollout."""
    torch = _torch()
    m = _handle(32, warm)

    def unrelated():
        if warm:
            m.reset_tick_warm_start()

    unrelated()
    _assert_same_sweep(_sweep(m, _named("S1")), _fresh_sweep("S1", warm), "S1")
    own = [m.get_device_rollout_sweep()]

    rec = records.pack_records(synthetic.make_batch(20, H, "standing", seed=104, phase="random"), H)
    fresh = _handle(32, warm)
    fresh.upload(rec)
    fresh.solve()
    want_forces, want_status = fresh.download()
    fresh.close()
    unrelated()
    m.upload(rec)
    m.solve()
    forces, status = m.download()
    np.testing.assert_array_equal(_bits(forces), _bits(want_forces), err_msg="plain solve after S1: forces")
    np.testing.assert_array_equal(status, want_status, err_msg="plain solve after S1: status")
    assert (interface.status_code(status) == 0).all()

    unrelated()
    _assert_same_sweep(_sweep(m, _named("S2")), _fresh_sweep("S2", warm), "S2")
    own.append(m.get_device_rollout_sweep())

    nb, n = 7, 4
    t7 = synthetic.make_ticks(nb, H, "standing", seed=105)
    lg, bufs = _caller_log(nb, n)
    d_t = _to_device(t7)
    p = _plant(rm.default_plant(dtMPC=DT))
    unrelated()
    torch.cuda.synchronize()
    interface._check(m.L.hmpc_rollout_device(m.h, C.c_void_p(d_t.data_ptr()), nb, n, DT, 8, 0, C.byref(p), C.byref(lg), None), "rollout")
    log = m.download_rollout(nb, n)
    np.testing.assert_array_equal(_bits(log["state"]), _bits(bufs["state"].cpu().numpy()))  # (it is the caller's buffers that were read)
    assert (log["summary"][:, 0] == n).all()
    cost_d = sm.default_cost(**COST_FULL)
    scored = m.rollout_score(t7, None, cost_struct(cost_d), n_ticks=n)
    want_cost, want_score = sm.score(t7, log, cost_d)
    np.testing.assert_array_equal(_bits(scored["cost"]), _bits(want_cost), err_msg="rollout into a caller's log: cost")
    np.testing.assert_array_equal(_bits(scored["score"]), _bits(want_score), err_msg="rollout into a caller's log: score")
    chosen = m.rollout_select(scored["score"], nb)
    for k, v in sm.select(want_score, None, nb, log).items():
        np.testing.assert_array_equal(_bits(chosen[k]), _bits(v), err_msg=f"rollout into a caller's log: choice {k}")
    assert chosen["index"][0] >= 0

    unrelated()
    _assert_same_sweep(_sweep(m, _named("S3")), _fresh_sweep("S3", warm), "S3")
    own.append(m.get_device_rollout_sweep())
    assert own[0] == own[1] == own[2] and all(own[0].values())
    m.close()
    del bufs


# ---------------------------------------------------------------------------------------------- 3. a candidate's place in the batch
def test_a_candidate_does_not_depend_on_where_it_stands():
    """5 states x 6 commands = 30 instances (the last score workgroup has two idle waves), walking, 9 ticks, GYRO + PLACE_FEET, every
    expanded instance with its own mass, push and penalty.  Run again on a fresh handle with the states permuted and the commands of every
    group permuted by a permutation of their own, mass, push and penalty moving with their instances: per instance the log rows, cost and
    score are the same bits, and every group's winner is the same candidate with the same score, wrench, tau and summary.  The first run has
    no two equal finite scores inside a group, so the tie rule cannot hide a difference.  Then one group gets six identical candidates:
    its six logs and scores are equal bit for bit and the winner is index 0."""
    ns, K = 5, 6
    nb = ns * K
    s = _scenario(ns, K, 9, "walking", 106, flags=rm.PLANT_GYRO | rm.PLANT_PLACE_FEET, sub0=6, cost=COST_FULL, per_instance=True)

    def run(sc):
        m = _handle(nb)
        out = _sweep(m, sc)
        m.close()
        return out

    first = run(s)
    total = (first["all_scores"] + s["pen"]).reshape(ns, K)
    for g in range(ns):
        finite = total[g][np.isfinite(total[g])]
        assert len(finite) >= 2 and len(np.unique(finite)) == len(finite), (g, total[g])
    assert (first["index"] >= 0).all()

    rng = np.random.default_rng(107)
    ps = rng.permutation(ns)
    while (ps == np.arange(ns)).any():
        ps = rng.permutation(ns)
    pc = np.stack([rng.permutation(K) for _ in range(ns)])
    assert all((pc[g] != np.arange(K)).any() for g in range(ns))
    src = (ps[:, None] * K + pc).reshape(-1)  # new instance g' K + k' = old instance ps[g'] K + pc[g'][k']
    moved = dict(s, t=s["t"][ps], cmd=s["cmd"][ps][np.arange(ns)[:, None], pc], mass=s["mass"][src], ext=s["ext"][src],
                 pen=s["pen"][src])
    np.testing.assert_array_equal(_bits(sm.expand(moved["t"], moved["cmd"])), _bits(sm.expand(s["t"], s["cmd"])[src]))
    second = run(moved)
    for k in _lib.ROLLOUT_LOG:
        np.testing.assert_array_equal(_bits(second["log"][k]), _bits(first["log"][k][src]), err_msg=f"moved: log {k}")
    for k in ("cost", "all_scores", "ticks"):
        np.testing.assert_array_equal(_bits(second[k]), _bits(first[k][src]), err_msg=f"moved: {k}")
    np.testing.assert_array_equal(pc[np.arange(ns), second["index"]], first["index"][ps], err_msg="moved: the winner")
    for k in ("score", "wrench", "tau", "summary"):
        np.testing.assert_array_equal(_bits(second[k]), _bits(first[k][ps]), err_msg=f"moved: the winner's {k}")

    g = 2
    same = dict(s, cmd=s["cmd"].copy(), mass=s["mass"].copy(), ext=s["ext"].copy(), pen=s["pen"].copy())
    same["cmd"][g, :] = s["cmd"][g, 3]
    rows = slice(g * K, (g + 1) * K)
    same["mass"][rows], same["ext"][rows], same["pen"][rows] = s["mass"][g * K + 3], s["ext"][g * K + 3], 0.25
    third = run(same)
    for k in _lib.ROLLOUT_LOG:
        got = third["log"][k][rows]
        np.testing.assert_array_equal(_bits(got), _bits(np.repeat(got[:1], K, axis=0)), err_msg=f"identical candidates: log {k}")
        np.testing.assert_array_equal(_bits(got[3]), _bits(first["log"][k][g * K + 3]), err_msg=f"identical candidates: log {k} is candidate 3's")
    for k in ("cost", "all_scores"):
        got = third[k][rows]
        np.testing.assert_array_equal(_bits(got), _bits(np.repeat(got[:1], K, axis=0)), err_msg=f"identical candidates: {k}")
    assert np.isfinite(third["all_scores"][rows]).all() and third["index"][g] == 0
    others = np.delete(np.arange(ns), g)
    for k in _lib.ROLLOUT_CHOICE:  # (the other groups: untouched by their neighbour)
        np.testing.assert_array_equal(_bits(third[k][others]), _bits(first[k][others]), err_msg=f"identical candidates: other groups' {k}")


# ---------------------------------------------------------------------------------------------- 4. a caller's stream
def _sweep_on_stream(m, s, stream):
    """``_sweep`` through the device entry on ``stream`` (a torch stream): nothing waits before ``hmpc_download_rollout``, which itself
    waits for the rollout's stream; the choice and the handle's cost and score are read after the stream is synchronised"""
    torch = _torch()
    ns, K = s["cmd"].shape
    nb = ns * K
    p, keep = m._stage_plant(_plant(s["plant"]), nb, s["mass"], s["ext"])
    d_t = _to_device(s["t"])
    d_c = torch.from_numpy(s["cmd"].view(np.uint8).reshape(nb, -1).copy()).cuda()
    d_p = None if s["pen"] is None else torch.from_numpy(s["pen"].copy()).cuda()
    ch, bufs = m._choice_buffers(ns, _lib.ROLLOUT_CHOICE)
    torch.cuda.synchronize()  # (the uploads, on torch's stream)
    m.rollout_sweep(d_t.data_ptr(), d_c.data_ptr(), s["n"], s["tps"], s["sub0"], plant=p, cost=cost_struct(s["cost"]),
                    penalty=0 if d_p is None else d_p.data_ptr(), device=True, n_states=ns, group_size=K, choice=ch, dt_mpc=DT,
                    stream=stream.cuda_stream)
    log = m.download_rollout(nb, s["n"])
    stream.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    own = m.get_device_rollout_sweep()
    out["ticks"] = m._device_bytes(own["ticks"], nb * interface.TICK_DTYPE.itemsize).view(interface.TICK_DTYPE).copy()
    out["cost"] = m._device_bytes(own["cost"], nb * 32).view(np.float64).reshape(nb, 4).copy()
    out["all_scores"] = m._device_bytes(own["score"], nb * 8).view(np.float64).copy()
    out["log"] = log
    np.testing.assert_array_equal(_bits(_ticks_back(d_t)), _bits(s["t"]))  # (the states are not modified)
    del keep
    return out


def test_sweep_on_a_callers_stream():
    """S1 of the test above on a non-blocking stream of the caller's: a fresh handle's null-stream result bit for bit.  Then a sweep with
    more ticks on the null stream of the same handle, whose log has to grow (and waits for the side stream before it frees): again a
    fresh handle's."""
    torch = _torch()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    m = _handle(32)
    _assert_same_sweep(_sweep_on_stream(m, _named("S1"), stream), _fresh_sweep("S1"), "S1 on a caller's stream")
    _assert_same_sweep(_sweep(m, _named("S1-longer")), _fresh_sweep("S1-longer"), "more ticks on the null stream afterwards")
    m.close()


# ---------------------------------------------------------------------------------------------- 5. unsolved ticks
def test_unsolved_candidates_in_a_sweep():
    """Two iterations at most and no repair (the recipe of test_rollout_with_unsolved_ticks_is_the_loop_and_counts_them): 3 standing states
    x 4 commands, 5 ticks.  With unsolved_penalty = +inf and a finite fall penalty the chain is its parts on a second such handle and the
    mirror of its own log; some instance has unsolved ticks (asserted), every such instance scores +inf, none of them wins, and a group
    without a wholly solved candidate (there is one, asserted) reports no winner.  With unsolved_penalty = 10 the penalty column is the
    mirror's and every group has a winner."""
    ns, K = 3, 4
    nb = ns * K
    s = _scenario(ns, K, 5, "standing", 108, cost=dict(fall_penalty=1e6, unsolved_penalty=np.inf))
    s["cmd"][:, 0] = np.zeros((), dtype=interface.COMMAND_DTYPE)  # (candidate 0 of every state: stand still)
    s["cmd"][2, 2:] = s["cmd"][2, :2]  # (the last state has two commands, each twice: neither is solved within two iterations)
    a = _handle(nb, max_iter=2, auto_resolve=False)
    got = _sweep(a, s)
    a.close()
    b = _handle(nb, max_iter=2, auto_resolve=False)
    _assert_same_sweep(got, _parts(b, s), "unsolved ticks: the chain against its parts")
    b.close()
    _assert_is_the_mirror(got, s, "unsolved ticks")
    summary = got["log"]["summary"]
    code = interface.status_code(got["log"]["status"])
    np.testing.assert_array_equal(summary[:, 2], ((code != rm.S_OK) & (code != rm.S_OK_RELAXED)).sum(axis=1))
    unsolved = summary[:, 2] > 0
    print(f"max_iterations 2, {ns} x {K} x 5: unsolved ticks per candidate\n{summary[:, 2].reshape(ns, K)}\nwinners {got['index'].tolist()}")
    assert unsolved.any()
    assert np.isposinf(got["all_scores"][unsolved]).all() and np.isposinf(got["cost"][unsolved, 3]).all()
    assert (summary[:, 1] < 0).all() and np.isfinite(got["all_scores"][~unsolved]).all()  # (nobody fell: only the unsolved are masked)
    assert (got["summary"][:, 2] == 0).all()
    assert unsolved.reshape(ns, K).all(axis=1).any() and (got["index"] >= 0).any()  # (both kinds of group occur)
    for g in range(ns):
        rows = unsolved[g * K:(g + 1) * K]
        if rows.all():
            assert got["index"][g] == -1 and np.isposinf(got["score"][g])
            assert not got["wrench"][g].any() and not got["tau"][g].any() and (got["summary"][g] == sm.NO_WINNER_SUMMARY).all()
        else:
            assert got["index"][g] >= 0 and not rows[got["index"][g]]

    finite = dict(s, cost=dict(s["cost"], unsolved_penalty=10.0))
    c = _handle(nb, max_iter=2, auto_resolve=False)
    soft = _sweep(c, finite)
    c.close()
    _assert_same(soft["log"], got["log"], "the log does not depend on the cost", keys=_lib.ROLLOUT_LOG)
    _assert_is_the_mirror(soft, finite, "unsolved_penalty 10")
    np.testing.assert_array_equal(_bits(soft["cost"][:, 3]), _bits(summary[:, 2] * 10.0))
    assert (soft["index"] >= 0).all() and np.isfinite(soft["score"]).all()


# ---------------------------------------------------------------------------------------------- 6. device repair
def test_sweep_with_device_repair_is_its_parts():
    """The 24 states of test_rollout_with_device_repair_is_the_loop_and_solves (scale 6: eight of them end with more than 64 active rows,
    that test's docstring) x 2 commands, the state's own and the same with v_des_robot negated, 3 ticks, the device repair on: the chain is
    its parts on a second handle of the same setting bit for bit, every tick-0 status of the candidates that carry the state's own command
    is OK and at least two of them hold more than 64 active rows (that test's own asserts)."""
    t = _scaled_ticks(6.0)
    ns, K = len(t), 2
    nb = ns * K
    cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
    for f in cmd.dtype.names:
        cmd[f][:, 0] = t[f]
        cmd[f][:, 1] = -t[f] if f == "v_des_robot" else t[f]
    s = dict(t=t, cmd=cmd, n=3, tps=8, sub0=0, plant=rm.default_plant(dtMPC=DT), cost=sm.default_cost(**COST_FULL), mass=None, ext=None, pen=None)
    np.testing.assert_array_equal(_bits(sm.expand(t, cmd)[::2]), _bits(t))
    a = _handle(nb, repair=True, auto_resolve=False)
    got = _sweep(a, s)
    a.close()
    b = _handle(nb, repair=True, auto_resolve=False)
    _assert_same_sweep(got, _parts(b, s), "device repair: the chain against its parts")
    b.close()
    own = got["log"]["status"][::2, 0]
    print(f"device repair, 24 x 2 x 3: tick-0 codes {interface.status_code(got['log']['status'][:, 0]).tolist()}, active rows of the own command "
          f"{interface.status_nactive(own).tolist()}")
    assert (interface.status_code(own) == 0).all(), interface.status_code(own)
    assert (interface.status_nactive(own) > QCAP_FAST).sum() >= 2
