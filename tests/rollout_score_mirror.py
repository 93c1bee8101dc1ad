"""Numpy restatement of the closed-loop command sweep's definitions, written from the comment of include/hector_mpc.h above ``struct
hmpc_rollout_cost`` (NOT from the kernels): the score of a rollout's log, the selection per group, the expansion of states x commands.  Every
operation is one correctly rounded binary64 operation in the comment's order -- elementwise numpy only, no ``sum``, no ``dot`` -- and there
is no libm call (``np.rint`` is exact, ties to even), so the kernels are compared with it BIT FOR BIT.  The cases both the CPU test of the
kernels' source (tests/test_rollout_score_kernel_on_host.py) and the GPU test (tests/test_gpu_rollout_score.py) run are built here, once."""
import functools

import numpy as np

from hector_simulation_amd import interface, synthetic

W = 64
TWO_PI = 6.283185307179586
H = 10
NO_WINNER_SUMMARY = np.array([0, -1, 0, 0], dtype=np.int32)


def default_cost(**over):
    c = dict(w_state=[100.0, 100.0, 250.0, 200.0, 200.0, 300.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], w_terminal=[0.0] * 12,
             w_wrench=[1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2], w_tau=[0.0] * 10, height=0.55, dt_tick=0.005,
             fall_penalty=np.inf, unsolved_penalty=0.0)
    c.update(over)
    return c


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _row_error(ticks0, state_k, k, cost, vdw):
    """e of row k for every instance: [batch, 12]"""
    nb = len(ticks0)
    t = np.float64(k + 1) * np.float64(cost["dt_tick"])
    zero = np.zeros(nb)
    ref = [_f64(ticks0["roll_des"]), _f64(ticks0["pitch_des"]), ticks0["rpy"][:, 2] + t * ticks0["yaw_rate_des"],
           ticks0["position"][:, 0] + t * vdw[0], ticks0["position"][:, 1] + t * vdw[1], np.full(nb, np.float64(cost["height"])),
           zero, zero, _f64(ticks0["yaw_rate_des"]), vdw[0], vdw[1], zero]
    e = [state_k[:, s] - ref[s] for s in range(12)]
    e[2] = e[2] - TWO_PI * np.rint(e[2] / TWO_PI)
    return e


def _weighted_square(w, e, acc=None):
    acc = np.zeros(len(e[0])) if acc is None else acc
    for s in range(len(e)):
        acc = acc + (np.float64(w[s]) * e[s]) * e[s]
    return acc


def _butterfly(P):
    """P [batch, W] -> the contract's sum, [batch]"""
    lanes = np.arange(W)
    for off in (32, 16, 8, 4, 2, 1):
        P = P + P[:, lanes ^ off]
    assert (P.view(np.uint64) == P[:, :1].view(np.uint64)).all()  # (every lane ends with the same bits)
    return P[:, 0].copy()


def score(ticks0, log, cost):
    """-> cost [batch, 4], score [batch].  ``log``: dict with ``state`` [batch, n, 12] and, each optional / None, ``wrench`` (float32), ``tau``,
    ``summary``; ``cost``: the dict of ``default_cost``."""
    with np.errstate(all="ignore"):
        state = _f64(log["state"])
        nb, n = state.shape[:2]
        wrench, tau, summary = log.get("wrench"), log.get("tau"), log.get("summary")
        R0 = _f64(ticks0["rBody"])
        cx, cy = _f64(ticks0["v_des_robot"][:, 0]), _f64(ticks0["v_des_robot"][:, 1])
        vdw = [(R0[:, a] * cx + R0[:, 3 + a] * cy) + R0[:, 6 + a] * 0.0 for a in range(2)]
        P_trk, P_eff = np.zeros((nb, W)), np.zeros((nb, W))
        e = None
        for k in range(n):
            e = _row_error(ticks0, state[:, k], k, cost, vdw)
            P_trk[:, k % W] = P_trk[:, k % W] + _weighted_square(cost["w_state"], e)
            eff = np.zeros(nb)
            if wrench is not None:
                u = np.asarray(wrench, dtype=np.float32)[:, k].astype(np.float64)
                eff = _weighted_square(cost["w_wrench"], [u[:, j] for j in range(12)], eff)
            if tau is not None:
                u = _f64(tau)[:, k]
                eff = _weighted_square(cost["w_tau"], [u[:, j] for j in range(10)], eff)
            P_eff[:, k % W] = P_eff[:, k % W] + eff
        out = np.zeros((nb, 4))
        out[:, 0], out[:, 1] = _butterfly(P_trk), _butterfly(P_eff)
        out[:, 2] = _weighted_square(cost["w_terminal"], e)  # (e of row n - 1)
        if summary is not None:
            sm = np.asarray(summary, dtype=np.int32)
            fall = np.where(sm[:, 1] >= 0, np.float64(cost["fall_penalty"]), 0.0)
            uns = np.zeros(nb)
            m = sm[:, 2] > 0
            uns[m] = sm[m, 2].astype(np.float64) * np.float64(cost["unsolved_penalty"])
            out[:, 3] = fall + uns
        return out, ((out[:, 0] + out[:, 1]) + out[:, 2]) + out[:, 3]


def select(score_, penalty, group_size, log=None):
    """-> dict(index, score, and wrench / tau / summary for the members ``log`` has): the definition, a plain loop per group"""
    with np.errstate(all="ignore"):
        s = _f64(score_) if penalty is None else _f64(score_) + _f64(penalty)
    nb = len(s)
    assert nb % group_size == 0
    G = nb // group_size
    out = dict(index=np.full(G, -1, dtype=np.int32), score=np.full(G, np.inf))
    log = log or {}
    if log.get("wrench") is not None:
        out["wrench"] = np.zeros((G, 12), dtype=np.float32)
    if log.get("tau") is not None:
        out["tau"] = np.zeros((G, 10))
    if log.get("summary") is not None:
        out["summary"] = np.tile(NO_WINNER_SUMMARY, (G, 1))
    for g in range(G):
        best = -1
        for k in range(group_size):
            v = s[g * group_size + k]
            if np.isfinite(v) and (best < 0 or v < s[g * group_size + best]):
                best = k
        if best < 0:
            continue
        i = g * group_size + best
        out["index"][g], out["score"][g] = best, s[i]
        if "wrench" in out:
            out["wrench"][g] = np.asarray(log["wrench"], dtype=np.float32)[i, 0]
        if "tau" in out:
            out["tau"][g] = _f64(log["tau"])[i, 0]
        if "summary" in out:
            out["summary"][g] = np.asarray(log["summary"], dtype=np.int32)[i]
    return out


def expand(ticks, commands):
    """instance g K + k = ticks[g] with its five command fields replaced by commands[g][k]"""
    commands = np.asarray(commands, dtype=interface.COMMAND_DTYPE)
    ns, K = commands.shape
    out = np.repeat(np.ascontiguousarray(ticks, dtype=interface.TICK_DTYPE), K)
    flat = commands.reshape(-1)
    for f in ("v_des_robot", "yaw_rate_des", "roll_des", "pitch_des"):
        out[f] = flat[f]
    return out


# ---------------------------------------------------------------------------------------------- the cases
SCORE_TICKS = (1, 63, 64, 65, 130)  # empty lanes, an exactly full wave, a second pass
SCORE_BATCHES = (1, 5, 257)         # a partial workgroup, many workgroups


def synthetic_log(nb, n, seed):
    """ticks0 and a log that looks like a standing rollout's: the state near the reference, forces near the weight, some torques"""
    rng = np.random.default_rng(seed)
    t = synthetic.make_ticks(nb, H, "standing", seed=seed)
    t["v_des_robot"] = rng.uniform(-0.3, 0.3, (nb, 2))
    t["yaw_rate_des"] = rng.uniform(-0.5, 0.5, nb)
    t["roll_des"], t["pitch_des"] = rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.05, 0.05, nb)
    state = np.zeros((nb, n, 12))
    state[:, :, 0:3] = t["rpy"][:, None, :] + rng.normal(0, 0.02, (nb, n, 3))
    state[:, :, 3:6] = t["position"][:, None, :] + rng.normal(0, 0.01, (nb, n, 3))
    state[:, :, 6:12] = rng.normal(0, 0.1, (nb, n, 6))
    wrench = rng.normal(0, 5.0, (nb, n, 12)).astype(np.float32)
    wrench[:, :, [2, 5]] += np.float32(44.0)
    tau = rng.normal(0, 3.0, (nb, n, 10))
    summary = np.tile(np.array([n, -1, 0, 0], dtype=np.int32), (nb, 1))
    summary[:, 3] = rng.integers(1, 30, nb)
    status = rng.integers(0, 2 ** 16, (nb, n)).astype(np.uint32) << 8
    return t, dict(state=state, wrench=wrench, status=status, tau=tau, summary=summary)


@functools.lru_cache(maxsize=None)
def score_cases():
    """(name, ticks0, log, cost dict), every array left unchanged by its users"""
    cases = []
    w_term = [50.0, 50.0, 10.0, 20.0, 20.0, 100.0, 0.5, 0.5, 0.5, 2.0, 2.0, 2.0]
    w_tau = [1e-3 * (j + 1) for j in range(10)]
    for nb in SCORE_BATCHES:
        for n in SCORE_TICKS:
            t, log = synthetic_log(nb, n, seed=1000 + 10 * nb + n)
            cases.append((f"shape-b{nb}-n{n}", t, log, default_cost(w_terminal=w_term, w_tau=w_tau, unsolved_penalty=3.0)))
    nb, n = 5, 65
    t, log = synthetic_log(nb, n, seed=7)
    yaw = dict(log, state=log["state"].copy())
    yaw["state"][0, :, 2] += np.pi + 0.5          # beyond +pi: wrapped down
    yaw["state"][1, :, 2] -= np.pi + 0.5          # beyond -pi
    yaw["state"][2, 3, 2] += 3 * TWO_PI           # three turns
    yaw["state"][3, :, 2] = t["rpy"][3, 2] + np.pi + (np.arange(n) + 1) * 0.005 * t["yaw_rate_des"][3]  # (half a turn, either side of the tie)
    cases.append(("yaw", t, yaw, default_cost(w_terminal=w_term)))
    nan = dict(log, state=log["state"].copy())
    nan["state"][2, 17, 4] = np.nan
    nan["state"][4, n - 1, 9] = np.inf
    cases.append(("nan", t, nan, default_cost(w_terminal=w_term)))
    fallen = dict(log, summary=log["summary"].copy())
    fallen["summary"][1, 1], fallen["summary"][3, 1] = 0, 40
    fallen["summary"][3, 2] = 2
    cases.append(("fallen-inf", t, fallen, default_cost(unsolved_penalty=1.5)))
    cases.append(("fallen-finite", t, fallen, default_cost(fall_penalty=1000.0, unsolved_penalty=1.5)))
    cases.append(("unsolved-inf", t, log, default_cost(unsolved_penalty=np.inf)))  # summary[2] == 0 everywhere: the score stays finite
    unsolved = dict(log, summary=log["summary"].copy())
    unsolved["summary"][0, 2] = 1
    cases.append(("unsolved-inf-one", t, unsolved, default_cost(unsolved_penalty=np.inf)))
    for drop in (("wrench",), ("tau",), ("summary",), ("wrench", "tau", "summary")):
        part = {k: (None if k in drop else v) for k, v in fallen.items()}
        cases.append(("null-" + "-".join(drop), t, part, default_cost(w_tau=w_tau, fall_penalty=77.0)))
    return tuple(cases)


SELECT_GROUPS = (1, 3, 64, 300)  # either side of a wave and of the workgroup


@functools.lru_cache(maxsize=None)
def select_cases():
    """(name, score, penalty or None, group_size, log, n_ticks)"""
    cases = []
    n = 3
    for K in SELECT_GROUPS:
        G = 4
        nb = G * K
        rng = np.random.default_rng(50 + K)
        _, log = synthetic_log(nb, n, seed=60 + K)
        log["summary"][:, 1] = np.where(rng.random(nb) < 0.3, rng.integers(0, n, nb), -1)
        sc = np.round(rng.uniform(0, 20, nb), 1)  # (rounded: exact ties)
        sc[rng.random(nb) < 0.15] = np.inf
        sc[rng.random(nb) < 0.05] = np.nan
        pen = rng.integers(0, 3, nb) * 0.5
        pen[rng.random(nb) < 0.1] = np.nan
        pen[rng.random(nb) < 0.05] = -np.inf
        if K > 1:
            sc[K:2 * K] = np.inf   # group 1: wholly masked
            lo = 2 * K             # group 2: -0.0 against +0.0, the lower index wins
            sc[lo:3 * K] = np.abs(sc[lo:3 * K]) + 1.0
            sc[lo + K - 1], sc[lo + K // 2] = -0.0, 0.0
            pen[lo:3 * K] = 0.0
        else:
            sc[1], pen[1] = np.inf, 0.0
            sc[2], pen[2] = -0.0, 0.0
        cases.append((f"K{K}-penalty", sc, pen, K, log, n))
        cases.append((f"K{K}-plain", sc, None, K, log, n))
    K = 3
    _, log = synthetic_log(4 * K, n, seed=99)
    sc = np.arange(4 * K, dtype=np.float64)[::-1].copy()
    cases.append(("K3-index-and-score-only", sc, None, K, dict(state=log["state"]), n))
    return tuple(cases)
