"""The definition of hmpc_sweep_select (include/hector_mpc.h) restated in numpy, and the comparison against it.

Fed with the GPU's OWN downloaded cost, states, status words and forces, every comparison is exact: two binary64 additions per instance,
which numpy rounds as the device does, then comparisons and bit copies.  No tolerance enters."""
import numpy as np

SELECT_NONE = np.uint32(0xFFFFFFFF)
ELIGIBLE_CODES = (0, 6)  # HMPC_S_OK, HMPC_S_OK_RELAXED


def scores(cost, penalty=None):
    """score_i = (cost[i][0] + cost[i][1]) + penalty[i]: two plain binary64 additions in that order, the second only with a penalty."""
    cost = np.asarray(cost, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = cost[:, 0] + cost[:, 1]
        if penalty is not None:
            s = s + np.asarray(penalty, dtype=np.float64)
    return s


def select(cost, states, status, forces, group_size, penalty=None):
    """dict(index int32[G], score float64[G], forces float32[G, nvar], status uint32[G], states float32[G, h, 13]), by a plain loop."""
    status = np.asarray(status, dtype=np.uint32)
    forces = np.asarray(forces, dtype=np.float32)
    states = np.asarray(states, dtype=np.float32)
    b, k = status.shape[0], int(group_size)
    assert k >= 1 and b % k == 0
    groups = b // k
    s = scores(cost, penalty)
    eligible = np.isin(status & np.uint32(0xFF), ELIGIBLE_CODES) & np.isfinite(s)
    out = dict(index=np.full(groups, -1, dtype=np.int32), score=np.full(groups, np.inf, dtype=np.float64),
               forces=np.zeros((groups,) + forces.shape[1:], dtype=np.float32), status=np.full(groups, SELECT_NONE, dtype=np.uint32),
               states=np.zeros((groups,) + states.shape[1:], dtype=np.float32))
    for g in range(groups):
        best = -1
        for j in range(k):
            i = g * k + j
            if eligible[i] and (best < 0 or s[i] < s[g * k + best]):  # strictly smaller: equal scores (==) keep the lowest index
                best = j
        if best >= 0:
            i = g * k + best
            out["index"][g], out["score"][g], out["status"][g] = best, s[i], status[i]
            out["forces"][g], out["states"][g] = forces[i], states[i]
    return out


def assert_equal(got, want, what=""):
    """index equal; score, forces, states and status equal as bit patterns"""
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=f"{what} index")
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=f"{what} status")
    np.testing.assert_array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64), err_msg=f"{what} score")
    np.testing.assert_array_equal(got["forces"].view(np.uint32), want["forces"].view(np.uint32), err_msg=f"{what} forces")
    np.testing.assert_array_equal(got["states"].view(np.uint32), want["states"].view(np.uint32), err_msg=f"{what} states")


def expand_ticks(ticks, commands):
    """ticks[G] x commands[G, K] -> ticks[G * K]: tick g repeated K times with its five command fields replaced."""
    groups, k = commands.shape
    out = np.repeat(ticks, k)
    flat = commands.reshape(groups * k)
    for name in ("v_des_robot", "yaw_rate_des", "roll_des", "pitch_des"):
        out[name] = flat[name]
    return out
