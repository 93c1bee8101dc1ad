"""The inputs of the swing update's reference pins (tests/golden/swing_ref.npz, written by tests/golden/make_swing_golden.py from the
reference's own GaitGenerator.cpp and LegController.cpp through oracle/caller_py.py), shared by the generator, the CPU test
(tests/test_swing_reference.py) and the GPU test (tests/test_gpu_swing.py)."""
import os

import numpy as np

import swing_mirror as sm
from hector_simulation_amd import interface

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swing_ref.npz")
TICKS_PER_STEP = (2, 8)


def gait_rows():
    """[(offsets, durations, ticks_per_step, current_iteration)]: every sub-iteration of a cycle of the tables of swing_mirror.cycle_cases"""
    return [(o, d, tps, cur) for _, o, d in sm.cycle_cases() for tps in TICKS_PER_STEP for cur in range(tps * sm.H)]


def motor_angles():
    """[32, 10]: 64 random joint vectors (two legs each), raw motor angles around the standing pose"""
    rng = np.random.default_rng(64)
    q = np.zeros((32, 2, 5))
    q[:, :, 0], q[:, :, 1] = rng.uniform(-0.4, 0.4, (32, 2)), rng.uniform(-0.4, 0.4, (32, 2))
    q[:, :, 2], q[:, :, 3], q[:, :, 4] = rng.uniform(-0.2, 1.2, (32, 2)), rng.uniform(-2.0, -0.2, (32, 2)), rng.uniform(-0.2, 1.2, (32, 2))
    return q.reshape(32, 10)


def phase_ticks(rows):
    """one tick struct per gait row (identity attitude, at the origin) and its ticks_per_step / subtick"""
    t = np.zeros(len(rows), dtype=interface.TICK_DTYPE)
    t["orientation"][:, 0] = 1.0
    t["rBody"][:, [0, 4, 8]] = 1.0
    tps, sub = np.zeros(len(rows), dtype=int), np.zeros(len(rows), dtype=int)
    for n, (o, d, k, cur) in enumerate(rows):
        t["gait_offsets"][n], t["gait_durations"][n], t["gait_iteration"][n] = o, d, cur // k
        tps[n], sub[n] = k, cur % k
    return t, tps, sub


def leg_ticks(q10):
    """tick structs (identity attitude, at the origin) that carry raw motor angles: pFoot_w[0:2] = (hipYaw + data[leg].p)[0:2]"""
    t = np.zeros(len(q10), dtype=interface.TICK_DTYPE)
    t["orientation"][:, 0] = 1.0
    t["rBody"][:, [0, 4, 8]] = 1.0
    t["leg_q"] = q10
    t["flags"] = interface.TICK_LEG_Q_MOTOR
    t["gait_durations"] = 5
    t["gait_offsets"][:, 1] = 5
    return t
