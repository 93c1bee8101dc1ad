"""ctypes binding of oracle/_ref/libswing_ref.so.  TEST INFRASTRUCTURE ONLY.

That library is the reference's OWN swing-leg controller -- ``src/common/SwingLegController.cpp`` with the caller-side sources of
``libcaller_ref.so`` -- compiled unmodified from the reference checkout against the Eigen stand-in ``oracle/mini_eigen`` (recipe:
``oracle/Makefile``); ``oracle/swing_ref_shim.cpp`` says what the shim supplies.  Used by tests/ (and
tests/golden/make_swing_update_golden.py) only.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from . import ref_py

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libswing_ref.so")
REFERENCE = os.environ.get("REF", "/root/reference")  # (oracle/Makefile's REF)
STAMP_PATH = LIB_PATH + ".srchash"
SHIM_PATH = os.path.join(HERE, "swing_ref_shim.cpp")
SWING_FIELDS = (("swing_time", 0, 1), ("first_swing", 1, 2), ("p0", 2, 5), ("pf", 5, 8), ("swing", 8, 9), ("pFoot_w", 9, 12),
                ("pFoot_b", 12, 15), ("vFoot_b", 15, 18), ("pDes_w", 18, 21), ("vDes_w", 21, 24))  # swr_get_swing's row of 24
COMMAND_FIELDS = (("qDes", 0, 5), ("qdDes", 5, 10), ("pDes", 10, 13), ("vDes", 13, 16), ("kp", 16, 21), ("kd", 21, 26),
                  ("feedforwardForce", 26, 32), ("kptoe", 32, 33), ("kdtoe", 33, 34))  # swr_get_command's row of 34


def available() -> bool:
    return os.path.exists(LIB_PATH)


def _shim_hash() -> str:
    with open(SHIM_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _stamp() -> str | None:
    try:
        with open(STAMP_PATH) as f:
            return f.read().strip()
    except OSError:
        return None


def build() -> None:
    """Builds the library through oracle/Makefile; a library left by an earlier build is judged by the content of the shim it was built from
    (a stamp beside it), as oracle/caller_py.py does.  Where the reference's sources are absent the prebuilt file is kept as it is."""
    want = _shim_hash()
    if os.path.exists(LIB_PATH) and _stamp() == want:
        return
    can_rebuild = os.path.isdir(REFERENCE)
    subprocess.check_call(["make", "-C", HERE, "-s"] + (["-B"] if can_rebuild and os.path.exists(LIB_PATH) else []) + [LIB_PATH])
    if can_rebuild:
        with open(STAMP_PATH, "w") as f:
            f.write(want + "\n")


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.swr_set_solution.argtypes = [vp, C.c_int]
        L.swr_create.restype = vp
        L.swr_create.argtypes = [C.c_int] * 5 + [C.c_double]
        L.swr_create_run.restype = vp
        L.swr_create_run.argtypes = [C.c_double, C.c_int, C.c_char_p]
        L.swr_destroy.argtypes = [vp]
        L.swr_set_state.argtypes = [vp] * 7
        L.swr_set_command.argtypes = [vp, vp]
        L.swr_update_leg_data_from_motors.argtypes = [vp, vp]
        L.swr_poke_leg_q.argtypes = [vp, vp]
        L.swr_get_leg.argtypes = [vp, C.c_int, vp, vp]
        L.swr_update.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.swr_compute_ik.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, vp]
        L.swr_get_swing.argtypes = [vp, C.c_int, vp]
        L.swr_set_swing.argtypes = [vp, C.c_int, vp]
        L.swr_get_command.argtypes = [vp, C.c_int, vp]
        L.swr_set_q_des.argtypes = [vp, vp]
        L.swr_run_tick.argtypes = [vp, C.c_int, vp]
        L.swr_tau_of.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data


def set_solution(sol) -> None:
    s = np.ascontiguousarray(sol, dtype=np.float64)
    lib().swr_set_solution(_p(s), s.size)


class Swing:
    """One swingLegController of the reference with the object graph main.cpp builds around it.  ``Swing(offsets, durations, dt_swing)``: with
    a Gait(horizon, offsets, durations) of its own, for ``update``; ``Swing.whole_ticks(dt, iterations_between_mpc)``: inside a
    ConvexMPCLocomotion, for ``run_tick``."""

    def __init__(self, offsets=(0, 5), durations=(5, 5), dt_swing=0.04, horizon=10, _run=None):
        L = lib()
        self._scratch = None
        if _run is None:
            self.h = L.swr_create(int(horizon), int(offsets[0]), int(offsets[1]), int(durations[0]), int(durations[1]), float(dt_swing))
        else:
            self._scratch = tempfile.TemporaryDirectory(prefix="refswing_")  # the constructor opens ./foot_pos.txt
            self.h = L.swr_create_run(float(_run[0]), int(_run[1]), self._scratch.name.encode())
        assert self.h

    @classmethod
    def whole_ticks(cls, dt, iterations_between_mpc):
        return cls(_run=(dt, iterations_between_mpc))

    def close(self):
        if self.h:
            lib().swr_destroy(self.h)
            self.h = None
            if self._scratch is not None:
                self._scratch.cleanup()

    def set_tick(self, t):
        """the state estimate, stateDes[6..7] and the leg data of one ``hmpc_tick_inputs`` row.  HMPC_TICK_LEG_Q_MOTOR set: leg_q holds motor
        angles (binary32 values, as MotorState::q) and goes through the reference's updateData.  Not set: leg_q holds data[leg].q as stored; the
        motor angles that give it are ``t['leg_q']`` less the LegController's offsets in binary32 -- updateData runs on those (for data[leg].p),
        then the stored angles are poked."""
        a = [np.ascontiguousarray(t[k], dtype=np.float64).reshape(-1) for k in ("position", "vWorld", "omegaWorld", "orientation", "rpy", "rBody")]
        lib().swr_set_state(self.h, *[_p(x) for x in a])
        s = np.zeros(12)
        s[3], s[4], s[6], s[7], s[11] = t["roll_des"], t["pitch_des"], t["v_des_robot"][0], t["v_des_robot"][1], t["yaw_rate_des"]
        lib().swr_set_command(self.h, _p(s))
        q = np.ascontiguousarray(t["leg_q"], dtype=np.float64).reshape(10)
        if int(t["flags"]) & 1:
            m = q.astype(np.float32)
            assert (m.astype(np.float64) == q).all(), "motor angles must be binary32 values"
            lib().swr_update_leg_data_from_motors(self.h, _p(m))
        else:
            off = np.tile([0.0, 0.0, 0.3 * 3.14159, -0.6 * 3.14159, 0.3 * 3.14159], 2)
            m = (q - off).astype(np.float32)
            assert (m.astype(np.float64) + off == q).all(), "stored angles must be binary32 motor angles + the LegController's offsets"
            lib().swr_update_leg_data_from_motors(self.h, _p(m))
            lib().swr_poke_leg_q(self.h, _p(q))

    def leg(self, leg):
        q, p = np.zeros(5), np.zeros(3)
        lib().swr_get_leg(self.h, int(leg), _p(q), _p(p))
        return dict(q=q, p=p)

    def update(self, ticks_per_step, cur, updates=2):
        lib().swr_update(self.h, int(ticks_per_step), int(cur), int(updates))

    def compute_ik(self, pFoot_b, leg, q2, q3):
        p, q = np.ascontiguousarray(pFoot_b, dtype=np.float64), np.zeros(5)
        lib().swr_compute_ik(self.h, _p(p), int(leg), float(q2), float(q3), _p(q))
        return q

    def swing_row(self, leg):
        r = np.zeros(24)
        lib().swr_get_swing(self.h, int(leg), _p(r))
        return r

    def swing(self, leg):
        r = self.swing_row(leg)
        return {k: (r[a] if b == a + 1 else r[a:b].copy()) for k, a, b in SWING_FIELDS}

    def set_swing(self, leg, **fields):
        r = self.swing_row(leg)
        for k, a, b in SWING_FIELDS:
            if k in fields:
                r[a:b] = fields[k]
        lib().swr_set_swing(self.h, int(leg), _p(r))

    def command_row(self, leg):
        r = np.zeros(34)
        lib().swr_get_command(self.h, int(leg), _p(r))
        return r

    def command(self, leg):
        r = self.command_row(leg)
        return {k: (r[a] if b == a + 1 else r[a:b].copy()) for k, a, b in COMMAND_FIELDS}

    def set_q_des(self, q10):
        q = np.ascontiguousarray(q10, dtype=np.float64).reshape(10)
        lib().swr_set_q_des(self.h, _p(q))

    def run_tick(self, gait_number=2):
        """setGaitNum, ConvexMPCLocomotion::run, LegController::updateCommand: float32 [10, 5] = q, dq, Kp, Kd, tau of the ten motors"""
        out = np.zeros((10, 5), dtype=np.float32)
        with ref_py.quiet():
            lib().swr_run_tick(self.h, int(gait_number), _p(out))
        return out

    def tau_of(self, f_ff):
        f = np.ascontiguousarray(f_ff, dtype=np.float64).reshape(12)
        tau = np.zeros(10, dtype=np.float32)
        lib().swr_tau_of(self.h, _p(f), _p(tau))
        return tau
