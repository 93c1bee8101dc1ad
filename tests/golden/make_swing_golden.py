"""Generates tests/golden/swing_ref.npz FROM THE REFERENCE'S OWN GaitGenerator.cpp and LegController.cpp.

Provenance: oracle/_ref/libcaller_ref.so = ConvexMPC/GaitGenerator.cpp + src/common/LegController.cpp (+ the rest of the caller) compiled
unmodified from the reference checkout against the Eigen stand-in oracle/mini_eigen (recipe oracle/Makefile; what the shim supplies:
oracle/caller_ref_shim.cpp).  These are the two pieces the swing update takes from those files: the swing sub-phase and the leg's foot
position.  The reference's SwingLegController.cpp itself is executed by oracle/_ref/libswing_ref.so and recorded by
tests/golden/make_swing_update_golden.py (timer, touchdown point, first-swing capture, Bezier target, computeIK, gains, whole ticks).

Run where the reference checkout is (oracle/Makefile's REF):  python tests/golden/make_swing_golden.py

Contents (data only)
  gait_rows    [n, 6] int32: offsets[2], durations[2], ticks_per_step, current_iteration (tests/swing_ref_cases.gait_rows)
  swing_ref    [n, 2] Gait::getSwingSubPhase() after setIterations(ticks_per_step, current_iteration), horizon 10
  q_motor      [32, 10] raw motor angles (tests/swing_ref_cases.motor_angles)
  q_ref        [32, 2, 5] data[leg].q after computeLegJacobianAndPosition (the 3.14159-based offsets added in place)
  p_ref        [32, 2, 3] data[leg].p
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import caller_py  # noqa: E402
import swing_mirror as sm  # noqa: E402
import swing_ref_cases as cases  # noqa: E402


def through_reference():
    rows = cases.gait_rows()
    swing = np.array([caller_py.gait(sm.H, o, d, tps, cur)["swing"] for o, d, tps, cur in rows])
    q10 = cases.motor_angles()
    c = caller_py.Caller()
    q_ref, p_ref = np.zeros((len(q10), 2, 5)), np.zeros((len(q10), 2, 3))
    for n, q in enumerate(q10):
        c.set_leg_q(q)
        for leg in range(2):
            d = c.leg(leg)
            q_ref[n, leg], p_ref[n, leg] = d["q"], d["p"]
    c.close()
    flat = np.array([list(o) + list(d) + [tps, cur] for o, d, tps, cur in rows], dtype=np.int32)
    return dict(gait_rows=flat, swing_ref=swing, q_motor=q10, q_ref=q_ref, p_ref=p_ref)


def main():
    caller_py.build()
    out = through_reference()
    np.savez_compressed(cases.GOLDEN, **out)
    print(cases.GOLDEN, os.path.getsize(cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
