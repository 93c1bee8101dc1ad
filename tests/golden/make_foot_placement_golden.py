"""Generates tests/golden/foot_placement_ref.npz FROM THE REFERENCE'S OWN run() (ConvexMPCLocomotion.cpp:31-269).

Provenance: oracle/_ref/libcaller_ref.so = ConvexMPC/GaitGenerator.cpp + ConvexMPC/ConvexMPCLocomotion.cpp + src/common/LegController.cpp
(+ FootSwingTrajectory.cpp, DesiredCommand.cpp) compiled unmodified from /root/reference against the Eigen stand-in oracle/mini_eigen
(recipe oracle/Makefile; what the shim supplies: oracle/caller_ref_shim.cpp).

Run in the build container (needs /root/reference):  python tests/golden/make_foot_placement_golden.py

Contents (data only)
  ticks        hmpc_tick_inputs rows of tests/plant_physics_cases.foot_inputs() (bytes): the state, command and gait phase run() was given
  pf_ref       [16, 2, 3] the final position run() handed to footSwingTrajectories[leg] (the foot-placement heuristic, :148-166), both legs
  swing_time   [16, 2] the swingTimeRemaining[leg] run() extrapolated the hip over (dtMPC * gait->_swing: firstSwing is never cleared)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import caller_py  # noqa: E402
import plant_physics_cases as cases  # noqa: E402

WALKING = 2  # ConvexMPCLocomotion.cpp:42


def through_run(t):
    """each tick through the reference's run() -> (pf_ref [n, 2, 3], swing_time [n, 2])"""
    c = caller_py.Caller()
    c.set_solution(np.zeros(12 * 10))
    pf, rem = np.zeros((len(t), 2, 3)), np.zeros((len(t), 2))
    for k, row in enumerate(t):
        c.set_state(row["position"], row["vWorld"], row["omegaWorld"], row["orientation"], row["rpy"], row["rBody"])
        c.set_command(row["roll_des"], row["pitch_des"], row["v_des_robot"][0], row["v_des_robot"][1], row["yaw_rate_des"])
        c.poke_leg_q(row["leg_q"])
        c.set_members(row["world_position_desired"], row["pFoot"], caller_py.ITERATIONS_BETWEEN_MPC * int(row["gait_iteration"]), WALKING)
        c.run(WALKING)
        for leg in range(2):
            pf[k, leg], rem[k, leg] = c.swing_final(leg)
    c.close()
    return pf, rem


def main():
    caller_py.build()
    t = cases.foot_inputs()
    pf, rem = through_run(t)
    path = os.path.join(HERE, cases.FOOT_GOLDEN)
    np.savez_compressed(path, ticks=t.view(np.uint8).reshape(len(t), -1), pf_ref=pf, swing_time=rem)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
