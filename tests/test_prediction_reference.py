"""The prediction's definition (include/hector_mpc.h hmpc_predict_states: the step-by-step recurrence over the contract's binary32 Acd,
Bcd, x0, in binary64) pinned to an execution of the reference's own source: its A_qp x_0 + B_qp q_soln (SolverMPC.cpp:457-461, the
matrices c2qp leaves behind) for the same record and the same forces.  What separates the two is the binary32 round-off of the
reference's matrix powers, nothing else.  Needs the reference's source compiled (oracle/_ref): skipped where that is absent."""
import numpy as np
import pytest

import prediction_mirror as pm
from hector_simulation_amd import records, synthetic
from oracle import ref_py

pytestmark = pytest.mark.skipif(not ref_py.available(), reason="oracle/_ref (the reference's own source, compiled) is not here")

H, NB = 10, 16
# max |recurrence - (A_qp x_0 + B_qp q_soln)| over the 16 instances of each case, measured on the CPU for these seeds (states of order 1,
# the gravity entry 9.81: absolute figures); asserted at 4x, the margin for the seed-to-seed spread of binary32 round-off
MEASURED = {"standing": 4.385e-07, "walking": 6.159e-07}
MARGIN = 4.0


@pytest.mark.parametrize("gait,seed,phase", [("standing", 201, 0), ("walking", 202, "random")])
def test_recurrence_is_the_reference_s_own_prediction(oracle, gait, seed, phase):
    f = synthetic.make_batch(NB, H, gait, seed=seed, phase=phase)
    rec = records.pack_records(f, H)
    un = records.unpack_records(rec, H)
    worst = 0.0
    for k in range(NB):
        t = ref_py.tick({key: np.asarray(v)[k] for key, v in f.items()}, H, synthetic.DT_MPC, 0.25, synthetic.F_MAX)
        q = t["q_soln"]
        theirs = t["A_qp"].astype(np.float64) @ t["x_0"].astype(np.float64).reshape(13) + t["B_qp"].astype(np.float64) @ q
        o = oracle.assemble_record(rec[k], H, synthetic.DT_MPC, synthetic.F_MAX, reduce=False)
        ours, _ = pm.rollout(o["Acd"], o["Bcd"], o["x0"], q.reshape(H, 12), un["weights"][k], un["traj"][k], un["Alpha_K"][k])
        assert np.abs(theirs).max() > 9.0  # (the comparison is not vacuous: the gravity entry is there)
        worst = max(worst, float(np.abs(ours.reshape(-1) - theirs).max()))
    print(gait, "max abs gap", worst, "bound", MARGIN * MEASURED[gait])
    assert worst <= MARGIN * MEASURED[gait], worst
