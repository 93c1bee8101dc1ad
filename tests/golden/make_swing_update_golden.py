"""Generates tests/golden/swing_update_ref.npz FROM THE REFERENCE'S OWN SwingLegController.cpp.

Provenance: oracle/_ref/libswing_ref.so = src/common/SwingLegController.cpp + ConvexMPC/GaitGenerator.cpp, ConvexMPCLocomotion.cpp,
src/common/LegController.cpp, FootSwingTrajectory.cpp, DesiredCommand.cpp compiled unmodified from the reference checkout against the Eigen
stand-in oracle/mini_eigen (recipe oracle/Makefile; what the shim supplies: oracle/swing_ref_shim.cpp).

Run where the reference checkout is (oracle/Makefile's REF):  python tests/golden/make_swing_update_golden.py

Eighty-one ticks of four instances in binary64 do not fit one file of 200 KB, so the three runs at ticks_per_step 8 go into a second file,
tests/golden/swing_update_ref_tps8.npz; swing_update_cases.load_golden reads both as one.

Contents (data only; the inputs come from tests/swing_update_cases.py and only their SHA-256 is stored)
  inputs_sha256  [32] uint8
  a_<n>          [n_ticks, 4, 2, 44] run n of swing_update_cases.runs(), per tick, instance and leg (COLS): swing sub-phase, swing_time,
                 first_swing, p0, pf, pFoot_w, pDes, vDes (the trajectory's, world frame), pFoot_b, vFoot_b, qDes, qdDes, diag kpJoint, diag
                 kdJoint after the tick's two updateSwingLeg().  pDes .. vFoot_b of a leg that is not in swing are written as 0 (the reference
                 leaves them as an earlier tick set them; the tick defines nothing there).
  ik_q           [n, 5] computeIK of swing_update_cases.ik_rows()
  c_cmd          [51, 4, 10, 5] float32: q, dq, Kp, Kd, tau of LowlevelCmd::motorCmd after run() + updateCommand
  c_tau_ff       [51, 4, 10] float32: what updateCommand makes of feedforwardForce = the tick's f_ff on BOTH legs at the same leg data
                 (f_ff: the reference's updateMPCIfNeeded through oracle/_ref/libcaller_ref.so on the unmasked forces; zero for a leg that
                 step 0 of the tick's MPC table has in swing)
  edge_q         [48, 5], edge_pFoot_b [48, 3]: qDes and pFoot_b of leg 0 on swing_update_cases.edge_ticks()
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import caller_py, swing_py  # noqa: E402
import swing_mirror as sm  # noqa: E402
import swing_update_cases as cases  # noqa: E402

COLS = cases.COLS


def leg_row(s, leg):
    sw, cm = s.swing(leg), s.command(leg)
    row = np.zeros(44)
    for k, src in (("swing", sw["swing"]), ("swing_time", sw["swing_time"]), ("first_swing", sw["first_swing"]), ("p0", sw["p0"]),
                   ("pf", sw["pf"]), ("pFoot_w", sw["pFoot_w"]), ("qDes", cm["qDes"]), ("qdDes", cm["qdDes"]), ("kp", cm["kp"]), ("kd", cm["kd"])):
        row[slice(*COLS[k])] = src
    if sw["swing"] > 0:
        for k, src in (("pDes", sw["pDes_w"]), ("vDes", sw["vDes_w"]), ("pFoot_b", sw["pFoot_b"]), ("vFoot_b", sw["vFoot_b"])):
            row[slice(*COLS[k])] = src
        # commands[leg].pDes / vDes are the body-frame target and velocity; a swing leg carries no feed-forward force and the toe gains
        assert (cm["pDes"] == sw["pFoot_b"]).all() and (cm["vDes"] == sw["vFoot_b"]).all() and not cm["feedforwardForce"].any()
        assert cm["kptoe"] == 5 and cm["kdtoe"] == 0.1
    return row


def group_a(n, seed=None):
    name, o, d, tps, dtmpc = cases.runs()[n]
    seq, cfgs = cases.run_inputs(n, seed)
    inst = [swing_py.Swing(o, d, dtmpc, sm.H) for _ in range(cases.NB)]
    out = np.zeros((len(seq), cases.NB, 2, 44))
    for k, t in enumerate(seq):
        for i, s in enumerate(inst):
            s.set_tick(t[i])
            if not int(t["flags"][i]) & 1:  # the reference holds the tick's stored angles bit for bit
                assert (np.concatenate([s.leg(0)["q"], s.leg(1)["q"]]) == t["leg_q"][i]).all()
            s.update(tps, k, cfgs[k]["updates"])
            for leg in range(2):
                out[k, i, leg] = leg_row(s, leg)
    for s in inst:
        s.close()
    return out


def group_b():
    rows, region = cases.ik_rows()
    s = swing_py.Swing()
    q = np.array([s.compute_ik(r[:3], int(r[3]), r[4], r[5]) for r in rows])
    s.close()
    assert np.isfinite(q).all()
    # every region holds its rows, read off the reference's own results: out of reach the knee term is 2 asin(1) - pi = 0, inside the sphere
    # the NaN of the square root comes out of the clamp as -1 (2 asin(-1) - pi = -2 pi), on the floor of distance_vertical the second acos
    # is acos(sqrt(0.00001) / dxz)
    inr = cases.in_region(rows)
    f, d3, dyz, m, r1 = cases.ik_intermediates(rows)
    for r, name in enumerate(cases.REGIONS):
        sel = region == r
        for leg in range(2):
            assert (sel & (rows[:, 3] == leg) & inr[:, r]).sum() >= 8, name
        for sign in (-1.0, 1.0):
            assert (sel & (np.sign(f[:, 0]) == sign)).sum() >= 4, name
    assert (q[region == 0, 3] == 0.6 * sm.PI).all() and (q[region == 1, 3] == (2.0 * np.arcsin(-1.0) - sm.PI) + 0.6 * sm.PI).all()
    fl = region == 2
    dxz = np.sqrt(d3[fl] * d3[fl] - 0.0205 ** 2)
    want = np.arccos(dxz / 0.44) - np.arccos(np.sqrt(0.00001) / dxz) * np.sign(f[fl, 0]) - 0.3 * sm.PI
    assert np.abs(q[fl, 2] - want).max() < 1e-12
    assert (f[region == -1, 0] < 0).sum() >= 64 and (f[region == -1, 0] > 0).sum() >= 64
    return q


def group_c():
    seq, forces, _ = cases.whole_tick_inputs()
    cmd, tau_ff = np.zeros((len(seq), cases.NB, 10, 5), dtype=np.float32), np.zeros((len(seq), cases.NB, 10), dtype=np.float32)
    for i in range(cases.NB):
        # f_ff of this instance (the attitude stays, so one tick serves): the reference's updateMPCIfNeeded on the same state and forces
        c = caller_py.Caller()
        c.set_solution(forces[i])
        t0 = seq[0][i]
        c.set_state(t0["position"], t0["vWorld"], t0["omegaWorld"], t0["orientation"], t0["rpy"], t0["rBody"])
        c.set_command(t0["roll_des"], t0["pitch_des"], t0["v_des_robot"][0], t0["v_des_robot"][1], t0["yaw_rate_des"])
        c.poke_leg_q(t0["leg_q"])
        c.set_members(t0["world_position_desired"], t0["pFoot"], 0, 2)
        c.update_mpc()
        f_ff = c.members()["f_ff"].copy()
        c.close()
        s = swing_py.Swing.whole_ticks(cases.RUN_DT, cases.RUN_TPS)
        for k, t in enumerate(seq):
            s.set_tick(t[i])
            swing_py.set_solution(cases.tick_forces(forces[i], k))
            cmd[k, i] = s.run_tick(2)
            table = np.array([[cases.mpc_stance(k, leg)] for leg in range(2)])
            tau_ff[k, i] = s.tau_of(np.where(table, f_ff, 0.0))
            # a leg the run() treated as a stance leg carries exactly that f_ff, or none where the table gives it no force
            for leg in range(2):
                ff = s.command(leg)["feedforwardForce"]
                assert not ff.any() or (ff == f_ff[leg]).all()
        s.close()
    return cmd, tau_ff


def group_d():
    t, st, cfg, region = cases.edge_ticks()
    q, pb = np.zeros((len(t), 5)), np.zeros((len(t), 3))
    for i in range(len(t)):
        s = swing_py.Swing((0, 5), (5, 5), cfg["dtMPC"], sm.H)
        s.set_tick(t[i])
        for leg in range(2):
            s.set_swing(leg, swing_time=st["swing_time"][i, leg], first_swing=float(st["first_swing"][i, leg]), p0=st["p0"][i, leg], pf=st["pf"][i, leg])
        s.update(cfg["ticks_per_step"], int(t["gait_iteration"][i]) * cfg["ticks_per_step"] + cfg["subtick"], cfg["updates"])
        assert s.swing(0)["swing"] == 0.5 and s.swing(1)["swing"] == 0.0
        q[i], pb[i] = s.command(0)["qDes"], s.swing(0)["pFoot_b"]
        s.close()
    assert np.isfinite(q).all()
    rows = np.concatenate([pb, np.zeros((len(t), 3))], axis=1)
    inr = cases.in_region(rows)
    for r, name in enumerate(cases.REGIONS):
        assert inr[region == r, r].all(), (name, inr[region == r])
    return q, pb


def leave_out_share(a):
    """share of the swing-leg rows of a group-a array whose q_des[2] or q_des[3] is ill-conditioned, on the reference's own pFoot_b"""
    sw = a[..., 0] > 0
    ill = cases.ill_conditioned(a[..., 18:21])[..., 2:4].any(axis=-1)
    return float((ill & sw).sum()) / float(sw.sum())


def through_reference():
    out = dict(inputs_sha256=cases.inputs_digest())
    for n in range(len(cases.runs())):
        out[f"a_{n}"] = group_a(n)
        assert np.isfinite(out[f"a_{n}"]).all()
        share = leave_out_share(out[f"a_{n}"])
        # (the cap of the issue: were a seed to exceed it, swing_update_cases.run_inputs would get another seed)
        assert share <= cases.LEAVE_OUT_CAP, (cases.runs()[n][0], share)
    out["ik_q"] = group_b()
    out["c_cmd"], out["c_tau_ff"] = group_c()
    out["edge_q"], out["edge_pFoot_b"] = group_d()
    return out


def main():
    swing_py.build()
    caller_py.build()
    out = through_reference()
    for path, part in cases.split_golden(out):
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
