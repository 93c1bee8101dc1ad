"""The swing update on the device (hmpc_swing_legs_device, hmpc_tick_command_device).

1. One call against the CPU build of the same header (tests/src/swing_on_host.cpp): bit for bit, every output and the whole state -- batches
   1, 24, 129 (a second workgroup at two threads per instance) and 257, both leg_q flag settings, updates 1 and 2, with and without the
   detail buffer and the torques, fresh state and state in mid swing.
2. The 20-tick gait cycle with carried state against the Python mirror (tests/swing_mirror.py) under the tolerance measured on the CPU.
3. The reference's swing sub-phase and foot position of tests/golden/swing_ref.npz.
4. hmpc_tick_command_device against hmpc_tick_solve_device followed by hmpc_swing_legs_device, and its forces, status, f_ff and wpd against
   a plain hmpc_tick_solve_device on a fresh handle: bit for bit; the tick's wrench within 1e-4 of qpOASES, so that nothing upstream moved."""
import numpy as np
import pytest

import swing_mirror as sm
import swing_ref_cases as cases
from hector_simulation_amd import interface, synthetic
from test_swing_kernel_on_host import build_exe, run_cycle, run_on_host
from test_swing_reference import check_kernel_against_golden

pytestmark = pytest.mark.gpu
H = sm.H
NB = 24


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("swinggpu") / "swing_on_host"))


@pytest.fixture(scope="module")
def mpc():
    m = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, 257)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


# ---------------------------------------------------------------------------------------------- 1. one call against the host build
@pytest.mark.parametrize("motor", [False, True])
@pytest.mark.parametrize("nb", [1, 24, 129, 257])
def test_one_call_is_the_host_build_bit_for_bit(mpc, exe, tmp_path, nb, motor):
    t = sm.walking_ticks(nb, seed=500 + nb, motor=False)
    t["gait_iteration"] = np.arange(nb) % H
    t["gait_offsets"][2::4], t["gait_durations"][2::4] = (0, 7), (6, 3)  # an irregular table
    t["gait_offsets"][3::4], t["gait_durations"][3::4] = (0, 0), (H, H)  # standing
    t["vWorld"][4::9, :2] = (4.0, -4.0)                                  # drives the touchdown clamp
    if motor:
        t["flags"] |= interface.TICK_LEG_Q_MOTOR
    rng = np.random.default_rng(nb)
    swinging = 0
    for updates in (1, 2):
        for rich in (False, True):
            cfg = sm.default_swing(updates=updates, ticks_per_step=8 if rich else 40, subtick=3 if rich else 0)
            st = sm.mid_swing_state(t, nb + updates) if rich else interface.initial_swing_state(nb)
            tau = rng.normal(0.0, 10.0, (nb, 10)) if rich else None
            got = mpc.swing_legs(t, st, sm.swing_struct(cfg), tau=tau, detail=rich)
            wc, ws, wd = run_on_host(exe, tmp_path, t, st, cfg, tau)
            what = f"b{nb} motor {motor} updates {updates} rich {rich}"
            np.testing.assert_array_equal(_bits(got["cmd"]), _bits(wc), err_msg=what + ": cmd")
            np.testing.assert_array_equal(_bits(got["state"]), _bits(ws), err_msg=what + ": state")
            if rich:
                np.testing.assert_array_equal(_bits(got["detail"]), _bits(wd), err_msg=what + ": detail")
            else:
                assert not got["cmd"]["tau"].any()
            swinging += int((wd[:, :, 0] > 0).sum())
    assert swinging > 0 or nb == 1


# ---------------------------------------------------------------------------------------------- 2. the gait cycle against the mirror
@pytest.mark.parametrize("case", sm.cycle_cases(), ids=lambda c: c[0])
def test_gait_cycle_with_carried_state_against_the_mirror(mpc, case):
    name, offsets, durations = case

    def step(t, st, cfg, tau):
        out = mpc.swing_legs(t, st, sm.swing_struct(cfg), tau=tau, detail=True)
        return out["cmd"], out["state"], out["detail"]

    worst = run_cycle(step, name, offsets, durations)
    print(f"{name}: largest |device - mirror| in what passes through trigonometry {worst!r} (tolerance {sm.TRIG_TOL!r})")
    assert worst <= sm.TRIG_TOL


# ---------------------------------------------------------------------------------------------- 3. the reference's phase and p
def test_golden_swing_phase_and_leg_position(mpc):
    def step(t, st, cfg):
        out = mpc.swing_legs(t, st, sm.swing_struct(cfg), detail=True)
        return out["cmd"], out["state"], out["detail"]

    check_kernel_against_golden(np.load(cases.GOLDEN), step)


def test_state_init_on_the_device_is_the_initial_state(mpc):
    d_s = _torch().full((NB * interface.SWING_STATE_DTYPE.itemsize,), 0x5A, dtype=_torch().uint8, device="cuda")
    mpc.swing_state(NB - 1, device_ptr=d_s.data_ptr())
    _torch().cuda.synchronize()
    raw = d_s.cpu().numpy()
    used = (NB - 1) * interface.SWING_STATE_DTYPE.itemsize
    np.testing.assert_array_equal(raw[:used], _bits(interface.initial_swing_state(NB - 1)))
    assert (raw[used:] == 0x5A).all()


# ---------------------------------------------------------------------------------------------- 4. ticks in, motor commands out
def test_tick_command_is_tick_solve_then_swing_legs(oracle):
    torch = _torch()
    t = sm.walking_ticks(NB, seed=610, motor=True)
    t["gait_iteration"] = np.arange(NB) % H
    st = sm.mid_swing_state(t, 611)
    cfg = interface.default_swing(ticks_per_step=8, subtick=5)
    a = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, NB)
    got = a.tick_command(t, st, cfg, dt_mpc=synthetic.DT_MPC)
    a.close()
    # the same tick through hmpc_tick_solve_device, then hmpc_swing_legs_device reading its torques, on a fresh handle
    b = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, NB)
    d_t, d_s = _dev(t), _dev(st)
    d_tau, d_wpd = torch.zeros((NB, 10), dtype=torch.float64, device="cuda"), torch.zeros((NB, 2), dtype=torch.float64, device="cuda")
    d_fff = torch.zeros((NB, 2, 6), dtype=torch.float64, device="cuda")
    d_cmd = torch.zeros(NB * interface.MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    b.tick_solve_device(d_t.data_ptr(), NB, synthetic.DT_MPC, d_tau.data_ptr(), d_fff.data_ptr(), d_wpd.data_ptr(), 0)
    b.swing_legs(d_t.data_ptr(), d_s.data_ptr(), cfg, tau=d_tau.data_ptr(), device=True, batch=NB, cmd=d_cmd.data_ptr())
    forces, status = b.download()
    torch.cuda.synchronize()
    b.close()
    want = dict(cmd=d_cmd.cpu().numpy().view(interface.MOTOR_CMD_DTYPE), state=d_s.cpu().numpy().view(interface.SWING_STATE_DTYPE),
                f_ff=d_fff.cpu().numpy(), wpd=d_wpd.cpu().numpy(), forces=forces, status=status)
    for k, v in want.items():
        np.testing.assert_array_equal(_bits(got[k]), _bits(v), err_msg=k)
    np.testing.assert_array_equal(_bits(got["cmd"]["tau"]), _bits(d_tau.cpu().numpy()))
    # ... and a plain hmpc_tick_solve_device alone on another fresh handle
    c = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, NB)
    d_tau2, d_wpd2, d_fff2 = torch.zeros_like(d_tau), torch.zeros_like(d_wpd), torch.zeros_like(d_fff)
    c.tick_solve_device(d_t.data_ptr(), NB, synthetic.DT_MPC, d_tau2.data_ptr(), d_fff2.data_ptr(), d_wpd2.data_ptr(), 0)
    forces2, status2 = c.download()
    torch.cuda.synchronize()
    c.close()
    for k, v in dict(forces=forces2, status=status2, f_ff=d_fff2.cpu().numpy(), wpd=d_wpd2.cpu().numpy()).items():
        np.testing.assert_array_equal(_bits(got[k]), _bits(v), err_msg="plain tick solve: " + k)
    np.testing.assert_array_equal(_bits(got["cmd"]["tau"]), _bits(d_tau2.cpu().numpy()))
    # a swing leg carries gains and a target, a stance leg neither; the ticks were only read
    np.testing.assert_array_equal(_bits(d_t.cpu().numpy()), _bits(t))
    _, _, det = sm.update(t, st, sm.default_swing(ticks_per_step=8, subtick=5))
    sw = np.repeat(det[:, :, 0] > 0, 5, axis=1)
    assert sw.any() and (~sw).any()
    assert (got["cmd"]["Kp"][sw] > 0).all() and not got["cmd"]["Kp"][~sw].any() and not got["cmd"]["dq"].any()
    # nothing upstream moved: the tick's wrench against qpOASES, the suite's bound
    rec, _ = oracle.build_records(t, H, synthetic.DT_MPC)
    ref = oracle.solve_records(rec, H, synthetic.DT_MPC, synthetic.F_MAX)
    assert ref["n_bad"] == 0
    q = ref["q_soln"]
    err = np.abs(got["forces"] - q).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))
    print(f"tick command: forces vs qpOASES {err.max():.2e}")
    assert err.max() < 1e-4
