#!/usr/bin/env python3
"""What the swing legs cost on the device (profiles/r35/swing.txt), in ONE run, 8 192 standing and 8 192 walking
instances from synthetic.make_ticks(seed 90), after scripts/dev/rollout_time.py:
  a) one launch of swing_legs_kernel (hmpc_swing_legs_device, with the torques, without the detail buffer) next to one launch of the plant
     step and one of build_records_kernel, HIP events, median of five windows of 50 launches each
  b) hmpc_tick_command_device against hmpc_tick_solve_device, 40 calls back to back on the same ticks (host clock around the calls and one
     stream synchronisation; warmed up, median of five)
  c) a 40-tick hmpc_rollout_device with hmpc_set_rollout_swing on (state and command log) against off
Nothing is asserted.

    python scripts/dev/swing_time.py [batch] [ticks]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import interface, synthetic  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n_ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 40
H, TPS, WINDOWS = 10, 8, 5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def median_of(fn, windows=WINDOWS):
    fn()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def events(fn, reps=50):
    fn()
    ms = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms)


for gait in ("standing", "walking"):
    t = synthetic.make_ticks(nb, H, gait, seed=90)
    t["v_des_robot"] = (0.2, 0.0) if gait == "walking" else (0.0, 0.0)
    t["yaw_rate_des"] = 0.0
    t["world_position_desired"] = t["position"][:, :2]
    t["gait_iteration"] = np.arange(nb) % H  # (walking: every phase of the cycle, so that half the legs run the trajectory and the IK)
    plant = interface.default_plant(flags=interface.PLANT_PLACE_FEET if gait == "walking" else 0, dtMPC=synthetic.DT_MPC)
    cfg = interface.default_swing(ticks_per_step=TPS, subtick=3)
    m = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, nb)
    m.set_tick_warm_start(True, 0)
    m.set_auto_resolve(False)
    d_t, fresh = dev(t), dev(t)
    d_s, fresh_s = dev(interface.initial_swing_state(nb)), dev(interface.initial_swing_state(nb))
    d_cmd = torch.zeros(nb * interface.MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_log = torch.zeros(nb * n_ticks * interface.MOTOR_CMD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_tau = torch.zeros((nb, 10), dtype=torch.float64, device="cuda")
    d_wpd = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
    d_sum = torch.zeros((nb, 4), dtype=torch.int32, device="cuda")

    def reset():
        d_t.copy_(fresh)
        d_s.copy_(fresh_s)
        m.reset_tick_warm_start()

    print(f"--- {gait}, {nb} instances")
    # a) one launch each, HIP events
    reset()
    m.tick_solve_device(d_t.data_ptr(), nb, synthetic.DT_MPC, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)
    torch.cuda.synchronize()
    t_swing = events(lambda: m.swing_legs(d_t.data_ptr(), d_s.data_ptr(), cfg, tau=d_tau.data_ptr(), device=True, batch=nb, cmd=d_cmd.data_ptr()))
    plant.dt_tick = 0.0  # (the same arithmetic on a state that does not run away over thousands of launches)
    t_plant = events(lambda: m.plant_step(d_t.data_ptr(), plant, wpd=d_wpd.data_ptr(), summary=d_sum.data_ptr(), device=True, batch=nb))
    plant.dt_tick = 0.005
    t_build = events(lambda: interface._check(m.L.hmpc_build_records_device(m.h, C.c_void_p(d_t.data_ptr()), nb, synthetic.DT_MPC, C.c_void_p(d_wpd.data_ptr()),
                                                                             None), "hmpc_build_records_device"))
    print(f"a) swing_legs_kernel {1e3 * t_swing:7.2f} us per launch, plant_step_kernel {1e3 * t_plant:7.2f} us, build_records_kernel {1e3 * t_build:7.2f} us "
          f"(swing / builder {t_swing / t_build:.2f})")

    # b) whole-call cost of a tick
    def solves():
        reset()
        for _ in range(n_ticks):
            m.tick_solve_device(d_t.data_ptr(), nb, synthetic.DT_MPC, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)

    def commands():
        reset()
        for _ in range(n_ticks):
            m.tick_command(d_t.data_ptr(), d_s.data_ptr(), cfg, device=True, batch=nb, cmd=d_cmd.data_ptr(), wpd=d_wpd.data_ptr(), dt_mpc=synthetic.DT_MPC)

    # c) rollouts
    def rollout_off():
        reset()
        m.rollout(d_t.data_ptr(), n_ticks, TPS, 0, plant=plant, device=True, batch=nb, dt_mpc=synthetic.DT_MPC)

    def rollout_on():
        reset()
        m.rollout(d_t.data_ptr(), n_ticks, TPS, 0, plant=plant, device=True, batch=nb, dt_mpc=synthetic.DT_MPC,
                  swing=dict(cfg=cfg, state=d_s.data_ptr(), cmd_log=d_log.data_ptr()))

    for name, fn in (("b) hmpc_tick_solve_device x n", solves), ("b) hmpc_tick_command_device x n", commands),
                     ("c) hmpc_rollout_device, swing off", rollout_off), ("c) hmpc_rollout_device, swing on", rollout_on)):
        med, lo, hi = median_of(fn)
        print(f"{name:36s} {1e3 * med:8.3f} ms per {n_ticks} ticks (min {1e3 * lo:.3f}, max {1e3 * hi:.3f})  = {nb * n_ticks / med / 1e6:7.3f} M ticks/s")
    m.close()
