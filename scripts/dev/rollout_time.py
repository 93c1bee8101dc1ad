#!/usr/bin/env python3
"""What a closed loop on the device costs (profiles/r27/rollout.txt), in ONE run, 8 192 standing and 8 192 walking
instances, 40 ticks, zero commands from synthetic.make_ticks(seed 90):
  a) hmpc_rollout_device: ticks/s (host clock around the call and one stream synchronisation; warmed up, median of five)
  b) the host-driven loop: per tick hmpc_tick_solve_device, a synchronisation, a download of forces and status, hmpc_plant_step_device, a
     synchronisation (what tests/test_gpu_rollout.py compares the rollout with)
  c) hmpc_tick_solve_device alone, 40 times back to back on the same ticks: the ceiling
  d) one launch of the plant step next to one launch of build_records_kernel (hmpc_build_records_device), HIP events, median of five windows
     of 50 launches each
Nothing is asserted.

    python scripts/dev/rollout_time.py [batch] [ticks]"""
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


def dev(t):
    return torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).reshape(len(t), -1).copy()).cuda()


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


for gait in ("standing", "walking"):
    t = synthetic.make_ticks(nb, H, gait, seed=90)
    t["v_des_robot"] = (0.2, 0.0) if gait == "walking" else (0.0, 0.0)
    t["yaw_rate_des"] = 0.0
    t["world_position_desired"] = t["position"][:, :2]
    t["gait_iteration"] = 0
    plant = interface.default_plant(flags=interface.PLANT_PLACE_FEET if gait == "walking" else 0, dtMPC=synthetic.DT_MPC)
    m = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, nb)
    m.set_tick_warm_start(True, 0)
    m.set_auto_resolve(False)
    d_t = dev(t)
    d_tau = torch.zeros((nb, 10), dtype=torch.float64, device="cuda")
    d_wpd = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
    d_sum = torch.zeros((nb, 4), dtype=torch.int32, device="cuda")
    fresh = dev(t)

    def reset():
        d_t.copy_(fresh)
        m.reset_tick_warm_start()

    def rollout():
        reset()
        m.rollout(d_t.data_ptr(), n_ticks, TPS, 0, plant=plant, device=True, batch=nb, dt_mpc=synthetic.DT_MPC)

    def host_loop():
        reset()
        shift = 0
        for k in range(n_ticks):
            m.set_tick_warm_start(True, shift)
            m.tick_solve_device(d_t.data_ptr(), nb, synthetic.DT_MPC, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)
            torch.cuda.synchronize()
            m.download()
            plant.advance_gait = 1 if (k + 1) % TPS == 0 else 0
            m.plant_step(d_t.data_ptr(), plant, wpd=d_wpd.data_ptr(), summary=d_sum.data_ptr(), device=True, batch=nb)
            torch.cuda.synchronize()
            shift = plant.advance_gait
        plant.advance_gait = 0

    def solves_alone():
        reset()
        m.set_tick_warm_start(True, 0)
        for _ in range(n_ticks):
            m.tick_solve_device(d_t.data_ptr(), nb, synthetic.DT_MPC, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)

    print(f"--- {gait}, {nb} instances, {n_ticks} ticks (reset of the ticks and of the warm start inside every window)")
    for name, fn in (("a) hmpc_rollout_device", rollout), ("b) host-driven loop", host_loop), ("c) hmpc_tick_solve_device alone", solves_alone)):
        med, lo, hi = median_of(fn)
        print(f"{name:34s} {1e3 * med:8.3f} ms per {n_ticks} ticks (min {1e3 * lo:.3f}, max {1e3 * hi:.3f})  = {nb * n_ticks / med / 1e6:7.3f} M ticks/s")
    # (the rollout's log stays on the device: nothing is downloaded in the timed windows)

    # d) one launch each, HIP events
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

    reset()
    m.tick_solve_device(d_t.data_ptr(), nb, synthetic.DT_MPC, d_tau.data_ptr(), 0, d_wpd.data_ptr(), 0)
    torch.cuda.synchronize()
    plant.dt_tick = 0.0  # (the same arithmetic on a state that does not run away over thousands of launches)
    t_plant = events(lambda: m.plant_step(d_t.data_ptr(), plant, wpd=d_wpd.data_ptr(), summary=d_sum.data_ptr(), device=True, batch=nb))
    t_build = events(lambda: interface._check(m.L.hmpc_build_records_device(m.h, C.c_void_p(d_t.data_ptr()), nb, synthetic.DT_MPC, C.c_void_p(d_wpd.data_ptr()),
                                                                             None), "hmpc_build_records_device"))
    print(f"d) plant_step_kernel {1e3 * t_plant:7.2f} us per launch, build_records_kernel {1e3 * t_build:7.2f} us per launch (ratio {t_plant / t_build:.2f})")
    m.close()
