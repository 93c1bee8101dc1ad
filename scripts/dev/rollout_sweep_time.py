#!/usr/bin/env python3
"""What a closed-loop command sweep costs (profiles/r30/rollout_sweep.txt), in ONE run: 1 024 standing robot states x
8 candidate commands = 8 192 instances, 40 ticks, states from synthetic.make_ticks(seed 90):
  a) one launch of rollout_score_kernel and one of rollout_select_kernel next to one of plant_step_kernel: HIP events, median of five
     windows of 50 launches each, with the spread; the score's achieved bytes/s over the log's 228 B per row (state 96, wrench 48, torques
     80, status 4 -- the status word is not read, so the kernel itself moves 224)
  b) hmpc_rollout_sweep_device against hmpc_rollout_device alone on the same expanded ticks, and against rollout + hmpc_download_rollout +
     scoring and argmin in numpy: host clock around the call and one synchronisation, warmed up, median of five with the spread
Nothing is asserted.

    python scripts/dev/rollout_sweep_time.py [states] [commands] [ticks]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import _lib, interface, synthetic  # noqa: E402

ns = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
K = int(sys.argv[2]) if len(sys.argv) > 2 else 8
n_ticks = int(sys.argv[3]) if len(sys.argv) > 3 else 40
nb = ns * K
H, TPS, WINDOWS = 10, 8, 5
DT = synthetic.DT_MPC


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
    return statistics.median(ms), min(ms), max(ms)


t = synthetic.make_ticks(ns, H, "standing", seed=90)
t["world_position_desired"] = t["position"][:, :2]
t["gait_iteration"] = 0
cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
cmd["v_des_robot"][:, :, 1] = np.linspace(-0.3, 0.4, K)[None, :]
expanded = np.repeat(t, K)
for f in cmd.dtype.names:
    expanded[f] = cmd.reshape(-1)[f]
plant, cost = interface.default_plant(dtMPC=DT), interface.default_rollout_cost()
m = interface.BatchedMPC(DT, H, synthetic.F_MAX, nb)
m.set_tick_warm_start(True, 0)
m.set_auto_resolve(False)
d_states, d_cmd, d_ex, fresh = dev(t), dev(cmd.reshape(-1)), dev(expanded), dev(expanded)
ch, bufs = m._choice_buffers(ns, _lib.ROLLOUT_CHOICE)


def sweep():
    m.reset_tick_warm_start()
    m.rollout_sweep(d_states.data_ptr(), d_cmd.data_ptr(), n_ticks, TPS, 0, plant=plant, cost=cost, device=True, n_states=ns, group_size=K,
                    choice=ch, dt_mpc=DT)


def rollout_alone():
    d_ex.copy_(fresh)
    m.reset_tick_warm_start()
    m.rollout(d_ex.data_ptr(), n_ticks, TPS, 0, plant=plant, device=True, batch=nb, dt_mpc=DT)


w_state = np.array(list(cost.w_state))
ref0 = np.zeros((nb, 1, 12))
ref0[:, 0, 2], ref0[:, 0, 3], ref0[:, 0, 4], ref0[:, 0, 5] = expanded["rpy"][:, 2], expanded["position"][:, 0], expanded["position"][:, 1], cost.height
vdw = np.einsum("bka,bk->ba", expanded["rBody"].reshape(nb, 3, 3)[:, :2, :2], expanded["v_des_robot"])
ref0[:, 0, 9:11] = vdw
tt = ((np.arange(n_ticks) + 1) * cost.dt_tick)[None, :]


def rollout_download_numpy():
    rollout_alone()
    log = m.download_rollout(nb, n_ticks)
    ref = np.repeat(ref0, n_ticks, axis=1)
    ref[:, :, 3] += tt * vdw[:, :1]
    ref[:, :, 4] += tt * vdw[:, 1:]
    e = log["state"] - ref
    e[:, :, 2] -= 2 * np.pi * np.rint(e[:, :, 2] / (2 * np.pi))
    s = (e * e * w_state).sum(axis=(1, 2)) + (log["wrench"].astype(np.float64) ** 2 * np.array(list(cost.w_wrench))).sum(axis=(1, 2))
    s[log["summary"][:, 1] >= 0] = np.inf
    return s.reshape(ns, K).argmin(axis=1)


print(f"--- {ns} states x {K} commands = {nb} instances, {n_ticks} ticks, standing (reset of the warm start inside every window)")
for name, fn in (("hmpc_rollout_sweep_device", sweep), ("hmpc_rollout_device alone", rollout_alone),
                 ("rollout + download + numpy scoring", rollout_download_numpy)):
    med, lo, hi = median_of(fn)
    print(f"b) {name:36s} {1e3 * med:8.3f} ms (min {1e3 * lo:.3f}, max {1e3 * hi:.3f})")
sweep()
torch.cuda.synchronize()
print(f"   winners of the first 8 states: {bufs['index'].cpu().numpy()[:8].tolist()}; numpy's: {rollout_download_numpy()[:8].tolist()}")

# a) one launch each, over the log the last rollout left
d_cost =torch.zeros((nb, 4), dtype=torch.float64, device="cuda")
d_score = torch.zeros((nb,), dtype=torch.float64, device="cuda")
d_sum = torch.zeros((nb, 4), dtype=torch.int32, device="cuda")
d_wpd = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
rollout_alone()
torch.cuda.synchronize()
score_fn = lambda: m.rollout_score(fresh.data_ptr(), None, cost, device=True, batch=nb, n_ticks=n_ticks, cost_ptr=d_cost.data_ptr(), score_ptr=d_score.data_ptr())
select_fn = lambda: m.rollout_select(d_score.data_ptr(), K, 0, None, device=True, batch=nb, choice=ch)
plant.dt_tick = 0.0  # (the same arithmetic on a state that does not run away over hundreds of launches)
plant_fn = lambda: m.plant_step(d_ex.data_ptr(), plant, wpd=d_wpd.data_ptr(), summary=d_sum.data_ptr(), device=True, batch=nb)
for name, fn in (("rollout_score_kernel", score_fn), ("rollout_select_kernel", select_fn), ("plant_step_kernel", plant_fn)):
    med, lo, hi = events(fn)
    extra = ""
    if name == "rollout_score_kernel":
        rows = nb * n_ticks
        extra = f"  = {rows * 228 / (med * 1e-3) / 1e9:.1f} GB/s over 228 B per row ({rows * 224 / (med * 1e-3) / 1e9:.1f} GB/s over the 224 B read)"
    print(f"a) {name:24s} {1e3 * med:7.2f} us per launch (min {1e3 * lo:.2f}, max {1e3 * hi:.2f}){extra}")
m.close()
