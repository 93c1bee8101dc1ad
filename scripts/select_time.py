#!/usr/bin/env python3
"""Time of hmpc_sweep_select next to the prediction and the sweep solve it follows, the host route it replaces, and the whole
hmpc_tick_sweep_device, in the same run (HIP events on the null stream; warmed up, median of five windows of `reps` launches each; the
host route by the wall clock, it ends on the host).  Default: 128 states x 64 commands at h = 10 (profiles/r11/select.txt, DESIGN.md
section 4.12).

    python scripts/select_time.py [states] [commands] [gait]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import interface, synthetic  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 128
K = int(sys.argv[2]) if len(sys.argv) > 2 else 64
gait = sys.argv[3] if len(sys.argv) > 3 else "standing"
H, REPS, WINDOWS = 10, 20, 5
B = G * K

rng = np.random.default_rng(11)
ticks = synthetic.make_ticks(G, H, gait, seed=11)
cmd = np.zeros((G, K), dtype=interface.COMMAND_DTYPE)
cmd["v_des_robot"] = rng.uniform(-0.5, 0.5, (G, K, 2))
cmd["yaw_rate_des"] = rng.uniform(-0.3, 0.3, (G, K))
cmd["roll_des"], cmd["pitch_des"] = rng.uniform(-0.02, 0.02, (G, K)), rng.uniform(-0.02, 0.02, (G, K))
d_t = torch.from_numpy(ticks.view(np.uint8).reshape(G, -1).copy()).cuda()
d_c = torch.from_numpy(cmd.view(np.uint8).reshape(B, -1).copy()).cuda()
d_p = torch.from_numpy(rng.uniform(0.0, 5.0, B)).cuda()
d_tau = torch.zeros((G, 10), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
m = interface.BatchedMPC(synthetic.DT_MPC, H, synthetic.F_MAX, B)


def whole():
    m.tick_sweep_device(d_t.data_ptr(), G, d_c.data_ptr(), K, synthetic.DT_MPC, d_tau.data_ptr(), penalty_ptr=d_p.data_ptr())


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


def host_route():
    """what the selection replaces: every cost to the host, argmin per group there, the winners' force rows gathered from the device"""
    _, cost = m.download_prediction()
    s = (cost[:, 0] + cost[:, 1] + pen_host).reshape(G, K)
    win = np.arange(G) * K + s.argmin(axis=1)
    return d_forces[torch.from_numpy(win).cuda()].cpu().numpy()


for _ in range(3):  # warm-up: builds the batch, allocates the prediction and selection buffers, loads the code objects
    whole()
_, st = m.download()
m.predict_states()
m.sweep_select(K, d_p.data_ptr())
sel = m.download_selection()
pen_host = d_p.cpu().numpy()
d_forces = torch.zeros((B, 12 * H), dtype=torch.float32, device="cuda")  # (a torch view of the force buffer for the host route's gather)
m.set_device_outputs(d_forces.data_ptr(), 0, keepalive=d_forces)
m.solve_command_sweep(K)
m.predict_states()
host_route()
t = dict(select=[], predict=[], sweep=[], whole=[], host=[])
for _ in range(WINDOWS):
    t["sweep"].append(events(lambda: m.solve_command_sweep(K)))
    t["predict"].append(events(m.predict_states))
    t["select"].append(events(lambda: m.sweep_select(K, d_p.data_ptr())))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        host_route()
    t["host"].append(1e3 * (time.perf_counter() - t0) / REPS)
m.set_device_outputs(0, 0)
for _ in range(WINDOWS):
    t["whole"].append(events(whole))
again = m.download_selection()
m.close()
med = {k: statistics.median(v) for k, v in t.items()}
print(f"{G} {gait} states x {K} commands = {B} instances, h = {H}; {int((interface.status_code(st) != 0).sum())} not ok; "
      f"median of {WINDOWS} windows of {REPS} launches")
for name, key in (("hmpc_sweep_select", "select"), ("hmpc_predict_states", "predict"), ("hmpc_solve_command_sweep", "sweep"),
                  ("host route (download_prediction + numpy argmin + row gather)", "host"), ("hmpc_tick_sweep_device (whole)", "whole")):
    print(f"{name:62s} {med[key]:8.4f} ms   (windows: {' '.join('%.4f' % v for v in t[key])})")
print(f"selection / prediction {100 * med['select'] / med['predict']:6.2f} %, / sweep solve {100 * med['select'] / med['sweep']:6.2f} %, "
      f"host route / selection {med['host'] / med['select']:6.1f} x")
print(f"bytes per selection: in {28 * B} (cost, status, penalty) + {G * (12 * H + 13 * H) * 4} (winner rows), out {G * ((12 * H + 13 * H) * 4 + 16)}")
print(f"winners: {np.bincount(sel['index'][sel['index'] >= 0], minlength=K).tolist()} per position, {int((sel['index'] < 0).sum())} groups without one; "
      f"same winners from the whole call: {bool((again['index'] == sel['index']).all())}")
