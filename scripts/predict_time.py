#!/usr/bin/env python3
"""Kernel time of hmpc_predict_states next to hmpc_time_solve of the same batch, in the same run (HIP events; warmed up, median of
five windows of `reps` launches each).  Default: 8192 standing instances at h = 10 (profiles/r09/predict.txt).

    python scripts/predict_time.py [batch] [gait] [horizon] [contacts]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import interface, records, synthetic  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
gait = sys.argv[2] if len(sys.argv) > 2 else "standing"
h = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nc = int(sys.argv[4]) if len(sys.argv) > 4 else 2
REPS, WINDOWS = 20, 5

f = synthetic.make_batch3(nb, h, gait, seed=5) if nc == 3 else synthetic.make_batch(nb, h, gait, seed=2, phase="random")
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
m.upload(records.pack_records(f, h, nc))
m.solve()
_, st = m.download()
for _ in range(3):  # warm-up: allocates the prediction buffers, loads the code object
    m.predict_states()
m.download_prediction()
solve_ms, predict_ms = [], []
for _ in range(WINDOWS):
    solve_ms.append(m.time_solve(REPS))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        m.predict_states()
    e1.record()
    e1.synchronize()
    predict_ms.append(e0.elapsed_time(e1) / REPS)
states, cost = m.download_prediction()
m.close()
s, p = statistics.median(solve_ms), statistics.median(predict_ms)
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} launches")
print(f"hmpc_time_solve      {s:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in solve_ms)})")
print(f"hmpc_predict_states  {p:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in predict_ms)})")
print(f"prediction / solve   {100 * p / s:6.2f} %       bytes out per instance {13 * h * 4 + 16}, in {int(m.stride) + 24 * nc * h}")
print(f"mean predicted tracking cost {cost[:, 0].mean():.4f}, force cost {cost[:, 1].mean():.4f}")
