#!/usr/bin/env python3
"""Kernel time of hmpc_feedback_gains and hmpc_first_order_wrench next to hmpc_kkt_certificate (the yardstick) and hmpc_time_solve of the
same batch, behind the same solve, in the same run (HIP events on the null stream; warmed up, median of five windows of `reps` launches
each).  Default: 8192 standing instances at h = 10 (profiles/r19/feedback.txt).

    python scripts/dev/feedback_time.py [batch] [gait] [horizon] [contacts]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import interface, records, synthetic  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
gait = sys.argv[2] if len(sys.argv) > 2 else "standing"
h = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nc = int(sys.argv[4]) if len(sys.argv) > 4 else 2
REPS, WINDOWS = 20, 5

f = synthetic.make_batch3(nb, h, gait, seed=5) if nc == 3 else synthetic.make_batch(nb, h, gait, seed=2, phase="random")
rec = records.pack_records(f, h, nc)
d_rec = torch.from_numpy(rec).cuda()
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
m.upload(rec)
m.solve()
_, st = m.download()
for _ in range(3):  # warm-up: allocates the certificate, gain and wrench buffers, loads the code objects
    m.kkt_certificate()
    m.feedback_gains()
    m.first_order_wrench(d_rec.data_ptr())
m.download_gains()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


t = dict(solve=[], certificate=[], gains=[], first_order=[])
for _ in range(WINDOWS):
    t["solve"].append(m.time_solve(REPS))
    t["certificate"].append(events(m.kkt_certificate))
    t["gains"].append(events(m.feedback_gains))
    t["first_order"].append(events(lambda: m.first_order_wrench(d_rec.data_ptr())))
g = m.download_gains()
m.close()
med = {k: statistics.median(v) for k, v in t.items()}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} launches")
for name, key in (("hmpc_time_solve", "solve"), ("hmpc_kkt_certificate", "certificate"), ("hmpc_feedback_gains", "gains"),
                  ("hmpc_first_order_wrench", "first_order")):
    print(f"{name:26s} {med[key]:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in t[key])})")
out_bytes = 6 * nc * (13 + 12 * h) * 8 + 2 * 8 + 4 * h
print(f"gains / certificate {med['gains'] / med['certificate']:6.2f} x, / solve {100 * med['gains'] / med['solve']:6.2f} %;  bytes out per instance "
      f"{out_bytes} ({out_bytes * nb / 1e6:.1f} MB per launch), in {int(m.stride) + 24 * nc * h}")
print(f"free directions per step: mean {g['free_dims'].mean():.2f} of {6 * nc}, largest {int(g['free_dims'].max())};  max |K_0| over the batch "
      f"{g['summary'][:, 1].max():.1f};  smallest pivot ratio {g['summary'][:, 0].min():.3g}")
