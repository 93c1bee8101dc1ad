#!/usr/bin/env python3
"""Kernel time of hmpc_kkt_certificate next to hmpc_predict_states, hmpc_constraint_margins and hmpc_time_solve of the same batch, in the
same run (HIP events on the null stream; warmed up, median of five windows of `reps` launches each), and of hmpc_certificate_penalty.
Default: 8192 standing instances at h = 10 (profiles/r18/certificate.txt).

    python scripts/certificate_time.py [batch] [gait] [horizon] [contacts]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
m.upload(records.pack_records(f, h, nc))
m.solve()
_, st = m.download()
d_pen = torch.zeros(nb, dtype=torch.float64, device="cuda")
ceil = [1e-2, float("nan"), 1e-5]
for _ in range(3):  # warm-up: allocates the prediction, margin and certificate buffers, loads the code objects
    m.predict_states()
    m.constraint_margins()
    m.kkt_certificate()
    m.certificate_penalty(ceil, d_pen.data_ptr())
m.download_certificate()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


t = dict(solve=[], predict=[], margins=[], certificate=[], penalty=[])
for _ in range(WINDOWS):
    t["solve"].append(m.time_solve(REPS))
    t["predict"].append(events(m.predict_states))
    t["margins"].append(events(m.constraint_margins))
    t["certificate"].append(events(m.kkt_certificate))
    t["penalty"].append(events(lambda: m.certificate_penalty(ceil, d_pen.data_ptr())))
cert = m.download_certificate()
torch.cuda.synchronize()
masked = int(np.isinf(d_pen.cpu().numpy()).sum())
m.close()
med = {k: statistics.median(v) for k, v in t.items()}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} launches")
for name, key in (("hmpc_time_solve", "solve"), ("hmpc_predict_states", "predict"), ("hmpc_constraint_margins", "margins"),
                  ("hmpc_kkt_certificate", "certificate"), ("hmpc_certificate_penalty", "penalty")):
    print(f"{name:26s} {med[key]:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in t[key])})")
out_bytes = 22 * nc * h * 8 + 4 * 8 + 2 * 4
print(f"certificate / prediction {100 * med['certificate'] / med['predict']:6.2f} %, / margins {100 * med['certificate'] / med['margins']:6.2f} %, "
      f"/ solve {100 * med['certificate'] / med['solve']:6.2f} %;  bytes out per instance {out_bytes} ({out_bytes * nb / 1e6:.1f} MB per launch), "
      f"in {int(m.stride) + 24 * nc * h}")
s = cert["summary"]
print(f"summary maxima over the batch: {' '.join('%.4g' % v for v in s.max(axis=0))};  multipliers > 0: {int((cert['lambda'] > 0).sum())} of "
      f"{cert['lambda'].size};  above the ceiling {ceil}: {masked} instances")
