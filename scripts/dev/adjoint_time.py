#!/usr/bin/env python3
"""Kernel time of hmpc_solve_adjoint next to hmpc_feedback_gains (the kernel it shares the matrix recursion with), hmpc_kkt_certificate and
hmpc_time_solve of the same batch, behind the same solve, in the same run (HIP events on the null stream; warmed up, median of five
windows of `reps` launches each).  Default: 8192 standing instances at h = 10 (profiles/r20/adjoint.txt).

    python scripts/dev/adjoint_time.py [batch] [gait] [horizon] [contacts]"""
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
seed = np.random.default_rng(5).uniform(-1.0, 1.0, (nb, h, 6 * nc))
d_seed = torch.from_numpy(seed / np.abs(seed).sum(axis=(1, 2), keepdims=True)).cuda()
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
m.upload(rec)
m.solve()
_, st = m.download()
for _ in range(3):  # warm-up: allocates the certificate, gain and adjoint buffers, loads the code objects
    m.kkt_certificate()
    m.feedback_gains()
    m.solve_adjoint(d_seed.data_ptr())
m.download_adjoint()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


t = dict(solve=[], certificate=[], gains=[], adjoint=[])
for _ in range(WINDOWS):
    t["solve"].append(m.time_solve(REPS))
    t["certificate"].append(events(m.kkt_certificate))
    t["gains"].append(events(m.feedback_gains))
    t["adjoint"].append(events(lambda: m.solve_adjoint(d_seed.data_ptr())))
a = m.download_adjoint()
m.close()
med = {k: statistics.median(v) for k, v in t.items()}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} launches")
for name, key in (("hmpc_time_solve", "solve"), ("hmpc_kkt_certificate", "certificate"), ("hmpc_feedback_gains", "gains"), ("hmpc_solve_adjoint", "adjoint")):
    print(f"{name:26s} {med[key]:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in t[key])})")
out_bytes = (13 + 12 * h + 12 + 6 * nc + 6 * nc * h + 2) * 8
print(f"adjoint / gains {med['adjoint'] / med['gains']:6.2f} x, / solve {100 * med['adjoint'] / med['solve']:6.2f} %;  bytes out per instance "
      f"{out_bytes} ({out_bytes * nb / 1e6:.1f} MB per launch), in {int(m.stride) + 4 * 6 * nc * h + 8 * 6 * nc * h}")
print(f"max |dir| over the batch {a['summary'][:, 1].max():.3g};  smallest pivot ratio {a['summary'][:, 0].min():.3g};  "
      f"max |grad_x0| {np.abs(a['grad_x0']).max():.3g}")
