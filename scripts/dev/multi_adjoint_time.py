#!/usr/bin/env python3
"""Kernel time of hmpc_solve_adjoint_multi under S seeds next to a loop of S hmpc_solve_adjoint launches and hmpc_time_solve of the same
batch, behind the same solve, in the same run (HIP events on the null stream; warmed up, median of five windows of `reps` launches
each).  Default: 8192 standing instances at h = 10, S = 1, 2, 6, 12, 13 (profiles/r24/multi_adjoint.txt).  On a
library without hmpc_solve_adjoint_multi (the parent commit's) the loops alone are timed.

    python scripts/dev/multi_adjoint_time.py [batch] [gait] [horizon] [contacts] [S,S,...]"""
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
counts = [int(s) for s in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1, 2, 6, 12, 13]
REPS, WINDOWS = 20, 5
U = 6 * nc

f = synthetic.make_batch3(nb, h, gait, seed=5) if nc == 3 else synthetic.make_batch(nb, h, gait, seed=2, phase="random")
rec = records.pack_records(f, h, nc)
smax = max(counts)
seeds = np.random.default_rng(5).uniform(-1.0, 1.0, (smax, nb, h, U))
d_seeds = torch.from_numpy(seeds / np.abs(seeds).sum(axis=(2, 3), keepdims=True)).cuda()
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
has_multi = hasattr(m, "solve_adjoint_multi")
m.upload(rec)
m.solve()
_, st = m.download()
for _ in range(3):  # warm-up: allocates the buffers, loads the code objects
    m.solve_adjoint(d_seeds[0].data_ptr())
    if has_multi:
        m.solve_adjoint_multi(d_seeds.data_ptr(), smax)
m.download_adjoint()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


def loop(S):
    for s in range(S):
        m.solve_adjoint(d_seeds[s].data_ptr())


t = {"solve": []}
for S in counts:
    t[("loop", S)], t[("multi", S)] = [], []
for _ in range(WINDOWS):
    t["solve"].append(m.time_solve(REPS))
    for S in counts:
        t[("loop", S)].append(events(lambda: loop(S)))
        if has_multi:
            t[("multi", S)].append(events(lambda: m.solve_adjoint_multi(d_seeds.data_ptr(), S)))
same = None
if has_multi:  # the last slice against the single-seed launch, bit for bit
    m.solve_adjoint_multi(d_seeds.data_ptr(), smax)
    mm = m.download_adjoint_multi()
    m.solve_adjoint(d_seeds[smax - 1].data_ptr())
    a = m.download_adjoint()
    same = all((mm[k][smax - 1].view(np.uint64) == a[k].view(np.uint64)).all() for k in m.ADJOINT_KEYS)
m.close()
med = {k: statistics.median(v) for k, v in t.items() if v}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} "
      f"launches; library {'with' if has_multi else 'WITHOUT'} hmpc_solve_adjoint_multi")
print(f"{'hmpc_time_solve':34s} {med['solve']:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in t['solve'])})")
for S in counts:
    lo = t[("loop", S)]
    print(f"{'loop of %2d hmpc_solve_adjoint' % S:34s} {med[('loop', S)]:8.4f} ms   (windows: {' '.join('%.4f' % v for v in lo)}; spread "
          f"{max(lo) - min(lo):.4f})")
    if has_multi:
        mu = t[("multi", S)]
        print(f"{'hmpc_solve_adjoint_multi, S = %2d' % S:34s} {med[('multi', S)]:8.4f} ms   (windows: {' '.join('%.4f' % v for v in mu)}; spread "
              f"{max(mu) - min(mu):.4f});  loop / multi {med[('loop', S)] / med[('multi', S)]:5.2f} x, per seed {med[('multi', S)] / S:.4f} ms")
if has_multi:
    print(f"slice {smax - 1} of the multi-seed launch is the single-seed launch bit for bit: {same}")
