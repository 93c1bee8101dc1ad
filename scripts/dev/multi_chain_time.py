#!/usr/bin/env python3
"""Kernel time of hmpc_adjoint_chain_multi under S seeds next to the loop of S x (hmpc_select_adjoint_seed, hmpc_adjoint_model,
hmpc_adjoint_limits, hmpc_adjoint_record), behind one solve and one multi-seed adjoint of the same batch, in the same run (HIP events on
the null stream; warmed up, median of five windows of `reps` launches each), and ``autograd.wrench_jacobian`` end to end.  Default: 8192
standing instances at h = 10, S = 1, 2, 6, U, U + 1 (profiles/r25/multi_chain.txt).  On a library without
hmpc_adjoint_chain_multi (the parent commit's) the loop and the Jacobian alone are timed: run both trees in turn for the comparison.

    python scripts/dev/multi_chain_time.py [batch] [gait] [horizon] [contacts] [S,S,...]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (brings the HIP runtime up first, see tests/conftest.py)

torch.zeros(1, device="cuda")
from hector_simulation_amd import autograd, interface, records, synthetic  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
gait = sys.argv[2] if len(sys.argv) > 2 else "standing"
h = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nc = int(sys.argv[4]) if len(sys.argv) > 4 else 2
U = 6 * nc
counts = [int(s) for s in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1, 2, 6, U, U + 1]
REPS, WINDOWS = 20, 5

f = synthetic.make_batch3(nb, h, gait, seed=5) if nc == 3 else synthetic.make_batch(nb, h, gait, seed=2, phase="random")
rec = records.pack_records(f, h, nc)
smax = max(counts)
seeds = np.random.default_rng(5).uniform(-1.0, 1.0, (smax, nb, h, U))
d_seeds = torch.from_numpy(seeds / np.abs(seeds).sum(axis=(2, 3), keepdims=True)).cuda()
m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, nb, contacts=nc)
has_chain = hasattr(m, "adjoint_chain_multi")
m.upload(rec)
m.solve()
_, st = m.download()


def loop(S):
    for s in range(S):
        m.select_adjoint_seed(s)
        m.adjoint_model()
        m.adjoint_limits(d_seeds[s].data_ptr())
        m.adjoint_record()


m.solve_adjoint_multi(d_seeds.data_ptr(), smax)
for _ in range(3):  # warm-up: allocates the buffers, loads the code objects
    loop(2)
    if has_chain:
        m.adjoint_chain_multi(d_seeds.data_ptr())
m.download_adjoint_record()


def events(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


t = {}
for S in counts:
    t[("loop", S)], t[("chain", S)] = [], []
for _ in range(WINDOWS):
    for S in counts:
        m.solve_adjoint_multi(d_seeds.data_ptr(), S)
        t[("loop", S)].append(events(lambda: loop(S)))
        if has_chain:
            t[("chain", S)].append(events(lambda: m.adjoint_chain_multi(d_seeds.data_ptr())))
same = None
if has_chain:  # the last slice against the three single-seed launches, bit for bit
    m.solve_adjoint_multi(d_seeds.data_ptr(), smax)
    m.adjoint_chain_multi(d_seeds.data_ptr())
    c = m.download_adjoint_chain_multi()
    loop(smax)
    want = dict(grad_record=m.download_adjoint_record()["grad_record"], grad_params=m.download_adjoint_model()["grad_params"],
                grad_limits=m.download_adjoint_limits()["grad_limits"])
    same = all((c[k][smax - 1].view(np.uint64) == want[k].view(np.uint64)).all() for k in want)
autograd.wrench_jacobian(m)  # (warm-up: torch-owned buffers)
jac = [events(lambda: autograd.wrench_jacobian(m)) for _ in range(WINDOWS)]
m.close()
med = {k: statistics.median(v) for k, v in t.items() if v}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} windows of {REPS} "
      f"launches; library {'with' if has_chain else 'WITHOUT'} hmpc_adjoint_chain_multi")
for S in counts:
    lo = t[("loop", S)]
    print(f"{'loop of %2d x (select, model, limits, record)' % S:46s} {med[('loop', S)]:8.4f} ms   (windows: {' '.join('%.4f' % v for v in lo)}; spread "
          f"{max(lo) - min(lo):.4f})")
    if has_chain:
        ch = t[("chain", S)]
        print(f"{'hmpc_adjoint_chain_multi, S = %2d' % S:46s} {med[('chain', S)]:8.4f} ms   (windows: {' '.join('%.4f' % v for v in ch)}; spread "
              f"{max(ch) - min(ch):.4f});  loop / chain {med[('loop', S)] / med[('chain', S)]:5.2f} x, per seed {med[('chain', S)] / S:.4f} ms")
print(f"{'autograd.wrench_jacobian, end to end':46s} {statistics.median(jac):8.4f} ms   (windows: {' '.join('%.4f' % v for v in jac)})")
if has_chain:
    print(f"slice {smax - 1} of the chain launch is the three single-seed launches bit for bit: {same}")
