#!/usr/bin/env python3
"""Kernel time of hmpc_adjoint_record next to the three launches it follows -- hmpc_solve_adjoint, hmpc_adjoint_model, hmpc_adjoint_limits --,
hmpc_kkt_certificate (the yardstick for a kernel of this build) and hmpc_time_solve of the same batch, behind the same solve and the same
adjoints, in the same run (HIP events on the null stream; warmed up, median of five windows of `reps` launches each).  Default: 8192
standing instances at h = 10 (profiles/r23/pose_adjoint.txt).

    python scripts/dev/pose_adjoint_time.py [batch] [gait] [horizon] [contacts] [f_max]"""
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
f_max = float(sys.argv[5]) if len(sys.argv) > 5 else synthetic.F_MAX
REPS, WINDOWS = 20, 5

f = synthetic.make_batch3(nb, h, gait, seed=5) if nc == 3 else synthetic.make_batch(nb, h, gait, seed=2, phase="random")
rec = records.pack_records(f, h, nc)
seed = np.random.default_rng(5).uniform(-1.0, 1.0, (nb, h, 6 * nc))
d_seed = torch.from_numpy(seed / np.abs(seed).sum(axis=(1, 2), keepdims=True)).cuda()
m = interface.BatchedMPC(synthetic.DT_MPC, h, f_max, nb, contacts=nc)
m.upload(rec)
m.solve()
_, st = m.download()
for _ in range(3):  # warm-up: allocates the certificate, adjoint, model-, limit- and record-gradient buffers, loads the code objects
    m.kkt_certificate()
    m.solve_adjoint(d_seed.data_ptr())
    m.adjoint_model()
    m.adjoint_limits(d_seed.data_ptr())
    m.adjoint_record()
m.download_adjoint_record()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch's current stream is the null stream the launches below go to)
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


t = dict(solve=[], certificate=[], adjoint=[], model=[], limits=[], record=[])
for _ in range(WINDOWS):
    t["solve"].append(m.time_solve(REPS))
    t["certificate"].append(events(m.kkt_certificate))
    t["adjoint"].append(events(lambda: m.solve_adjoint(d_seed.data_ptr())))
    t["model"].append(events(m.adjoint_model))  # (behind the window's last adjoint)
    t["limits"].append(events(lambda: m.adjoint_limits(d_seed.data_ptr())))  # (likewise)
    t["record"].append(events(m.adjoint_record))  # (behind the window's last adjoint, model and limit gradients)
g = m.download_adjoint_record()
m.close()
med = {k: statistics.median(v) for k, v in t.items()}
print(f"{nb} {gait} instances, h = {h}, {nc} contacts, f_max = {f_max:g}; {int((interface.status_code(st) != 0).sum())} not ok; median of {WINDOWS} "
      f"windows of {REPS} launches")
for name, key in (("hmpc_time_solve", "solve"), ("hmpc_kkt_certificate", "certificate"), ("hmpc_solve_adjoint", "adjoint"), ("hmpc_adjoint_model", "model"),
                  ("hmpc_adjoint_limits", "limits"), ("hmpc_adjoint_record", "record")):
    print(f"{name:26s} {med[key]:8.4f} ms per launch   (windows: {' '.join('%.4f' % v for v in t[key])})")
nf = records.N_FIXED3 if nc == 3 else records.N_FIXED
out_bytes = (nf + 12 * h + 9 * (1 + nc) + 3) * 8
in_bytes = int(m.stride) + (13 + 12 * h + 12 + 6 * nc + 9 + 18 * nc + 3 * nc + 1 + 48 * nc * nc) * 8
print(f"record / model {med['record'] / med['model']:6.2f} x, / limits {med['record'] / med['limits']:6.2f} x, / certificate {med['record'] / med['certificate']:6.2f} x, "
      f"/ adjoint {med['record'] / med['adjoint']:6.2f} x, / solve {100 * med['record'] / med['solve']:6.2f} %;  bytes out per instance {out_bytes} "
      f"({out_bytes * nb / 1e6:.1f} MB per launch), read {in_bytes}")
q, ja = g["grad_record"][:, 6:10], g["grad_record"][:, (22 if nc == 3 else 19):(32 if nc == 3 else 29)]
print(f"max |grad q| {np.abs(q).max():.3g}, max |grad joint angles| {np.abs(ja).max():.3g}, max |grad_rpy| {' '.join('%.3g' % v for v in np.abs(g['grad_rpy']).max(axis=0))}; "
      f"instances with a non-zero joint-angle gradient {int((np.abs(ja).max(axis=1) > 0).sum())}")
