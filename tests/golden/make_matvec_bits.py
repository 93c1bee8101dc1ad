#!/usr/bin/env python3
"""Generates tests/golden/matvec_bits.npz: forces and status words of solves whose number of stance leg-steps ng sits at the
borders of the solver's mat-vec path, as the commit named in the file computed them, for tests/test_gpu_matvec_bits.py.

What it is for: gather_w (w = N_W' coef, one lane per variable) and the reduction at the end of the staged mat-vec (variable i sums
the partials of the ng source leg-steps, rows >= ng of the staging are never written) are index work around a fixed sequence of
arithmetic instructions; a change there that keeps every operation on data, its operands and its order reproduces these outputs bit
for bit.  The file holds this project's OWN outputs and is regenerated, on the GPU with the build of the commit one wants to pin,
whenever a change alters the arithmetic on purpose:

    python tests/golden/make_matvec_bits.py                  (from the repository root; HEAD's hash goes into the file)

The cases (cases() below, shared with the test) are the smallest that can go wrong: irregular gait tables (tests/irregular_gaits.py:
ng stance leg-steps at random positions), four instances of each ng, one batch per shape:
  h10_c2   ng = 1, 2, 10, 11, 19, 20 of 20: the 60- and the 120-variable variants; 20 = every leg-step in stance, the unmasked sum
  h10_c3   ng = 1, 14, 15, 16, 29, 30 of 30: three contacts, the partials staged in two halves of 15 source leg-steps
  h20_c2   ng = 1, 10, 11, 19, 20, 21, 39, 40 of 40: the class borders at 60 and 120 variables and the wide variant's halves of 20
Each batch is followed by a SECOND solve on the same handle (other states, the tables in reverse order), so that whatever the first
solve left behind is there when the second one runs.  tests/test_matvec_index.py shows on the CPU that qpOASES solves every instance."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import irregular_gaits as ig  # noqa: E402
from hector_simulation_amd import records, synthetic  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "matvec_bits.npz")
DT, FMAX = synthetic.DT_MPC, synthetic.F_MAX
PER_NG = 4
SHAPES = [("h10_c2", 10, 2, (1, 2, 10, 11, 19, 20), 261),
          ("h10_c3", 10, 3, (1, 14, 15, 16, 29, 30), 262),
          ("h20_c2", 20, 2, (1, 10, 11, 19, 20, 21, 39, 40), 263)]
NAMES = [s[0] for s in SHAPES]


def pack(fields: dict, h: int, nc: int) -> np.ndarray:
    return records.pack_records(fields, h, nc)


def cases() -> list:
    """(name, horizon, contacts, field dict of the first solve, field dict of the second solve)"""
    out = []
    for name, h, nc, ngs, seed in SHAPES:
        rng = np.random.default_rng(seed)
        tables = np.stack([ig.exact_count(h, nc, k, rng) for k in ngs for _ in range(PER_NG)])
        out.append((name, h, nc, ig.fields(h, nc, tables, seed), ig.fields(h, nc, tables[::-1], seed + 50)))
    return out


def check_cases(cs: list) -> None:
    """What the shapes are chosen for really occurs in them."""
    for (name, h, nc, first, second), (_, _, _, ngs, _) in zip(cs, SHAPES):
        k = ig.stance_count(first["gait"])
        assert k.tolist() == [g for g in ngs for _ in range(PER_NG)] and ig.stance_count(second["gait"]).tolist() == k[::-1].tolist(), name
        assert k.max() == nc * h and k.min() == 1, name  # every leg-step in stance (the largest variant runs, nothing is masked), and one
        t = np.asarray(first["gait"]).reshape(len(k), h * nc)
        for g in ngs:  # irregular: the tables of one ng (1 < ng < all) are not all the same
            assert g in (1, nc * h) or len({tuple(r) for r in t[k == g]}) > 1, (name, g)


def solve_case(h: int, nc: int, first: dict, second: dict):
    """[(forces float32 [b, 6 nc h], status words [b])] of the two solves on one handle, as the library built in this tree gives them"""
    from hector_simulation_amd import interface

    m = interface.BatchedMPC(DT, h, FMAX, len(first["gait"]), contacts=nc)
    out = []
    for f in (first, second):
        m.upload(pack(f, h, nc))
        m.solve()
        forces, status = m.download()
        out.append((np.array(forces, copy=True), np.array(status, copy=True)))
    m.close()
    return out


def main():
    import torch  # (first: one HIP runtime per process, tests/conftest.py)

    torch.zeros(1, device="cuda")
    from hector_simulation_amd import interface

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else PATH
    commit = os.environ.get("HMPC_GOLDEN_COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    cs = cases()
    check_cases(cs)
    out = {"commit": np.array(commit)}
    for name, h, nc, first, second in cs:
        for tag, (forces, status) in zip(("a", "b"), solve_case(h, nc, first, second)):
            code = interface.status_code(status)
            out[f"{name}_{tag}_forces"] = forces.view(np.uint32)
            out[f"{name}_{tag}_status"] = status
            print(f"{name}_{tag} b {forces.shape[0]:3d} codes {dict(zip(*np.unique(code, return_counts=True)))} "
                  f"iterations {interface.status_iters(status).min()}..{interface.status_iters(status).max()} "
                  f"|W| {interface.status_nactive(status).min()}..{interface.status_nactive(status).max()}")
            assert (code == 0).all(), (name, tag, code)  # nominal inputs that qpOASES solves: nothing ends flagged
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes, commit", commit)


if __name__ == "__main__":
    main()
