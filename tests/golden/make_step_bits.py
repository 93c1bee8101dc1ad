#!/usr/bin/env python3
"""Generates tests/golden/step_bits.npz: forces and status words of solves whose number of block-pivot steps ends at every
position of a tile row, as the commit named in the file computed them, for tests/test_gpu_step_bits.py.

What it is for: the block-pivot steps of the matrix-core sweeps (mfs_steps: stage S on the 8 x 8 grid, the block start's Schur
inversion on 3 x 3 ... 6 x 6 grids) run ceil(n / 4) steps, four to a tile row, and which step of its row a step is decides which
accumulator register holds the pivot rows, which quarter of a tile's columns is published, which panel buffer is written and
whether the next publish belongs to the next tile row.  A change that fixes any of this at compile time, and leaves every
arithmetic instruction on data alone, must reproduce these outputs bit for bit wherever the steps end.  The file holds this
project's OWN outputs and is regenerated, on the GPU with the build of the commit one wants to pin, whenever a change alters the
arithmetic on purpose:

    python tests/golden/make_step_bits.py [--out FILE]       (from the repository root; HEAD's hash goes into the file, or
                                                              HMPC_GOLDEN_COMMIT where there is no .git; the library's sha256 too)

Cases (shared with the test):

  stage S     irregular gait tables (tests/irregular_gaits.py) with ng = 8, 11, 12, 10, 19, 20 stance leg-steps, four instances each:
              n = 6 ng variables, ceil(6 ng / 4) = 12, 17, 18, 15, 29, 30 steps, the last one at place 3, 0, 1, 2, 0, 1 of its tile row.
              The 20-leg-step instances make the host pick the 120-variable variant for the whole batch.
                h10_c2     h = 10: the FAST variant of the shape
                h20_c2     h = 20: the same spread on the h = 20 variant
                sweep_h10  h = 10 as a command sweep, two commands per state: the SWEEP variant
              Each batch is followed by a SECOND solve on the same handle (other states, the tables in reverse order).
  schur_k0    the block start's first round pinned at k0 = 9, 10, 12, 21, 24, 41, 44 rows (four instances each) on the FAST
              120-variable variant (3 x 3 tiles): ceil(k0 / 4) = 3, 3, 3, 6, 6, 11, 11 steps, all of which end inside a tile row.
              Built and verified on the host by the helpers of make_schur_bits.py (a separable QP through hmpc_debug_solve_external_qp);
              main() asserts on the status words that the round took exactly k0 rows and nothing followed it.
tests/test_gpu_step_bits.py shows on the CPU that qpOASES solves every stage-S instance."""
import hashlib
import importlib.util
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

_spec = importlib.util.spec_from_file_location("make_schur_bits_for_steps", os.path.join(ROOT, "tests", "golden", "make_schur_bits.py"))
sb = importlib.util.module_from_spec(_spec)  # (a copy of its own: K0_TARGETS below replaces that module's list in this copy only)
_spec.loader.exec_module(sb)

PATH = os.path.join(ROOT, "tests", "golden", "step_bits.npz")
DT, FMAX = synthetic.DT_MPC, synthetic.F_MAX
PER_NG = 4
NGS = (8, 11, 12, 10, 19, 20)
LAST_RR = (3, 0, 1, 2, 0, 1)  # place of the last step in its tile row
SHAPES = [("h10_c2", 10, 2, 271, 0), ("h20_c2", 20, 2, 272, 0), ("sweep_h10", 10, 2, 273, 2)]  # (name, h, nc, seed, commands per state)
NAMES = [s[0] for s in SHAPES]
K0_TARGETS = [9, 10, 12, 21, 24, 41, 44] * 4
K0_SEED = 274
SCHUR_BITS_K0 = list(sb.K0_TARGETS)  # what tests/test_gpu_schur_bits.py pins already: 1, 15-17, 31-33, 47, 48, 52, 54


def pack(fields: dict, h: int, nc: int) -> np.ndarray:
    return records.pack_records(fields, h, nc)


def _sweep(h, nc, tables, seed, k):
    b = ig.Batch("steps", h, nc, [(f"t{i}", t) for i, t in enumerate(tables)], seed)
    return ig.sweep_batch(b, k).fields


def cases() -> list:
    """(name, horizon, contacts, commands per state or 0, field dict of the first solve, field dict of the second solve)"""
    out = []
    for name, h, nc, seed, k in SHAPES:
        rng = np.random.default_rng(seed)
        tables = np.stack([ig.exact_count(h, nc, g, rng) for g in NGS for _ in range(PER_NG)])
        if k:
            out.append((name, h, nc, k, _sweep(h, nc, tables, seed, k), _sweep(h, nc, tables[::-1], seed + 50, k)))
        else:
            out.append((name, h, nc, k, ig.fields(h, nc, tables, seed), ig.fields(h, nc, tables[::-1], seed + 50)))
    return out


def check_cases(cs: list) -> None:
    """What the shapes are chosen for really occurs in them."""
    assert [(-(-6 * g // 4) - 1) % 4 for g in NGS] == list(LAST_RR) and set(LAST_RR) == {0, 1, 2, 3}
    for name, h, nc, k, first, second in cs:
        reps = max(k, 1)
        want = [g for g in NGS for _ in range(PER_NG * reps)]
        got = ig.stance_count(first["gait"])
        assert got.tolist() == want and ig.stance_count(second["gait"]).tolist() == want[::-1], name
        assert got.max() == 20  # the 120-variable variant runs the batch
        t = np.asarray(first["gait"]).reshape(len(got), h * nc)
        for g in NGS:  # irregular: the tables of one ng are not all the same
            assert g == nc * h or len({tuple(r) for r in t[got == g]}) > 1, (name, g)


def solve_case(h: int, nc: int, k: int, first: dict, second: dict):
    """[(forces float32 [b, 6 nc h], status words [b])] of the two solves on one handle, as the library built in this tree gives them"""
    from hector_simulation_amd import interface

    m = interface.BatchedMPC(DT, h, FMAX, len(first["gait"]), contacts=nc)
    out = []
    for f in (first, second):
        m.upload(pack(f, h, nc))
        if k:
            m.solve_command_sweep(k)
        else:
            m.solve()
        forces, status = m.download()
        out.append((np.array(forces, copy=True), np.array(status, copy=True)))
    m.close()
    return out


def k0_instances():
    """(H, g, Fc, k0) of the schur_k0 case: make_schur_bits.k0_instances with this file's targets"""
    sb.K0_TARGETS = list(K0_TARGETS)
    return sb.k0_instances(K0_SEED)


def k0_inputs_from(golden):
    """(H, g, Fc, k0) of the schur_k0 case as the golden file keeps them"""
    hd = golden["schur_k0_hdiag"]
    hx = np.zeros((hd.shape[0], 120, 120), np.float32)
    hx[:, np.arange(120), np.arange(120)] = hd
    return hx, golden["schur_k0_g"], golden["schur_k0_fc"], golden["schur_k0_k0"]


def main():
    import torch  # (first: one HIP runtime per process, tests/conftest.py)

    torch.zeros(1, device="cuda")
    from hector_simulation_amd import _lib, interface

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else PATH
    commit = os.environ.get("HMPC_GOLDEN_COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    cs = cases()
    check_cases(cs)
    hx, gx, fx, k0 = k0_instances()
    host = np.array([sb.verify_instance(hx[i], gx[i], fx[i]) for i in range(len(k0))])
    assert (host == k0).all(), (host, k0)
    out = {"commit": np.array(commit)}
    for name, h, nc, k, first, second in cs:
        for tag, (forces, status) in zip(("a", "b"), solve_case(h, nc, k, first, second)):
            code = interface.status_code(status)
            out[f"{name}_{tag}_forces"] = forces.view(np.uint32)
            out[f"{name}_{tag}_status"] = status
            print(f"{name}_{tag} b {forces.shape[0]:3d} codes {dict(zip(*np.unique(code, return_counts=True)))} "
                  f"iterations {interface.status_iters(status).min()}..{interface.status_iters(status).max()} "
                  f"|W| {interface.status_nactive(status).min()}..{interface.status_nactive(status).max()}")
            assert (code == 0).all(), (name, tag, code)  # nominal inputs that qpOASES solves: nothing ends flagged
    forces, status = sb.solve_k0_edges(hx, gx, fx)
    code, it, nact = interface.status_code(status), interface.status_iters(status), interface.status_nactive(status)
    for t in sorted(set(k0.tolist())):
        sel = k0 == t
        print(f"schur_k0     target {t:2d}: codes {code[sel].tolist()} iterations {it[sel].tolist()} |W| {nact[sel].tolist()}")
    out["schur_k0_forces"], out["schur_k0_status"], out["schur_k0_k0"] = forces.view(np.uint32), status, k0
    out["schur_k0_hdiag"], out["schur_k0_g"], out["schur_k0_fc"] = np.ascontiguousarray(np.diagonal(hx, axis1=1, axis2=2)), gx, fx
    with open(_lib.lib_path(), "rb") as f:
        out["library_sha256"] = np.array(hashlib.sha256(f.read()).hexdigest())
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes, commit", commit, "library", out["library_sha256"])
    # (after the file is written, so that a failed statement leaves the evidence behind)
    assert ((code == 0) & (nact == k0) & (it == 0)).all(), ("first-round row count not confirmed by the status words", code, it, nact, k0)


if __name__ == "__main__":
    main()
