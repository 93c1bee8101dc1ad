#!/usr/bin/env python3
"""Generates tests/golden/fast_path_bits.npz: forces and status words of the first-pass (FAST / SWEEP) variants as the commit
named in the file computed them, for tests/test_gpu_fast_path_bits.py.

What it is for: a change to stage S or to the block start that moves data or index arithmetic and leaves every arithmetic
instruction on data alone must reproduce these outputs bit for bit.  The file holds this project's OWN outputs -- what the
numbers are worth against qpOASES is the rest of the suite's business -- so it is regenerated (on the GPU, with the build of the
commit one wants to pin) whenever a change alters the arithmetic on purpose:

    python tests/golden/make_fast_path_bits.py                  (from the repository root; HEAD's hash goes into the file)

The cases (cases() below, shared with the test) are the smallest at which the loader and hand-back of stage S and the release
loop of the block start can go wrong:
  standing      h = 10, 64 instances: n = 120 is 7.5 tiles of 16 -- a half-padded last tile row and column
  mixed         h = 10, 64 instances, duty factors 5/10 .. 10/10 per leg: reduced sizes n = 66, 72, .. 114 -- rows >= n in several
                tiles, and steps that straddle the border between tiles I and I + 1 (asserted below)
  single_h20    h = 20, 32 instances: the folded-triangle staging of H (hs_index)
  sweep120/60   command sweeps of 8 states x 8 commands: the SWEEP variants, 120 and 60 variables
  walking       h = 10, 32 instances: the 60-variable FAST variant (scalar stage S: the block start only)
  standing_3x   64 instances at 3x the input ranges: more flips and releases per round, some hand-overs"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hector_simulation_amd import records, synthetic  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "fast_path_bits.npz")
# (stance steps of leg 0, of leg 1) out of 10: n = 6 * their sum
MIXED_DUTY = [(6, 5), (6, 6), (7, 6), (7, 7), (8, 7), (8, 8), (9, 8), (9, 9), (10, 9)]


def mixed_fields(batch: int, h: int, seed: int) -> dict:
    """synthetic.make_batch's mixed gait with the duty factor varied from instance to instance (and a random phase)."""
    f = synthetic.make_batch(batch, h, "mixed", seed=seed, phase="random")
    rng = np.random.default_rng(seed + 7)
    ph = rng.integers(0, h, size=batch)
    for k in range(batch):
        f["gait"][k] = synthetic.mpc_gait(h, (0, h // 2), MIXED_DUTY[k % len(MIXED_DUTY)], int(ph[k]))
    return f


def sweep_fields(groups: int, k: int, h: int, gait: str, seed: int) -> dict:
    """`groups` random states, each under `k` velocity / yaw-rate commands (the reference trajectory rebuilt per command as
    synthetic.make_batch builds it)."""
    base = synthetic.make_batch(groups, h, gait, seed=seed, phase="random")
    f = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in base.items()}
    rng = np.random.default_rng(seed + 99)
    b = groups * k
    vx, vy, yr = rng.uniform(-0.5, 0.5, b), rng.uniform(-0.2, 0.2, b), rng.uniform(-0.3, 0.3, b)
    tr = f["traj"].reshape(b, h, 12).copy()
    steps = np.arange(h)[None, :]
    tr[:, :, 9], tr[:, :, 10], tr[:, :, 8] = vx[:, None], vy[:, None], yr[:, None]
    tr[:, :, 3] = f["p"][:, 0:1] + steps * synthetic.DT_MPC * vx[:, None]
    tr[:, :, 4] = f["p"][:, 1:2] + steps * synthetic.DT_MPC * vy[:, None]
    tr[:, 1:, 2] = tr[:, 0:1, 2] + steps[:, 1:] * synthetic.DT_MPC * yr[:, None]
    f["traj"] = tr.reshape(b, 12 * h)
    return f


def reduced_sizes(fields: dict) -> np.ndarray:
    return 6 * np.asarray(fields["gait"]).sum(axis=1)


def cases() -> list:
    """(name, horizon, field dict, command-sweep group size or 0)"""
    return [("standing", 10, synthetic.make_batch(64, 10, "standing", seed=101, phase="random"), 0),
            ("mixed", 10, mixed_fields(64, 10, seed=102), 0),
            ("single_h20", 20, synthetic.make_batch(32, 20, "single", seed=103, phase="random"), 0),
            ("sweep120", 10, sweep_fields(8, 8, 10, "standing", seed=104), 8),
            ("sweep60", 10, sweep_fields(8, 8, 10, "walking", seed=105), 8),
            ("walking", 10, synthetic.make_batch(32, 10, "walking", seed=106, phase="random"), 0),
            ("standing_3x", 10, synthetic.hard_batch(64, 10, "standing", 107, 3), 0)]


def check_cases(cs: list) -> None:
    """What the shapes are chosen for really occurs in them."""
    by = {name: f for name, _, f, _ in cs}
    assert (reduced_sizes(by["standing"]) == 120).all() and (reduced_sizes(by["standing_3x"]) == 120).all()
    n = reduced_sizes(by["mixed"])
    assert n.min() >= 66 and n.max() <= 114 and len(set(n.tolist())) >= 4, sorted(set(n.tolist()))
    # a horizon step whose variables lie on both sides of a multiple of 16 in the sweep order (leg-steps of 6 variables, sorted by
    # step): the tiles (I, I + 1) then hold entries of one and the same step
    g = np.asarray(by["mixed"]["gait"]).reshape(len(n), 10, 2)
    ends = 6 * np.cumsum(g.sum(axis=2), axis=1)  # variables up to and including each step
    starts = ends - 6 * g.sum(axis=2)
    straddles = ((starts // 16) != ((ends - 1) // 16)) & (g.sum(axis=2) > 0)
    assert straddles.any(axis=1).all()
    assert (reduced_sizes(by["single_h20"]) == 120).all()
    assert (reduced_sizes(by["walking"]) == 60).all() and (reduced_sizes(by["sweep60"]) == 60).all()


def solve_case(h: int, fields: dict, k: int):
    """forces [b, 12 h] float32 and status words [b] of one case, as the library that is built in this tree gives them"""
    from hector_simulation_amd import interface

    rec = records.pack_records(fields, h)
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, rec.shape[0])
    m.upload(rec)
    if k:
        m.solve_command_sweep(k)
    else:
        m.solve()
    forces, status = m.download()
    m.close()
    return np.ascontiguousarray(forces), np.ascontiguousarray(status)


def main():
    import torch  # (first: one HIP runtime per process, tests/conftest.py)

    torch.zeros(1, device="cuda")
    from hector_simulation_amd import interface

    commit = os.environ.get("HMPC_GOLDEN_COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    cs = cases()
    check_cases(cs)
    out = {"commit": np.array(commit)}
    for name, h, fields, k in cs:
        forces, status = solve_case(h, fields, k)
        code = interface.status_code(status)
        out[name + "_forces"] = forces.view(np.uint32)
        out[name + "_status"] = status
        print(f"{name:12s} b {forces.shape[0]:3d} n {sorted(set(reduced_sizes(fields).tolist()))} codes {dict(zip(*np.unique(code, return_counts=True)))} "
              f"iterations {interface.status_iters(status).min()}..{interface.status_iters(status).max()} "
              f"|W| {interface.status_nactive(status).min()}..{interface.status_nactive(status).max()}")
    np.savez_compressed(PATH, **out)
    print("wrote", os.path.relpath(PATH, ROOT), os.path.getsize(PATH), "bytes, commit", commit)


if __name__ == "__main__":
    main()
