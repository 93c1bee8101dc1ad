#!/usr/bin/env python3
"""Generates tests/golden/schur_bits.npz: forces and status words of the variants that invert the block start's Schur matrix
on the matrix cores, as the commit named in the file computed them, for tests/test_gpu_schur_bits.py.

What it is for: a change to the tile loader / store of the Schur inversion (schur_load, schur_store, the CHECK = true
instantiation of mfs_steps) that moves data, computes addresses or skips tiles nothing reads, and leaves every arithmetic
instruction on data alone, must reproduce these outputs bit for bit.  The file holds this project's OWN outputs; it is
regenerated (on the GPU, with the build of the commit one wants to pin) whenever a change alters the arithmetic on purpose:

    python tests/golden/make_schur_bits.py [--out FILE]         (from the repository root; HEAD's hash goes into the file,
                                                                 or HMPC_GOLDEN_COMMIT where there is no .git)

Cases (cases() below, shared with the test):

  k0_edges      the FAST 120-variable variant (3 x 3 tiles of 16 rows) with the row count k0 of the block start's FIRST round pinned
                at 1, 15, 16, 17, 31, 32, 33, 47, 48 (four instances each) and at 52 and 54 candidates (two each; the round takes
                48 of them).  Route: hmpc_debug_solve_external_qp with a DIAGONAL H and a constraint block of this file's own, so
                that the QP falls apart into one 6-variable problem per leg-step and everything can be said on the host:
                  * the rows the first round takes are the rows 0..6 violated at x_u = -g_i / H_ii (one friction row per axis);
                    k0_instances() builds x_u from a target set V per leg-step and verify_instance() recomputes, from the binary32
                    H and g that are handed in, that exactly V is violated, every slack at least 1e-3 from zero;
                  * the minimiser on V has multipliers > 0 and satisfies every other row (all eight) with slack >= 1e-3: it is
                    the optimum, so the round releases nothing and nothing enters after it.
                main() then ASSERTS on the status words: code ok, |W| = k0, 0 counted iterations (a second round or a single-row
                iteration would have counted) for k0 <= 48.  For 52 / 54 candidates it asserts code ok, |W| = the candidate count
                and at least candidates - 48 counted iterations; that the first round took exactly 48 rows follows from the
                kernel's cap and is NOT observable from the status word.
  contacts3     three contacts standing (make_batch3), 32 instances: 4 x 4 tiles on four waves
  wide_h20      double support h = 20, 32 instances: the wide variant, 5 x 5 tiles on eight waves
  cont_6x       standing at 6x the input ranges through the default repair chain, 32 instances: the continuation variant's
                6 x 6 tiles (main() asserts that some instance was handed over: a working set beyond the fast variant's 64 rows)
  sweep_4x8     command sweep, 4 states x 8 commands: the SWEEP variant of the 120-variable shape, 3 x 3 tiles"""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hector_simulation_amd import records, synthetic  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_fast_path_bits", os.path.join(ROOT, "tests", "golden", "make_fast_path_bits.py"))
_fp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_fp)

PATH = os.path.join(ROOT, "tests", "golden", "schur_bits.npz")
H10 = 10
KB = 48  # rows a block round of the FAST 120-variable variant takes (3 tiles of 16)
K0_TARGETS = [1, 15, 16, 17, 31, 32, 33, 47, 48] * 4 + [52, 54] * 2
MARGIN = 1e-3
UB4 = float(np.float32(0.01))  # upper bound of the moment window (row 4); rows 5, 6: <= 0; rows 0-3: >= 0; row 7: 0 <= . <= cap


def leg_rows(leg: int, mu: float, lt: float, lh: float) -> np.ndarray:
    """The eight rows of a leg over its six variables (F then M) for a contact frame aligned with the axes."""
    c = np.zeros((8, 6))
    c[0, 0], c[0, 2] = -mu, 1.0
    c[1, 0], c[1, 2] = mu, 1.0
    c[2, 1], c[2, 2] = -mu, 1.0
    c[3, 1], c[3, 2] = mu, 1.0
    c[4, 3] = 1.0
    c[5, 2], c[5, 4] = -lt, 1.0
    c[6, 2], c[6, 4] = -lh, (-1.0 if leg != 1 else 1.0)
    c[7, 2] = 2.0
    return c.astype(np.float32).astype(np.float64)


def fc_block(mu: float, lt: float, lh: float) -> np.ndarray:
    """[16][12] constraint block of a step: row 8 leg + rr; columns 3 leg + k (F), 6 + 3 leg + k (M)."""
    fc = np.zeros((16, 12), np.float32)
    for leg in range(2):
        c = leg_rows(leg, mu, lt, lh)
        fc[8 * leg:8 * leg + 8, 3 * leg:3 * leg + 3] = c[:, :3]
        fc[8 * leg:8 * leg + 8, 6 + 3 * leg:6 + 3 * leg + 3] = c[:, 3:]
    return fc


def row_slacks(c: np.ndarray, x: np.ndarray, cap: float):
    """(slack on the tighter side, side) of the eight rows at x: side +1 lower bound, -1 upper bound (the kernel's my_slack)."""
    s = c @ x
    sl = np.where((np.arange(8) <= 4) | (np.arange(8) == 7), s, np.inf)
    ub = np.array([0, 0, 0, 0, UB4, 0, 0, cap])
    su = np.where(np.arange(8) >= 4, ub - s, np.inf)
    return np.minimum(sl, su), np.where(sl <= su, 1, -1), ub


def first_round_rows(c: np.ndarray, xu: np.ndarray, cap: float):
    """Rows 0..6 the first round takes at xu (violated; a friction row only if its partner on the axis is not), their sides, and
    the smallest distance of any of the seven slacks from zero."""
    slack, side, _ = row_slacks(c, xu, cap)
    viol = slack[:7] < 0
    take = viol.copy()
    for rr in range(4):
        take[rr] = viol[rr] and not viol[rr ^ 1]
    return np.flatnonzero(take), side[:7], float(np.abs(slack[:7]).min())


def minimiser_on(c: np.ndarray, hd: np.ndarray, xu: np.ndarray, rows: np.ndarray, side: np.ndarray, cap: float):
    """x and multipliers of min 1/2 (x - xu)' diag(hd) (x - xu) with the given rows held at their bounds."""
    if len(rows) == 0:
        return xu.copy(), np.zeros(0)
    ub = np.array([0, 0, 0, 0, UB4, 0, 0, cap])
    n = c[rows] * side[rows, None]
    b = np.where(side[rows] > 0, 0.0, -ub[rows])
    m = 1.0 / hd
    s0 = (n * m) @ n.T
    u = np.linalg.solve(s0, b - n @ xu)
    return xu + m * (n.T @ u), u


def verify_legstep(c, hd, xu, cap):
    """Number of rows the first round takes for this leg-step, provided that set is also the optimal active set (else -1)."""
    rows, side, dist = first_round_rows(c, xu, cap)
    if dist < MARGIN:
        return -1
    if len(rows) and np.linalg.cond(c[rows]) > 1e6:
        return -1
    x, u = minimiser_on(c, hd, xu, rows, side, cap)
    if len(u) and u.min() < MARGIN:
        return -1
    slack, _, _ = row_slacks(c, x, cap)
    others = np.setdiff1d(np.arange(8), rows)
    if slack[others].min() < MARGIN:
        return -1
    return len(rows)


GROUPS = [(0, 1), (2, 3), (4,), (5,), (6,)]  # at most one row of each group in a set (friction: one per axis)


def make_legstep(rng, c, hd, nrows: int, cap: float):
    """x_u of a leg-step whose first-round set has `nrows` rows and is optimal: a target set V, a point on its faces that is strictly
    inside every other row, and x_u = that point - M N_V' u with u > 0 (KKT read backwards); accepted only if verify_legstep agrees."""
    m = 1.0 / hd
    ub = np.array([0, 0, 0, 0, UB4, 0, 0, cap])
    for _ in range(300):
        fz = rng.uniform(10.0, 30.0)
        xf = np.array([rng.uniform(-0.2, 0.2) * fz, rng.uniform(-0.2, 0.2) * fz, fz, rng.uniform(0.002, 0.008),
                       rng.uniform(-0.03, 0.03) * fz, rng.uniform(-1.0, 1.0)])
        if nrows == 0:
            xu = xf
        else:
            gs = rng.choice(len(GROUPS), size=nrows, replace=False)
            rows = np.array(sorted(int(rng.choice(GROUPS[g])) for g in gs))
            side = np.ones(8, int)
            side[5] = side[6] = -1
            side[4] = int(rng.choice([-1, 1]))
            n = c[rows] * side[rows, None]
            b = np.where(side[rows] > 0, 0.0, -ub[rows])
            xs = xf + m * (n.T @ np.linalg.solve((n * m) @ n.T, b - n @ xf))
            u = rng.uniform(0.5, 2.0, nrows) * 5.0 / np.einsum("ij,j,ij->i", n, m, n)
            xu = xs - m * (n.T @ u)
        # what the kernel sees: binary32 g = -H x_u, so x_u = -g / H with both rounded
        g32 = (-(hd * xu)).astype(np.float32)
        xu32 = -g32.astype(np.float64) / hd
        if verify_legstep(c, hd, xu32, cap) == nrows:
            return g32
    return None  # (a diagonal with a very soft F_z drags every friction row along: the caller draws another)


def k0_instances(seed: int = 151):
    """(H [b, 120, 120], g [b, 120], Fc [b, 16, 12], k0 [b]) of the k0_edges case."""
    rng = np.random.default_rng(seed)
    b = len(K0_TARGETS)
    hx, gx, fx = np.zeros((b, 120, 120), np.float32), np.zeros((b, 120), np.float32), np.zeros((b, 16, 12), np.float32)
    for k, target in enumerate(K0_TARGETS):
        mu, lt, lh = rng.uniform(0.3, 0.7), 0.09, 0.06
        fx[k] = fc_block(mu, lt, lh)
        # rows per leg-step: as many threes as fit, the rest spread, in a random order of the 20 leg-steps
        per = np.zeros(20, int)
        left = target
        for e in rng.permutation(20):
            per[e] = min(3, left)
            left -= per[e]
        assert left == 0
        for e in range(20):
            step, leg = e // 2, e % 2
            idx = np.concatenate([12 * step + 3 * leg + np.arange(3), 12 * step + 6 + 3 * leg + np.arange(3)])
            g32 = None
            while g32 is None:
                hd = (10.0 ** rng.uniform(-1.5, 1.5, 6)).astype(np.float32)  # (three decades: the scaling exponents of S0 vary from row to row)
                g32 = make_legstep(rng, leg_rows(leg, mu, lt, lh), hd.astype(np.float64), int(per[e]), synthetic.F_MAX)
            hx[k][idx, idx], gx[k, idx] = hd, g32
    return hx, gx, fx, np.array(K0_TARGETS)


def k0_inputs_from(golden):
    """(H, g, Fc, k0) of the k0_edges case as the golden file keeps them"""
    hd = golden["k0_edges_hdiag"]
    hx = np.zeros((hd.shape[0], 120, 120), np.float32)
    hx[:, np.arange(120), np.arange(120)] = hd
    return hx, golden["k0_edges_g"], golden["k0_edges_fc"], golden["k0_edges_k0"]


def verify_instance(hx, gx, fx) -> int:
    """The first round's row count of one instance, recomputed from the binary32 data alone (-1: some leg-step does not verify)."""
    total = 0
    for e in range(20):
        step, leg = e // 2, e % 2
        idx = np.concatenate([12 * step + 3 * leg + np.arange(3), 12 * step + 6 + 3 * leg + np.arange(3)])
        c = fx[8 * leg:8 * leg + 8][:, np.concatenate([3 * leg + np.arange(3), 6 + 3 * leg + np.arange(3)])].astype(np.float64)
        hd = hx[idx, idx].astype(np.float64)
        r = verify_legstep(c, hd, -gx[idx].astype(np.float64) / hd, synthetic.F_MAX)
        if r < 0:
            return -1
        total += r
    return total


def cases() -> list:
    """(name, horizon, contacts, field dict, command-sweep group size or 0) of the cases that go through the ordinary solve"""
    return [("contacts3", 10, 3, synthetic.make_batch3(32, 10, "standing", seed=152, phase="random", hand="contact"), 0),
            ("wide_h20", 20, 2, synthetic.make_batch(32, 20, "standing", seed=153, phase="random"), 0),
            ("cont_6x", 10, 2, synthetic.hard_batch(32, 10, "standing", 154, 6), 0),
            ("sweep_4x8", 10, 2, _fp.sweep_fields(4, 8, 10, "standing", seed=155), 8)]


def solve_case(h: int, nc: int, fields: dict, k: int):
    """forces float32 [b, 6 nc h] and status words [b] of one case, as the library that is built in this tree gives them (default
    repair chain: hmpc_download runs whatever the first pass flagged through the continuation and safe passes)"""
    from hector_simulation_amd import interface

    rec = records.pack_records(fields, h, nc)
    m = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, rec.shape[0], contacts=nc)
    m.upload(rec)
    if k:
        m.solve_command_sweep(k)
    else:
        m.solve()
    forces, status = m.download()
    m.close()
    return np.ascontiguousarray(forces), np.ascontiguousarray(status)


def solve_k0_edges(hx, gx, fx):
    """the k0_edges case through hmpc_debug_solve_external_qp (first pass only); the records supply the gait table (all stance)"""
    from hector_simulation_amd import interface

    b = hx.shape[0]
    rec = records.pack_records(synthetic.make_batch(b, H10, "standing", seed=150, phase="random"), H10)
    m = interface.BatchedMPC(synthetic.DT_MPC, H10, synthetic.F_MAX, b)
    m.upload(rec)
    m.set_auto_resolve(False)
    m.solve_external_qp(hx, gx, fx)
    forces, status = m.download()
    m.close()
    return np.ascontiguousarray(forces), np.ascontiguousarray(status)


def main():
    import torch  # (first: one HIP runtime per process, tests/conftest.py)

    torch.zeros(1, device="cuda")
    from hector_simulation_amd import interface

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else PATH
    commit = os.environ.get("HMPC_GOLDEN_COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": np.array(commit)}

    hx, gx, fx, k0 = k0_instances()
    host = np.array([verify_instance(hx[k], gx[k], fx[k]) for k in range(len(k0))])
    assert (host == k0).all(), (host, k0)
    forces, status = solve_k0_edges(hx, gx, fx)
    code, it, nact = interface.status_code(status), interface.status_iters(status), interface.status_nactive(status)
    for t in sorted(set(k0.tolist())):
        sel = k0 == t
        print(f"k0_edges     target {t:2d}: codes {code[sel].tolist()} iterations {it[sel].tolist()} |W| {nact[sel].tolist()}")
    out["k0_edges_forces"], out["k0_edges_status"], out["k0_edges_k0"] = forces.view(np.uint32), status, k0
    # (the inputs as well: building them is a random search of half a minute; the test reads them back and verifies them again)
    out["k0_edges_hdiag"], out["k0_edges_g"], out["k0_edges_fc"] = np.ascontiguousarray(np.diagonal(hx, axis1=1, axis2=2)), gx, fx
    proved = (code == 0) & (nact == k0) & np.where(k0 <= KB, it == 0, it >= k0 - KB)
    out["k0_edges_proved"] = proved

    ordinary = {}
    for name, h, nc, fields, k in cases():
        forces, status = solve_case(h, nc, fields, k)
        c = interface.status_code(status)
        ordinary[name] = status
        out[name + "_forces"] = forces.view(np.uint32)
        out[name + "_status"] = status
        print(f"{name:12s} b {forces.shape[0]:3d} codes {dict(zip(*np.unique(c, return_counts=True)))} "
              f"iterations {interface.status_iters(status).min()}..{interface.status_iters(status).max()} "
              f"|W| {interface.status_nactive(status).min()}..{interface.status_nactive(status).max()}")
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes, commit", commit)
    # (after the file is written, so that a failed statement leaves the evidence behind)
    assert proved.all(), ("first-round row count not confirmed by the status words", np.flatnonzero(~proved), code[~proved], it[~proved], nact[~proved], k0[~proved])
    assert interface.status_nactive(ordinary["cont_6x"]).max() > 64, "cont_6x: no working set beyond the fast variant's 64 rows, the continuation variant did not run"
    for name in ("contacts3", "wide_h20", "sweep_4x8"):  # (nominal inputs; at 6x an instance may legitimately end flagged)
        assert np.isin(interface.status_code(ordinary[name]), (0, 6)).all(), name


if __name__ == "__main__":
    main()
