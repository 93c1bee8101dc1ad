"""Irregular gait tables on the GPU (tests/irregular_gaits.py; CPU side: tests/test_irregular_gaits.py, which also shows that the
reference's qpOASES solves every instance compared here).

The gait table drives everything that sizes and indexes the solve: the prefix counts of stance leg-steps, the swing elimination, var_ind
and the scatter, the variant an instance runs on, the pivot steps and tiles of stage S and of the block start.  Checked on tables the
periodic gaits never produce -- flight steps, a lone stance leg-step, stance at the last step only, random asymmetric tables, every
horizon 1 .. 20, every reduced size on every variant that holds it, the sizes either side of the class borders:

a. the assembly, bit for bit against the oracle;
b. every reduced size k = 1 .. nc h on every variant that holds it, against qpOASES: forces and objective within the project's 1e-4,
   eliminated variables exactly 0, the binary64 copy-out within 1e-7 on the <= 120-variable variants and 1e-6 on the wide and the
   three-contact one (the bars of test_gpu_solve.py and test_gpu_contacts3.py);
c. every horizon h = 1 .. 20, plus the explicit all-swing instance (n = 0: zeros, status OK), on every variant of the horizon;
d. the routing at the class borders, bit for bit against each class solved alone under its own hint; a hint one class too small;
   the same through the device-side record builder;
e. what hangs off the solve: command sweep, tick warm start with the table advancing, margins, prediction.

Each solve test prints its figures before it asserts; the session's maxima per variant are printed at the end of the module."""
import numpy as np
import pytest

import irregular_gaits as ig
import margins_mirror as mm
import prediction_mirror as pm
from hector_simulation_amd import interface, synthetic

pytestmark = pytest.mark.gpu

DT, FMAX = synthetic.DT_MPC, synthetic.F_MAX
TOL = 1e-4                      # north_star: forces and objective within 1e-4 relative of qpOASES (TOL of test_gpu_solve.py)
BAR64_NARROW, BAR64_WIDE = 1e-7, 1e-6
S_TOO_LARGE = 3

_refs = {}
_report = {}


def rel_inf(a, b):
    return np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))


def variant_of(h, nc, n_max):
    """(name, binary64 bar) of the fast variant that holds a batch whose widest reduced QP has n_max variables (pick_variant of
    csrc/hmpc_plan.h, restated): 60 / 120 variables at h <= 10 or h <= 20, the wide 240-variable one, the three-contact one."""
    if nc == 3:
        return "180/10 three contacts", BAR64_WIDE
    if n_max > 120:
        return "240/20 wide", BAR64_WIDE
    return f"{60 if n_max <= 60 else 120}/{10 if h <= 10 else 20}", BAR64_NARROW


def reference(oracle, b):
    """qpOASES on the batch, once per session: q [nb, 6 nc h], obj [nb]; the explicit n = 0 rows are zeros and never handed over."""
    if b.name not in _refs:
        keep = np.flatnonzero(~b.zero)
        assert (b.n[keep] >= 6).all() and (b.n[b.zero] == 0).all()
        r = oracle.solve_records(np.ascontiguousarray(b.rec[keep]), b.h, DT, FMAX, nc=b.nc)
        assert r["n_bad"] == 0, (b.name, np.flatnonzero(r["bad"]))
        q, obj = np.zeros((len(b), 6 * b.nc * b.h)), np.zeros(len(b))
        q[keep], obj[keep] = r["q_soln"], r["obj"]
        q.setflags(write=False), obj.setflags(write=False)
        _refs[b.name] = dict(q=q, obj=obj)
    return _refs[b.name]


def device(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def solve(rec, h, nc=2, hint=None, auto=True, sweep=0):
    """(forces, status, x64, obj64) of a fresh handle: host upload (hint None: the handle sizes the batch from the tables) or
    device-resident records under ``hint`` (-1 = none: classified on the device)."""
    nb = rec.shape[0]
    mpc = interface.BatchedMPC(DT, h, FMAX, nb, contacts=nc)
    mpc.set_auto_resolve(auto)
    if hint is None:
        mpc.upload(rec)
    else:
        d = device(rec)
        mpc.set_device_records(d.data_ptr(), nb, max_reduced_vars=hint, keepalive=d)
    if sweep:
        mpc.solve_command_sweep(sweep)
    else:
        mpc.solve()
    forces, status = mpc.download()
    x64, obj64 = mpc.download_f64()
    mpc.close()
    return forces, status, x64, obj64


def swing_mask(b, idx):
    """[len(idx), 6 nc h] bool: the variables of the swing leg-steps ([step][F of each contact, M of each contact])."""
    sw = b.tables[idx].reshape(len(idx), b.h, 1, b.nc, 1) == 0
    return np.broadcast_to(sw, (len(idx), b.h, 2, b.nc, 3)).reshape(len(idx), 6 * b.nc * b.h)


def check_against_qpoases(oracle, b, idx, hint, what):
    """The assertions of parts b and c on rows ``idx`` of batch ``b`` solved as one batch (host upload, or device records + hint)."""
    idx = np.asarray(idx)
    ref = reference(oracle, b)
    rec = np.ascontiguousarray(b.rec[idx])
    name, bar64 = variant_of(b.h, b.nc, int(b.n[idx].max()) if hint is None else hint)
    _, st_fast, _, _ = solve(rec, b.h, b.nc, hint, auto=False)
    forces, status, x64, obj64 = solve(rec, b.h, b.nc, hint)
    q, obj = ref["q"][idx], ref["obj"][idx]
    e32, e64 = rel_inf(forces.astype(np.float64), q), rel_inf(x64, q)
    og = np.abs(obj64 - obj) / np.maximum(1.0, np.abs(obj))
    flagged = int((interface.status_code(st_fast) != 0).sum())
    print(f"{what} [{name}] {len(idx)} instances, n {b.n[idx].min()}..{b.n[idx].max()}: force {e32.max():.3e} binary64 {e64.max():.3e} "
          f"(bar {bar64:.0e}, worst {b.table_names[idx[int(np.argmax(e64))]]}) objective {og.max():.3e} flagged by the fast pass {flagged}")
    r = _report.setdefault(name, dict(instances=0, force=0.0, f64=0.0, obj=0.0, flagged=0, sizes=set()))
    r["instances"] += len(idx)
    r["force"], r["f64"], r["obj"] = max(r["force"], e32.max()), max(r["f64"], e64.max()), max(r["obj"], og.max())
    r["flagged"] += flagged
    r["sizes"] |= set(int(n) for n in b.n[idx])
    code = interface.status_code(status)
    assert (code == 0).all(), (what, [(b.table_names[i], int(c)) for i, c in zip(idx, code) if c])
    assert e32.max() < TOL, (what, e32.max(), b.table_names[idx[int(np.argmax(e32))]])
    assert og.max() < TOL, (what, og.max())
    sw = swing_mask(b, idx)
    assert np.all(forces[sw] == 0.0) and np.all(x64[sw] == 0.0), what     # eliminated variables: exact zeros
    assert np.all(forces[b.zero[idx]] == 0.0)                              # the all-swing instance: zeros
    assert e64.max() < bar64, (what, e64.max(), b.table_names[idx[int(np.argmax(e64))]])


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nirregular gait tables against qpOASES, maxima per variant")
    print(f"{'variant':24s} {'instances':>9s} {'sizes':>6s} {'n':>9s} {'force':>10s} {'binary64':>10s} {'objective':>10s} {'flagged by the fast pass':>25s}")
    for name in sorted(_report):
        r = _report[name]
        print(f"{name:24s} {r['instances']:9d} {len(r['sizes']):6d} {min(r['sizes']):4d}..{max(r['sizes']):<4d} {r['force']:10.3e} {r['f64']:10.3e} "
              f"{r['obj']:10.3e} {r['flagged']:25d}")


# ------------------------------------------------------------------------------------------------ a. assembly
@pytest.mark.parametrize("h,nc", ig.ASSEMBLY_SHAPES)
def test_assembly_bitwise_on_irregular_tables(oracle, h, nc):
    b = ig.cached(ig.assembly_batch, h, nc)
    if nc == 3:
        assert "hand_is_the_only_contact_in_stance" in b.table_names
    mpc = interface.BatchedMPC(DT, h, FMAX, len(b), contacts=nc)
    mpc.upload(b.rec)
    for k in range(len(b)):
        what = b.table_names[k]
        o = oracle.assemble_record(b.rec[k], h, DT, FMAX, nc=nc)
        d = mpc.debug_assemble(k)
        assert d["n"] == o["n"] == b.n[k] and d["m"] == o["m"], what
        np.testing.assert_array_equal(d["var_ind"], o["var_ind"], err_msg=what)
        for name in ("x0", "Acd", "Bcd", "Fc", "lb", "ub"):
            np.testing.assert_array_equal(d[name].view(np.uint32), o[name].view(np.uint32), err_msg=f"{what} {name}")
        Ho, go = o["H_red"].astype(np.float32), o["g_red"].astype(np.float32)
        assert np.array_equal(Ho.astype(np.float64), o["H_red"])  # the oracle's doubles are widened floats
        np.testing.assert_array_equal(d["g"].view(np.uint32), go.view(np.uint32), err_msg=f"{what} g")
        np.testing.assert_array_equal(d["H"].view(np.uint32), Ho.view(np.uint32), err_msg=f"{what} H")
    mpc.close()


# ------------------------------------------------------------------------------------------------ b. every reduced size
@pytest.mark.parametrize("h,nc", ig.SIZES_SHAPES)
def test_every_reduced_size_on_every_variant_that_holds_it(oracle, h, nc):
    """Two instances of each k = 1 .. nc h: as a host upload the whole batch runs on the widest variant; the subsets n <= 60 and n <= 120
    again as device-resident records under the hints 60 and 120, i.e. on the 60- and 120-variable variants of the horizon."""
    b = ig.cached(ig.sizes_batch, h, nc)
    assert sorted(set(b.k)) == list(range(1, nc * h + 1)) and len(b) == 2 * nc * h
    check_against_qpoases(oracle, b, np.arange(len(b)), None, f"sizes h{h} c{nc} host upload")
    if nc == 2:
        for hint in (60, 120):
            idx = np.flatnonzero(b.n <= hint)
            check_against_qpoases(oracle, b, idx, hint, f"sizes h{h} c{nc} hint {hint}")


# ------------------------------------------------------------------------------------------------ c. every horizon
@pytest.mark.parametrize("h", range(1, 21))
def test_every_horizon(oracle, h):
    b = ig.cached(ig.horizon_batch, h)
    assert b.zero.sum() == 1 and b.table_names[-1] == "all_swing"
    check_against_qpoases(oracle, b, np.arange(len(b)), None, f"horizon {h}")
    # the host upload puts the whole batch on the variant of its widest instance; the narrower variants of this horizon get the
    # instances they hold as device-resident records under their hint (the all-swing one among them)
    host = variant_of(h, 2, int(b.n.max()))[0]
    for hint in (60, 120):
        idx = np.flatnonzero(b.n <= hint)
        if variant_of(h, 2, hint)[0] != host and len(idx) >= 2:
            check_against_qpoases(oracle, b, idx, hint, f"horizon {h} hint {hint}")


# ------------------------------------------------------------------------------------------------ d. routing at the class borders
def classes_of(b_n, h):
    """[(hint, rows)]: the size classes the device sorts a two-contact batch into (csrc/hmpc_plan.h class_launches)."""
    out = [(60, np.flatnonzero(b_n <= 60)), (120, np.flatnonzero((b_n > 60) & (b_n <= 120)))]
    if h > 10:
        out.append((240, np.flatnonzero(b_n > 120)))
    return out


def assert_routed_per_class(rec, n, h, forces, status):
    """Forces and status words of an unhinted solve equal, bit for bit, those of each size class solved alone under its own hint."""
    for hint, rows in classes_of(n, h):
        assert len(rows) >= 2
        f1, s1, _, _ = solve(np.ascontiguousarray(rec[rows]), h, 2, hint)
        np.testing.assert_array_equal(status[rows], s1, err_msg=f"class {hint}")
        np.testing.assert_array_equal(forces[rows].view(np.uint32), f1.view(np.uint32), err_msg=f"class {hint}")


@pytest.mark.parametrize("h", [20, 10])
def test_routing_at_the_class_borders_is_bitwise_the_hinted_solve(oracle, h):
    b = ig.cached(ig.border_batch, h)
    assert sorted(set(b.n)) == sorted(ig.BORDER_SIZES[h]) and (np.bincount(b.n)[list(ig.BORDER_SIZES[h])] == 2).all()
    ref = reference(oracle, b)
    forces, status, _, _ = solve(b.rec, h, 2, hint=-1)
    assert (interface.status_code(status) == 0).all(), interface.status_code(status)
    err = rel_inf(forces.astype(np.float64), ref["q"])
    print(f"borders h{h}: unhinted, force error against qpOASES {err.max():.3e}")
    assert err.max() < TOL
    assert_routed_per_class(b.rec, b.n, h, forces, status)
    # a hint one class too small: HMPC_S_TOO_LARGE and zero forces for exactly the instances that exceed it; the rest are untouched by
    # their neighbours: bit for bit what the hinted variant gives them when they are solved without the oversize instances (under hint
    # 120 at h = 20 the n <= 60 instances run on the 120-variable variant, whose last bits are not the 60-variable variant's: measured,
    # one force of 2 400 differs by one unit in the last place from the unhinted solve), and they are what qpOASES gives
    for hint in (60, 120):
        if (b.n <= hint).all():
            continue
        f2, s2, _, _ = solve(b.rec, h, 2, hint)
        big = b.n > hint
        assert big.any() and (~big).any()
        np.testing.assert_array_equal(interface.status_code(s2) == S_TOO_LARGE, big, err_msg=f"hint {hint}")
        assert (f2[big] == 0).all()
        f3, s3, _, _ = solve(np.ascontiguousarray(b.rec[~big]), h, 2, hint)
        np.testing.assert_array_equal(s2[~big], s3, err_msg=f"hint {hint}")
        np.testing.assert_array_equal(f2[~big].view(np.uint32), f3.view(np.uint32), err_msg=f"hint {hint}")
        assert (interface.status_code(s3) == 0).all() and rel_inf(f3.astype(np.float64), ref["q"][~big]).max() < TOL
        same = b.n <= 60 if hint == 60 else (b.n > 60) & ~big      # the instances the unhinted solve puts on this very variant
        np.testing.assert_array_equal(s2[same], status[same], err_msg=f"hint {hint}")
        np.testing.assert_array_equal(f2[same].view(np.uint32), forces[same].view(np.uint32), err_msg=f"hint {hint}")


def test_routing_of_records_built_on_the_device_at_the_class_borders(oracle):
    """The unhinted h = 10 batch through the device-side record builder: ticks whose random offsets and durations give the border
    sizes.  The built records are the oracle's, bit for bit; the builder's size classes route each instance as the hint would."""
    h = 10
    t, sizes = ig.border_ticks(h)
    want, _ = oracle.build_records(t, h, DT)
    mpc = interface.BatchedMPC(DT, h, FMAX, len(t))
    mpc.build_records(t, DT)
    rec = mpc.download_records()
    np.testing.assert_array_equal(rec, want)
    mpc.solve()
    forces, status = mpc.download()
    mpc.close()
    assert (interface.status_code(status) == 0).all(), interface.status_code(status)
    ref = oracle.solve_records(want, h, DT, FMAX)
    assert ref["n_bad"] == 0
    err = rel_inf(forces.astype(np.float64), ref["q_soln"])
    print(f"borders h{h} built on the device: force error against qpOASES {err.max():.3e}")
    assert err.max() < TOL
    assert_routed_per_class(want, sizes, h, forces, status)


# ------------------------------------------------------------------------------------------------ e. what hangs off the solve
def test_sweep_on_irregular_tables_is_bitwise_the_independent_solve(oracle):
    """Groups of 3 commands sharing one irregular table.  Device-resident records without a hint: every group runs on the sweep variant
    of its size class (60 and 120 variables, both present), as the independent solve's instances do; host upload: all on the
    120-variable one; the n <= 60 groups alone: all on the 60-variable one."""
    b = ig.hangs_sweep()
    k = 3
    assert (b.n <= 60).any() and (b.n > 60).any()
    ref = reference(oracle, b)
    small = np.flatnonzero(b.n <= 60)
    for what, rows, hint in (("device records, no hint", np.arange(len(b)), -1), ("host upload", np.arange(len(b)), None),
                             ("host upload, n <= 60", small, None)):
        rec = np.ascontiguousarray(b.rec[rows])
        f0, s0, _, _ = solve(rec, b.h, 2, hint)
        f1, s1, _, _ = solve(rec, b.h, 2, hint, sweep=k)
        assert (interface.status_code(s0) == 0).all(), (what, interface.status_code(s0))
        np.testing.assert_array_equal(s1, s0, err_msg=what)
        np.testing.assert_array_equal(f1.view(np.uint32), f0.view(np.uint32), err_msg=what)
        err = rel_inf(f1.astype(np.float64), ref["q"][rows])
        print(f"sweep, {what}: force error against qpOASES {err.max():.3e}")
        assert err.max() < TOL
        g = f1.reshape(len(rows) // k, k, -1)
        assert np.abs(g[:, 0] - g[:, 1]).max() > 1e-3  # the commands really differ inside a group


@pytest.mark.parametrize("shift", ig.WARM_SHIFTS)
def test_tick_warm_start_with_an_irregular_table_advancing(oracle, shift):
    """The second tick's table is the first advanced by ``shift`` steps with fresh random leg-steps entering at the end: leg-steps leave
    and enter stance in the middle of the saved working set."""
    b0 = ig.cached(ig.hangs_batch, 10, 2)
    b1 = ig.warm_second(shift)
    ref = reference(oracle, b1)
    mpc = interface.BatchedMPC(DT, b0.h, FMAX, len(b0))
    mpc.set_tick_warm_start(True, horizon_shift=0)
    mpc.upload(b0.rec)
    mpc.solve()
    _, s0 = mpc.download()
    mpc.set_tick_warm_start(True, horizon_shift=shift)
    mpc.upload(b1.rec)
    mpc.solve()
    forces, s1 = mpc.download()
    mpc.close()
    assert (interface.status_code(s0) == 0).all()
    err = rel_inf(forces.astype(np.float64), ref["q"])
    print(f"tick warm start, shift {shift}: force error against qpOASES {err.max():.3e}, iterations {interface.status_iters(s1).tolist()}")
    assert (interface.status_code(s1) == 0).all(), [(n, int(c)) for n, c in zip(b1.table_names, interface.status_code(s1)) if c]
    assert err.max() < TOL, (err.max(), b1.table_names[int(np.argmax(err))])
    assert np.all(forces[swing_mask(b1, np.arange(len(b1)))] == 0.0)


def solved(b):
    """One solve of the batch with margins and prediction behind it."""
    mpc = interface.BatchedMPC(DT, b.h, FMAX, len(b), contacts=b.nc)
    mpc.upload(b.rec)
    mpc.solve()
    forces, status = mpc.download()
    mpc.constraint_margins()
    m = mpc.download_margins()
    mpc.predict_states()
    states, cost = mpc.download_prediction()
    mpc.close()
    return forces, status, m, states, cost


_solved = {}


def solved_shape(h, nc):
    if (h, nc) not in _solved:
        _solved[(h, nc)] = solved(ig.cached(ig.hangs_batch, h, nc))
    return _solved[(h, nc)]


@pytest.mark.parametrize("h,nc", ig.HANGS_SHAPES)
def test_margins_on_irregular_tables_are_the_definition(oracle, h, nc):
    from test_gpu_margins import assert_is_the_definition

    b = ig.cached(ig.hangs_batch, h, nc)
    forces, status, m, _, _ = solved_shape(h, nc)
    assert (interface.status_code(status) == 0).all(), interface.status_code(status)
    assert m["slack"].shape == (len(b), h, nc, 10)
    assert_is_the_definition(m, mm.margins_records(oracle, b.rec, h, nc, forces), b.rec, h, nc, b.name)
    swing = b.tables.reshape(len(b), h, nc) == 0
    assert swing.any() and (~swing).any()
    pos_inf = np.isposinf(m["slack"])
    np.testing.assert_array_equal(pos_inf.all(axis=-1), swing)   # all ten slacks +inf exactly on the swing leg-steps ...
    np.testing.assert_array_equal(pos_inf.any(axis=-1), swing)   # ... and nowhere else
    assert np.isfinite(m["slack"][~swing]).all()
    # where: 10 (nc step + contact) + j of a STANCE leg-step (every instance here has one, so there is always a candidate for the
    # classes 0 .. 4; class 5 may have none: -1)
    where = m["where"]
    assert (where[:, :5] >= 0).all() and (where >= -1).all() and (where < 10 * nc * h).all()
    for i in range(len(b)):
        for c in range(6):
            if where[i, c] >= 0:
                assert b.tables[i][where[i, c] // 10] == 1, (b.table_names[i], c, where[i, c])


@pytest.mark.parametrize("h,nc", ig.HANGS_SHAPES)
def test_prediction_on_irregular_tables_is_the_definition(oracle, h, nc):
    b = ig.cached(ig.hangs_batch, h, nc)
    forces, status, _, states, cost = solved_shape(h, nc)
    assert (interface.status_code(status) == 0).all(), interface.status_code(status)
    assert states.shape == (len(b), h, 13) and cost.shape == (len(b), 2)
    ref_states, ref_cost = pm.predict_records(oracle, b.rec, h, nc, forces)
    x0g = np.array([oracle.assemble_record(r, h, DT, FMAX, reduce=False, nc=nc)["x0"][12] for r in b.rec], dtype=np.float32)
    pm.assert_matches_definition(states, cost, ref_states, ref_cost, x0g)
    assert (cost > 0).all()
