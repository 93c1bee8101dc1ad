"""Irregular gait tables for the result kernels: what hangs off a solve beyond margins and prediction -- the KKT certificate, the feedback
gains and the first-order wrench, the adjoint, the model / limit / pose gradients, the multi-seed adjoint and its chain.

Built on ``irregular_gaits`` (its tables, its ``fields`` at the nominal ranges: a failure is an indexing failure), deterministic from
``(h, nc, seed)``.  Each batch is also a case tuple ``(name, "irregular", h, nb, nc, seed)`` of the shape of ``prediction_mirror.SHAPES``,
and ``reference_case`` below enters it into ``test_certificate_mirror`` through that module's ``enter_case``: from then on ``mirror_case``,
``fd_case``, ``adjoint_case``, ``model_case`` ... of the other mirrors' tests take the tuple unchanged.  The one thing those helpers cannot
do is hand an instance without any stance leg-step (``all_swing``, n = 0) to qpOASES: its answer is all zeros by definition
(include/hector_mpc.h), and ``EmptyAware`` wraps the oracle so that ``solve_records`` returns exactly that for such rows.

Batches (<= 16 instances; the three-contact h = 4 one holds all nine pinned edges that exist there):

1. h = 10, nc = 2: the pinned edges, 6 random densities, all_swing;
2. h = 20, nc = 2: flight in the middle, alternating single support with flight between, a lone leg-step at the last step, full stance
   except one leg-step, exactly 21 and 40 stance leg-steps (40 = full double support, the wide variant's largest QP), 2 densities;
3. h = 13, nc = 2: full stance (behind a wide solve, below HMAX), flight at step 0, 2 densities;
4. h = 10, nc = 3: the hand as the only contact (over the first half, flight after it), left only then right only (hand swinging), flight
   in the middle, full stance, all_swing, 3 densities;
5. h = 4, nc = 3: the pinned edges;
6. h = 1, one stance leg-step: each contact alone, for nc = 2 and nc = 3."""
import numpy as np

import certificate_mirror as cm
import feedback_mirror as fm
import irregular_gaits as ig
import limit_adjoint_mirror as lam
from hector_simulation_amd import records, synthetic

DT, FMAX = synthetic.DT_MPC, synthetic.F_MAX
SALT = 12   # (the first salt from 11 on at which the multiplier check against qpOASES' duals leaves out no leg-step of any batch)


def _named(edges, names):
    return [(n, edges[n]) for n in names]


def _full(h, nc):
    return np.ones(nc * h, dtype=np.int32)


def _densities(h, nc, nb, rng):
    return [(f"density_{j}", t) for j, t in enumerate(ig.random_density(h, nc, nb, rng))]


def hand_alone_then_flight(h, nc):
    """The hand as the only contact in stance over the first half of the horizon, flight after it.  (With the hand alone in stance to
    the last step -- ``hand_is_the_only_contact_in_stance`` of irregular_gaits -- qpOASES unloads the hand over the last steps under
    every seed tried: eight active limits of rank 5, whose multipliers are not unique, so that the multiplier check against qpOASES'
    duals could not keep its cap of 0 left-out leg-steps.  The h = 4 batch keeps that table; the unloaded contact beside swinging ones
    comes back through crafted forces.)"""
    t = np.zeros((h, nc), dtype=np.int32)
    t[: h // 2, 2] = 1
    return t.reshape(nc * h)


def derived_batch(h, nc):
    """The batch of one shape (see the module's list)."""
    seed = ig.seed_of(h, nc, SALT)
    rng = np.random.default_rng(seed)
    edges = dict(ig.pinned_edges(h, nc))
    if (h, nc) == (10, 2):
        named = ig.pinned_edges(h, nc) + _densities(h, nc, 6, rng) + [("all_swing", ig.all_swing(h, nc))]
    elif (h, nc) == (20, 2):
        named = _named(edges, ["flight_in_the_middle", "alternating_single_support_with_flight_between", "lone_leg_step_at_the_last_step",
                               "full_stance_except_one_leg_step"])
        named += [(f"exact_{k}", ig.exact_count(h, nc, k, rng)) for k in (21, 40)] + _densities(h, nc, 2, rng)
    elif (h, nc) == (13, 2):
        named = [("full_stance", _full(h, nc)), ("flight_at_step_0", edges["flight_at_step_0"])] + _densities(h, nc, 2, rng)
    elif (h, nc) == (10, 3):
        named = [("hand_is_the_only_contact_in_stance_then_flight", hand_alone_then_flight(h, nc))]
        named += _named(edges, ["left_only_then_right_only", "flight_in_the_middle"])
        named += [("full_stance", _full(h, nc)), ("all_swing", ig.all_swing(h, nc))] + _densities(h, nc, 3, rng)
    elif (h, nc) == (4, 3):
        named = ig.pinned_edges(h, nc)
    elif h == 1:
        named = [(f"contact_{c}_alone", np.eye(nc, dtype=np.int32)[c]) for c in range(nc)]
    else:
        raise ValueError((h, nc))
    return ig.Batch(f"irr_h{h}_c{nc}", h, nc, named, seed)


SHAPES = [(10, 2), (20, 2), (13, 2), (10, 3), (4, 3), (1, 2), (1, 3)]   # batches 1 .. 5, and the two of batch 6
NO_STANCE_AT_STEP_0 = ("flight_at_step_0", "lone_leg_step_at_the_last_step", "stance_at_the_last_step_only", "all_swing")
WIDE_SHAPES = [(20, 2), (13, 2)]                 # behind the wide variant: a batch whose widest QP has more than 120 variables
FIRST_ORDER_SHAPES = [(10, 2), (20, 2), (10, 3)]  # batches 1, 2, 4
RE_SOLVE_SHAPES = [(10, 2), (13, 2), (10, 3)]     # batches 1, 3, 4
CRAFTED_SHAPES = [(10, 2), (10, 3)]               # condition (f) through crafted forces
MULTI_SHAPES = [(10, 2), (20, 2), (10, 3), (4, 3)]  # batches 1, 2, 4, 5


def batch_of(h, nc):
    return ig.cached(derived_batch, h, nc)


def case_of(h, nc):
    """(name, "irregular", h, nb, nc, seed): a case tuple of the other mirrors' kind."""
    b = batch_of(h, nc)
    return (b.name, "irregular", h, len(b), nc, ig.seed_of(h, nc, SALT))


CASES = [case_of(h, nc) for h, nc in SHAPES]
CASE_IDS = [c[0] for c in CASES]
BY_SHAPE = {(c[2], c[4]): c for c in CASES}


def batch_of_case(case):
    return batch_of(case[2], case[4])


class EmptyAware:
    """The oracle with ``solve_records`` extended to instances without a stance leg-step: all zeros, objective 0, never handed to qpOASES
    (the header's answer for n = 0).  Everything else is the oracle's own."""

    def __init__(self, oracle):
        self._oracle = oracle

    def __getattr__(self, key):
        return getattr(self._oracle, key)

    def qpoases_solve(self, H, g, A, lb, ub, **kw):
        if np.asarray(g).size == 0:
            return np.zeros(0), np.zeros(np.asarray(lb).size), 0.0, 0, 0
        return self._oracle.qpoases_solve(H, g, A, lb, ub, **kw)

    def solve_records(self, rec, h, dt, f_max, nc=2, **kw):
        assert not kw
        rec = np.ascontiguousarray(rec)
        keep = np.flatnonzero(np.asarray(records.unpack_records(rec, h, nc)["gait"]).reshape(rec.shape[0], -1).any(axis=1))
        r = self._oracle.solve_records(np.ascontiguousarray(rec[keep]), h, dt, f_max, nc=nc)
        nb = rec.shape[0]
        q, obj, nwsr, bad = np.zeros((nb, 6 * nc * h)), np.zeros(nb), np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=bool)
        q[keep], obj[keep], nwsr[keep], bad[keep] = r["q_soln"], r["obj"], r["nwsr"], r["bad"]
        return dict(q_soln=q, nwsr=nwsr, obj=obj, n_bad=r["n_bad"], bad=bad, t_assemble=r["t_assemble"], t_solve=r["t_solve"])


def aware(oracle):
    return oracle if isinstance(oracle, EmptyAware) else EmptyAware(oracle)


LEFT_OUT_CAP = 0.0   # the multiplier check against qpOASES' duals leaves out nothing: these shapes are regular in all but the table
# the groups of limit_adjoint_mirror.GROUPS with at least one admitted active row at qpOASES' forces, counted on the CPU
# (tests/test_derived_irregular_mirror.py asserts the count)
LIMIT_COVERS = dict(irr_h10_c2="mu lt lh cap", irr_h20_c2="mu lt lh cap", irr_h13_c2="lt lh", irr_h10_c3="mu lt lh cap", irr_h4_c3="mu lt",
                    irr_h1_c2="mu", irr_h1_c3="mu lh")


def limit_groups(name):
    return lam.cover(name, LIMIT_COVERS[name])


def reference_case(oracle, case):
    """``test_certificate_mirror.reference_case`` for a case of this module: the same dict, built once and entered there under the
    case's name through ``enter_case`` (an all_swing row: zero forces and multipliers, no QP handed over), with the groups the limit
    gradients' tests must find covered; left unchanged."""
    import test_certificate_mirror as tcm

    name, h, nb, nc = case[0], case[2], case[3], case[4]

    def build():
        b = batch_of_case(case)
        assert b.name == name and len(b) == nb
        u32, y = np.zeros((nb, h, 6 * nc), dtype=np.float32), np.zeros((nb, h, nc, 10))
        for k in range(nb):
            if not b.zero[k]:
                u, y[k] = cm.qpoases_primal_dual(oracle, b.rec[k], h, nc)
                u32[k] = u.astype(np.float32)
        return dict(rec=b.rec, u32=u32, y=y, m=cm.certificate_records(oracle, b.rec, h, nc, u32, with_bounds=True))

    limit_groups(name)
    return tcm.enter_case(name, build, LEFT_OUT_CAP)


# ------------------------------------------------------------------------------------------------ coverage conditions
def normals_held(m, k, i, c):
    """The number of normals the mirror admits on stance leg-step (i, c) of instance k (6 - the free directions of the leg-step)."""
    return fm.free_directions(m["N"][k][c], m["active"][k][(i, c)])[0]


def coverage(m, nc):
    """Which of the conditions a .. f of the module's tests the steps of one mirrored batch (feedback_mirror.gains_records) meet:
    {letter: count of steps}."""
    n = dict.fromkeys("abcdef", 0)
    n["a0"] = n["a1"] = 0
    stance = m["stance"]
    nb, h = stance.shape[:2]
    for k in range(nb):
        r = [int(stance[k, i].any()) for i in range(h)]
        for i in range(h):
            st = stance[k, i]
            held = [normals_held(m, k, i, c) if st[c] else -1 for c in range(nc)]
            if nc == 2:
                if not st[0] and st[1] and 1 <= held[1] <= 5:
                    n["a0"] += 1
                if st[0] and not st[1] and 1 <= held[0] <= 5:
                    n["a1"] += 1
            if not r[i] and any(r[:i]) and any(r[i + 1:]):
                assert m["free_dims"][k, i] == 0
                n["b"] += 1
            if nc == 3:
                if not st[0] and not st[1] and st[2] and 1 <= held[2] <= 5:
                    n["c"] += 1
                if not st[0] and st[1] and st[2]:
                    n["d"] += 1
                if not st[2] and any(st[c] and held[c] >= 1 for c in range(2)):
                    n["e"] += 1
            for c in range(nc):
                if st[c] and not st.all():
                    act = m["active"][k][(i, c)]
                    if len(act) >= 6 and np.linalg.matrix_rank(m["N"][k][c][:, act], tol=1e-9) < 6:
                        n["f"] += 1
    n["a"] = min(n.pop("a0"), n.pop("a1"))
    return n


def unloaded_beside_a_swing(forces, tables, h, nc):
    """Crafted forces: at the first step of every instance where a stance leg-step stands beside a swing one, all six forces of the
    first stance contact are 0 (rows 0-4, 6, 7, 8 active, of rank 5).  Returns (forces [nb, h, 6 nc] float32, [(k, i, c)] crafted)."""
    out = np.array(forces, dtype=np.float32).reshape(len(tables), h, 6 * nc).copy()
    where = []
    for k, t in enumerate(np.asarray(tables).reshape(len(tables), h, nc)):
        for i in range(h):
            if t[i].any() and not t[i].all():
                c = int(np.flatnonzero(t[i])[0])
                out[k, i, cm.cols(c, nc)] = 0.0
                where.append((k, i, c))
                break
    return out, where
