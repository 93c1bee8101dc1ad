"""Irregular gait tables: caller data the four periodic gaits of ``synthetic.make_batch`` never produce.

Everything the solve is sized and indexed by comes from the gait table (the prefix counts of stance leg-steps, the swing elimination,
``var_ind``, the scatter, the kernel variant an instance runs on, the number of pivot steps and tiles of the block start), and the C ABI
accepts any ``gait[]``.  This module builds such tables -- k stance leg-steps at random positions, random densities, a set of pinned
edge tables -- and the batches the tests of ``test_irregular_gaits.py`` (CPU) and ``test_gpu_irregular_gaits.py`` (GPU) share.
Deterministic from ``(h, nc, seed)`` through ``numpy.random.default_rng``.  The body state, feet and trajectory are those of
``make_batch(..., "standing", yaw_rate_cmd=True)`` at the nominal ranges, so that a failure is an indexing failure and not a conditioning
one.  A table is an int32 array ``[nc * h]``, entry ``[nc * step + contact]``, 1 = stance; a reduced QP has n = 6 x (stance leg-steps)
variables.  Instances without any stance leg-step (n = 0: nothing to hand to qpOASES, the answer is all zeros) come from ``all_swing``
alone."""
import numpy as np

from hector_simulation_amd import records, synthetic


# ------------------------------------------------------------------------------------------------ tables
def exact_count(h, nc, k, rng):
    """k stance leg-steps at random positions."""
    assert 0 <= k <= nc * h
    t = np.zeros(nc * h, dtype=np.int32)
    t[rng.choice(nc * h, size=k, replace=False)] = 1
    return t


def random_density(h, nc, nb, rng):
    """nb tables, each leg-step in stance with a probability drawn per instance from [0.15, 0.95]; an empty row is redrawn (n >= 6)."""
    out = np.zeros((nb, nc * h), dtype=np.int32)
    for i in range(nb):
        while not out[i].any():
            out[i] = rng.random(nc * h) < rng.uniform(0.15, 0.95)
    return out


def all_swing(h, nc):
    """No stance leg-step at all: n = 0.  The one table that is checked against zeros instead of qpOASES."""
    return np.zeros(nc * h, dtype=np.int32)


def pinned_edges(h, nc):
    """[(name, table)]: the edge tables.  Contact 0 / 1 = left / right foot, 2 = the hand (which swings unless the name says otherwise)."""
    def table(fill=0):
        return np.full((h, nc), fill, dtype=np.int32)

    out = []
    t = table()
    t[0, 0] = 1
    out.append(("lone_leg_step_at_step_0", t))            # n = 6
    t = table()
    t[h - 1, nc - 1] = 1
    out.append(("lone_leg_step_at_the_last_step", t))     # n = 6, every prefix count before it 0
    t = table()
    t[h - 1, :] = 1
    out.append(("stance_at_the_last_step_only", t))
    if h >= 2:
        t = table(1)
        t[0, :] = 0
        out.append(("flight_at_step_0", t))
    if h >= 3:
        t = table(1)
        t[h // 2, :] = 0
        out.append(("flight_in_the_middle", t))
    t = table()
    t[: h // 2, 0] = 1
    t[h // 2:, 1] = 1
    out.append(("left_only_then_right_only", t))
    t = table()
    t[0::4, 0] = 1
    t[2::4, 1] = 1
    out.append(("alternating_single_support_with_flight_between", t))
    t = table(1)
    t[h // 2, 1] = 0
    out.append(("full_stance_except_one_leg_step", t))
    if nc == 3:
        t = table()
        t[:, 2] = 1
        out.append(("hand_is_the_only_contact_in_stance", t))
    assert all(t.any() for _, t in out)
    return [(name, t.reshape(nc * h)) for name, t in out]


def stance_count(tables):
    return np.asarray(tables).reshape(len(tables), -1).sum(axis=1)


# ------------------------------------------------------------------------------------------------ field dicts
def fields(h, nc, tables, seed):
    """The field dict of ``make_batch`` (nc = 2) / ``make_batch3`` (nc = 3, hand fields of the same seed) with ``gait`` replaced."""
    tables = np.asarray(tables, dtype=np.int32).reshape(-1, nc * h)
    nb = tables.shape[0]
    f = synthetic.make_batch(nb, h, "standing", seed=seed, yaw_rate_cmd=True)
    if nc == 3:
        f3 = synthetic.make_batch3(nb, h, "standing", seed=seed, hand="contact")
        for key in ("p", "v", "q", "w", "joint_angles"):
            assert np.array_equal(f3[key], f[key])  # same seed -> same body and feet
        f3["traj"] = f["traj"]
        f = f3
    f["gait"] = tables.copy()
    return f


def pack(f, h, nc):
    return records.pack_records(f, h, nc)


def rows(f, idx):
    return {k: np.asarray(v)[idx] for k, v in f.items()}


def seed_of(h, nc, salt):
    return 1600 + 97 * salt + 7 * h + nc


# ------------------------------------------------------------------------------------------------ the batches of the tests
class Batch:
    """name, h, nc, table names [nb], tables [nb, nc h], fields, records; ``zero`` [nb] bool: the explicit n = 0 rows."""

    def __init__(self, name, h, nc, named_tables, seed):
        self.name, self.h, self.nc = name, h, nc
        self.table_names = [n for n, _ in named_tables]
        self.tables = np.stack([t for _, t in named_tables]).astype(np.int32)
        self.fields = fields(h, nc, self.tables, seed)
        self.rec = pack(self.fields, h, nc)
        self.k = stance_count(self.tables)
        self.n = 6 * self.k
        self.zero = np.array([n == "all_swing" for n in self.table_names])

    def __len__(self):
        return len(self.table_names)


def assembly_batch(h, nc):
    """Part a: the pinned edges, and exact counts around the sizes where the variants and the pivot blocks change."""
    rng = np.random.default_rng(seed_of(h, nc, 1))
    named = pinned_edges(h, nc)
    ks = {(10, 2): (1, 9, 10, 11, 19, 20), (20, 2): (10, 11, 20, 21, 39, 40), (10, 3): (1, 15, 29, 30)}.get((h, nc), ())
    named += [(f"exact_{k}", exact_count(h, nc, k, rng)) for k in ks]
    return Batch(f"assembly_h{h}_c{nc}", h, nc, named, seed_of(h, nc, 1))


ASSEMBLY_SHAPES = [(1, 2), (2, 2), (3, 2), (10, 2), (11, 2), (19, 2), (20, 2), (10, 3)]


def sizes_batch(h, nc):
    """Part b: two instances of every size k = 1 .. nc h."""
    rng = np.random.default_rng(seed_of(h, nc, 2))
    named = [(f"exact_{k}_{j}", exact_count(h, nc, k, rng)) for k in range(1, nc * h + 1) for j in range(2)]
    return Batch(f"sizes_h{h}_c{nc}", h, nc, named, seed_of(h, nc, 2))


SIZES_SHAPES = [(10, 2), (20, 2), (10, 3)]


def horizon_batch(h):
    """Part c: 8 random densities, the pinned edges and the explicit all-swing instance at one horizon."""
    rng = np.random.default_rng(seed_of(h, 2, 3))
    named = [(f"density_{j}", t) for j, t in enumerate(random_density(h, 2, 8, rng))] + pinned_edges(h, 2)
    named.append(("all_swing", all_swing(h, 2)))
    return Batch(f"horizon_h{h}", h, 2, named, seed_of(h, 2, 3))


BORDER_SIZES = {20: (54, 60, 66, 114, 120, 126, 132), 10: (54, 60, 66, 120)}


def border_batch(h):
    """Part d: two irregular tables of every size either side of a class border, interleaved (size varies fastest)."""
    rng = np.random.default_rng(seed_of(h, 2, 4))
    named = [(f"exact_{n // 6}_{j}", exact_count(h, 2, n // 6, rng)) for j in range(2) for n in BORDER_SIZES[h]]
    return Batch(f"borders_h{h}", h, 2, named, seed_of(h, 2, 4))


def border_ticks(h=10):
    """Part d, through the record builder: ticks whose random offsets and durations give the sizes of ``BORDER_SIZES[h]`` (the
    generator's tables are one stance window per leg, cyclic: leg j is in stance for min(duration_j, h) steps)."""
    sizes = BORDER_SIZES[h]
    nb = 2 * len(sizes)
    rng = np.random.default_rng(seed_of(h, 2, 5))
    t = synthetic.make_ticks(nb, h, "walking", seed=seed_of(h, 2, 5))
    for i in range(nb):
        k = sizes[i % len(sizes)] // 6
        d0 = int(rng.integers(max(0, k - h), min(h, k) + 1))
        t["gait_durations"][i] = (d0, k - d0)
        t["gait_offsets"][i] = rng.integers(0, h, size=2)
        t["gait_iteration"][i] = rng.integers(0, h)
    return t, np.array([sizes[i % len(sizes)] for i in range(nb)])


def hangs_batch(h=10, nc=2):
    """Part e: the pinned edges plus 8 random densities (h = 10, two contacts); 6 irregular instances for the other shapes."""
    rng = np.random.default_rng(seed_of(h, nc, 6))
    if (h, nc) == (10, 2):
        named = pinned_edges(h, nc) + [(f"density_{j}", t) for j, t in enumerate(random_density(h, nc, 8, rng))]
    else:
        edges = dict(pinned_edges(h, nc))
        pick = ["flight_in_the_middle", "alternating_single_support_with_flight_between",
                "hand_is_the_only_contact_in_stance" if nc == 3 else "lone_leg_step_at_the_last_step"]
        named = [(n, edges[n]) for n in pick] + [(f"density_{j}", t) for j, t in enumerate(random_density(h, nc, 3, rng))]
    return Batch(f"hangs_h{h}_c{nc}", h, nc, named, seed_of(h, nc, 6))


HANGS_SHAPES = [(10, 2), (20, 2), (10, 3)]
WARM_SHIFTS = (0, 1, 3)


def second_tick(b, shift):
    """The batch one tick later (``synthetic.advance_tick``), its tables those of ``b`` advanced by ``shift`` steps with fresh random
    leg-steps entering at the end; a row that would come out empty keeps its last leg-step in stance (n >= 6)."""
    h, nc = b.h, b.nc
    rng = np.random.default_rng(seed_of(h, nc, 7) + shift)
    old = b.tables.reshape(len(b), h, nc)
    new = np.zeros_like(old)
    new[:, : h - shift] = old[:, shift:]
    if shift:
        new[:, h - shift:] = rng.random((len(b), shift, nc)) < 0.5
    for i in range(len(b)):
        if not new[i].any():
            new[i, h - 1, nc - 1] = 1
    f = synthetic.advance_tick(b.fields, h, seed=seed_of(h, nc, 7) + shift)
    f["gait"] = new.reshape(len(b), nc * h)
    out = Batch.__new__(Batch)
    out.name, out.h, out.nc = f"{b.name}_tick2_shift{shift}", h, nc
    out.table_names = [f"{n}_shift{shift}" for n in b.table_names]
    out.tables, out.fields, out.rec = f["gait"], f, pack(f, h, nc)
    out.k = stance_count(out.tables)
    out.n = 6 * out.k
    out.zero = np.zeros(len(b), dtype=bool)
    return out


def sweep_batch(b, k=3):
    """Part e, command sweep: every instance of ``b`` under k velocity / yaw-rate commands (groups of k consecutive records that share
    state and table and differ in the reference trajectory, rebuilt per command as ``make_batch`` builds it)."""
    h = b.h
    f = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in b.fields.items()}
    nb = len(b) * k
    rng = np.random.default_rng(seed_of(h, b.nc, 8))
    vx, vy, yr = rng.uniform(-0.5, 0.5, nb), rng.uniform(-0.2, 0.2, nb), rng.uniform(-0.3, 0.3, nb)
    tr = f["traj"].reshape(nb, h, 12).copy()
    steps = np.arange(h)[None, :]
    tr[:, :, 9], tr[:, :, 10], tr[:, :, 8] = vx[:, None], vy[:, None], yr[:, None]
    tr[:, :, 3] = f["p"][:, 0:1] + steps * synthetic.DT_MPC * vx[:, None]
    tr[:, :, 4] = f["p"][:, 1:2] + steps * synthetic.DT_MPC * vy[:, None]
    tr[:, 1:, 2] = tr[:, 0:1, 2] + steps[:, 1:] * synthetic.DT_MPC * yr[:, None]
    f["traj"] = tr.reshape(nb, 12 * h)
    out = Batch.__new__(Batch)
    out.name, out.h, out.nc = f"{b.name}_sweep{k}", h, b.nc
    out.table_names = [n for n in b.table_names for _ in range(k)]
    out.tables, out.fields, out.rec = f["gait"], f, pack(f, h, b.nc)
    out.k = stance_count(out.tables)
    out.n = 6 * out.k
    out.zero = np.zeros(nb, dtype=bool)
    return out


_batches = {}


def cached(fn, *args):
    """One construction per batch and session; the batches are shared and left unchanged."""
    key = (fn.__name__,) + args
    if key not in _batches:
        _batches[key] = fn(*args)
    return _batches[key]


def warm_second(shift):
    return second_tick(cached(hangs_batch, 10, 2), shift)


def hangs_sweep():
    return sweep_batch(cached(hangs_batch, 10, 2), 3)


def solved_batches():
    """Every batch a GPU test compares with qpOASES, as (constructor, args): what the CPU test asks qpOASES to solve beforehand."""
    out = [(sizes_batch, s) for s in SIZES_SHAPES]
    out += [(horizon_batch, (h,)) for h in range(1, 21)]
    out += [(border_batch, (h,)) for h in (20, 10)]
    out += [(hangs_batch, s) for s in HANGS_SHAPES]
    out += [(warm_second, (s,)) for s in WARM_SHIFTS]
    out += [(hangs_sweep, ())]
    return out
