"""Where every result derived from a solve goes and how much of it a download copies: what tests/test_gpu_handle_buffers.py checks for
outputs, prediction and selection, for margins, certificate, gains, first-order wrench, adjoint, model, limit and record gradients, the
multi-seed adjoint and its chain.

Shapes: max_batch 5, batch 3, horizon 3, two and three contacts -- batch != max_batch, and the horizon differs from the contacts and from
every fixed dimension of a row (2, 3 + nc, 4, 6, 9, 10, 12, 13, 26 ...), so an array copied or allocated at another array's size shows: in
the guard elements round a caller's buffer, in the rows behind the batch, or in the tail behind a host array.  Every comparison is bit for
bit against the same handle's first run in its own buffers; the row shapes are tests/stream_cases.py's, written down independently of the
library's tables."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc
from hector_simulation_amd import _lib, interface, records, synthetic
from test_gpu_adjoint_chain import SOURCE
from test_gpu_adjoint_multi import chain_behind

pytestmark = pytest.mark.gpu
MB, NB, HZ, S = 5, 3, 3, 2
GUARD = 64
E_ARG, OK = -1, 0
SENT = {4: np.uint32(0xA5C3F00D), 8: np.uint64(0x7FF4DEADBEEF5A5A)}  # (as binary64 a NaN with a payload: no kernel computes it)
FAMILIES = ("prediction", "margins", "certificate", "gains", "first_order", "adjoint", "adjoint_model", "adjoint_limits", "adjoint_record")
NO_GET = ("first_order",)  # (the library exports no hmpc_get_device_first_order)


def uint(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(uint(got[k]), uint(want[k]), err_msg=f"{what}: {k}")


class Case:
    """a fresh handle of max_batch MB holding NB records, and the device-resident inputs of the chain"""

    def __init__(self, nc):
        f = synthetic.make_batch3(NB, HZ, "standing", seed=411) if nc == 3 else synthetic.make_batch(NB, HZ, "walking", seed=412, phase="random")
        self.nc, self.rec = nc, records.pack_records(f, HZ, nc)
        later = self.rec if nc == 3 else records.pack_records(synthetic.advance_tick(f, HZ, seed=3), HZ, nc)
        self.later = sc.device(later)
        self.seeds = sc.device(np.stack([sc.am.seeds(NB, HZ, 6 * nc, rng_seed=40 + s) for s in range(S)]))
        self.rows = sc.rows(nc, HZ)
        self.m = interface.BatchedMPC(synthetic.DT_MPC, HZ, synthetic.F_MAX, MB, contacts=nc)
        sc.torch_().cuda.synchronize()

    def seed(self, s=0):
        return self.seeds[s].data_ptr()

    def launch(self, fam):
        m = self.m
        {"prediction": m.predict_states, "margins": m.constraint_margins, "certificate": m.kkt_certificate, "gains": m.feedback_gains,
         "first_order": lambda: m.first_order_wrench(self.later.data_ptr()), "adjoint": lambda: m.solve_adjoint(self.seed()),
         "adjoint_model": m.adjoint_model, "adjoint_limits": lambda: m.adjoint_limits(self.seed()), "adjoint_record": m.adjoint_record}[fam]()

    def raw_launch(self, fam):
        """the family's enqueuing entry, its return code"""
        L, h, vp = self.m.L, self.m.h, C.c_void_p
        return {"prediction": lambda: L.hmpc_predict_states(h, None), "margins": lambda: L.hmpc_constraint_margins(h, None),
                "certificate": lambda: L.hmpc_kkt_certificate(h, None), "gains": lambda: L.hmpc_feedback_gains(h, None),
                "first_order": lambda: L.hmpc_first_order_wrench(h, vp(self.later.data_ptr()), None),
                "adjoint": lambda: L.hmpc_solve_adjoint(h, vp(self.seed()), None), "adjoint_model": lambda: L.hmpc_adjoint_model(h, None),
                "adjoint_limits": lambda: L.hmpc_adjoint_limits(h, vp(self.seed()), None),
                "adjoint_record": lambda: L.hmpc_adjoint_record(h, None)}[fam]()

    def solve(self, upload=True):
        if upload:
            self.m.upload(self.rec)
        self.m.solve()
        self.m.download()  # (the safe pass, should the fast one have flagged anything)

    def chain(self):
        for fam in FAMILIES:
            self.launch(fam)
        sc.torch_().cuda.synchronize()

    def host(self, fam, rows=NB, tail=0, lead=()):
        """sentinel-filled host arrays of the family, `rows` rows each and `tail` elements behind them (flat)"""
        out = {}
        for k, (dt, shape) in self.rows[fam].items():
            n = int(np.prod(lead + (rows,) + tuple(shape), dtype=np.int64)) + tail
            out[k] = np.full(n, SENT[np.dtype(dt).itemsize]).view(dt)
        return out

    def shaped(self, fam, flat, rows=NB, lead=()):
        out = {}
        for k, (dt, shape) in self.rows[fam].items():
            full = lead + (rows,) + tuple(shape)
            out[k] = flat[k][:int(np.prod(full, dtype=np.int64))].reshape(full)
        return out

    def raw_download(self, fam, dst):
        """hmpc_download_<family> into dst (name -> host array or None), its return code"""
        args = [None if dst.get(k) is None else C.c_void_p(dst[k].ctypes.data) for k in self.rows[fam]]
        return getattr(self.m.L, "hmpc_download_" + fam)(self.m.h, *args)

    def download(self, fam):
        """the family through the raw entry, into arrays of exactly NB rows and a sentinel tail that must stay"""
        flat = self.host(fam, tail=GUARD)
        assert self.raw_download(fam, flat) == OK, fam
        for k, a in flat.items():
            assert (uint(a)[-GUARD:] == SENT[a.dtype.itemsize]).all(), f"{fam}.{k}: the download wrote behind {NB} rows"
            assert not (uint(a)[:-GUARD] == SENT[a.dtype.itemsize]).all(), f"{fam}.{k}: the download copied nothing"
        return self.shaped(fam, flat)

    def download_all(self):
        return {fam: self.download(fam) for fam in FAMILIES}

    def set(self, fam, ptrs):
        interface._check(getattr(self.m.L, "hmpc_set_device_" + fam)(self.m.h, *[C.c_void_p(int(ptrs.get(k) or 0)) for k in self.rows[fam]]),
                         "hmpc_set_device_" + fam)

    def get(self, fam):
        p = [C.c_void_p() for _ in self.rows[fam]]
        interface._check(getattr(self.m.L, "hmpc_get_device_" + fam)(self.m.h, *[C.byref(x) for x in p]), "hmpc_get_device_" + fam)
        return {k: int(x.value or 0) for k, x in zip(self.rows[fam], p)}

    def get_all(self):
        return {fam: self.get(fam) for fam in FAMILIES if fam not in NO_GET}


class Guarded:
    """`rows` rows of a family's array inside a larger device tensor: GUARD sentinel elements on either side, the rows sentinel too"""

    def __init__(self, spec, rows):
        dt, shape = spec
        self.item = np.dtype(dt).itemsize
        self.n = rows * int(np.prod(shape, dtype=np.int64))
        self.t = sc.device(np.full(self.n + 2 * GUARD, SENT[self.item]).view({4: np.int32, 8: np.int64}[self.item]))
        self.ptr = self.t.data_ptr() + GUARD * self.item

    def check(self, used, want, what):
        """the first `used` elements hold want's bits, everything else the sentinel"""
        got = uint(self.t.cpu().numpy())
        assert (got[:GUARD] == SENT[self.item]).all() and (got[GUARD + self.n:] == SENT[self.item]).all(), f"{what}: a guard element was written"
        assert (got[GUARD + used:GUARD + self.n] == SENT[self.item]).all(), f"{what}: written behind the batch"
        np.testing.assert_array_equal(got[GUARD:GUARD + used], uint(want), err_msg=what)


@pytest.fixture(params=[2, 3], ids=["two_contacts", "three_contacts"])
def case(request):
    """every test its own fresh handle"""
    c = Case(request.param)
    yield c
    c.m.close()


# ------------------------------------------------------------------------------------------------ 1. guards, before anything else runs
def test_guards_fire_before_a_parent_exists_and_after_a_retarget(case):
    c, L, h = case, case.m.L, case.m.h
    none = {fam: {k: None for k in c.rows[fam]} for fam in FAMILIES}
    pen = sc.sentinel(MB * 8)
    fl, ce = np.zeros(6), np.zeros(3)
    penalty = {"margins": lambda: L.hmpc_margin_penalty(h, fl.ctypes.data, None, C.c_void_p(pen.data_ptr()), None),
               "certificate": lambda: L.hmpc_certificate_penalty(h, ce.ctypes.data, None, C.c_void_p(pen.data_ptr()), None),
               "prediction": lambda: L.hmpc_sweep_select(h, 1, None, None)}
    # batch == 0 (nothing uploaded): a launch asks for its parent first, a download for the batch first; the selection has no such shortcut
    assert c.m.batch == 0
    for fam in FAMILIES:
        assert c.raw_launch(fam) == E_ARG and c.raw_download(fam, none[fam]) == OK, fam
    assert all(f() == E_ARG for f in penalty.values())
    assert L.hmpc_download_selection(h, *[None] * 5) == E_ARG
    assert L.hmpc_solve_adjoint_multi(h, C.c_void_p(c.seed()), S, None) == E_ARG and L.hmpc_download_adjoint_multi(h, *[None] * 6) == OK
    assert L.hmpc_adjoint_chain_multi(h, C.c_void_p(c.seed()), None) == E_ARG and L.hmpc_download_adjoint_chain_multi(h, None) == OK
    # a batch, no solve: nothing has a parent
    c.m.upload(c.rec)
    for fam in FAMILIES:
        assert c.raw_launch(fam) == E_ARG and c.raw_download(fam, none[fam]) == E_ARG, fam
    assert all(f() == E_ARG for f in penalty.values())
    # a solve: every download before its launch, every launch before its parent's
    c.solve(upload=False)
    behind = {"prediction": "solve", "margins": "solve", "certificate": "solve", "gains": "solve", "first_order": "gains", "adjoint": "solve",
              "adjoint_model": "adjoint", "adjoint_limits": "adjoint", "adjoint_record": "adjoint_limits"}
    for fam in FAMILIES:
        assert c.raw_download(fam, none[fam]) == E_ARG, fam
        for child in FAMILIES:
            if behind[child] == fam or (child == "adjoint_record" and fam in ("adjoint", "adjoint_model")):
                assert c.raw_launch(child) == E_ARG, (fam, child)
        if fam in penalty:
            assert penalty[fam]() == E_ARG, fam
        c.launch(fam)
        assert c.raw_download(fam, none[fam]) == OK, fam
    assert L.hmpc_download_adjoint_multi(h, *[None] * 6) == E_ARG and L.hmpc_adjoint_chain_multi(h, C.c_void_p(c.seed()), None) == E_ARG
    assert L.hmpc_download_adjoint_chain_multi(h, None) == E_ARG and L.hmpc_download_selection(h, *[None] * 5) == E_ARG
    # hmpc_set_device_* moves a family: it and everything behind it is stale, nothing else is
    stale = {"prediction": (), "margins": (), "certificate": (), "gains": ("first_order",), "first_order": (),
             "adjoint": ("adjoint_model", "adjoint_limits", "adjoint_record"), "adjoint_model": ("adjoint_record",),
             "adjoint_limits": ("adjoint_record",), "adjoint_record": ()}
    for fam in FAMILIES:
        c.chain()
        c.set(fam, {})
        for other in FAMILIES:
            want = E_ARG if other == fam or other in stale[fam] else OK
            assert c.raw_download(other, none[other]) == want, (fam, other)
        for child in FAMILIES:
            if behind[child] == fam or (child == "adjoint_record" and fam in ("adjoint", "adjoint_model")):
                assert c.raw_launch(child) == E_ARG, (fam, child)
        if fam in penalty:
            assert penalty[fam]() == E_ARG, fam
    sc.torch_().cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. own, caller's, one of each, own again
def test_every_family_in_own_caller_mixed_and_own_buffers_again(case):
    c = case
    # (a) the handle's own buffers
    c.solve()
    c.chain()
    want = c.download_all()
    own = c.get_all()
    flat = [p for fam in own.values() for p in fam.values()]
    assert all(flat) and len(set(flat)) == len(flat), own
    # the wrappers of interface.py return the same arrays
    st, co = c.m.download_prediction()
    same_bits(dict(states=st, cost=co), want["prediction"], "download_prediction()")
    for fam, call in (("margins", c.m.download_margins), ("certificate", c.m.download_certificate), ("gains", c.m.download_gains),
                      ("first_order", c.m.download_first_order), ("adjoint", c.m.download_adjoint), ("adjoint_model", c.m.download_adjoint_model),
                      ("adjoint_limits", c.m.download_adjoint_limits), ("adjoint_record", c.m.download_adjoint_record)):
        got = call()
        same_bits({k: got[k].reshape(want[fam][k].shape) for k in want[fam]}, want[fam], f"download_{fam}()")
    # some destinations NULL: the others are filled
    for fam in FAMILIES:
        flat_ = c.host(fam)
        some = {k: (a if i % 2 else None) for i, (k, a) in enumerate(flat_.items())}
        assert c.raw_download(fam, some) == OK, fam
        got = c.shaped(fam, flat_)
        for i, k in enumerate(flat_):
            if i % 2:
                np.testing.assert_array_equal(uint(got[k]), uint(want[fam][k]), err_msg=f"{fam}.{k} beside NULL destinations")

    def run(buffers, what):
        """the whole chain into `buffers` (family -> array -> Guarded; what is missing is the handle's own)"""
        for fam in FAMILIES:
            c.set(fam, {k: g.ptr for k, g in buffers.get(fam, {}).items()})
        c.solve()
        c.chain()
        where = c.get_all()
        for fam in where:
            for k in c.rows[fam]:
                g = buffers.get(fam, {}).get(k)
                assert where[fam][k] == (g.ptr if g else own[fam][k]), f"{what}: hmpc_get_device_{fam} {k}"
        got = c.download_all()
        for fam in FAMILIES:
            same_bits(got[fam], want[fam], f"{what}: {fam}")
            for k, g in buffers.get(fam, {}).items():
                g.check(uint(want[fam][k]).size, want[fam][k], f"{what}: caller's {fam}.{k}")

    # (b) every array the caller's
    run({fam: {k: Guarded(spec, MB) for k, spec in c.rows[fam].items()} for fam in FAMILIES}, "caller's buffers")
    # (c) one array of every family the caller's, the rest the handle's own
    mixed = {}
    for i, fam in enumerate(FAMILIES):
        k = list(c.rows[fam])[i % len(c.rows[fam])]
        mixed[fam] = {k: Guarded(c.rows[fam][k], MB)}
    run(mixed, "one caller's buffer per family")
    # (d) NULL again: the pointers and the bits of (a)
    run({}, "own buffers again")


# ------------------------------------------------------------------------------------------------ 3. the per-seed families
def test_multi_seed_adjoint_and_chain_copy_seeds_times_batch_rows(case):
    c, m, L = case, case.m, case.m.L
    keys, ckeys = list(c.rows["adjoint"]), list(_lib.CHAIN_COMPACT + _lib.CHAIN_DETAIL)
    nf = records.N_FIXED3 if c.nc == 3 else records.N_FIXED
    f8 = np.float64
    chain_rows = {**c.rows["adjoint_chain"], **{k: c.rows["adjoint_model"][k] for k in ("grad_A", "grad_B", "grad_r", "costate")},
                  **{k: c.rows["adjoint_limits"][k] for k in ("grad_Fc", "grad_bound", "lambda", "nu")}}
    assert chain_rows["grad_record"] == (f8, (nf + 12 * HZ,)) and set(chain_rows) == set(ckeys)
    c.rows = dict(c.rows, chain_all={k: chain_rows[k] for k in ckeys})
    for fam in FAMILIES:
        c.set(fam, {})
    m.set_device_adjoint_multi(0)
    m.set_device_adjoint_chain_multi(0)
    c.solve()
    # the single-seed results under every seed
    single = []
    for s in range(S):
        m.solve_adjoint(c.seed(s))
        single.append(chain_behind(m, c.seed(s)))  # (adjoint, model, limit and record gradients, downloaded)

    def downloads(what, detail):
        flat = c.host("adjoint", tail=GUARD, lead=(S,))
        assert L.hmpc_download_adjoint_multi(m.h, *[C.c_void_p(flat[k].ctypes.data) for k in keys]) == OK
        fam = "chain_all" if detail else "adjoint_chain"
        cflat = c.host(fam, tail=GUARD, lead=(S,))
        assert L.hmpc_download_adjoint_chain_multi(m.h, C.byref(_lib.AdjointChain(**{k: a.ctypes.data for k, a in cflat.items()}))) == OK
        for k, a in {**flat, **{"chain " + k: a for k, a in cflat.items()}}.items():
            assert (uint(a)[-GUARD:] == SENT[8]).all(), f"{what}: {k} written behind {S} x {NB} rows"
        multi, chain = c.shaped("adjoint", flat, lead=(S,)), c.shaped(fam, cflat, lead=(S,))
        for s in range(S):
            for k in keys:
                np.testing.assert_array_equal(uint(multi[k][s]), uint(single[s][0][k]), err_msg=f"{what}: {k}, seed {s}")
            for k in chain:
                i, src = SOURCE[k]
                np.testing.assert_array_equal(uint(chain[k][s]), uint(single[s][i][src]), err_msg=f"{what}: chain {k}, seed {s}")

    # the handle's own buffers: compact arrays only
    m.solve_adjoint_multi(c.seeds.data_ptr(), S)
    m.adjoint_chain_multi(c.seeds.data_ptr())
    downloads("own buffers", detail=False)
    where = m.get_device_adjoint_chain_multi()
    assert where["n_seeds"] == S and all(where[k] for k in _lib.CHAIN_COMPACT) and not any(where[k] for k in _lib.CHAIN_DETAIL)
    # the caller's, S slices of max_batch rows each inside guards: hmpc_get_device_* names them, S x NB rows are written
    g = {k: Guarded(c.rows["adjoint"][k], S * MB) for k in keys}
    gc = {k: Guarded(chain_rows[k], S * MB) for k in ckeys}
    m.set_device_adjoint_multi(S, *[g[k].ptr for k in keys])
    m.set_device_adjoint_chain_multi(S, **{k + "_ptr": gc[k].ptr for k in ckeys})
    assert L.hmpc_download_adjoint_multi(m.h, *[None] * 6) == E_ARG and L.hmpc_download_adjoint_chain_multi(m.h, None) == E_ARG
    m.solve_adjoint_multi(c.seeds.data_ptr(), S)
    m.adjoint_chain_multi(c.seeds.data_ptr())
    sc.torch_().cuda.synchronize()
    got = m.get_device_adjoint_multi()
    assert got["n_seeds"] == S and all(got[k] == g[k].ptr for k in keys), got
    got = m.get_device_adjoint_chain_multi()
    assert got["n_seeds"] == S and all(got[k] == gc[k].ptr for k in ckeys), got
    downloads("caller's buffers", detail=True)
    for k in keys:
        want = np.stack([single[s][0][k] for s in range(S)])
        g[k].check(want.size, want, f"caller's multi-seed {k}")
    for k in ckeys:
        want = np.stack([single[s][SOURCE[k][0]][SOURCE[k][1]] for s in range(S)])
        gc[k].check(want.size, want, f"caller's chain {k}")
    m.set_device_adjoint_multi(0)
    m.set_device_adjoint_chain_multi(0)
