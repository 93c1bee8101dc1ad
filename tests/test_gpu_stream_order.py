"""Every stream-taking entry point on a BUSY caller's stream, and the blocking host-pointer entries called while work is pending there
(include/hector_mpc.h "Streams").

The rest of the suite runs the library on the legacy null stream with the host waiting between calls: a launch, a memset or a copy on the
wrong stream, a host copy into memory that enqueued work still reads, a buffer freed under pending work cannot fail a test there.  Here a
non-blocking stream S is held busy by a bounded sleep kernel (tests/stream_cases.py: no host flag, nothing unbounded), the calls under
test are enqueued behind it, and the test FAILS ("blocker too short") unless the blocker was still running when the last call that must
not wait had returned -- so nothing of the sequence had started on the device while the host ran ahead of it.

The reference, everywhere, is the QUIET RUN: the same calls on a fresh handle on the null stream with a device-wide wait after each --
what the existing suite pins to qpOASES and the numpy mirrors.  Every comparison is on bits, over every array the calls produce.

 A. every stream-taking entry behind pending work, per shape and per buffer set-up (the handle's own buffers; the caller's, pre-filled
    with a sentinel; a used handle whose own buffers hold another batch's results);
 B. the blocking host-pointer entries under pending work: the pending work's outputs AND the blocking call's own result;
 C. buffers that grow while their previous user is pending on another stream."""
import ctypes as C
import functools
import gc
import types

import numpy as np
import pytest

import stream_cases as sc
from hector_simulation_amd import _lib, interface, records, synthetic
from sweep_cases import sweep_fields

pytestmark = pytest.mark.gpu
DT, FMAX = sc.DT, sc.FMAX
H = 10


def _torch():
    return sc.torch_()


@pytest.fixture(autouse=True)
def _collector_back_on():
    """(stream_cases.Busy switches the garbage collector off while it holds a stream; a test that fails in between leaves it off)"""
    yield
    gc.enable()


def _codes(status):
    return interface.status_code(status)


# ================================================================================================ A. every entry behind pending work
@functools.lru_cache(maxsize=None)
def _flagged_by_the_fast_pass(name):
    """how many instances of the shape's batch the fast pass flags (a quiet run, every repair off)"""
    nc, h, nb, _, _ = sc.SHAPES[name]
    m = interface.BatchedMPC(DT, h, FMAX, nb, contacts=nc)
    m.set_auto_resolve(False)
    m.upload(sc.shape_records(name))
    m.solve()
    _, st = m.download()
    m.close()
    return int(np.isin(_codes(st), sc.FLAGGED).sum())


@pytest.mark.parametrize("buffers", sc.BUFFERS)
@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_every_entry_behind_pending_work_is_the_quiet_run(name, buffers):
    """upload (async, pinned) or device records -> solve -> prediction -> margins -> margin penalty -> certificate -> certificate penalty ->
    gains -> first-order wrench -> adjoint -> model, limit, record gradients -> multi-seed adjoint -> selection of its last slice -> chain ->
    model, limit, record gradients of the selection, all on S behind the blocker, no host wait before the downloads.
    (a) two contacts, h = 10, 24 standing, every second one from the 6x stress rows, device repair on: the chain's memset, list and counter;
    (b) 16 ticks through hmpc_tick_solve_device: builder, size classes, solve, torques; (c) three contacts, 19 seeds and (d) two contacts,
    13 seeds: two launches of the multi-seed calls; (e) double support, h = 20: the wide variant."""
    nc, h, nb, S, repair = sc.SHAPES[name]
    if repair:
        assert _flagged_by_the_fast_pass(name) >= 1  # (the device-side chain has something to repair)
    device_records = buffers == "caller" and name != "b"  # (the caller's set-up also hands the records in by device pointer)
    want = sc.quiet_a(name, device_records)
    mb = nb + 3
    m = sc.handle_a(name, mb)
    x = sc.inputs_a(name)
    bufs = sc.give_caller_buffers(m, x, mb) if buffers == "caller" else None
    if buffers == "used":
        y = sc.inputs_a(name, other=True)
        sc.run_a(m, y, 0, False, quiet=True)
        before = sc.read_a(m, y)
        assert not np.array_equal(sc.bits(before["forces"]), sc.bits(want["forces"]))  # (the own buffers hold OTHER values)
    busy = sc.Busy().hold()
    sc.run_a(m, x, busy.s, device_records, quiet=False)
    busy.still_held(f"A {name}/{buffers}")
    # the downloads wait for S -- the one called first, that is: a different one of the twelve in every case
    case = list(sc.SHAPES).index(name) * len(sc.BUFFERS) + sc.BUFFERS.index(buffers)
    got = sc.read_a(m, x, first=case % len(sc.DOWNLOADS_A))
    m.close()
    sc.assert_same(got, want, f"A {name}/{buffers}")
    if bufs is not None:
        sc.check_caller_buffers(bufs, x, mb, want, f"A {name}/{buffers}")


# ------------------------------------------------------------------------------------------------ A, second group: sweeps and rollouts
NS, K = 4, 4
NB = NS * K
N_TICKS = 6


def _commands(seed):
    rng = np.random.default_rng(seed)
    cmd = np.zeros((NS, K), dtype=interface.COMMAND_DTYPE)
    cmd["v_des_robot"] = rng.uniform(-0.3, 0.3, (NS, K, 2))
    cmd["yaw_rate_des"] = rng.uniform(-0.4, 0.4, (NS, K))
    cmd["roll_des"], cmd["pitch_des"] = rng.uniform(-0.03, 0.03, (NS, K)), rng.uniform(-0.03, 0.03, (NS, K))
    return cmd


def _sweep_inputs(other=False):
    """4 states (three walking, one standing) x 4 commands, a penalty per candidate, outputs pre-filled with the sentinel"""
    seed = 815 if other else 810
    t = synthetic.make_ticks(NS, H, "walking", seed=seed)
    t["gait_offsets"][3], t["gait_durations"][3] = (0, 0), (H, H)
    x = types.SimpleNamespace(d_ticks=sc.device_bytes(t), d_cmd=sc.device_bytes(_commands(seed + 1)),
                                 d_pen=sc.device(np.random.default_rng(seed + 2).integers(0, 3, NB) * 0.5))
    x.d_tau, x.d_fff, x.d_wpd = sc.sentinel(NS * 10 * 8), sc.sentinel(NS * 12 * 8), sc.sentinel(NB * 2 * 8)
    return x


def _sweep_handle():
    m = interface.BatchedMPC(DT, H, FMAX, NB + 3)
    m.set_auto_resolve(False)
    m.set_sweep_margin_floor([-1e-6] * 6)
    m.set_sweep_certificate_ceiling([1e-2, np.nan, 1e-1])
    return m


def _sweep_steps(m, x):
    """the planning tick, then a sweep solve, prediction and selection of their own over the records it built"""
    return [
        lambda s: m.tick_sweep_device(x.d_ticks.data_ptr(), NS, x.d_cmd.data_ptr(), K, DT, x.d_tau.data_ptr(), x.d_fff.data_ptr(),
                                      x.d_wpd.data_ptr(), x.d_pen.data_ptr(), s),
        lambda s: m.solve_command_sweep(K, s),
        lambda s: m.predict_states(s),
        lambda s: m.sweep_select(K, x.d_pen.data_ptr(), s),
    ]


def _sweep_read(m, x):
    out = {f"selection.{k}": v for k, v in m.download_selection().items()}  # (waits)
    out["forces"], out["status"] = m.download()
    out["states"], out["cost"] = m.download_prediction()
    out["records"] = m.download_records()
    _torch().cuda.synchronize()
    for k in ("tau", "fff", "wpd"):
        out[f"tick.{k}"] = getattr(x, "d_" + k).cpu().numpy().view(np.float64).copy()
    return out


SELECTION_ROWS = dict(index=(np.int32, ()), score=(np.float64, ()), forces=(np.float32, (12 * H,)), status=(np.uint32, ()),
                      states=(np.float32, (H, 13)))


@functools.lru_cache(maxsize=None)
def _quiet_sweep(other=False):
    m, x = _sweep_handle(), _sweep_inputs(other)
    _torch().cuda.synchronize()
    sc.quietly(_sweep_steps(m, x))
    out = _sweep_read(m, x)
    m.close()
    return out


@pytest.mark.parametrize("buffers", sc.BUFFERS)
def test_command_sweeps_behind_pending_work_are_the_quiet_run(buffers):
    """hmpc_tick_sweep_device with a margin floor and a certificate ceiling set, hmpc_solve_command_sweep, hmpc_predict_states and
    hmpc_sweep_select on S behind the blocker: 4 states x 4 commands."""
    want = _quiet_sweep()
    assert (want["selection.index"] >= 0).any()
    m, x = _sweep_handle(), _sweep_inputs()
    sel = None
    if buffers == "caller":
        sel = {k: sc.sentinel((NB + 3) * sc.row_bytes(spec)) for k, spec in SELECTION_ROWS.items()}
        m.set_device_selection(*[t.data_ptr() for t in sel.values()])
    if buffers == "used":
        y = _sweep_inputs(other=True)
        sc.quietly(_sweep_steps(m, y))
        assert not np.array_equal(sc.bits(_sweep_read(m, y)["forces"]), sc.bits(want["forces"]))
    busy = sc.Busy().hold()
    sc.enqueue(_sweep_steps(m, x), busy.s)
    busy.still_held(f"sweeps/{buffers}")
    got = _sweep_read(m, x)
    m.close()
    sc.assert_same(got, want, f"sweeps/{buffers}")
    if sel is not None:
        for k, spec in SELECTION_ROWS.items():
            raw, used = sel[k].cpu().numpy(), NS * sc.row_bytes(spec)
            np.testing.assert_array_equal(raw[:used], sc.bits(want["selection." + k]), err_msg=f"caller's selection {k}")
            assert (raw[used:] == sc.SENTINEL).all(), k


LOG_ROWS = dict(state=(np.float64, (N_TICKS, 12)), wrench=(np.float32, (N_TICKS, 12)), status=(np.uint32, (N_TICKS,)),
                tau=(np.float64, (N_TICKS, 10)), summary=(np.int32, (4,)))
CHOICE_ROWS = dict(index=(np.int32, ()), score=(np.float64, ()), wrench=(np.float32, (12,)), tau=(np.float64, (10,)), summary=(np.int32, (4,)))


def _rollout_inputs(other=False):
    seed = 825 if other else 820
    t = synthetic.make_ticks(NB, H, "walking", seed=seed)
    t["gait_offsets"][3::4], t["gait_durations"][3::4] = (0, 0), (H, H)
    x = types.SimpleNamespace(d_ticks=sc.device_bytes(t), d_ticks0=sc.device_bytes(t),
                                 d_pen=sc.device(np.random.default_rng(seed + 2).integers(0, 3, NB) * 0.25))
    x.d_cost, x.d_score = sc.sentinel(NB * 4 * 8), sc.sentinel(NB * 8)
    x.choice_bufs = {k: sc.sentinel(NS * sc.row_bytes(spec)) for k, spec in CHOICE_ROWS.items()}
    x.choice = _lib.RolloutChoice(**{k: t.data_ptr() for k, t in x.choice_bufs.items()})
    x.plant = interface.default_plant(dtMPC=DT)
    x.cost = interface.default_rollout_cost(fall_penalty=1e6, unsolved_penalty=10.0)
    return x


def _rollout_handle():
    m = interface.BatchedMPC(DT, H, FMAX, NB + 3)
    m.set_auto_resolve(False)
    m.set_tick_warm_start(True, 0)
    return m


def _rollout_steps(m, x):
    """6 closed-loop ticks (the gait advances after the third), their score, the cheapest of every four, one more plant step"""
    return [
        lambda s: m.rollout(x.d_ticks.data_ptr(), N_TICKS, 8, 5, plant=x.plant, device=True, batch=NB, dt_mpc=DT, stream=s),
        lambda s: m.rollout_score(x.d_ticks0.data_ptr(), None, x.cost, device=True, batch=NB, n_ticks=N_TICKS, cost_ptr=x.d_cost.data_ptr(),
                                  score_ptr=x.d_score.data_ptr(), stream=s),
        lambda s: m.rollout_select(x.d_score.data_ptr(), K, x.d_pen.data_ptr(), None, device=True, batch=NB, choice=x.choice, stream=s),
        lambda s: m.plant_step(x.d_ticks.data_ptr(), x.plant, device=True, batch=NB, stream=s),
    ]


def _rollout_read(m, x):
    out = {f"log.{k}": v for k, v in m.download_rollout(NB, N_TICKS).items()}  # (waits)
    _torch().cuda.synchronize()
    out["ticks"] = x.d_ticks.cpu().numpy().copy()
    out["cost"], out["score"] = x.d_cost.cpu().numpy().copy(), x.d_score.cpu().numpy().copy()
    out.update({f"choice.{k}": t.cpu().numpy().copy() for k, t in x.choice_bufs.items()})
    return out


@functools.lru_cache(maxsize=None)
def _quiet_rollout(other=False):
    m, x = _rollout_handle(), _rollout_inputs(other)
    _torch().cuda.synchronize()
    sc.quietly(_rollout_steps(m, x))
    out = _rollout_read(m, x)
    m.close()
    return out


@pytest.mark.parametrize("buffers", sc.BUFFERS)
def test_rollouts_behind_pending_work_are_the_quiet_run(buffers):
    """hmpc_rollout_device (tick warm start on), hmpc_rollout_score_device, hmpc_rollout_select_device and hmpc_plant_step_device on S behind
    the blocker: 16 instances in groups of 4, 6 ticks."""
    want = _quiet_rollout()
    assert (want["choice.index"].view(np.int32) >= 0).any()
    m, x = _rollout_handle(), _rollout_inputs()
    log = None
    if buffers == "caller":
        log = {k: sc.sentinel((NB + 3) * sc.row_bytes(spec)) for k, spec in LOG_ROWS.items()}
        lg = _lib.RolloutLog(**{k: t.data_ptr() for k, t in log.items()})
        interface._check(m.L.hmpc_set_device_rollout(m.h, C.byref(lg)), "hmpc_set_device_rollout")
    if buffers == "used":
        y = _rollout_inputs(other=True)
        sc.quietly(_rollout_steps(m, y))
        assert not np.array_equal(sc.bits(_rollout_read(m, y)["log.state"]), sc.bits(want["log.state"]))
        m.reset_tick_warm_start()  # (a fresh handle starts from no saved working sets)
    busy = sc.Busy().hold()
    sc.enqueue(_rollout_steps(m, x), busy.s)
    busy.still_held(f"rollouts/{buffers}")
    got = _rollout_read(m, x)
    m.close()
    sc.assert_same(got, want, f"rollouts/{buffers}")
    if log is not None:
        for k, spec in LOG_ROWS.items():
            raw, used = log[k].cpu().numpy(), NB * sc.row_bytes(spec)
            np.testing.assert_array_equal(raw[:used], sc.bits(want["log." + k]), err_msg=f"caller's log {k}")
            assert (raw[used:] == sc.SENTINEL).all(), k


# ================================================================================================ B. blocking entries under pending work
def _outputs(nb, h=H, nc=2):
    """caller-owned force and status buffers, every byte the sentinel"""
    return sc.sentinel(nb * 6 * nc * h * 4), sc.sentinel(nb * 4)


def _read_outputs(bufs, nb):
    f, st = bufs
    return dict(forces=f.cpu().numpy().view(np.float32).reshape(nb, -1).copy(), status=st.cpu().numpy().view(np.uint32).copy())


def _plain_handle(nb, h=H, nc=2, repair=False, warm=False):
    m = interface.BatchedMPC(DT, h, FMAX, nb, contacts=nc)
    m.set_auto_resolve(False)
    if repair:
        m.set_device_repair(1)
    if warm:
        m.set_tick_warm_start(True, 0)
    return m


@functools.lru_cache(maxsize=None)
def _quiet_solve(name, other=False, repair=False):
    """raw forces and status of one quiet solve of a shape's batch (no repair on the host)"""
    nc, h, nb, _, _ = sc.SHAPES[name]
    m = _plain_handle(nb, h, nc, repair)
    m.upload(sc.shape_records(name, other))
    m.solve()
    f, st = m.download()
    m.close()
    return dict(forces=f, status=st)


def test_upload_under_a_pending_solve():
    """hmpc_upload_records of batch B while the solve of batch A is pending on S: A's forces are A's, the records are B's, and so is the
    next solve."""
    nb = sc.SHAPES["a"][2]
    rec_a, rec_b = sc.shape_records("a"), sc.shape_records("a", other=True)
    want_a, want_b = _quiet_solve("a"), _quiet_solve("a", other=True)
    assert not np.array_equal(sc.bits(want_a["forces"]), sc.bits(want_b["forces"]))
    m = _plain_handle(nb)
    out_a, out_b = _outputs(nb), _outputs(nb)
    m.upload(rec_a)
    m.set_device_outputs(out_a[0].data_ptr(), out_a[1].data_ptr())
    busy = sc.Busy().hold()
    m.solve(busy.s)
    busy.still_held("B upload: the solve of A")
    m.upload(rec_b)  # (must wait for the solve of A)
    np.testing.assert_array_equal(m.download_records(), rec_b)
    m.set_device_outputs(out_b[0].data_ptr(), out_b[1].data_ptr())
    m.solve(busy.s)
    busy.wait()
    m.close()
    sc.assert_same(_read_outputs(out_a, nb), want_a, "the pending solve of A")
    sc.assert_same(_read_outputs(out_b, nb), want_b, "the solve of B behind the upload")


def _pending_tick_sweep(m, x):
    """caller-owned selection buffers for the handle, and a stream held busy with a planning tick enqueued behind the blocker"""
    sel = {k: sc.sentinel((NB + 3) * sc.row_bytes(spec)) for k, spec in SELECTION_ROWS.items()}
    m.set_device_selection(*[t.data_ptr() for t in sel.values()])
    busy = sc.Busy().hold()
    _sweep_steps(m, x)[0](busy.s)
    return sel, busy


def _check_pending_tick_sweep(sel, x, want):
    for k, spec in SELECTION_ROWS.items():
        np.testing.assert_array_equal(sel[k].cpu().numpy()[:NS * sc.row_bytes(spec)], sc.bits(want["selection." + k]), err_msg=f"pending sweep: {k}")
    for k in ("tau", "fff", "wpd"):
        np.testing.assert_array_equal(getattr(x, "d_" + k).cpu().numpy(), sc.bits(want["tick." + k]), err_msg=f"pending sweep: {k}")


@functools.lru_cache(maxsize=None)
def _quiet_tick_sweep():
    """the planning tick alone, quietly: its selection, torques, and the forces of all 16 candidates"""
    m, x = _sweep_handle(), _sweep_inputs()
    _torch().cuda.synchronize()
    sc.quietly(_sweep_steps(m, x)[:1])
    out = _sweep_read(m, x)
    ticks = x.d_ticks.cpu().numpy().view(interface.TICK_DTYPE)
    rb, lq = np.repeat(ticks["rBody"], K, axis=0), np.repeat(ticks["leg_q"], K, axis=0)
    out["body_wrench"] = m.body_wrench(rb)
    out["leg_fff"], out["leg_tau"] = m.leg_torques(rb, lq)
    m.close()
    return out, rb, lq


def test_build_records_under_a_pending_tick_sweep():
    """hmpc_build_records of 12 host ticks while a planning tick of 16 candidates is pending on S: its expansion lives in the scratch the
    host ticks are copied to, its records in the store the builder writes."""
    want, _, _ = _quiet_tick_sweep()
    t_b = synthetic.make_ticks(12, H, "walking", seed=840)
    q = _plain_handle(NB + 3)
    want_wpd = q.build_records(t_b, DT)
    want_rec = q.download_records()
    q.close()
    m, x = _sweep_handle(), _sweep_inputs()
    sel, busy = _pending_tick_sweep(m, x)
    busy.still_held("B build_records: the planning tick")
    wpd = m.build_records(t_b, DT)  # (must wait)
    rec = m.download_records()
    busy.wait()
    m.close()
    np.testing.assert_array_equal(sc.bits(wpd), sc.bits(want_wpd))
    np.testing.assert_array_equal(rec, want_rec)
    _check_pending_tick_sweep(sel, x, want)


@pytest.mark.parametrize("entry", ["body_wrench", "leg_torques"])
def test_wrench_and_torques_under_a_pending_tick_sweep(entry):
    """hmpc_body_wrench / hmpc_leg_torques while a planning tick is pending on S: they copy their inputs into the scratch its expansion
    lives in and read the forces its solve writes."""
    want, rb, lq = _quiet_tick_sweep()
    m, x = _sweep_handle(), _sweep_inputs()
    sel, busy = _pending_tick_sweep(m, x)
    busy.still_held(f"B {entry}: the planning tick")
    if entry == "body_wrench":
        np.testing.assert_array_equal(sc.bits(m.body_wrench(rb)), sc.bits(want["body_wrench"]))
    else:
        fff, tau = m.leg_torques(rb, lq)
        np.testing.assert_array_equal(sc.bits(fff), sc.bits(want["leg_fff"]))
        np.testing.assert_array_equal(sc.bits(tau), sc.bits(want["leg_tau"]))
    busy.wait()
    m.close()
    _check_pending_tick_sweep(sel, x, want)


def test_reset_of_the_saved_working_sets_under_a_pending_solve():
    """solve (quiet), then on S: a warm-started solve, hmpc_reset_tick_warm_start, a solve from no saved sets.  The reset is ordered on the
    handle's stream: it neither waits nor overtakes the solve that is still to read and write the sets."""
    nb = sc.SHAPES["a"][2]
    rec = sc.shape_records("a")

    def run(m, s, outs, sync):
        m.upload(rec)
        m.solve()
        _torch().cuda.synchronize()
        for k, step in enumerate((lambda: m.solve(s), lambda: m.reset_tick_warm_start(), lambda: m.solve(s))):
            if k != 1:
                m.set_device_outputs(outs[k // 2][0].data_ptr(), outs[k // 2][1].data_ptr())
            step()
            sync()

    q, q_outs = _plain_handle(nb, warm=True), (_outputs(nb), _outputs(nb))
    run(q, 0, q_outs, _torch().cuda.synchronize)
    q.close()
    want = [_read_outputs(o, nb) for o in q_outs]
    assert not np.array_equal(want[0]["status"], want[1]["status"])  # (the warm start shows in the iteration counts)
    sc.assert_same(want[1], _quiet_solve("a"), "a solve after the reset is a fresh handle's")
    m, outs = _plain_handle(nb, warm=True), (_outputs(nb), _outputs(nb))
    busy = sc.Busy()
    m.upload(rec)
    m.solve()
    busy.hold()
    for k, step in enumerate((lambda: m.solve(busy.s), lambda: m.reset_tick_warm_start(), lambda: m.solve(busy.s))):
        if k != 1:
            m.set_device_outputs(outs[k // 2][0].data_ptr(), outs[k // 2][1].data_ptr())
        step()
    busy.still_held("B reset: warm solve, reset, solve")
    busy.wait()
    m.close()
    for k in range(2):
        sc.assert_same(_read_outputs(outs[k], nb), want[k], f"solve {k}")


def test_first_warm_start_and_device_repair_switch_then_a_solve_at_once():
    """The first hmpc_set_tick_warm_start(on) and hmpc_set_device_repair(on) of a handle allocate and clear buffers on the null stream; a
    solve on S, which the null stream does not order, follows at once and reads them.  No blocker here: one in front of the solve would
    give the fills the time whose absence is the point (and the two calls may themselves wait for the null stream)."""
    nb = sc.SHAPES["a"][2]
    want = _quiet_solve("a", repair=True)
    assert _flagged_by_the_fast_pass("a") >= 1
    m, out = interface.BatchedMPC(DT, H, FMAX, nb), _outputs(nb)
    m.set_auto_resolve(False)
    m.upload(sc.shape_records("a"))
    m.set_device_outputs(out[0].data_ptr(), out[1].data_ptr())
    busy = sc.Busy()
    _torch().cuda.synchronize()
    m.set_tick_warm_start(True, 0)
    m.set_device_repair(1)
    m.solve(busy.s)
    busy.wait()
    m.close()
    sc.assert_same(_read_outputs(out, nb), want, "the solve behind the switches")


@pytest.mark.parametrize("entry", ["download", "download_f64"])
def test_host_driven_repair_behind_a_solve_on_a_callers_stream(entry):
    """hmpc_download with flagged instances (the host-driven repair) and hmpc_download_f64 without hmpc_enable_f64_output (it solves once
    more), each after a solve on S."""
    nc, h, nb, _, _ = sc.SHAPES["a"]
    assert _flagged_by_the_fast_pass("a") >= 1
    rec = sc.shape_records("a")

    def result(m):
        if entry == "download":
            f, st = m.download()
            return dict(forces=f, status=st)
        x64, obj = m.download_f64()
        return dict(x=x64, obj=obj)

    q = interface.BatchedMPC(DT, h, FMAX, nb)
    q.upload(rec)
    q.solve()
    _torch().cuda.synchronize()
    want = result(q)
    q.close()
    m = interface.BatchedMPC(DT, h, FMAX, nb)
    m.upload(rec)
    busy = sc.Busy().hold()
    m.solve(busy.s)
    busy.still_held(f"B {entry}: the solve")
    got = result(m)  # (waits)
    m.close()
    sc.assert_same(got, want, entry)
    if entry == "download":
        assert (_codes(got["status"]) == 0).all()


# ================================================================================================ C. growth under a pending user
# where the growing call goes: the null stream, a second caller's stream, or S itself.  On another stream the call settles the handle
# because it changes streams; on S nothing but the growth's own wait (grow(), the whole-device wait of the multi-seed buffers) stands
# between the free and the pending user -- so "same" is the case that pins that wait.
SECOND_STREAMS = ["null", "S2", "same"]


def _second_stream(which, busy):
    if which == "null":
        return 0
    if which == "same":
        return busy.s
    s2 = _torch().cuda.Stream()
    assert s2.cuda_stream not in (0, busy.s)
    busy.keep = s2
    return s2.cuda_stream


@functools.lru_cache(maxsize=None)
def _sweep_records(groups, seed):
    return records.pack_records(sweep_fields(groups, K, H, "standing", seed=seed), H)


@functools.lru_cache(maxsize=None)
def _quiet_command_sweep(groups, seed):
    nb = groups * K
    m = _plain_handle(nb)
    d = sc.device(_sweep_records(groups, seed))
    _torch().cuda.synchronize()
    m.set_device_records(d.data_ptr(), nb)
    m.solve_command_sweep(K)
    f, st = m.download()
    m.close()
    return dict(forces=f, status=st)


@pytest.mark.parametrize("second", SECOND_STREAMS)
def test_a_larger_command_sweep_on_another_stream_while_the_smaller_is_pending(second):
    """A sweep of 2 groups pending on S, then one of 8 groups on the null stream / a second stream / S: the buffer of the groups' H^-1 has
    to grow, and the old one is the pending sweep's.  The growing call has waited for S when it returns."""
    want_2, want_8 = _quiet_command_sweep(2, 850), _quiet_command_sweep(8, 851)
    m = _plain_handle(8 * K)
    d2, d8 = sc.device(_sweep_records(2, 850)), sc.device(_sweep_records(8, 851))
    out2, out8 = _outputs(2 * K), _outputs(8 * K)
    busy = sc.Busy()
    s2 = _second_stream(second, busy)
    m.set_device_records(d2.data_ptr(), 2 * K)
    m.set_device_outputs(out2[0].data_ptr(), out2[1].data_ptr())
    busy.hold()
    m.solve_command_sweep(K, busy.s)
    m.set_device_records(d8.data_ptr(), 8 * K)
    m.set_device_outputs(out8[0].data_ptr(), out8[1].data_ptr())
    busy.still_held("C command sweep: the sweep of 2 groups")
    m.solve_command_sweep(K, s2)  # (must wait for S before it frees the smaller buffer)
    busy.was_waited_for("the sweep of 8 groups, which frees the smaller buffer")
    _torch().cuda.synchronize()
    m.close()
    sc.assert_same(_read_outputs(out2, 2 * K), want_2, "the pending sweep of 2 groups")
    sc.assert_same(_read_outputs(out8, 8 * K), want_8, "the sweep of 8 groups")


@functools.lru_cache(maxsize=None)
def _wide_records(nb, seed):
    return records.pack_records(synthetic.hard_batch(nb, 20, "standing", seed, 6), 20)


@functools.lru_cache(maxsize=None)
def _quiet_wide(nb, seed):
    m = _plain_handle(nb, h=20, repair=True)
    d = sc.device(_wide_records(nb, seed))
    _torch().cuda.synchronize()
    m.set_device_records(d.data_ptr(), nb, max_reduced_vars=240)
    m.solve()
    f, st = m.download()
    m.close()
    return dict(forces=f, status=st)


@pytest.mark.parametrize("second", SECOND_STREAMS)
def test_a_larger_wide_repair_on_another_stream_while_the_smaller_is_pending(second):
    """Double support at h = 20 with the device-side repair: the safe variant keeps its packed Schur inverse in global scratch, one slice
    per workgroup of the launch.  2 instances pending on S, then 6 on another stream or on S: the scratch has to grow, and the growing
    call has waited for S when it returns."""
    want_2, want_6 = _quiet_wide(2, 860), _quiet_wide(6, 861)
    m = _plain_handle(6, h=20, repair=True)
    d2, d6 = sc.device(_wide_records(2, 860)), sc.device(_wide_records(6, 861))
    out2, out6 = _outputs(2, 20), _outputs(6, 20)
    busy = sc.Busy()
    s2 = _second_stream(second, busy)
    m.set_device_records(d2.data_ptr(), 2, max_reduced_vars=240)
    m.set_device_outputs(out2[0].data_ptr(), out2[1].data_ptr())
    busy.hold()
    m.solve(busy.s)
    m.set_device_records(d6.data_ptr(), 6, max_reduced_vars=240)
    m.set_device_outputs(out6[0].data_ptr(), out6[1].data_ptr())
    busy.still_held("C wide repair: the solve of 2 instances")
    m.solve(s2)
    busy.was_waited_for("the solve of 6 instances, which frees the smaller scratch")
    _torch().cuda.synchronize()
    m.close()
    sc.assert_same(_read_outputs(out2, 2), want_2, "the pending solve of 2 instances")
    sc.assert_same(_read_outputs(out6, 6), want_6, "the solve of 6 instances")


@pytest.mark.parametrize("second", SECOND_STREAMS)
def test_more_seeds_on_another_stream_while_fewer_are_pending(second):
    """A multi-seed adjoint and its chain under 6 seeds pending on S, then under 13 seeds on another stream or on S itself: the handle's own buffers
    grow behind a whole-device wait -- on S that wait is all that keeps the free behind the pending launches, and the call has waited for S
    when it returns."""
    nc, h, nb, S, _ = sc.SHAPES["d"]
    seeds = sc.shape_seeds("d")
    q = _plain_handle(nb)
    q.upload(sc.shape_records("d"))
    q.solve()
    d_seeds = sc.device(seeds)
    _torch().cuda.synchronize()
    q.solve_adjoint_multi(d_seeds.data_ptr(), S)
    q.adjoint_chain_multi(d_seeds.data_ptr())
    want = {f"multi.{k}": v for k, v in q.download_adjoint_multi().items()}
    want.update({f"chain.{k}": v for k, v in q.download_adjoint_chain_multi().items()})
    q.close()
    m = _plain_handle(nb)
    m.upload(sc.shape_records("d"))
    busy = sc.Busy()
    s2 = _second_stream(second, busy)
    busy.hold()
    m.solve(busy.s)
    m.solve_adjoint_multi(d_seeds.data_ptr(), 6, busy.s)
    m.adjoint_chain_multi(d_seeds.data_ptr(), busy.s)
    busy.still_held("C seeds: solve, 6 seeds and their chain")
    m.solve_adjoint_multi(d_seeds.data_ptr(), S, s2)  # (must wait: the buffers of the 6 seeds are freed)
    busy.was_waited_for("the adjoint under 13 seeds, which frees the buffers of 6")
    m.adjoint_chain_multi(d_seeds.data_ptr(), s2)
    got = {f"multi.{k}": v for k, v in m.download_adjoint_multi().items()}
    got.update({f"chain.{k}": v for k, v in m.download_adjoint_chain_multi().items()})
    m.close()
    sc.assert_same(got, want, "13 seeds behind 6")
