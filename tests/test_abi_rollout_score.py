"""The closed-loop command sweep's calls of the C ABI (score, selection, chain): exported with the signatures include/hector_mpc.h declares,
the structs laid out as the Python types say, the defaults, HMPC_E_ARG for a NULL handle -- no GPU -- and, on a GPU, every argument error the
header lists for the three calls, with nothing enqueued."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_BATCH = -1, -3
SIGNATURES = {
    "hmpc_default_rollout_cost": "void hmpc_default_rollout_cost(struct hmpc_rollout_cost *c);",
    "hmpc_rollout_score_device": "int hmpc_rollout_score_device(hmpc_handle *h, const void *device_ticks0, int batch, int n_ticks, "
                                 "const struct hmpc_rollout_cost *cost, const struct hmpc_rollout_log *log, double *device_cost, "
                                 "double *device_score, void *stream);",
    "hmpc_rollout_select_device": "int hmpc_rollout_select_device(hmpc_handle *h, const double *device_score, const double *device_penalty, "
                                  "int batch, int group_size, const struct hmpc_rollout_log *log, const struct hmpc_rollout_choice *choice, "
                                  "void *stream);",
    "hmpc_rollout_sweep_device": "int hmpc_rollout_sweep_device(hmpc_handle *h, const void *device_ticks, int n_states, "
                                 "const struct hmpc_command *device_commands, int K, int n_ticks, double dtMPC, int ticks_per_step, int subtick0, "
                                 "const struct hmpc_plant *plant, const struct hmpc_rollout_cost *cost, const double *device_penalty, "
                                 "const struct hmpc_rollout_choice *choice, void *stream);",
    "hmpc_get_device_rollout_sweep": "int hmpc_get_device_rollout_sweep(hmpc_handle *h, void **ticks_final, double **cost, double **score);",
}


def test_the_five_symbols_are_exported_as_declared():
    L = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hector_mpc.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    syms = os.popen(f"nm -D --defined-only {_lib.lib_path()}").read()
    for name, sig in SIGNATURES.items():
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(rf"\bT {name}\b", syms), name
        assert re.sub(r"\s+", " ", sig) in flat, name
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    cost, log, choice = C.POINTER(_lib.RolloutCost), C.POINTER(_lib.RolloutLog), C.POINTER(_lib.RolloutChoice)
    assert L.hmpc_rollout_score_device.argtypes == [vp, vp, ci, ci, cost, log, vp, vp, vp]
    assert L.hmpc_rollout_select_device.argtypes == [vp, vp, vp, ci, ci, log, choice, vp]
    assert L.hmpc_rollout_sweep_device.argtypes == [vp, vp, ci, vp, ci, ci, cd, ci, ci, C.POINTER(_lib.Plant), cost, vp, choice, vp]
    assert L.hmpc_get_device_rollout_sweep.argtypes == [vp] + [C.POINTER(vp)] * 3
    # the unit is one of the library's (build.py's list is what every hand-made build takes its units from)
    from hector_simulation_amd import build

    assert "hmpc_rollout_score.hip" in build.HOST_SOURCES


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "hector_mpc.h"
#define F(s, m) printf(#s "." #m " %zu %zu\n", offsetof(struct s, m), sizeof(((struct s *)0)->m))
int main(void) {
  printf("hmpc_rollout_cost %zu\n", sizeof(struct hmpc_rollout_cost));
  F(hmpc_rollout_cost, w_state); F(hmpc_rollout_cost, w_terminal); F(hmpc_rollout_cost, w_wrench); F(hmpc_rollout_cost, w_tau);
  F(hmpc_rollout_cost, height); F(hmpc_rollout_cost, dt_tick); F(hmpc_rollout_cost, fall_penalty); F(hmpc_rollout_cost, unsolved_penalty);
  printf("hmpc_rollout_choice %zu\n", sizeof(struct hmpc_rollout_choice));
  F(hmpc_rollout_choice, index); F(hmpc_rollout_choice, score); F(hmpc_rollout_choice, wrench); F(hmpc_rollout_choice, tau);
  F(hmpc_rollout_choice, summary);
  printf("hmpc_command %zu\n", sizeof(struct hmpc_command));
  return 0;
}
"""


def test_struct_sizes_and_offsets_match_the_python_types(tmp_path):
    """the header compiled as C: every member of hmpc_rollout_cost and hmpc_rollout_choice where the ctypes structures have it"""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    types = {"hmpc_rollout_cost": _lib.RolloutCost, "hmpc_rollout_choice": _lib.RolloutChoice, "hmpc_command": _lib.Command}
    seen = {k: 0 for k in types}
    for ln in filter(None, lines):
        w = ln.split()
        if w[0] in types:
            assert C.sizeof(types[w[0]]) == int(w[1]), ln
        else:
            s, m = w[0].split(".")
            fld = getattr(types[s], m)
            assert (fld.offset, fld.size) == (int(w[1]), int(w[2])), ln
            seen[s] += 1
    assert seen["hmpc_rollout_cost"] == len(_lib.RolloutCost._fields_) and seen["hmpc_rollout_choice"] == len(_lib.RolloutChoice._fields_)
    assert interface.COMMAND_DTYPE.itemsize == C.sizeof(_lib.Command)


def test_defaults():
    c = interface.default_rollout_cost()
    assert list(c.w_state) == [100, 100, 250, 200, 200, 300, 1, 1, 1, 1, 1, 1] and list(c.w_terminal) == [0.0] * 12
    assert list(c.w_wrench) == [1e-4, 1e-4, 5e-4, 1e-4, 1e-4, 5e-4] + [1e-2] * 6 and list(c.w_tau) == [0.0] * 10
    assert (c.height, c.dt_tick, c.unsolved_penalty) == (0.55, 0.005, 0.0) and c.fall_penalty == float("inf")
    import rollout_score_mirror as sm

    d = sm.default_cost()
    assert all(list(getattr(c, k)) == list(d[k]) for k in ("w_state", "w_terminal", "w_wrench", "w_tau"))
    assert all(getattr(c, k) == d[k] for k in ("height", "dt_tick", "fall_penalty", "unsolved_penalty"))
    c = interface.default_rollout_cost(fall_penalty=5.0, w_tau=range(10))
    assert c.fall_penalty == 5.0 and list(c.w_tau) == list(range(10))
    _lib.load().hmpc_default_rollout_cost(None)  # (a NULL pointer is ignored)


def test_a_null_handle_is_an_argument_error():
    L = _lib.load()
    c, p, log, ch = interface.default_rollout_cost(), interface.default_plant(), _lib.RolloutLog(), _lib.RolloutChoice()
    buf = np.zeros(64, dtype=np.float64)  # (never dereferenced: the handle is checked first)
    ptr = buf.ctypes.data
    assert L.hmpc_rollout_score_device(None, ptr, 1, 1, C.byref(c), C.byref(log), ptr, ptr, None) == E_ARG
    assert L.hmpc_rollout_select_device(None, ptr, None, 1, 1, C.byref(log), C.byref(ch), None) == E_ARG
    assert L.hmpc_rollout_sweep_device(None, ptr, 1, ptr, 1, 1, 0.04, 8, 0, C.byref(p), C.byref(c), None, C.byref(ch), None) == E_ARG
    out = [C.c_void_p() for _ in range(3)]
    assert L.hmpc_get_device_rollout_sweep(None, *[C.byref(x) for x in out]) == E_ARG
    assert all(x.value is None for x in out)


@pytest.mark.gpu
def test_every_argument_error_and_nothing_enqueued():
    import torch

    import rollout_score_mirror as sm
    from hector_simulation_amd import synthetic

    nb, n, K = 6, 3, 3
    t, log = sm.synthetic_log(nb, n, seed=3)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, 10, synthetic.F_MAX, nb)
    mpc3 = interface.BatchedMPC(synthetic.DT_MPC, 10, synthetic.F_MAX, nb, contacts=3)
    L = mpc.L
    d_t = torch.from_numpy(t.view(np.uint8).reshape(nb, -1).copy()).cuda()
    lg, keep = mpc._stage_log(log, nb, n)
    POISON = -7.0
    d_cost = torch.full((nb, 4), POISON, dtype=torch.float64, device="cuda")
    d_score = torch.full((nb,), POISON, dtype=torch.float64, device="cuda")
    ch, bufs = mpc._choice_buffers(nb // K, _lib.ROLLOUT_CHOICE)
    for b in bufs.values():
        b.fill_(7)
    cost = interface.default_rollout_cost()
    tp = C.c_void_p(d_t.data_ptr())

    def score(h=mpc.h, ticks=tp, batch=nb, n_ticks=n, c=cost, log=lg):
        return L.hmpc_rollout_score_device(h, ticks, batch, n_ticks, C.byref(c) if c is not None else None,
                                           C.byref(log) if log is not None else None, C.c_void_p(d_cost.data_ptr()), C.c_void_p(d_score.data_ptr()),
                                           None)

    def select(sc=d_score.data_ptr(), batch=nb, k=K, log=lg, choice=ch):
        return L.hmpc_rollout_select_device(mpc.h, C.c_void_p(sc), None, batch, k, C.byref(log) if log is not None else None,
                                            C.byref(choice) if choice is not None else None, None)

    # the selection before any score or rollout: a caller's log has no known row count yet, and there is no last rollout
    assert select() == E_ARG and select(log=None) == E_ARG
    no_state = _lib.RolloutLog.from_buffer_copy(lg)
    no_state.state = None
    assert score(ticks=None) == E_ARG and score(c=None) == E_ARG and score(batch=-1) == E_ARG
    assert score(n_ticks=0) == E_ARG and score(log=no_state) == E_ARG
    assert score(log=None) == E_ARG  # no rollout yet
    torch.cuda.synchronize()
    assert (d_cost.cpu().numpy() == POISON).all() and (d_score.cpu().numpy() == POISON).all()
    assert score() == 0
    torch.cuda.synchronize()
    assert (d_score.cpu().numpy() != POISON).all()
    assert select(sc=0) == E_ARG and select(choice=None) == E_ARG and select(batch=-3) == E_ARG
    assert select(k=0) == E_ARG and select(k=4) == E_ARG and select(batch=nb - K) == E_ARG  # (another batch than the scored one)
    for member in ("wrench", "tau", "summary"):
        part = _lib.RolloutLog.from_buffer_copy(lg)
        setattr(part, member, None)
        assert select(log=part) == E_ARG, member
    assert select(log=None) == E_ARG  # still no rollout
    torch.cuda.synchronize()
    assert all((b.cpu().numpy() == 7).all() for b in bufs.values())
    assert select() == 0
    # the chain
    ticks = synthetic.make_ticks(2, 10, "standing", seed=90)
    cmd = np.zeros((2, K), dtype=interface.COMMAND_DTYPE)
    d_s = torch.from_numpy(ticks.view(np.uint8).reshape(2, -1).copy()).cuda()
    d_c = torch.from_numpy(cmd.view(np.uint8).reshape(2 * K, -1).copy()).cuda()
    good, bad = interface.default_plant(), interface.default_plant(substeps=0)

    def sweep(h=mpc.h, ticks=d_s.data_ptr(), ns=2, cmds=d_c.data_ptr(), k=K, n_ticks=2, tps=8, sub0=0, plant=good, c=cost, choice=ch):
        return L.hmpc_rollout_sweep_device(h, C.c_void_p(ticks), ns, C.c_void_p(cmds), k, n_ticks, synthetic.DT_MPC, tps, sub0,
                                           C.byref(plant) if plant is not None else None, C.byref(c) if c is not None else None, None,
                                           C.byref(choice) if choice is not None else None, None)

    assert sweep(ticks=0) == E_ARG and sweep(cmds=0) == E_ARG and sweep(plant=None) == E_ARG and sweep(c=None) == E_ARG
    assert sweep(choice=None) == E_ARG and sweep(ns=0) == E_ARG and sweep(k=0) == E_ARG
    assert sweep(n_ticks=0) == E_ARG and sweep(tps=0) == E_ARG and sweep(sub0=-1) == E_ARG and sweep(plant=bad) == E_ARG
    assert sweep(h=mpc3.h) == E_ARG
    assert sweep(ns=3) == E_BATCH  # 9 > max_batch 6
    out = [C.c_void_p() for _ in range(3)]
    assert L.hmpc_get_device_rollout_sweep(mpc.h, *[C.byref(x) for x in out]) == E_ARG  # no sweep yet
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_s.cpu().numpy().reshape(-1), ticks.view(np.uint8).reshape(-1))
    assert mpc.batch == 0  # nothing was built or solved
    assert sweep() == 0  # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert L.hmpc_get_device_rollout_sweep(mpc.h, *[C.byref(x) for x in out]) == 0 and all(x.value for x in out)
    assert (bufs["index"].cpu().numpy() >= 0).all()
    del keep
    mpc.close(), mpc3.close()
