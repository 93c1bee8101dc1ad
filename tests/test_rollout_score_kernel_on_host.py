"""The score and selection kernels' own source (csrc/hmpc_rollout_score.h) run on the CPU, no GPU needed: compiled with g++ against the
stand-in hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim), checked against the plain loops of
tests/src/rollout_score_on_host.cpp and, case by case, against the numpy mirror written from the header comment
(tests/rollout_score_mirror.py) -- bit for bit: the contract has no libm call.  The GPU tests (tests/test_gpu_rollout_score.py) run the same
cases on the machine code; the mirror's expansion is checked here against a field-by-field copy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_score_mirror as sm
from hector_simulation_amd import _lib, interface, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cost_struct(d: dict) -> _lib.RolloutCost:
    """the ctypes struct of a mirror cost dict, filled member by member (no library call)"""
    c = _lib.RolloutCost()
    for k, v in d.items():
        if k.startswith("w_"):
            getattr(c, k)[:] = [float(x) for x in v]
        else:
            setattr(c, k, float(v))
    return c


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rollout_score") / "rollout_score_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "rollout_score_on_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _run(exe, tmp_path, header, blobs):
    src, dst = tmp_path / "case.in", tmp_path / "case.out"
    with open(src, "wb") as f:
        f.write(np.array(header, dtype=np.int32).tobytes())
        for b in blobs:
            if b is not None:
                f.write(b if isinstance(b, bytes) else np.ascontiguousarray(b).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(dst, "rb").read()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_kernel_source_against_the_plain_loops(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 problems" in r.stdout, r.stdout + r.stderr


def test_score_kernel_source_is_the_mirror_bit_for_bit(exe, tmp_path):
    for name, t, log, cost in sm.score_cases():
        if name.startswith("shape-b257") and not name.endswith("n65"):
            continue  # (one thread per lane: many workgroups once is enough here; the GPU test runs them all)
        nb, n = log["state"].shape[:2]
        has = [log.get(k) is not None for k in ("wrench", "tau", "summary")]
        raw = _run(exe, tmp_path, [0, nb, n, *has, 0, 0],
                   [bytes(cost_struct(cost)), t, log["state"], log.get("wrench"), log.get("tau"), log.get("summary")])
        got = np.frombuffer(raw, dtype=np.float64)
        want_cost, want_score = sm.score(t, log, cost)
        np.testing.assert_array_equal(_bits(got[:4 * nb]), _bits(want_cost).reshape(-1), err_msg=name)
        np.testing.assert_array_equal(_bits(got[4 * nb:]), _bits(want_score), err_msg=name)


def test_the_recorded_score_cases_are_what_they_say():
    """what each named case is for happens in the mirror's own result"""
    by = {name: (sm.score(t, log, cost), t, log, cost) for name, t, log, cost in sm.score_cases() if not name.startswith("shape-")}
    (cost, score), t, log, c = by["yaw"]
    e = log["state"][:, :, 2] - (t["rpy"][:, None, 2] + (np.arange(65) + 1)[None, :] * 0.005 * t["yaw_rate_des"][:, None])
    assert (np.abs(e[:3]).max(axis=1) > np.pi).all() and np.isfinite(score).all()
    assert (cost[:4, 0] < 250.0 * 65 * np.pi ** 2 * 1.01 + 1e3).all()  # (every yaw error was wrapped into [-pi, pi])
    (cost, score), *_ = by["nan"]
    # (an infinite entry under a positive weight is +inf, not NaN: masked in the selection all the same)
    assert np.isnan(score[2]) and np.isposinf(score[4]) and np.isposinf(cost[4, 2]) and np.isfinite(np.delete(score, [2, 4])).all()
    (cost, score), *_ = by["fallen-inf"]
    assert np.isinf(score[[1, 3]]).all() and np.isfinite(np.delete(score, [1, 3])).all() and (cost[[0, 2, 4], 3] == 0).all()
    (cost, score), *_ = by["fallen-finite"]
    assert cost[1, 3] == 1000.0 and cost[3, 3] == 1003.0 and np.isfinite(score).all()
    (cost, score), *_ = by["unsolved-inf"]
    assert np.isfinite(score).all() and (cost[:, 3] == 0).all()
    (cost, score), *_ = by["unsolved-inf-one"]
    assert np.isinf(score[0]) and np.isfinite(score[1:]).all()
    full = sm.score(by["fallen-inf"][1], by["fallen-inf"][2], by["null-wrench"][3])[0]
    assert (by["null-wrench"][0][0][:, 1] < full[:, 1]).all() and (by["null-tau"][0][0][:, 1] < full[:, 1]).all()
    assert (by["null-summary"][0][0][:, 3] == 0).all() and (by["null-wrench-tau-summary"][0][0][:, [1, 3]] == 0).all()
    assert np.signbit(by["null-wrench-tau-summary"][0][0]).sum() == 0  # (+0.0, not -0.0)


def test_select_kernel_source_is_the_mirror_bit_for_bit(exe, tmp_path):
    for name, sc, pen, K, log, n in sm.select_cases():
        nb, G = len(sc), len(sc) // K
        has = [log.get(k) is not None for k in ("wrench", "tau", "summary")]
        raw = _run(exe, tmp_path, [1, nb, n, *has, K, pen is not None], [sc, pen, log.get("wrench"), log.get("tau"), log.get("summary")])
        want = sm.select(sc, pen, K, log)
        off = 0
        for k, dt, per in (("index", np.int32, 1), ("score", np.float64, 1), ("wrench", np.float32, 12), ("tau", np.float64, 10),
                           ("summary", np.int32, 4)):
            if k not in want:
                continue
            size = G * per * np.dtype(dt).itemsize
            np.testing.assert_array_equal(np.frombuffer(raw[off:off + size], dtype=np.uint8), _bits(want[k]).reshape(-1), err_msg=f"{name}: {k}")
            off += size
        assert off == len(raw), name
        if K > 1 and "index-and-score" not in name:
            assert want["index"][1] == -1 and np.isposinf(want["score"][1]) and (want["summary"][1] == sm.NO_WINNER_SUMMARY).all()
            assert not want["wrench"][1].any() and not want["tau"][1].any() and not np.signbit(want["tau"][1]).any()
            assert want["index"][2] == K // 2 and want["score"][2] == 0.0  # (+0.0 at the lower index beats -0.0 at the higher)
            if pen is None:
                assert not np.signbit(want["score"][2])


def test_mirror_expansion_is_a_field_by_field_copy():
    ns, K = 5, 7
    t = synthetic.make_ticks(ns, sm.H, "walking", seed=4)
    rng = np.random.default_rng(5)
    cmd = np.zeros((ns, K), dtype=interface.COMMAND_DTYPE)
    for f in cmd.dtype.names:
        cmd[f] = rng.normal(size=cmd[f].shape)
    out = sm.expand(t, cmd)
    assert out.shape == (ns * K,)
    for i in range(ns * K):
        want = t[i // K].copy()
        for f in cmd.dtype.names:
            want[f] = cmd[i // K, i % K][f]
        assert out[i].tobytes() == want.tobytes()


def test_struct_sizes_the_case_files_rely_on():
    assert C.sizeof(_lib.RolloutCost) == 50 * 8 and interface.TICK_DTYPE.itemsize == C.sizeof(_lib.TickInputs)
