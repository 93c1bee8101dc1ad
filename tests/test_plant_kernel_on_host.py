"""The plant step's own source (csrc/hmpc_plant.h) run on the CPU, no GPU needed: compiled with g++ (no contraction) against a stand-in
hip_runtime.h that gives every lane a thread (tests/src/hip_lane_shim).

1. Against a plain loop (tests/src/plant_on_host.cpp): batches 1, 24 and 257, substeps 1 and 3, every flag combination, bit for bit.
2. Against the numpy mirror (tests/rollout_mirror.py, written from the header comment) on the cases the GPU test uses too
   (``rollout_mirror.step_cases``): every field but rpy and every summary row bit for bit.  rpy is the one output the mirror cannot match bit
   for bit -- the kernel evaluates it with det_atan2 / det_asin of csrc/hmpc_math.h, numpy with libm.  The largest difference over all those
   cases, measured here on the CPU, is 2.2204460492503131e-16 (printed by the test); ``rollout_mirror.RPY_TOL`` is fixed at four times
   that maximum and is the tolerance of this test and of tests/test_gpu_rollout.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_mirror as rm
from hector_simulation_amd import _lib, interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plant") / "plant_on_host")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "tests", "src", "hip_lane_shim"),
           "-I" + os.path.join(ROOT, "hector_simulation_amd", "csrc"), os.path.join(ROOT, "tests", "src", "plant_on_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def plant_struct(p: dict) -> "_lib.Plant":
    """the mirror's plant dict as struct hmpc_plant, without the library (no defaults are read from it)"""
    s = _lib.Plant()
    for k in ("dt_tick", "dtMPC", "substeps", "advance_gait", "flags", "mass", "gravity", "fall_cos"):
        setattr(s, k, p[k])
    s.inertia[:] = p["inertia"]
    for leg in range(2):
        s.hip[leg][:] = p["hip"][leg]
    return s


def run_on_host(exe, tmp_path, ticks, forces, status, wpd, plant, summary=None, instance_mass=None, ext_wrench=None):
    nb = len(ticks)
    forces = np.ascontiguousarray(forces, dtype=np.float32).reshape(nb, -1)
    summary = np.tile(np.array([0, -1, 0, 0], dtype=np.int32), (nb, 1)) if summary is None else summary
    path_in, path_out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(path_in, "wb") as f:
        f.write(np.array([nb, rm.H, forces.shape[1], wpd is not None, instance_mass is not None, ext_wrench is not None], dtype=np.int32).tobytes())
        f.write(bytes(plant_struct(plant)))
        for a, dt in ((ticks, interface.TICK_DTYPE), (forces, np.float32), (status, np.uint32), (summary, np.int32), (wpd, np.float64),
                      (instance_mass, np.float64), (ext_wrench, np.float64)):
            if a is not None:
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    r = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    raw = open(path_out, "rb").read()
    nt = nb * interface.TICK_DTYPE.itemsize
    return np.frombuffer(raw[:nt], dtype=interface.TICK_DTYPE).copy(), np.frombuffer(raw[nt:], dtype=np.int32).reshape(nb, 4).copy()


def test_plant_kernel_source_against_a_plain_loop(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "48 cases, 0 problems" in r.stdout, r.stdout + r.stderr


def test_plant_kernel_source_against_the_mirror(exe, tmp_path):
    worst, n = 0.0, 0
    for name, t, forces, status, wpd, plant in rm.step_cases():
        got, got_sum = run_on_host(exe, tmp_path, t, forces, status, wpd, plant)
        want, want_sum = rm.plant_step(t, plant, rm.H, forces, status, wpd)
        diff = float(np.abs(got["rpy"] - want["rpy"]).max())
        worst = max(worst, diff)
        rm.assert_ticks_equal(got, want, name)
        np.testing.assert_array_equal(got_sum, want_sum, err_msg=name)
        # stance feet and leg_q: the input's bits
        np.testing.assert_array_equal(got["leg_q"].view(np.uint64), t["leg_q"].view(np.uint64))
        if not plant["flags"] & rm.PLANT_PLACE_FEET or name.startswith("standing"):
            np.testing.assert_array_equal(got["pFoot"].view(np.uint64), t["pFoot"].view(np.uint64))
        n += 1
    print(f"largest |rpy(det_atan2 / det_asin) - rpy(libm)| over {n} cases: {worst!r}")
    assert n == 48
    assert worst <= rm.RPY_TOL  # (fixed at 4 x the maximum measured when the test was written, rollout_mirror.RPY_MEASURED)


def test_per_instance_mass_and_push_against_the_mirror(exe, tmp_path):
    t, forces, status, wpd = rm.step_inputs("walking", 24)
    rng = np.random.default_rng(5)
    mass = np.where(np.arange(24) % 2 == 0, 9.0, 12.0)
    ext = rng.normal(0.0, 20.0, (24, 6))
    plant = rm.default_plant(flags=3, substeps=3)
    got, got_sum = run_on_host(exe, tmp_path, t, forces, status, wpd, plant, instance_mass=mass, ext_wrench=ext)
    want, want_sum = rm.plant_step(t, plant, rm.H, forces, status, wpd, instance_mass=mass, ext_wrench=ext)
    rm.assert_ticks_equal(got, want, "mass + push")
    np.testing.assert_array_equal(got_sum, want_sum)
    plain, _ = rm.plant_step(t, plant, rm.H, forces, status, wpd)
    assert (plain["vWorld"][3:] != want["vWorld"][3:]).any()


def test_struct_defaults_and_mirror_defaults_agree():
    """hmpc_default_plant (host code of the library: no GPU needed) fills what the mirror's default_plant holds"""
    p = interface.default_plant()
    d = rm.default_plant()
    assert bytes(p) == bytes(plant_struct(d))
    assert C.sizeof(_lib.Plant) == 144
