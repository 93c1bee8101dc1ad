"""The plant step kernel (``hmpc_plant_step_device`` through ``BatchedMPC.plant_step``) against physics it was not written from: the cases
and assertions of tests/test_plant_physics.py (shared: tests/plant_physics_cases.py), on the device.  The truth is tests/rigid_body_truth.py;
the reference's foot placement comes from the fixture tests/golden/foot_placement_ref.npz (recorded from the reference's own run() by
tests/golden/make_foot_placement_golden.py) -- nothing here reads the reference."""
import os

import numpy as np
import pytest

import plant_physics_cases as cases
from hector_simulation_amd import interface, synthetic

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _plant(d: dict):
    return interface.default_plant(**d)


@pytest.fixture(scope="module")
def step():
    mpc = interface.BatchedMPC(synthetic.DT_MPC, cases.rm.H, synthetic.F_MAX, 2 * cases.EDGE_N + 1)

    def one(ticks, forces, plant, instance_mass, ext_wrench):
        got, _ = mpc.plant_step(ticks, _plant(plant), forces=forces, status=np.zeros(len(ticks), dtype=np.uint32),
                                instance_mass=instance_mass, ext_wrench=ext_wrench)
        return got

    yield one
    mpc.close()


def _report(lines):
    for line in lines:
        print(line)


@pytest.mark.parametrize("gyro", [False, True])
def test_order_of_convergence_against_the_truth(step, gyro):
    _report(cases.check_convergence(step, gyro))


@pytest.mark.parametrize("gyro", [False, True])
def test_wrong_physics_is_told_from_the_truth(step, gyro):
    _report(cases.check_teeth(step, gyro))


@pytest.mark.parametrize("substeps", [1, 4])
def test_pure_yaw_spin_is_exact(step, substeps):
    _report(cases.check_yaw_spin(step, substeps))


@pytest.mark.parametrize("substeps", [1, 3])
def test_free_fall_and_torque_free_spin(step, substeps):
    _report(cases.check_free_fall(step, substeps))


@pytest.mark.parametrize("gyro", [False, True])
def test_attitude_representation(step, gyro):
    _report(cases.check_attitude_representation(step, gyro))


def test_momentum_and_energy_drift_is_first_order(step):
    _report(cases.check_conservation(step))


def test_foot_placement_against_the_recorded_reference(step):
    z = np.load(os.path.join(HERE, "golden", cases.FOOT_GOLDEN))
    t = z["ticks"].reshape(-1).view(interface.TICK_DTYPE).copy()
    _report(cases.check_foot_placement(step, t, z["pf_ref"], z["swing_time"]))


def test_pitch_edge_is_finite_and_flagged(step):
    _report(cases.check_pitch_edge(step))
