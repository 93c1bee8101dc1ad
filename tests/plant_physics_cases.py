"""The plant step (csrc/hmpc_plant.h) against physics it was not written from: the cases and assertions shared by the CPU test
(tests/test_plant_physics.py: the kernel's source built for the host) and the GPU test (tests/test_gpu_plant_physics.py: the kernel).

Every check takes ``step(ticks, forces, plant_dict, instance_mass, ext_wrench) -> ticks after one tick`` and returns the lines it measured
(the callers print them); the truth is tests/rigid_body_truth.py (Newton-Euler, RK4, longdouble, no quaternion)."""
import functools

import numpy as np

import rigid_body_truth as truth
import rollout_mirror as rm
from hector_simulation_amd import interface, synthetic

LD = np.longdouble
NB = 8
TILTED, PUSHED, HEAVY = 3, 4, 5
SUBSTEPS = (1, 2, 4, 8, 16, 32, 64)
FLOAT_FIELDS = tuple(k for k in interface.TICK_DTYPE.names if interface.TICK_DTYPE[k].base.kind == "f")


def _set_attitude(t, i, roll, pitch, yaw):
    t["rpy"][i] = (roll, pitch, yaw)
    t["orientation"][i] = synthetic.quat_from_rpy(roll, pitch, yaw)
    t["rBody"][i] = synthetic.rotation_world_to_body(t["orientation"][i]).reshape(9)


def inputs():
    """rollout_mirror.step_inputs("standing", 8) with no instance fallen, + instance 3 tilted to rpy (0.3, -0.2, 0.7) and spinning with
    (3, -2, 4) rad/s, instance 4 pushed with a wrench of 20 N / 20 N m scale, instance 5 of mass 12 -> (ticks, forces, mass, ext)"""
    t, forces, _, _ = rm.step_inputs("standing", NB)
    t["flags"] = 0
    _set_attitude(t, TILTED, 0.3, -0.2, 0.7)
    t["omegaWorld"][TILTED] = (3.0, -2.0, 4.0)
    mass = np.full(NB, 9.0)
    mass[HEAVY] = 12.0
    ext = np.zeros((NB, 6))
    ext[PUSHED] = np.random.default_rng(28).normal(0.0, 20.0, 6)
    return t, forces, mass, ext


def plant(**over):
    return rm.default_plant(**dict(dict(fall_cos=-2.0, flags=0), **over))


@functools.lru_cache(maxsize=None)
def _truth(gyro, variant=None):
    t, forces, mass, ext = inputs()
    d = plant()
    return truth.integrate(t["position"], t["vWorld"], t["omegaWorld"], t["rBody"], t["pFoot"], forces, dt=d["dt_tick"], mass=mass,
                           inertia=d["inertia"], gravity=d["gravity"], gyro=gyro, ext_wrench=ext, steps=256, variant=variant)


def _err(got, want, k, who=slice(None)):
    """largest Euclidean distance over the instances (longdouble)"""
    d = (LD(1) * got[k][who] - want[k][who]).reshape(len(got[k][who]), -1)
    return float(np.sqrt((d * d).sum(-1)).max())


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------- a. order of convergence
def check_convergence(step, gyro):
    """first order: the error against the truth halves with every doubling of the sub-steps, ratio in [1.9, 2.1] for p, omega and rBody;
    v is exact up to rounding (the force is constant): |v - truth| <= 2 s 2^-53 max(1, |v|).  The truth starts from the INPUT rBody, the
    kernel recomputes rBody from the orientation: a convention that disagrees is an O(1) error here."""
    t, forces, mass, ext = inputs()
    want = _truth(gyro)
    lines, errs = [], {k: [] for k in ("position", "omegaWorld", "rBody")}
    worst_v = 0.0
    for s in SUBSTEPS:
        got = step(t, forces, plant(substeps=s, flags=rm.PLANT_GYRO if gyro else 0), mass, ext)
        for k in errs:
            errs[k].append(_err(got, want, k))
        dv = np.abs(LD(1) * got["vWorld"] - want["vWorld"])
        bound = 2 * s * 2.0 ** -53 * np.maximum(1.0, np.abs(got["vWorld"]))
        worst_v = max(worst_v, float(dv.max()))
        assert (dv <= bound).all(), (s, float(dv.max()), float(bound.min()))
    lines.append(f"gyro {int(gyro)}: largest |v - truth| over s = 1..64: {worst_v:.3e}")
    for k, e in errs.items():
        ratios = [e[i] / e[i + 1] for i in range(len(e) - 1)]
        lines.append(f"gyro {int(gyro)} {k}: error at s = 1 {e[0]:.3e}, at s = 64 {e[-1]:.3e}, ratios e(s) / e(2 s) " +
                     " ".join(f"{r:.4f}" for r in ratios))
        assert e[0] < 0.1, (k, e[0])  # (an O(1) error is a convention mismatch, not a truncation error)
        assert all(1.9 <= r <= 2.1 for r in ratios), (k, ratios)
    return lines


# ---------------------------------------------------------------------------------------------- b. the comparison has teeth
def check_teeth(step, gyro):
    """the tilted, spinning instance at s = 64: the kernel's omega is at least 10 x farther from every wrong-on-purpose truth than from the
    right one (the gyro-sign variant differs from the truth with HMPC_PLANT_GYRO only)"""
    t, forces, mass, ext = inputs()
    who = slice(TILTED, TILTED + 1)
    flags = rm.PLANT_GYRO if gyro else 0
    got = {s: step(t, forces, plant(substeps=s, flags=flags), mass, ext) for s in (16, 64)}
    right = _err(got[64], _truth(gyro), "omegaWorld", who)
    lines = [f"gyro {int(gyro)}: |omega - truth| at s = 64 {right:.3e}, e(16) / e(64) {_err(got[16], _truth(gyro), 'omegaWorld', who) / right:.3f}"]
    assert right < 1e-3
    for variant in truth.VARIANTS:
        if variant == "gyro_sign" and not gyro:
            continue
        wrong = _truth(gyro, variant)
        e64, e16 = _err(got[64], wrong, "omegaWorld", who), _err(got[16], wrong, "omegaWorld", who)
        lines.append(f"gyro {int(gyro)} against '{variant}': {e64:.3e} = {e64 / right:.1f} x, e(16) / e(64) {e16 / e64:.3f}")
        assert e64 >= 10 * right, (variant, e64, right)
    return lines


# ---------------------------------------------------------------------------------------------- c. closed forms
def check_yaw_spin(step, substeps):
    """q = (1, 0, 0, 0), omega = (0, 0, 2), no forces: every sub-step of length d turns the body by exactly 2 atan(omega d / 2) about z"""
    t, forces, mass, ext = inputs()
    t, forces = t[:1].copy(), np.zeros_like(forces[:1])
    t["orientation"][0], t["rBody"][0], t["rpy"][0] = (1, 0, 0, 0), np.eye(3).reshape(9), 0.0
    t["omegaWorld"][0] = (0.0, 0.0, 2.0)
    d = plant(substeps=substeps)
    worst = [0.0, 0.0]
    for k in range(10):
        t = step(t, forces, d, None, None)
        n = (k + 1) * substeps
        yaw = 2 * n * np.arctan(LD(2.0) * (LD(d["dt_tick"]) / substeps) / 2)
        q = LD(1) * t["orientation"][0]
        from_q = 2 * np.arctan2(q[3], q[0])
        tol = 4 * n * _ulp(float(yaw))
        diffs = [abs(float(LD(t["rpy"][0, 2]) - yaw)), abs(float(from_q - yaw))]
        worst = [max(a, b) for a, b in zip(worst, diffs)]
        assert max(diffs) <= tol, (k, diffs, tol)
        assert (t["orientation"][0, 1:3] == 0).all() and (t["rpy"][0, :2] == 0).all()
    return [f"yaw spin, substeps {substeps}, 10 ticks: largest |rpy[2] - 2 n atan(w d / 2)| {worst[0]:.3e}, from the quaternion {worst[1]:.3e}"]


def check_free_fall(step, substeps):
    """no forces: v and p are the discrete sums of -g d, omega keeps its bits without GYRO"""
    t, forces, mass, ext = inputs()
    forces = np.zeros_like(forces)
    d = plant(substeps=substeps)
    dd = LD(d["dt_tick"] / substeps)  # (the contract's d is the binary64 quotient)
    got = t
    v, p = LD(1) * t["vWorld"], LD(1) * t["position"]
    worst = [0.0, 0.0]
    for k in range(5):
        got = step(got, forces, d, mass, None)
        n = (k + 1) * substeps
        for _ in range(substeps):
            v = v - dd * np.array([0, 0, LD(d["gravity"])])
            p = p + dd * v
        for i, (name, want) in enumerate((("vWorld", v), ("position", p))):
            once = want.astype(np.float64)
            ulps = np.abs(got[name] - once) / np.maximum(_ulp(once), np.finfo(np.float64).tiny)
            worst[i] = max(worst[i], float(ulps.max()) / n)
            assert (ulps <= 2 * n).all(), (name, k, float(ulps.max()))
        np.testing.assert_array_equal(got["omegaWorld"].view(np.uint64), t["omegaWorld"].view(np.uint64))
    return [f"free fall, substeps {substeps}, 5 ticks: largest error / (n ulp) of v {worst[0]:.3f}, of p {worst[1]:.3f}"]


def check_attitude_representation(step, gyro):
    """|q| = 1 within 2 ulp, rBody orthonormal within 8 ulp, rpy = the Euler angles of the kernel's own orientation within RPY_TOL"""
    t, forces, mass, ext = inputs()
    got = step(t, forces, plant(substeps=3, flags=rm.PLANT_GYRO if gyro else 0), mass, ext)
    eps = 2.0 ** -52
    q = LD(1) * got["orientation"]
    norm = float(np.abs(np.sqrt((q * q).sum(-1)) - 1).max())
    R = (LD(1) * got["rBody"]).reshape(NB, 3, 3)
    orth = float(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max())
    rpy = float(np.abs(LD(1) * got["rpy"] - truth.euler_zyx(got["orientation"])).max())
    assert norm <= 2 * eps and orth <= 8 * eps and rpy <= rm.RPY_TOL, (norm, orth, rpy)
    return [f"gyro {int(gyro)}: | |q| - 1 | {norm:.3e}, |rBody rBody' - I| {orth:.3e}, |rpy - Euler angles of the orientation| {rpy:.3e}"]


# ---------------------------------------------------------------------------------------------- d. conservation
def check_conservation(step):
    """GYRO on, no forces, 20 ticks, the spinning instance: the drift of the angular momentum L = R' I R omega and of the rotational energy
    is first order in the sub-step: it halves per doubling of s, ratios in [1.9, 2.1] for s = 1 .. 16"""
    t, forces, mass, ext = inputs()
    t, forces = t[TILTED:TILTED + 1].copy(), np.zeros_like(forces[TILTED:TILTED + 1])
    I = LD(1) * np.array(plant()["inertia"])

    def L_and_E(tk):
        R = (LD(1) * tk["rBody"][0]).reshape(3, 3)
        w = LD(1) * tk["omegaWorld"][0]
        L = R.T @ (I * (R @ w))
        return L, w @ L / 2

    L0, E0 = L_and_E(t)
    dL, dE = [], []
    for s in (1, 2, 4, 8, 16):
        got = t
        for _ in range(20):
            got = step(got, forces, plant(substeps=s, flags=rm.PLANT_GYRO), None, None)
        L1, E1 = L_and_E(got)
        dL.append(float(np.sqrt(((L1 - L0) ** 2).sum()) / np.sqrt((L0 ** 2).sum())))
        dE.append(float((E1 - E0) / E0))
    lines = []
    for name, e in (("|dL| / |L|", dL), ("dE / E", dE)):
        ratios = [e[i] / e[i + 1] for i in range(len(e) - 1)]
        lines.append(f"{name} for s = 1 .. 16: " + " ".join(f"{x:.3e}" for x in e) + "; ratios " + " ".join(f"{r:.4f}" for r in ratios))
        assert all(1.9 <= r <= 2.1 for r in ratios), (name, ratios)
    return lines


# ---------------------------------------------------------------------------------------------- foot placement against the reference's run()
FOOT_NB = 16
FOOT_GOLDEN = "foot_placement_ref.npz"
# Pf_ref - vWorld (dtMPC swing) against the plant's pFoot: the reference rounds p + R' hip, + vWorld T and + rel, the plant p + R' hip and
# + rel, the comparison the product vWorld T and its subtraction -- at most five roundings that are not shared, each of a quantity below 4 in
# magnitude, so each at most 2^-51 (half an ulp of [2, 4)) and 5 * 2^-50 bounds their sum with a factor of two to spare.  (R' hip and the
# rotated command are sums of three products below 0.2 and 0.5: their roundings, and the plant's re-evaluation of rBody from the orientation,
# are below 2^-54 each and live in that spare factor.)
FOOT_TOL = 5 * 2.0 ** -50


def foot_inputs():
    """16 walking ticks of synthetic.make_ticks (seed 41), every command nonzero, every gait phase, both legs in swing in turn; instances 0
    and 1 move at 4.4 .. 4.7 m/s, which drives the heuristic's offset beyond its clamp of 0.4 m on both sides and both axes"""
    t = synthetic.make_ticks(FOOT_NB, rm.H, "walking", seed=41)
    t["flags"] = 0
    t["gait_iteration"] = np.arange(FOOT_NB) % rm.H
    cmd = t["v_des_robot"]
    cmd[cmd == 0] = 0.15
    t["v_des_robot"] = cmd
    t["vWorld"][0, :2] = (4.5, -4.4)
    t["vWorld"][1, :2] = (-4.6, 4.7)
    return t


def check_foot_placement(step, t, pf_ref, swing_time):
    """``pf_ref`` [16, 2, 3], ``swing_time`` [16, 2]: what the reference's own run() handed to footSwingTrajectories[leg] for these ticks and
    the swingTimeRemaining it extrapolated the hip over.  The plant places a foot on the tick it touches down (swing time remaining 0), so
    Pf_ref - vWorld * (dtMPC * swing) must be the plant's pFoot; dt_tick = 0 keeps the state where the reference saw it."""
    d = plant(flags=rm.PLANT_PLACE_FEET, dt_tick=0.0, dtMPC=synthetic.DT_MPC)
    got = step(t, np.zeros((len(t), 12), dtype=np.float32), d, None, None)
    for k in ("position", "vWorld", "omegaWorld"):
        np.testing.assert_array_equal(got[k].view(np.uint64), t[k].view(np.uint64), err_msg=k)
    assert (swing_time == synthetic.DT_MPC * (rm.H - t["gait_durations"][:, :1])).all()
    worst, placed, clamped = 0.0, 0, [0, 0]
    R = t["rBody"].reshape(-1, 3, 3)
    for j in range(2):
        progress = (t["gait_iteration"] % rm.H - t["gait_offsets"][:, j]) % rm.H
        swing = ~(progress < t["gait_durations"][:, j])
        np.testing.assert_array_equal(got["pFoot"][~swing, 3 * j:3 * j + 3].view(np.uint64), t["pFoot"][~swing, 3 * j:3 * j + 3].view(np.uint64))
        want = LD(1) * pf_ref[swing, j, :2] - LD(1) * t["vWorld"][swing, :2] * swing_time[swing, j, None]
        diff = np.abs(got["pFoot"][swing, 3 * j:3 * j + 2] - want)
        worst = max(worst, float(diff.max()))
        assert (got["pFoot"][swing, 3 * j + 2] == 0).all() and (pf_ref[swing, j, 2] == 0).all()
        rel = got["pFoot"][swing, 3 * j:3 * j + 2] - (t["position"][swing] + np.einsum("bki,k->bi", R[swing], np.array(d["hip"][j])))[:, :2]
        clamped[0] += int((np.abs(rel - float(np.float32(0.4))) < 1e-12).sum())
        clamped[1] += int((np.abs(rel + float(np.float32(0.4))) < 1e-12).sum())
        placed += int(swing.sum())
    line = (f"foot placement: {placed} feet placed, largest |Pf_ref - vWorld (dtMPC swing) - pFoot| {worst:.3e} = {worst / FOOT_TOL:.3f} of the "
            f"bound {FOOT_TOL:.3e}; offsets at the clamp +0.4: {clamped[0]}, -0.4: {clamped[1]}")
    assert worst <= FOOT_TOL, line
    assert placed == FOOT_NB and clamped[0] >= 2 and clamped[1] >= 2, line
    return [line]


# ---------------------------------------------------------------------------------------------- the pitch +-90 degree edge
EDGE_N = 2000
PITCH_LEFT = float(np.arcsin(LD(1)) - np.arcsin(LD(0.99999)))  # what a clamp of the sine at +-0.99999 leaves: 0.0044721...
PITCH_TOL = 0.0045
assert PITCH_LEFT < PITCH_TOL < 1.01 * PITCH_LEFT


def edge_inputs():
    """2000 attitudes quat_from_rpy(roll, -pi/2 + eps, yaw), |eps| <= 3e-8, their mirror images at +pi/2 and one exact
    q = (sqrt(1/2), 0, -sqrt(1/2), 0); |omega| ~ 1e-6, no forces -> (ticks, forces, the pitch each one lies at)"""
    rng = np.random.default_rng(5)
    nb = 2 * EDGE_N + 1
    t = synthetic.make_ticks(nb, rm.H, "standing", seed=90)
    t["flags"] = 0
    roll, yaw = rng.uniform(-np.pi, np.pi, EDGE_N), rng.uniform(-np.pi, np.pi, EDGE_N)
    eps = rng.uniform(-3e-8, 3e-8, EDGE_N)
    side = np.concatenate([np.full(EDGE_N, -1.0), np.full(EDGE_N, 1.0), [-1.0]])
    q = np.concatenate([synthetic.quat_from_rpy(roll, -np.pi / 2 + eps, yaw), synthetic.quat_from_rpy(roll, np.pi / 2 - eps, yaw),
                        np.array([[np.sqrt(0.5), 0.0, -np.sqrt(0.5), 0.0]])])
    t["orientation"] = q
    t["rBody"] = np.stack([synthetic.rotation_world_to_body(x).reshape(9) for x in q])
    t["omegaWorld"] = rng.normal(0.0, 1e-6, (nb, 3))
    t["vWorld"] = 0.0
    return t, np.zeros((nb, 12), dtype=np.float32), side * (np.pi / 2)


def check_pitch_edge(step):
    t, forces, pitch = edge_inputs()
    lines = []
    for fall_cos in (-2.0, rm.default_plant()["fall_cos"]):
        got = step(t, forces, plant(fall_cos=fall_cos), None, None)
        bad = sum(int((~np.isfinite(got[k])).reshape(len(got), -1).any(axis=1).sum()) for k in FLOAT_FIELDS)
        off = np.abs(got["rpy"][:, 1] - pitch)
        lines.append(f"fall_cos {fall_cos}: instances with a non-finite float {bad} of {len(got)}, largest |rpy[1] -+ pi/2| "
                     f"{np.nanmax(off):.7f} (asin(1) - asin(0.99999) = {PITCH_LEFT:.7f}, bound {PITCH_TOL})")
        assert bad == 0, lines[-1]
        assert (off <= PITCH_TOL).all(), lines[-1]
        fallen = (got["flags"] & rm.TICK_FALLEN) != 0
        assert fallen.all() if fall_cos > 0 else not fallen.any()
    return lines
