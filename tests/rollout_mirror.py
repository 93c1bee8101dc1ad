"""numpy restatement of the plant step, written from the comment above ``struct hmpc_plant`` in include/hector_mpc.h -- not from the
kernel (csrc/hmpc_plant.h).  numpy's binary64 element-wise operations are IEEE operations without contraction, and every expression below
is written in the comment's operation order, so every output is comparable with the kernel BIT FOR BIT -- except ``rpy``, which the kernel
evaluates with det_atan2 / det_asin (csrc/hmpc_math.h) and this file with numpy's libm: ``RPY_TOL``.

Also here: the plant as a plain dict (``default_plant``), and the one-step cases that the host test (tests/test_plant_kernel_on_host.py)
and the GPU test (tests/test_gpu_rollout.py) share (``step_cases``)."""
import numpy as np

from hector_simulation_amd import synthetic

TICK_FALLEN = 2
PLANT_GYRO, PLANT_PLACE_FEET = 1, 2
S_OK, S_OK_RELAXED = 0, 6

# Largest |rpy(kernel source on the host: det_atan2 / det_asin) - rpy(this mirror: numpy's libm)| over every case of step_cases(), measured
# on the CPU by tests/test_plant_kernel_on_host.py (which prints it): 2.2204460492503131e-16 (one ulp of a yaw in [0.25, 0.5); roll and pitch
# differ by less).  The tolerance is four times that maximum.
RPY_MEASURED = 2.2204460492503131e-16
RPY_TOL = 4 * RPY_MEASURED


def default_plant(**over):
    p = dict(dt_tick=0.005, dtMPC=0.04, substeps=1, advance_gait=0, flags=0, mass=9.0, inertia=(0.5413, 0.5200, 0.0691), gravity=9.81,
             hip=((-0.005, -0.057, -0.126), (-0.005, 0.057, -0.126)), fall_cos=0.5)
    p.update(over)
    return p


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], -1)


def _rbody(q):
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    M = [[1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
         [2 * (q1 * q2 + q0 * q3), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1)],
         [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 1 - 2 * (q1 * q1 + q2 * q2)]]
    return np.stack([M[c][r] for r in range(3) for c in range(3)], -1)  # R = transpose of M, row-major


def plant_step(ticks, plant, horizon, forces, status=None, wpd=None, summary=None, instance_mass=None, ext_wrench=None):
    """-> (ticks after one MPC tick, summary rows).  ``forces``: float32[batch, >= 12] (step 0 first); ``status``: uint32[batch] (None: all
    0); ``wpd``: float64[batch, 2] or None (the tick's own); ``summary``: int32[batch, 4] or None ({0, -1, 0, 0})."""
    t = ticks.copy()
    nb = len(t)
    status = np.zeros(nb, dtype=np.uint32) if status is None else np.asarray(status, dtype=np.uint32)
    row = np.tile(np.array([0, -1, 0, 0], dtype=np.int32), (nb, 1)) if summary is None else np.array(summary, dtype=np.int32)
    live = (t["flags"] & TICK_FALLEN) == 0
    m = np.full(nb, float(plant["mass"])) if instance_mass is None else np.asarray(instance_mass, dtype=np.float64)
    ext = np.zeros((nb, 6)) if ext_wrench is None else np.asarray(ext_wrench, dtype=np.float64).reshape(nb, 6)
    F_ext, tau_ext = ext[:, 0:3], ext[:, 3:6]
    I = np.array(plant["inertia"], dtype=np.float64)
    g = float(plant["gravity"])
    u0 = np.asarray(forces, dtype=np.float32).reshape(nb, -1)[:, :12].astype(np.float64)
    F_L, F_R, M_L, M_R = u0[:, 0:3], u0[:, 3:6], u0[:, 6:9], u0[:, 9:12]
    p, v, w, q = t["position"].copy(), t["vWorld"].copy(), t["omegaWorld"].copy(), t["orientation"].copy()
    R = t["rBody"].copy()
    foot = t["pFoot"].copy()
    cmd = t["v_des_robot"]
    vdw0 = np.stack([R[:, a] * cmd[:, 0] + R[:, 3 + a] * cmd[:, 1] + R[:, 6 + a] * 0.0 for a in range(2)], -1)
    d = float(plant["dt_tick"]) / float(int(plant["substeps"]))
    hd = 0.5 * d
    for _ in range(int(plant["substeps"])):
        r_L, r_R = foot[:, 0:3] - p, foot[:, 3:6] - p                                                       # 1
        tau = ((_cross(r_L, F_L) + M_L) + (_cross(r_R, F_R) + M_R)) + tau_ext                               # 2
        F = (F_L + F_R) + F_ext                                                                             # 3
        tb = np.stack([R[:, 3 * k] * tau[:, 0] + R[:, 3 * k + 1] * tau[:, 1] + R[:, 3 * k + 2] * tau[:, 2] for k in range(3)], -1)  # 4
        if plant["flags"] & PLANT_GYRO:                                                                     # 5
            wb = np.stack([R[:, 3 * k] * w[:, 0] + R[:, 3 * k + 1] * w[:, 1] + R[:, 3 * k + 2] * w[:, 2] for k in range(3)], -1)
            tb = tb - _cross(wb, I * wb)
        ab = tb / I                                                                                         # 6
        alpha = np.stack([R[:, k] * ab[:, 0] + R[:, 3 + k] * ab[:, 1] + R[:, 6 + k] * ab[:, 2] for k in range(3)], -1)
        a = F / m[:, None] + np.array([0.0, 0.0, -g])                                                       # 7
        w = w + d * alpha                                                                                   # 8
        v = v + d * a                                                                                       # 9
        p = p + d * v                                                                                       # 10
        q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]                                                 # 11
        w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
        e = np.stack([-(w0 * q1 + w1 * q2 + w2 * q3), (w0 * q0 + w1 * q3) - w2 * q2, (w1 * q0 + w2 * q1) - w0 * q3,
                      (w2 * q0 + w0 * q2) - w1 * q1], -1)
        q = q + hd * e
        n = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        q = q / n[:, None]
        R = _rbody(q)                                                                                       # 12
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2 * (q0 * q2 - q1 * q3)
    s = np.where(s < 0.99999, s, 0.99999)
    s = np.where(s < -0.99999, -0.99999, s)
    rpy = np.stack([np.arctan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2)), np.arcsin(s),
                    np.arctan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3))], -1)
    base = t["world_position_desired"] if wpd is None else np.asarray(wpd, dtype=np.float64).reshape(nb, 2)
    new_wpd = base + float(plant["dt_tick"]) * vdw0
    gi = t["gait_iteration"].copy()
    if plant["advance_gait"]:
        gi = (gi + 1) % horizon
    if plant["flags"] & PLANT_PLACE_FEET:
        vdw = np.stack([R[:, a] * cmd[:, 0] + R[:, 3 + a] * cmd[:, 1] + R[:, 6 + a] * 0.0 for a in range(2)], -1)
        stance_steps = t["gait_durations"][:, 0].astype(np.float64)
        for j in range(2):
            progress = gi % horizon - t["gait_offsets"][:, j]
            progress = np.where(progress < 0, progress + horizon, progress)
            swing = ~(progress < t["gait_durations"][:, j])
            hip = plant["hip"][j]
            rh = np.stack([R[:, k] * hip[0] + R[:, 3 + k] * hip[1] + R[:, 6 + k] * hip[2] for k in range(3)], -1)
            Pf = (p + rh) + v * 0.0
            rel = ((v[:, :2] * 0.5) * stance_steps[:, None]) * float(plant["dtMPC"]) + 0.02 * (v[:, :2] - vdw)
            rel = np.minimum(np.maximum(rel.astype(np.float32), np.float32(-0.4)), np.float32(0.4)).astype(np.float64)
            placed = np.concatenate([Pf[:, :2] + rel, np.zeros((nb, 1))], -1)
            foot[:, 3 * j:3 * j + 3] = np.where(swing[:, None], placed, foot[:, 3 * j:3 * j + 3])
    fell = R[:, 8] < float(plant["fall_cos"])
    # an instance that had fallen before keeps every bit of its tick struct and of its summary row
    for name, val in (("position", p), ("vWorld", v), ("omegaWorld", w), ("orientation", q), ("rBody", R), ("rpy", rpy), ("pFoot", foot),
                      ("world_position_desired", new_wpd)):
        t[name][live] = val[live]
    t["gait_iteration"][live] = gi[live]
    t["flags"][live & fell] |= TICK_FALLEN
    first = live & fell & (row[:, 1] < 0)
    row[first, 1] = row[first, 0]
    row[live, 0] += 1
    code = status & 0xFF
    row[live & (code != S_OK) & (code != S_OK_RELAXED), 2] += 1
    iters = ((status >> 8) & 0xFFF).astype(np.int32)
    row[:, 3] = np.where(live, np.maximum(row[:, 3], iters), row[:, 3])
    return t, row


def state_row(t):
    """the log's state row of a batch of ticks: rpy, position, omegaWorld, vWorld"""
    return np.concatenate([t["rpy"], t["position"], t["omegaWorld"], t["vWorld"]], -1)


BIT_FIELDS = ("position", "vWorld", "omegaWorld", "orientation", "rBody", "leg_q", "pFoot", "v_des_robot", "yaw_rate_des", "roll_des",
              "pitch_des", "world_position_desired", "gait_offsets", "gait_durations", "gait_iteration", "flags")


def assert_ticks_equal(got, want, what=""):
    """every field but rpy bit for bit, rpy within RPY_TOL; -> the largest rpy difference"""
    for k in BIT_FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{what}: {k}")
    diff = float(np.abs(got["rpy"] - want["rpy"]).max()) if len(got) else 0.0
    assert diff <= RPY_TOL, (what, diff)
    return diff


H = 10
GAITS, BATCHES, SUBSTEPS = ("standing", "walking"), (1, 24, 257), (1, 3)


def step_inputs(gait, nb, seed=90):
    """ticks of synthetic.make_ticks(seed 90) with made-up step-0 forces of order 50 N and 5 N m (force rows of 12 H floats, as a solve leaves
    them), random status words, a clamped world_position_desired; in batches of more than one, instance 1 has fallen before and instance 2
    lies at roll 1.2 rad (it falls on this step)."""
    t = synthetic.make_ticks(nb, H, gait, seed=seed)
    rng = np.random.default_rng(seed + 1000 + nb)
    forces = np.zeros((nb, 12 * H), dtype=np.float32)
    forces[:, 0:6] = rng.normal(0.0, 50.0, (nb, 6))
    forces[:, 6:12] = rng.normal(0.0, 5.0, (nb, 6))
    forces[:, 12:] = rng.normal(0.0, 50.0, (nb, 12 * H - 12))  # later steps: never read
    status = (rng.choice([0, 6, 1, 4, 5], size=nb) | (rng.integers(0, 80, size=nb) << 8) | (rng.integers(0, 64, size=nb) << 20)).astype(np.uint32)
    wpd = t["position"][:, :2] + rng.uniform(-0.05, 0.05, (nb, 2))
    if nb > 2:
        t["flags"][1] |= TICK_FALLEN
        rpy = t["rpy"][2].copy()
        rpy[0] = 1.2
        t["rpy"][2] = rpy
        t["orientation"][2] = synthetic.quat_from_rpy(rpy[0], rpy[1], rpy[2])
        t["rBody"][2] = synthetic.rotation_world_to_body(t["orientation"][2]).reshape(9)
    return t, forces, status, wpd


def step_cases():
    """(name, ticks, forces, status, wpd or None, plant dict): standing and walking, batches 1 / 24 / 257, every flag combination,
    substeps 1 and 3 (the gait advances, and the tick's own world_position_desired is used, in the cases with 3)."""
    for gait in GAITS:
        for nb in BATCHES:
            t, forces, status, wpd = step_inputs(gait, nb)
            for flags in range(4):
                for sub in SUBSTEPS:
                    plant = default_plant(flags=flags, substeps=sub, advance_gait=1 if sub == 3 else 0, dtMPC=synthetic.DT_MPC)
                    yield f"{gait}-b{nb}-f{flags}-s{sub}", t, forces, status, (wpd if sub == 1 else None), plant
