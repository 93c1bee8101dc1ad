"""The swing update of include/hector_mpc.h (the comment above ``struct hmpc_swing``) restated in Python floats with libm -- written from that
comment, step by step and with its numbering, not from csrc/hmpc_swing.h.  Python evaluates an expression as C does (parentheses first,
equal precedence from left to right) and its float is binary64 with correctly rounded + - * / sqrt, so everything the comment forms without
trigonometry comes out with the kernel's bits; what passes through sin / cos / asin / acos (libm here, csrc/hmpc_math.h there) agrees within
``TRIG_TOL``.

``TRIG_MEASURED`` is the largest difference between the CPU build of the kernel's header (tests/src/swing_on_host.cpp) and this mirror over
``cycle_cases()`` -- pFoot_w, p0, pDes, vDes, pFoot_b and q_des, instances with |foot_des_to_hip_roll[0]| < 1e-3 m left out of q_des[2]
(acos near 1 is ill-conditioned there: an ulp of its argument is up to 1.5e-8 rad) -- measured by tests/test_swing_kernel_on_host.py, which
prints it; ``TRIG_TOL`` is four times it (the plant's rule) and is the tolerance of that test and of tests/test_gpu_swing.py."""
import math

import numpy as np

from hector_simulation_amd import interface, synthetic

H = 10
PI3, PI = 3.14159, 3.141592653589793
TRIG_MEASURED = 2.8199664825478976e-14
TRIG_TOL = 4 * TRIG_MEASURED
# the largest |this mirror - the reference's own SwingLegController.cpp| (tests/golden/swing_update_ref.npz) in what passes through
# trigonometry or pow, over the gait cycles and the IK rows of tests/swing_update_cases.py: pow(x, 2) / pow(x, 0.5) against x * x / sqrt and
# libm's last bits.  Measured and printed by tests/test_swing_update_reference.py, which holds this mirror to four times it and the kernel to
# TRIG_TOL + four times it.  It is 2^-54: on this libm the mirror is the reference to the last bit almost everywhere, and four times it is one
# ulp at 1.0, less than an ulp of a q_des near -1.4 pi (8.9e-16) -- so the MIRROR's tolerance amounts to bit for bit, and a libm whose sin /
# cos / asin / acos differ in a last bit will fail the mirror's tests (not the kernel's, whose TRIG_TOL is 1.1e-13).  Re-measure there.
REF_MEASURED = 5.551115123125783e-17
F0_MIN = 1e-3  # |foot_des_to_hip_roll[0]| below which q_des[2] is left out of the tolerance comparison


def default_swing(**kw):
    c = dict(dt_update=0.001, dtMPC=0.04, updates=2, ticks_per_step=40, subtick=0, height=0.15, place_gain_v=1.75, place_gain_err=0.1,
             place_max=0.3, hip_yaw=[[-0.005, -0.057, -0.126], [-0.005, 0.057, -0.126]], hip_roll=[0.0465, 0.015, -0.0705],
             hip_width_offset=[[-0.015, 0.055, 0.0], [-0.015, -0.055, 0.0]], ik_link=0.22, ik_horizontal=0.0205, ik_hip_x=0.06,
             kp=[30.0, 30.0, 30.0, 30.0, 20.0], kd=[1.0, 1.0, 1.0, 1.0, 1.0])
    c.update(kw)
    return c


def swing_struct(c: dict):
    """the mirror's dict as struct hmpc_swing, without the library"""
    from hector_simulation_amd import _lib

    s = _lib.Swing()
    for k, v in c.items():
        if k in ("hip_yaw", "hip_width_offset"):
            for leg in range(2):
                getattr(s, k)[leg][:] = v[leg]
        elif k in ("hip_roll", "kp", "kd"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def sqrt(x):
    """IEEE sqrt: a negative argument gives NaN (math.sqrt raises)"""
    return math.sqrt(x) if x >= 0 else float("nan")


def clamp1(v):
    t = 1.0 if 1.0 < v else v
    return t if -1.0 < t else -1.0


def leg_q(tk, j):
    """step 1"""
    q = [float(x) for x in tk["leg_q"][5 * j:5 * j + 5]]
    if int(tk["flags"]) & interface.TICK_LEG_Q_MOTOR:
        q[2] = q[2] + 0.3 * PI3
        q[3] = q[3] - 0.6 * PI3
        q[4] = q[4] + 0.3 * PI3
    return q


def leg_p(q, side, toe=True):
    """step 2: data[leg].p; ``toe=False`` drops the two terms of the last link (the ankle's position: used by the IK identity test only)"""
    s0, c0, s1, c1, s2, c2, s3, c3, s4, c4 = [f(x) for x in q for f in (math.sin, math.cos)]
    A = c0 * c2 - s0 * s1 * s2
    B = c0 * s2 + c2 * s0 * s1
    C = c2 * s0 + c0 * s1 * s2
    D = s0 * s2 - c0 * c2 * s1
    t = 9 if toe else 0
    p0 = (-(3 * c0) / 200 - (t * s4 * (c3 * A - s3 * B)) / 250 - (11 * c0 * s2) / 50 - (side * s0) / 50 - (11 * c3 * B) / 50
          - (11 * s3 * A) / 50 - (t * c4 * (c3 * B + s3 * A)) / 250 - (23 * c1 * side * s0) / 1000 - (11 * c2 * s0 * s1) / 50)
    p1 = ((c0 * side) / 50 - (t * s4 * (c3 * C - s3 * D)) / 250 - (3 * s0) / 200 - (11 * s0 * s2) / 50 - (11 * c3 * D) / 50
          - (11 * s3 * C) / 50 - (t * c4 * (c3 * D + s3 * C)) / 250 + (23 * c0 * c1 * side) / 1000 + (11 * c0 * c2 * s1) / 50)
    p2 = ((23 * side * s1) / 1000 - (11 * c1 * c2) / 50 - (t * c4 * (c1 * c2 * c3 - c1 * s2 * s3)) / 250
          + (t * s4 * (c1 * c2 * s3 + c1 * c3 * s2)) / 250 - (11 * c1 * c2 * c3) / 50 + (11 * c1 * s2 * s3) / 50 - 3.0 / 50.0)
    return [p0, p1, p2]


def swing_phase(tk, c, h, j):
    """step 3"""
    cur = int(tk["gait_iteration"]) * c["ticks_per_step"] + c["subtick"]
    per = c["ticks_per_step"] * h
    phase = float(cur % per) / float(per)
    offP = float(int(tk["gait_offsets"][j])) / float(h)
    durP = float(int(tk["gait_durations"][j])) / float(h)
    so = offP + durP
    if so > 1:
        so = so - 1.
    sd = 1. - durP
    pr = phase - so
    if pr < 0:
        pr = pr + 1.
    return 0. if pr > sd else (0. if sd == 0 else pr / sd)


def bez(y0, yf, x):
    return y0 + (x * x * x + 3 * (x * x * (1 - x))) * (yf - y0)


def dbez(y0, yf, x):
    return (6 * x * (1 - x)) * (yf - y0)


def trajectory(p0, pf, height, swing):
    """step 6b, world frame: (pDes, vDes)"""
    pDes = [bez(p0[k], pf[k], swing) for k in range(2)] + [0.0]
    vDes = [dbez(p0[k], pf[k], swing) for k in range(2)] + [0.0]
    top = p0[2] + height
    if swing < 0.5:
        x = swing * 2
        pDes[2], vDes[2] = bez(p0[2], top, x), dbez(p0[2], top, x)
    else:
        x = swing * 2 - 1
        pDes[2], vDes[2] = bez(top, pf[2], x), dbez(top, pf[2], x)
    return pDes, vDes


def ik(pFoot_b, c, j, q2, q3, flip_side=False, flip_knee=False, pi3=False, info=None):
    """step 7.  ``flip_side`` / ``flip_knee``: two WRONG variants (the lateral offset on the other side; the knee bending the other way) that
    the geometry test must tell from the right one; ``pi3``: a third, PI3 where the three offsets have PI (8e-7 rad), which only the executed
    reference tells (tests/test_swing_update_reference.py).  ``info``: a dict that receives f and whether a clamp was active."""
    off = PI3 if pi3 else PI
    sideK = -1.0 if j == 0 else 1.0
    if flip_side:
        sideK = -sideK
    hr = [c["hip_roll"][0] - c["ik_hip_x"], 0.0, c["hip_yaw"][0][2] + c["hip_roll"][2] * 2]
    f = [pFoot_b[k] - hr[k] for k in range(3)]
    d3 = math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    dyz = math.sqrt(f[1] * f[1] + f[2] * f[2])
    dh, L = c["ik_horizontal"], c["ik_link"]
    m = dyz * dyz - dh * dh
    dv = math.sqrt(m if 0.00001 < m else 0.00001)
    dxz = sqrt(d3 * d3 - dh * dh)
    r1, r2 = dxz / (2.0 * L), dv / dxz
    a1, a2 = clamp1(r1), clamp1(r2)
    div = abs(f[0])
    if div == 0.0:
        div = 1e-6
    r3, r4, r5 = f[1] / dyz, dh * sideK / dyz, dxz / 2.0 / L
    out = [0.0] * 5
    out[1] = math.asin(clamp1(r3)) + math.asin(clamp1(r4))
    out[2] = math.acos(a1) - math.acos(a2) * f[0] / div
    out[3] = 2.0 * math.asin(clamp1(r5)) - PI
    if flip_knee:
        out[3] = -out[3]
    out[4] = -q3 - q2
    out[2] = out[2] - 0.3 * off
    out[3] = out[3] + 0.6 * off
    out[4] = out[4] - 0.3 * off
    if info is not None:
        info["f"] = f
        info["clamped"] = any(clamp1(r) != r for r in (r1, r2, r3, r4, r5)) or not 0.00001 < m
    return out


WRONG = ("flip_side", "flip_knee", "pi3", "swing_len_dur1", "timer_dtmpc")


def update(ticks, state, c, h=H, tau=None, wrong=()):
    """One launch: ``c['updates']`` updates per leg.  Returns (cmd MOTOR_CMD_DTYPE[nb], new state, detail [nb, 2, 16]); the inputs are left
    unchanged.  ``wrong``: names of ``WRONG`` -- deliberately wrong variants of this mirror (never of the product) that the reference test
    must tell from the right one: the three of ``ik``; ``swing_len_dur1``: h - durations[1] as the swing length (the reference: gait->_swing =
    h - durations[0]); ``timer_dtmpc``: the timer loses dtMPC per update (the reference: the constant _dt = 0.001)."""
    assert all(w in WRONG for w in wrong)
    nb = len(ticks)
    st = np.array(state, dtype=interface.SWING_STATE_DTYPE, copy=True)
    cmd = np.zeros(nb, dtype=interface.MOTOR_CMD_DTYPE)
    detail = np.zeros((nb, 2, 16))
    for i in range(nb):
        tk = ticks[i]
        R = [float(x) for x in tk["rBody"]]
        pos = [float(x) for x in tk["position"]]
        v = [float(x) for x in tk["vWorld"]]
        cx, cy = float(tk["v_des_robot"][0]), float(tk["v_des_robot"][1])
        dur0 = int(tk["gait_durations"][0])
        for j in range(2):
            q = leg_q(tk, j)  # 1
            hy = c["hip_yaw"][j]
            p = leg_p(q, 1.0 if j == 0 else -1.0)  # 2
            u = [hy[k] + p[k] for k in range(3)]
            pFoot_w = [pos[k] + (R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2]) for k in range(2)] + [0.0]
            swing = swing_phase(tk, c, h, j)  # 3
            first, timer = int(st["first_swing"][i, j]), float(st["swing_time"][i, j])
            p0, pf = [float(x) for x in st["p0"][i, j]], [float(x) for x in st["pf"][i, j]]
            vdw = [R[a] * cx + R[3 + a] * cy + R[6 + a] * 0.0 for a in range(2)]
            rh = [R[k] * hy[0] + R[3 + k] * hy[1] + R[6 + k] * hy[2] for k in range(3)]
            for _ in range(c["updates"]):
                if first:  # 4
                    timer = c["dtMPC"] * float(h - (int(tk["gait_durations"][1]) if "swing_len_dur1" in wrong else dur0))
                else:
                    timer = timer - (c["dtMPC"] if "timer_dtmpc" in wrong else c["dt_update"])
                    if timer <= 0:
                        first = 1
                for a in range(2):  # 5
                    Pf = (pos[a] + rh[a]) + v[a] * timer
                    rel = c["place_gain_v"] * v[a] * 0.5 * float(dur0) * c["dtMPC"] + c["place_gain_err"] * (v[a] - vdw[a])
                    r32 = max(np.float32(rel), np.float32(-c["place_max"]))
                    rel = float(min(r32, np.float32(c["place_max"])))
                    pf[a] = Pf + rel
                pf[2] = 0.0
                if swing > 0 and first:  # 6a
                    first = 0
                    p0 = list(pFoot_w)
            st["first_swing"][i, j], st["swing_time"][i, j] = first, timer
            st["p0"][i, j], st["pf"][i, j] = p0, pf
            pDes, vDes, pFoot_b, vFoot_b = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
            sl = slice(5 * j, 5 * j + 5)
            if swing > 0:
                pDes, vDes = trajectory(p0, pf, c["height"], swing)  # 6b
                d = [pDes[k] - pos[k] for k in range(3)]
                e = [vDes[k] * 0.0 - v[k] for k in range(3)]
                pFoot_b = [(R[3 * k] * d[0] + R[3 * k + 1] * d[1] + R[3 * k + 2] * d[2]) + c["hip_width_offset"][j][k] for k in range(3)]
                vFoot_b = [R[3 * k] * e[0] + R[3 * k + 1] * e[1] + R[3 * k + 2] * e[2] for k in range(3)]
                st["q_des"][i, sl] = ik(pFoot_b, c, j, q[2], q[3], **{w: True for w in wrong if w in WRONG[:3]})  # 7, 8
                cmd["Kp"][i, sl], cmd["Kd"][i, sl] = c["kp"], c["kd"]
            cmd["q"][i, sl] = st["q_des"][i, sl]
            if tau is not None:
                cmd["tau"][i, sl] = np.asarray(tau, dtype=np.float64).reshape(nb, 10)[i, sl]
            detail[i, j] = [swing] + pFoot_w + pDes + vDes + pFoot_b + vFoot_b
    return cmd, st, detail


# ------------------------------------------------------------------------------------------------ the shared cases
def walking_ticks(nb, seed, offsets=(0, 5), durations=(5, 5), motor=False, h=H):
    """``synthetic.make_ticks`` walking robots with the given gait, starting at gait_iteration 0; ``motor``: every other instance carries
    raw motor angles (HMPC_TICK_LEG_Q_MOTOR)."""
    t = synthetic.make_ticks(nb, h, "walking", seed=seed)
    t["gait_offsets"][:] = offsets
    t["gait_durations"][:] = durations
    t["gait_iteration"][:] = 0
    if motor:
        t["flags"][1::2] |= interface.TICK_LEG_Q_MOTOR
    return t


def drift(t, rng, k):
    """the ticks one tick later for a cycle test: the body moves a little (not a plant: any state sequence exercises the carried state)"""
    t = t.copy()
    t["position"][:, :2] += 0.005 * t["vWorld"][:, :2]
    t["vWorld"] += rng.normal(0.0, 0.01, t["vWorld"].shape)
    t["leg_q"] += rng.normal(0.0, 0.01, t["leg_q"].shape)
    return t


def ankle_rows(seed=0, n=4000):
    """(cfg, p [n, 3], leg [n], rows [n, 6] = pFoot_b, leg, q2, q3): body-frame foot positions p = hipYaw + a box reachable without any clamp
    of the IK, alternating legs -- the rows of the ankle identity (tests/test_swing_physics.py) and of the IK's reference pins"""
    c = default_swing()
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.08, 0.08, n), rng.uniform(-0.45, -0.28, n)], axis=1)
    leg = np.arange(n) % 2
    p = p + np.array(c["hip_yaw"])[leg]
    rows = np.concatenate([p + np.array(c["hip_width_offset"])[leg], leg[:, None].astype(np.float64), np.full((n, 1), 0.5), np.full((n, 1), -1.0)], axis=1)
    return c, p, leg, rows


def mid_swing_state(ticks, seed):
    """a state in mid swing: some legs before their first swing update, some timers about to run out, p0 / pf / q_des set"""
    rng = np.random.default_rng(seed)
    nb = len(ticks)
    st = interface.initial_swing_state(nb)
    st["first_swing"] = rng.integers(0, 3, (nb, 2)) == 0
    st["swing_time"] = np.where(rng.integers(0, 4, (nb, 2)) == 0, 0.0015, rng.uniform(0.0, 0.2, (nb, 2)))
    st["p0"][:, :, :2] = ticks["position"][:, None, :2] + rng.uniform(-0.2, 0.2, (nb, 2, 2))
    st["pf"][:, :, :2] = ticks["position"][:, None, :2] + rng.uniform(-0.2, 0.2, (nb, 2, 2))
    st["q_des"] = rng.uniform(-1.0, 1.0, (nb, 10))
    return st


def irregular_tables():
    """two (offsets, durations) of tests/irregular_gaits.py's ``border_ticks`` whose legs both swing for part of the cycle"""
    import irregular_gaits as ig

    t, _ = ig.border_ticks(H)
    out = []
    for i in range(len(t)):
        d, o = t["gait_durations"][i], t["gait_offsets"][i]
        if 0 < d[0] < H and 0 < d[1] < H and (tuple(o), tuple(d)) != ((0, 5), (5, 5)) and (tuple(int(x) for x in o), tuple(int(x) for x in d)) not in out:
            out.append((tuple(int(x) for x in o), tuple(int(x) for x in d)))
        if len(out) == 2:
            break
    assert len(out) == 2
    return out


def cycle_cases(nb=24):
    """[(name, offsets, durations)]: horizon 10, ticks_per_step 2, 20 ticks = one gait cycle"""
    return [("walk_0_5", (0, 5), (5, 5))] + [(f"irregular_{k}", o, d) for k, (o, d) in enumerate(irregular_tables())]


def cycle_inputs(name, offsets, durations, nb=24, n_ticks=20, tps=2):
    """the tick structs of every tick of a cycle case, [n_ticks] arrays of [nb], and the per-tick (gait_iteration advanced as a rollout does)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    t = walking_ticks(nb, seed=300 + len(name), offsets=offsets, durations=durations, motor=True)
    out = []
    for k in range(n_ticks):
        out.append(t)
        t = drift(t, rng, k)
        if (k + 1) % tps == 0:
            t["gait_iteration"] = (t["gait_iteration"] + 1) % H
    return out
