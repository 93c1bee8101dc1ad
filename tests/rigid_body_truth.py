"""A single rigid body under constant world-frame loads, integrated from Newton-Euler in ``np.longdouble`` with classical RK4 -- the
independent truth the plant step (csrc/hmpc_plant.h) is measured against by tests/plant_physics_cases.py.

Written from the equations of motion, not from the plant's contract: no quaternion, none of the contract's operation order, nothing
imported from the mirror of that contract.  State per body: position p, velocity v, angular velocity w (all world frame) and the attitude
R_wb (body -> world, the transpose of the tick struct's ``rBody``):

    p' = v                       v' = F / m - g e_z                  R_wb' = [w]x R_wb
    F   = F_L + F_R + F_ext                                          (constant in the world frame over the tick)
    tau = (foot_L - p) x F_L + M_L + (foot_R - p) x F_R + M_R + tau_ext      (feet fixed in the world: the arm moves with the body)
    gyro off (the MPC's model):   w' = R_wb I^-1 R_wb^T tau
    gyro on  (Euler's equation):  w' = R_wb I^-1 (R_wb^T tau - w_b x I w_b),   w_b = R_wb^T w     (w' = R_wb w_b' because w x w = 0)

``VARIANTS`` are wrong on purpose, one mistake each; they exist only so that a test can show it tells them from the truth."""
import numpy as np

LD = np.longdouble
VARIANTS = ("gyro_sign", "arm_reversed", "no_contact_moments", "inertia_not_rotated", "attitude_rate_right")


def _ld(a):
    return np.asarray(a, dtype=LD)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _mv(M, x):
    return (M * x[..., None, :]).sum(-1)


def _mtv(M, x):  # M^T x
    return (M * x[..., :, None]).sum(-2)


def _hat(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def integrate(position, vWorld, omegaWorld, rBody, pFoot, forces, *, dt, mass, inertia, gravity, gyro, ext_wrench=None, steps=256,
              variant=None):
    """-> dict(position, vWorld, omegaWorld, rBody) after ``dt`` seconds, longdouble, leading dimension = batch.
    ``forces``: [batch, >= 12] (F_L, F_R, M_L, M_R, world frame); ``mass``: scalar or [batch]; ``ext_wrench``: [batch, 6] (force, torque about
    the centre of mass) or None; ``rBody``: [batch, 9] row-major, world -> body.  ``steps`` RK4 steps (>= 256 for a tick of 5 ms)."""
    assert variant is None or variant in VARIANTS, variant
    assert steps >= 1
    p, v, w = _ld(position).copy(), _ld(vWorld).copy(), _ld(omegaWorld).copy()
    nb = len(p)
    R = np.swapaxes(_ld(rBody).reshape(nb, 3, 3), 1, 2).copy()  # R_wb
    foot = _ld(pFoot).reshape(nb, 2, 3)
    u = _ld(np.asarray(forces).reshape(nb, -1)[:, :12])
    F_L, F_R, M_L, M_R = u[:, 0:3], u[:, 3:6], u[:, 6:9], u[:, 9:12]
    ext = np.zeros((nb, 6), dtype=LD) if ext_wrench is None else _ld(ext_wrench).reshape(nb, 6)
    m = np.broadcast_to(_ld(mass), (nb,))[:, None]
    I = _ld(inertia)
    g = np.array([0, 0, gravity], dtype=LD)
    if variant == "no_contact_moments":
        M_L, M_R = np.zeros_like(M_L), np.zeros_like(M_R)
    F = F_L + F_R + ext[:, 0:3]
    acc = F / m - g

    def rhs(p, v, w, R):
        arm_L, arm_R = foot[:, 0] - p, foot[:, 1] - p
        if variant == "arm_reversed":
            arm_L, arm_R = -arm_L, -arm_R
        tau = _cross(arm_L, F_L) + M_L + _cross(arm_R, F_R) + M_R + ext[:, 3:6]
        tau_b = _mtv(R, tau)
        if variant == "inertia_not_rotated":
            w_dot = tau / I
            tau_b = np.zeros_like(tau_b)
        else:
            w_dot = np.zeros_like(tau)
        if gyro:
            w_b = _mtv(R, w)
            gy = _cross(w_b, I * w_b)
            tau_b = tau_b + gy if variant == "gyro_sign" else tau_b - gy
        w_dot = w_dot + _mv(R, tau_b / I)
        R_dot = R @ _hat(w) if variant == "attitude_rate_right" else _hat(w) @ R
        return v, acc, w_dot, R_dot

    h = LD(dt) / LD(steps)
    for _ in range(steps):
        y = (p, v, w, R)
        k1 = rhs(*y)
        k2 = rhs(*[a + h / 2 * b for a, b in zip(y, k1)])
        k3 = rhs(*[a + h / 2 * b for a, b in zip(y, k2)])
        k4 = rhs(*[a + h * b for a, b in zip(y, k3)])
        p, v, w, R = [a + h / 6 * (b1 + 2 * b2 + 2 * b3 + b4) for a, b1, b2, b3, b4 in zip(y, k1, k2, k3, k4)]
    return dict(position=p, vWorld=v, omegaWorld=w, rBody=np.swapaxes(R, 1, 2).reshape(nb, 9))


def euler_zyx(orientation):
    """(roll, pitch, yaw) of a unit quaternion (scalar first, body -> world) in longdouble: the rotation matrix first, the angles from its
    entries (R_wb = Rz(yaw) Ry(pitch) Rx(roll)); the sine of the pitch is limited to [-0.99999, 0.99999] as the plant's contract limits it."""
    q = _ld(orientation)
    q = q / np.sqrt((q * q).sum(-1))[..., None]
    a, b, c, d = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r00, r10, r20 = a * a + b * b - c * c - d * d, 2 * (b * c + a * d), 2 * (b * d - a * c)
    r21, r22 = 2 * (c * d + a * b), a * a - b * b - c * c + d * d
    lim = LD(0.99999)  # (the binary64 constant of the contract)
    return np.stack([np.arctan2(r21, r22), np.arcsin(np.clip(-r20, -lim, lim)), np.arctan2(r10, r00)], -1)
