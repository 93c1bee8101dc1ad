"""numpy restatement (float64) of the model gradients' definition (include/hector_mpc.h hmpc_adjoint_model; csrc/hmpc_model_adjoint.h), fed
with the oracle's binary32 assembly of a record, a force vector and the adjoint mirror's dir; a float64 restatement of stage A2's B; and
what the model-gradient tests share.  numpy has no fma, so the GPU's chains differ from these by binary64 round-off only."""
import numpy as np

import adjoint_mirror as am
import certificate_mirror as cm
import feedback_mirror as fm
from hector_simulation_amd import records, synthetic

MIRROR_TOL = am.MIRROR_TOL
KEYS = ("grad_A", "grad_B", "grad_r", "grad_params", "costate")
MASS, INERTIA = 9.0, (np.float32(0.5413), np.float32(0.5200), np.float32(0.0691))  # hmpc_default_params
# Central differences of l.u* in the dense frozen-set QP (adjoint_mirror.DenseModel, anchored at the given forces; float64) at a step of
# FD_DENSE_STEP, each error relative to max(1, |value|) of what it is compared with (per output: max(1, max|output|)):
#   under random dA (entries uniform(-1, 1)), dB (uniform(-1, 1) Bcd[9][0]) against <G_A, dA> + <G_B, dB>:  DENSE_AB_E_MEASURED
#   under moves of r, mass and inertia through stage_a2_B (float64) against grad_r / grad_params:  DENSE_P_E_MEASURED
# The largest error measured over CASES (tests/test_model_adjoint_mirror.py prints it per shape); each bound is twice that.
FD_DENSE_STEP = 1e-6
DENSE_AB_E_MEASURED = 1.24e-7  # (walking; per shape 4.3e-8, 1.2e-7, 2.2e-8, 1.2e-7, 5.9e-9, 1.3e-8, 1.4e-8, 2.0e-8)
DENSE_P_E_MEASURED = 9.38e-7  # (hard_6x, inertia; r: 5.4e-7, 1.9e-7, 1.4e-7, 2.5e-7, 1.6e-7, 1.5e-7, 2.3e-7, 8.1e-7; the mass <= 2.3e-8;
#                               it holds the binary32 rounding of the assembled dt Iinv that the chain rules read, ~6e-8 of an entry)
DENSE_AB = 2 * DENSE_AB_E_MEASURED
DENSE_P = 2 * DENSE_P_E_MEASURED
# The irregular gait tables of tests/derived_irregular.py under random dA, dB: l.u* is more strongly curved there and the central
# difference's truncation, which falls with the square of the step, exceeds DENSE_AB at FD_DENSE_STEP (full_stance_except_one_leg_step at
# h = 10: 4.2e-5, 4.2e-7, 5.0e-8 at steps of 1e-5, 1e-6, 1e-7).  The reference is stepped finer; the bound stays.
FD_DENSE_STEP_IRREGULAR = 1e-7


def quat_to_R32(q):
    """quat_to_R of csrc/hmpc_kernel.h, operation for operation in binary32."""
    f = np.float32
    qw, qx, qy, qz = (f(v) for v in np.asarray(q, dtype=np.float32).reshape(4))
    tx, ty, tz = f(2) * qx, f(2) * qy, f(2) * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = f(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=np.float32)


def cross_matrix(rc):
    r0, r1, r2 = (float(v) for v in rc)
    return np.array([[0.0, -r2, r1], [r2, 0.0, -r0], [-r1, r0, 0.0]])


def stage_a2_B(r, R, nc, dt, mass=MASS, inertia=INERTIA):
    """Stage A2's Bcd in float64: r[3 nc] in the record's order [axis][contact], R the body rotation."""
    U = 6 * nc
    R = np.asarray(R, dtype=np.float64)
    Iinv = np.linalg.inv(R @ np.diag(np.asarray(inertia, dtype=np.float64)) @ R.T)
    rr = np.asarray(r, dtype=np.float64).reshape(3, nc)
    B = np.zeros((13, U))
    for c in range(nc):
        B[6:9, 3 * c:3 * c + 3] = dt * (Iinv @ cross_matrix(rr[:, c]))
        B[6:9, 3 * nc + 3 * c:3 * nc + 3 * c + 3] = dt * Iinv
        B[9:12, 3 * c:3 * c + 3] = (dt / mass) * np.eye(3)
    return B


def model_adjoint(Acd, Bcd, x0, weights, traj, u, dirn, r, q, nc, dt=synthetic.DT_MPC, mass=MASS):
    """The definition for one instance: u[h, U] the forces, dirn[h, U] the adjoint's dir, r[3 nc], q[4] of the record."""
    A, B = np.asarray(Acd, dtype=np.float64), np.asarray(Bcd, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    u, du = np.asarray(u, dtype=np.float64), np.asarray(dirn, dtype=np.float64)
    h, U = u.shape
    tr = np.concatenate([np.asarray(traj, dtype=np.float64).reshape(h, 12), np.zeros((h, 1))], axis=1)
    q2 = np.concatenate([w + w, [0.0]])
    with np.errstate(invalid="ignore", over="ignore"):
        x, dx = np.zeros((h + 1, 13)), np.zeros((h + 1, 13))
        x[0] = np.asarray(x0, dtype=np.float64)
        for i in range(h):
            x[i + 1] = A @ x[i] + B @ u[i]
            dx[i + 1] = A @ dx[i] + B @ du[i]
        c, d = np.zeros((h + 2, 13)), np.zeros((h + 2, 13))
        for j in range(h, 0, -1):
            e = x[j] - tr[j - 1]
            e[12] = 0.0
            c[j] = q2 * e + A.T @ c[j + 1]
            d[j] = q2 * dx[j] + A.T @ d[j + 1]
        GA, GB = np.zeros((13, 13)), np.zeros((13, U))
        for i in range(h):
            GA += np.outer(c[i + 1], dx[i]) + np.outer(d[i + 1], x[i])
            GB += np.outer(c[i + 1], du[i]) + np.outer(d[i + 1], u[i])
        Mb = B[6:9, 3 * nc:3 * nc + 3]
        rr = np.asarray(r, dtype=np.float32).astype(np.float64).reshape(3, nc)
        gr = np.zeros((3, nc))
        Gam = np.zeros((3, 3))
        gm = 0.0
        for k in range(nc):
            T = Mb.T @ GB[6:9, 3 * k:3 * k + 3]
            gr[:, k] = (T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1])
            gm += GB[9, 3 * k] + GB[10, 3 * k + 1] + GB[11, 3 * k + 2]
            Gam += GB[6:9, 3 * nc + 3 * k:3 * nc + 3 * k + 3] + GB[6:9, 3 * k:3 * k + 3] @ cross_matrix(rr[:, k]).T
        R = quat_to_R32(q).astype(np.float64)
        gp = np.zeros(4)
        gp[0] = 0.0 - (gm * B[9, 0]) / float(mass)
        for k in range(3):
            wk = Mb @ R[:, k]
            gp[1 + k] = 0.0 - (wk @ (Gam @ wk)) / float(np.float32(dt))
    return dict(grad_A=GA, grad_B=GB, grad_r=gr, grad_params=gp, costate=np.stack([c[1], d[1]]))


def model_adjoint_records(oracle, rec, h, nc, forces, dirs, gains=None, mu=None, mass=MASS):
    """The definition over a batch of packed records: dict of grad_A[b, 13, 13], grad_B[b, 13, U], grad_r[b, 3, nc], grad_params[b, 4],
    costate[b, 2, 13].  gains: feedback_mirror.gains_records on the same records (for Acd, Bcd, x0; computed here unless handed in)."""
    nb, U = rec.shape[0], 6 * nc
    g = gains if gains is not None else fm.gains_records(oracle, rec, h, nc, forces, mu=mu)
    un = records.unpack_records(rec, h, nc)
    rows = []
    for k in range(nb):
        unk = cm.unpacked_row(un, k)
        rows.append(model_adjoint(g["Acd"][k], g["Bcd"][k], g["x0"][k], unk["weights"], unk["traj"], np.asarray(forces[k]).reshape(h, U),
                                  np.asarray(dirs[k]).reshape(h, U), un["r"][k], un["q"][k], nc, mass=mass))
    return {key: np.stack([r[key] for r in rows]) for key in KEYS}


class MovedModel:
    """l.u* of the dense frozen-set QP (adjoint_mirror.DenseModel) as a function of (Acd, Bcd), the anchor of the base point kept: at the
    base point the given forces are the optimum, so d(l.u*) = dir . d(H u0 + g)."""

    def __init__(self, Acd, Bcd, Z, u0, x0, traj, w, al):
        self.A, self.B = np.asarray(Acd, dtype=np.float64), np.asarray(Bcd, dtype=np.float64)
        self.Z, self.u0, self.theta = Z, u0, (np.asarray(x0, dtype=np.float64), traj, w, al)
        self.c = am.DenseModel(self.A, self.B, Z, u0).anchor(*self.theta).c

    def value(self, ell, dA=None, dB=None):
        dm = am.DenseModel(self.A if dA is None else self.A + dA, self.B if dB is None else self.B + dB, self.Z, self.u0)
        dm.c = self.c
        return float(np.asarray(ell, dtype=np.float64).reshape(-1) @ dm.solution(*self.theta))

    def central(self, ell, dA=None, dB=None, step=FD_DENSE_STEP):
        """(value(+step d) - value(-step d)) / (2 step)"""
        s = lambda m, sg: None if m is None else sg * step * m
        return (self.value(ell, s(dA, 1.0), s(dB, 1.0)) - self.value(ell, s(dA, -1.0), s(dB, -1.0))) / (2.0 * step)


# Finite differences of the reference's qpOASES against grad_r.dr and grad_params.dtheta, E = |pred - act| / max(1, max|u0|) over the kept
# instances (equal active sets), per parameter group; the step is halved until at most feedback_mirror.FD_LEFT_OUT_CAP of a shape is left out.
#   r:      every foot coordinate moved by uniform(-FD_R_STEP, FD_R_STEP) metres in the record
#   params: mass and the three inertia entries multiplied by 1 + uniform(-FD_P_STEP, FD_P_STEP), one draw per shape (orc_set_params is
#           process-global)
# Bounds: 2 x the largest E measured over CASES (tests/test_model_adjoint_mirror.py prints them per shape); pooled over all kept instances
# sum|pred - act| / sum|act| < adjoint_mirror.FD_W_POOLED.
FD_R_STEP = 1e-3
FD_P_STEP = 1e-2
MADJ_FD_R_E_MEASURED = 9.95e-5  # (per shape 7.1e-6, 8.5e-7, 5.6e-6, 2.8e-6, 1.4e-7, 1.2e-5, 4.4e-5, 9.9e-5 at s = 1e-3; pooled ratio 0.082)
MADJ_FD_P_E_MEASURED = 7.29e-5  # (per shape 9.4e-6, 3.7e-7, 3.8e-6, 1.4e-6, 6.0e-7, 1.5e-5, 1.5e-5, 7.3e-5 at s = 1e-2; pooled ratio 0.074)
MADJ_FD_R = 2 * MADJ_FD_R_E_MEASURED
MADJ_FD_P = 2 * MADJ_FD_P_E_MEASURED
# (the irregular gait tables of tests/derived_irregular.py, batches 1, 3, 4: measured by tests/test_derived_irregular_mirror.py, the same factor)
MADJ_FD_R_E_MEASURED_IRREGULAR = 1.08e-5  # (per batch 4.9e-6, 4.3e-6, 1.1e-5; left out none, 1 of 4, none)
MADJ_FD_P_E_MEASURED_IRREGULAR = 1.83e-5  # (per batch 3.6e-6, 1.8e-5, 1.4e-5; none left out)
MADJ_FD_R_IRREGULAR = 2 * MADJ_FD_R_E_MEASURED_IRREGULAR
MADJ_FD_P_IRREGULAR = 2 * MADJ_FD_P_E_MEASURED_IRREGULAR
FD_POOLED = am.FD_W_POOLED
_fdm = {}


def moved_feet(rec, h, nc, seed, s):
    """The records with every foot coordinate moved by uniform(-s, s): (records, dr[b, 3, nc]) with dr taken between the binary32 values."""
    rng = np.random.default_rng(seed)
    un = records.unpack_records(rec, h, nc)
    f = {k: np.array(v, copy=True) for k, v in un.items()}
    f["r"] = (f["r"].astype(np.float64) + rng.uniform(-s, s, f["r"].shape)).astype(np.float32)
    dr = f["r"].astype(np.float64) - np.asarray(un["r"], dtype=np.float64)
    return records.pack_records(f, h, nc), dr.reshape(rec.shape[0], 3, nc)


def moved_params(seed, s):
    """(kwargs of oracle.set_params / BatchedMPC.set_params, dtheta[4]) with the deltas taken between the binary32 values."""
    rng = np.random.default_rng(seed)
    base = np.array([MASS] + [float(v) for v in INERTIA])
    new = (base * (1.0 + rng.uniform(-s, s, 4))).astype(np.float32)
    return dict(mass=float(new[0]), inertia=tuple(float(v) for v in new[1:])), new.astype(np.float64) - np.float32(base).astype(np.float64)


def fd_model_case(oracle, case, base_mirror):
    """Per group the moved problem of a case, qpOASES on both, the kept instances; shared by tests/test_model_adjoint_mirror.py and
    tests/test_gpu_model_adjoint.py, left unchanged.  base_mirror: test_feedback_mirror.mirror_case of the case."""
    name, h, nb, nc = case[0], case[2], case[3], case[4]
    if name in _fdm:
        return _fdm[name]
    rec = base_mirror["rec"]
    u0 = fm.qpoases_forces(oracle, rec, h, nc)
    out = dict(rec=rec, u0=u0)
    s = FD_R_STEP
    for _ in range(8):
        rec2, dr = moved_feet(rec, h, nc, 3000 + case[5], s)
        u1 = fm.qpoases_forces(oracle, rec2, h, nc)
        keep = fm.same_active_sets(base_mirror["m"]["active"], fm.gains_records(oracle, rec2, h, nc, u1.astype(np.float32))["active"])
        if (~keep).mean() <= fm.FD_LEFT_OUT_CAP:
            break
        s *= 0.5
    out["r"] = dict(rec2=rec2, dr=dr, u1=u1, keep=keep, s=s)
    s = FD_P_STEP
    for _ in range(8):
        kw, dth = moved_params(4000 + case[5], s)
        try:
            oracle.set_params(**kw)
            u1 = fm.qpoases_forces(oracle, rec, h, nc)
            act2 = fm.gains_records(oracle, rec, h, nc, u1.astype(np.float32))["active"]
        finally:
            oracle.set_params()
        keep = fm.same_active_sets(base_mirror["m"]["active"], act2)
        if (~keep).mean() <= fm.FD_LEFT_OUT_CAP:
            break
        s *= 0.5
    out["params"] = dict(kw=kw, dtheta=dth, u1=u1, keep=keep, s=s)
    _fdm[name] = out
    return out


def predicted_change(g, dr=None, dtheta=None):
    """Per instance sum grad_r.dr + grad_params.dtheta over the deltas given."""
    nb = g["grad_r"].shape[0]
    out = np.zeros(nb)
    if dr is not None:
        out += (g["grad_r"] * dr).reshape(nb, -1).sum(axis=1)
    if dtheta is not None:
        out += g["grad_params"] @ np.asarray(dtheta, dtype=np.float64)
    return out
