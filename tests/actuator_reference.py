"""References for an actuator per robot on the contact plant (nmpc_contact_set_actuators) -- TEST INFRASTRUCTURE ONLY (helper module,
not collected by pytest), built on tests/contact_reference.py, implicit_reference.py, fd_reference.py, crba_reference.py and
push_reference.py without touching them.

The declaration (include/nmpc_torque.h): under the row (kp, kd, damping, armature) one substep of a robot is
  1. the motor torque  tau = clamp(tau_ff + kp (q_des - q_j) - kd v_j)            (`motor_torque`: contact_reference.pd_torque with the row's gains)
  2. the joint torque  t = tau - damping v_j                                      (`joint_torque`)
  3. the dynamics of the tree whose joint-space inertia is M + D, D = armature on the actuated diagonal:
         a = (M + D)^-1 (M a_nominal(t)),  M from crba_reference.crba            (`accel`)
  4. under the implicit integrator M + D in place of M in A and rhs, dt (kd + damping) + dt^2 kp on the diagonal of the actuated
     joints the clamp did not cut with rhs_i -= dt kp v_i, and dt damping alone on the others   (`implicit_system`)
Every function runs in float64 (the reference) or, with dtype=np.float32, the same formula with every operation in float32 (the
measure of what the number format costs: the floor of `torque_helpers.bar`)."""
import numpy as np

from tests import contact_reference as cr
from tests import crba_reference as cb
from tests import fd_reference as fr
from tests import implicit_reference as ir
from tests import push_reference as pr

COLUMNS = ("kp", "kd", "damping", "armature")


def nominal(kp, kd):
    """the row under which the plant is the plant without a table"""
    return np.array([kp, kd, 0.0, 0.0])


def motor_torque(m, g, q, v, tau_ff, q_des, row, t=np.float64):
    """step 1: the PD law with the row's gains, then the law's torque limit -- what tau_out reports"""
    return cr.pd_torque(m, g, q, v, tau_ff, q_des, row[0], row[1], t)


def joint_torque(m, tau, v, row, t=np.float64):
    """step 2: the passive damping acts after the clamp"""
    return tau - t(row[2]) * v[m.n - m.nu:]


def armature(m, row, t=np.float64):
    """the diagonal of D [n]: the rotor inertia on the actuated joints, nothing on the base"""
    D = np.zeros(m.n, t)
    D[m.n - m.nu:] = t(row[3])
    return D


def accel(m, q, v, t_joint, f, row, dtype=np.float64, mm=None):
    """step 3: a = (M + D)^-1 (M a_nominal), a_nominal the forward dynamics of the nominal tree under the joint torque t_joint and
    the forces f.  mm: the tree a_nominal runs on where it has one more force point than m (a push: push_reference.pushed_tree);
    its M is m's.  A row without armature returns a_nominal as it is."""
    t = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    mm = m if mm is None else mm
    a = np.asarray(fr.fd_ref(mm, q, v, t_joint, f), t) if f64 else fr.aba(mm, q, v, t_joint, f, dtype)
    if float(row[3]) == 0.0:
        return a
    M = cb.crba(m, np.asarray(q, t), dtype=dtype)[0].astype(t)
    A = M + np.diag(armature(m, row, t))
    b = M @ a
    out = np.linalg.solve(A, b) if f64 else ir.cholesky_solve(A, b)
    assert out.dtype == np.dtype(dtype)
    return out


def implicit_system(m, g, q, v, dt, tau, a_exp, pd_law, row, dtype=np.float64, inside=None):
    """step 4: (A, rhs) of the substep -- implicit_reference.implicit_system under the row's gains (M, the feet, dt kd + dt^2 kp
    and -dt kp v on the joints the clamp did not cut), then D on the diagonal and D a_exp on the right, and dt damping on every
    actuated joint, cut or not"""
    t = np.dtype(dtype).type
    A, rhs = ir.implicit_system(m, g, q, v, dt, tau, a_exp, pd_law, row[0], row[1], dtype, inside=inside)
    D = armature(m, row, t)
    A = A + np.diag(D)
    rhs = rhs + D * np.asarray(a_exp, t)
    for j in range(m.n - m.nu, m.n):
        A[j, j] = A[j, j] + t(dt) * t(row[2])
    assert A.dtype == rhs.dtype == np.dtype(dtype)
    return A, rhs


def step(m, g, row, q, v, dt, n_sub, tau_ff, q_des, push=None, dtype=np.float64, implicit=False, trace=None):
    """nmpc_contact_step_batch for one robot under the actuator `row` -> (q, v, a, f, tau): a, f (the ground's) and tau (the motor
    torque) of the last substep.  push: None or a dict F [3], joint, first_substep, n_substeps, s0 (default 0) with the meaning of
    `push_reference.pushed_step_ref`.  trace: a list that takes (q, v) after every substep."""
    t = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    q, v = np.array(q, t), np.array(v, t)
    if push is not None:
        m5 = pr.pushed_tree(m, push["joint"])
        F = np.asarray(push["F"], t).reshape(1, 3)
    a = f = tau = None
    for i in range(n_sub):
        tau = motor_torque(m, g, q, v, tau_ff, q_des, row, t)
        tj = joint_torque(m, tau, v, row, t)
        f = cr.contact_law(g, *cr.feet(m, q, v, dtype))
        mm, ff = m, f
        if push is not None and push["first_substep"] <= push.get("s0", 0) + i < push["first_substep"] + push["n_substeps"]:
            mm, ff = m5, np.concatenate([f, F])
        a = accel(m, q, v, tj, ff, row, dtype, mm)
        if implicit:
            A, rhs = implicit_system(m, g, q, v, dt, tau, a, q_des is not None, row, dtype)
            a = np.linalg.solve(A, rhs) if f64 else ir.cholesky_solve(A, rhs)
        v = v + t(dt) * a
        q = q + t(dt) * v
        if trace is not None:
            trace.append((q.copy(), v.copy()))
    assert q.dtype == v.dtype == np.dtype(dtype)
    return q, v, a, f, tau


def _of(x, b):
    return x[b] if isinstance(x, (list, tuple)) else x


def step_batch(ms, gs, rows, q, v, dt, n_sub, tau, q_des, pushes=None, dtype=np.float64, implicit=False):
    """`step` of every robot under its own row -> [q, v, a, f, tau] stacked.  ms, gs, pushes: one for all, or a list with one per
    robot (the tree with its payload baked in, its own ground, its own push window)."""
    out = [step(_of(ms, b), _of(gs, b), rows[b], q[b], v[b], dt, n_sub, tau[b], q_des[b], _of(pushes, b), dtype, implicit) for b in range(len(q))]
    return [np.stack(x) for x in zip(*out)]


def track_batch(ms, gs, rows, q, v, A, dt, n_sub, tau, pushes=None, dtype=np.float64, implicit=False):
    """nmpc_contact_track_batch of every robot under its own row: A[b, k] is the PD target of control step k, whose substep i is
    substep k n_sub + i of the push window -> [q, v, Q, V] stacked"""
    out = []
    for b in range(len(q)):
        qb, vb, Q, V = q[b], v[b], [], []
        for k in range(A.shape[1]):
            Q.append(np.array(qb)); V.append(np.array(vb))
            push = _of(pushes, b)
            push = None if push is None else dict(push, s0=k * n_sub)
            qb, vb = step(_of(ms, b), _of(gs, b), rows[b], qb, vb, dt, n_sub, tau[b], A[b, k], push, dtype, implicit)[:2]
        out.append((qb, vb, np.stack(Q), np.stack(V)))
    return [np.stack(x) for x in zip(*out)]
