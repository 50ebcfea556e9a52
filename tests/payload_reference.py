"""References for a payload per robot on the contact plant (nmpc_contact_set_payloads) -- TEST INFRASTRUCTURE ONLY (helper module,
not collected by pytest), built on the existing numpy references without touching them.

The declaration: a payload row (m_p, r) on body `joint` is the tree whose body `joint` has mass m + m_p, centre of
mass (m c + m_p r) / (m + m_p) and the parallel-axis inertia about that point.  `baked` builds that tree in float64; everything
else here runs an existing reference (tests/fd_reference.py, contact_reference.py, implicit_reference.py, crba_reference.py) on
it, one robot at a time, in float64 and in float32."""
import copy

import numpy as np

from tests import contact_reference as cr
from tests import crba_reference as cb
from tests import fd_reference as fr
from tests import implicit_reference as ir


def _sym(i6):
    xx, xy, xz, yy, yz, zz = i6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float64)


def _point(m, d):
    """the inertia of a point mass m at d about the origin: m (|d|^2 1 - d d^T)"""
    return m * (d @ d * np.eye(3) - np.outer(d, d))


def baked(m, row, joint):
    """A copy of oracle tree `m` whose body `joint` carries the payload row (m_p, r_x, r_y, r_z), in float64.  A row with
    m_p = 0 returns the arrays of `m` unchanged, bit for bit."""
    mp, r = float(row[0]), np.asarray(row[1:4], np.float64)
    out = copy.deepcopy(m)
    if mp == 0.0:
        return out
    mass, c = float(m.mass[joint]), np.asarray(m.com[joint], np.float64)
    total = mass + mp
    c_new = (mass * c + mp * r) / total
    I = _sym(m.inertia[joint]) + _point(mass, c - c_new) + _point(mp, r - c_new)
    out.mass[joint] = total
    out.com[joint] = c_new
    out.inertia[joint] = I[np.triu_indices(3)]
    return out


def tree_arrays(m):
    """the keyword arguments of `BatchedTorqueLayer` for an oracle tree (tests.torque_helpers.layer takes the tree itself)"""
    return dict(parent=m.parent, joint_type=m.jtype, axis=m.axis, placement_R=m.R_fix, placement_p=m.p_fix, mass=m.mass, com=m.com,
                inertia=m.inertia, foot_joint=m.foot_joint, foot_offset=m.foot_offset, n_actuated=m.nu, gravity=m.gravity)


def payload_point(m, q, r, joint):
    """the world position of the payload point r of body `joint` at q, float64"""
    Rw, pw = m.forward_kinematics(np.asarray(q, np.float64))
    return pw[joint] + Rw[joint] @ np.asarray(r, np.float64)


def foot_point(m, q, k):
    return cr.feet(m, np.asarray(q, np.float64))[0][k]


def central_jacobian(point, q, h):
    """J [3, n] of point(q) by central differences with step h"""
    q = np.asarray(q, np.float64)
    J = np.zeros((3, len(q)))
    for i in range(len(q)):
        e = np.zeros(len(q)); e[i] = h
        J[:, i] = (point(q + e) - point(q - e)) / (2 * h)
    return J


def mass_matrix(m, q, dtype=np.float64):
    """M(q) of tree m by crba_reference's composite-rigid-body pass"""
    out = cb.crba(m, np.asarray(q, dtype), dtype=dtype)
    return out[0] if isinstance(out, (tuple, list)) else out


def step(m, g, rows, joint, q, v, dt, n_sub, tau, q_des, kp, kd, dtype=np.float64, implicit=False):
    """contact_step of every robot on its own baked tree -> [q, v, a, f, tau] stacked; float32: the float32 loop of the same
    reference (fd = fr.aba), `implicit`: tests/implicit_reference.py"""
    out = []
    for b in range(len(q)):
        mb = baked(m, rows[b], joint)
        if implicit:
            out.append(ir.implicit_step_ref(mb, g, q[b], v[b], dt, n_sub, tau[b], q_des[b], kp, kd, dtype=dtype)[:5])
        elif dtype is np.float64:
            out.append(cr.contact_step_ref(mb, g, q[b], v[b], dt, n_sub, tau[b], q_des[b], kp, kd))
        else:
            out.append(cr.contact_step_ref(mb, g, q[b], v[b], dt, n_sub, tau[b], q_des[b], kp, kd, fd=fr.aba, dtype=dtype))
    return [np.stack(x) for x in zip(*out)]


def track(m, g, rows, joint, q, v, A, dt, n_sub, tau, kp, kd, dtype=np.float64, implicit=False):
    """contact_track of every robot on its own baked tree: A[b, k] is the PD target of control step k -> [q, v, Q, V] stacked"""
    out = []
    for b in range(len(q)):
        qb, vb, Q, V = q[b], v[b], [], []
        for k in range(A.shape[1]):
            Q.append(np.array(qb)); V.append(np.array(vb))
            qb, vb = step(m, g, rows[b:b + 1], joint, qb[None], vb[None], dt, n_sub, tau[b:b + 1], A[b:b + 1, k], kp, kd, dtype, implicit)[:2]
            qb, vb = qb[0], vb[0]
        out.append((qb, vb, np.stack(Q), np.stack(V)))
    return [np.stack(x) for x in zip(*out)]
