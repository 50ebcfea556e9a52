"""References for the tests of the ground-contact plant (nmpc_foot_kinematics_batch, nmpc_contact_forces_batch,
nmpc_contact_step_batch) -- TEST INFRASTRUCTURE ONLY, built on tests/fd_reference.py and oracle/torque_oracle.py without
touching either.

  feet              world position and velocity of every foot point from `TreeModel.forward_kinematics` and geometric Jacobian
                    columns (no recursion over body velocities, no finite differences).
  contact_law       the declared law of include/nmpc_torque.h in the number format of its arguments.
  contact_step_ref  the substeps of nmpc_contact_step_batch, shaped like `fd_reference.step_ref`: in float64 over `fd_ref` it is
                    the reference, in float32 over `aba` the measure of what the number format costs.
  drop              the settling run of tests/golden/contact_settle.npz: its inputs, stated once for the fixture script and the tests.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from oracle import torque_oracle as to
from tests import fd_reference as fr


@dataclass(frozen=True)
class Ground:
    """The fields of nmpc_contact_cfg; the defaults are the Python layer's (tau_max None: no limit)."""
    ground_z: float = 0.0
    stiffness: float = 1e4
    damping: float = 3.0
    mu: float = 0.8
    slip_velocity: float = 0.05
    tau_max: Optional[float] = None


def _forward_kinematics(m, q, t):
    """`TreeModel.forward_kinematics`; in another format than float64 the same pass with every operation in that format."""
    if t is np.float64:
        return m.forward_kinematics(q)
    Rw, pw = [None] * m.n, [None] * m.n
    for i in range(m.n):
        Rf, pf, ax = m.R_fix[i].astype(t), m.p_fix[i].astype(t), m.axis[i].astype(t)
        if m.jtype[i] == 0:
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=t)
            R, p = Rf @ (np.eye(3, dtype=t) + np.sin(q[i]) * K + (t(1) - np.cos(q[i])) * (K @ K)), pf
        else:
            R, p = Rf, pf + Rf @ (ax * q[i])
        par = m.parent[i]
        Rw[i], pw[i] = (R, p) if par < 0 else (Rw[par] @ R, pw[par] + Rw[par] @ p)
    return Rw, pw


def feet(m, q, v=None, dtype=np.float64):
    """(pos, vel) [n_feet, 3]: p = p_w[j] + R_w[j] r, and pd = sum over the joints k on the path from body j to the root of
    v_k (z_k x (p - p_w[k])) for a revolute joint, v_k z_k for a prismatic one (z_k the world axis of joint k)."""
    t = np.dtype(dtype).type
    q = np.asarray(q, t)
    v = np.zeros(m.n, t) if v is None else np.asarray(v, t)
    Rw, pw = _forward_kinematics(m, q, t)
    pos, vel = np.zeros((len(m.foot_joint), 3), t), np.zeros((len(m.foot_joint), 3), t)
    for f, j in enumerate(m.foot_joint):
        p = pw[j] + Rw[j] @ m.foot_offset[f].astype(t)
        k = j
        while k >= 0:
            z = Rw[k] @ m.axis[k].astype(t)
            vel[f] += v[k] * (np.cross(z, p - pw[k]) if m.jtype[k] == 0 else z)
            k = m.parent[k]
        pos[f] = p
    return pos, vel


def contact_law(g, pos, vel):
    """f [..., 3] for foot points at pos moving with vel [..., 3], every operation in the format of pos."""
    pos, vel = np.asarray(pos), np.asarray(vel)
    t = pos.dtype.type
    delta = t(g.ground_z) - pos[..., 2]
    fz = np.where(delta > 0, t(g.stiffness) * delta * np.maximum(t(0), t(1) - t(g.damping) * vel[..., 2]), t(0))
    s = -t(g.mu) * fz / np.sqrt(vel[..., 0] ** 2 + vel[..., 1] ** 2 + t(g.slip_velocity) ** 2)
    return np.stack([s * vel[..., 0], s * vel[..., 1], fz], axis=-1).astype(t)


def pd_torque(m, g, q, v, tau_ff, q_des, kp, kd, t=np.float64):
    """The PD law of step_ref, then the torque limit."""
    nu = m.nu
    tau = np.zeros(nu, t) if tau_ff is None else np.asarray(tau_ff, t).copy()
    if q_des is not None:
        tau = tau + t(kp) * (np.asarray(q_des, t) - q[m.n - nu:]) - t(kd) * v[m.n - nu:]
    if g.tau_max is not None and g.tau_max > 0:
        tau = np.clip(tau, -t(g.tau_max), t(g.tau_max))
    return tau


def contact_step_ref(m, g, q, v, dt, n_sub, tau_ff, q_des, kp, kd, fd=fr.fd_ref, dtype=np.float64, trace=None):
    """nmpc_contact_step_batch for one robot -> (q, v, a, f, tau), a, f, tau of the last substep.  trace: a list that takes
    (q, v) after every substep."""
    t = np.dtype(dtype).type
    q, v = np.array(q, t), np.array(v, t)
    a = f = tau = None
    for _ in range(n_sub):
        tau = pd_torque(m, g, q, v, tau_ff, q_des, kp, kd, t)
        f = contact_law(g, *feet(m, q, v, dtype))
        a = np.asarray(fd(m, q, v, tau, f), t) if fd is fr.fd_ref else fd(m, q, v, tau, f, dtype)
        v = v + t(dt) * a
        q = q + t(dt) * v
        if trace is not None:
            trace.append((q.copy(), v.copy()))
    return q, v, a, f, tau


def drop():
    """The settling run: the quadruped in its standing pose with the lowest foot 2 cm above the plane z = 0, held by
    tau_ff = the statics torques of the standing forces and the PD law on the standing joint angles, 2 000 substeps of 0.5 ms."""
    m = fr.quadruped()
    q, f = fr.standing(m)
    q[2] += 0.02 - feet(m, q)[0][:, 2].min()
    tau_ff = to.id_torques(m, q, np.zeros(m.n), np.zeros(m.n), f)[-m.nu:]
    q, tau_ff = q.astype(np.float32), tau_ff.astype(np.float32)      # what the device is handed
    return dict(m=m, g=Ground(), q=q, v=np.zeros(m.n, np.float32), tau_ff=tau_ff, q_des=fr.STAND.astype(np.float32), kp=20.0, kd=1.5, dt=5e-4, n_sub=2000)
