"""References for the tests of the push on the ground-contact plant (nmpc_contact_set_push) -- TEST INFRASTRUCTURE ONLY, built on
tests/fd_reference.py, tests/contact_reference.py and oracle/torque_oracle.py without touching them.

A push is a world-frame force with no moment at the origin of the body frame of a joint: to every forward-dynamics reference here
that is one more foot, on that joint, at offset 0.

  pushed_tree      a copy of an oracle tree with that extra foot (the last one).
  push_jacobian    J [3, n] of the push point: column k is its velocity under v = e_k, computed as `contact_reference.feet` does.
  pushed_step_ref  the substeps of nmpc_contact_step_batch under a push, shaped like `contact_reference.contact_step_ref`: a pushed
                   substep is fd(pushed tree, q, v, tau, concat(contact_law(the tree's own feet), F)), any other substep is
                   contact_step_ref's, operation for operation.  In float64 over `fd_ref` it is the reference, in float32 over
                   `aba` the measure of what the number format costs.
  general_ground   the soft ground at the median foot height that the general trees step on in tests/test_gpu_contact.py.
"""
import copy

import numpy as np

from tests import contact_reference as cr
from tests import fd_reference as fr

SOFT = dict(stiffness=200.0, damping=0.5)      # k delta c dt / m_foot < 2 with bodies of 0.1 kg a metre in the ground


def pushed_tree(m, joint):
    assert 0 <= joint < m.n
    m5 = copy.copy(m)
    m5.foot_joint = np.append(m.foot_joint, joint)
    m5.foot_offset = np.vstack([m.foot_offset, np.zeros((1, 3))])
    return m5


def push_jacobian(m, joint, q):
    m5 = pushed_tree(m, joint)
    return np.stack([cr.feet(m5, q, e)[1][-1] for e in np.eye(m.n)], axis=1)


def pushed_step_ref(m, g, q, v, dt, n_sub, tau_ff, q_des, kp, kd, F, joint, first_substep, n_substeps, s0=0, fd=fr.fd_ref,
                    dtype=np.float64):
    """nmpc_contact_step_batch for one robot under the push F [3] on `joint`: substep i of the call is substep s = s0 + i of the
    count the window is stated in, pushed iff first_substep <= s < first_substep + n_substeps -> (q, v, a, f, tau), a, f (the
    tree's own feet), tau of the last substep."""
    t = np.dtype(dtype).type
    m5 = pushed_tree(m, joint)
    q, v, F = np.array(q, t), np.array(v, t), np.asarray(F, t).reshape(1, 3)
    a = f = tau = None
    for i in range(n_sub):
        on = first_substep <= s0 + i < first_substep + n_substeps
        tau = cr.pd_torque(m, g, q, v, tau_ff, q_des, kp, kd, t)
        f = cr.contact_law(g, *cr.feet(m, q, v, dtype))
        mm, ff = (m5, np.concatenate([f, F])) if on else (m, f)
        a = np.asarray(fd(mm, q, v, tau, ff), t) if fd is fr.fd_ref else fd(mm, q, v, tau, ff, dtype)
        v = v + t(dt) * a
        q = q + t(dt) * v
    return q, v, a, f, tau


def general_ground(m, q):
    """feet of the states q [B, n] on both sides of the plane"""
    z = np.median([cr.feet(m, q[b])[0][:, 2] for b in range(len(q))])
    return cr.Ground(ground_z=float(np.float32(z)), **SOFT)
