"""Reference for the tests of the linearly implicit integrator of the ground-contact plant (nmpc_contact_set_integrator) -- TEST
INFRASTRUCTURE ONLY (helper module, not collected by pytest), built on tests/contact_reference.py, tests/push_reference.py,
tests/crba_reference.py, tests/fd_reference.py and oracle/torque_oracle.py without touching them.

  foot_jacobians     foot positions and the 3 x n world Jacobian of every foot point: the geometric columns of
                     `contact_reference.feet` (z_k x (p - p_w[k]) for a revolute joint, z_k for a prismatic one), kept as columns.
  implicit_system    (A, rhs) of one substep, steps 3 and 4 of the scheme in include/nmpc_torque.h, literally and dense.
  implicit_step_ref  the substeps of nmpc_contact_step_batch under the implicit integrator, shaped like
                     `contact_reference.contact_step_ref`.  In float64: M from `_mass_matrix_and_potential`, a_exp from `fd_ref`,
                     the solve `np.linalg.solve` -- the reference.  In float32: every operation in float32, M from
                     `crba_reference.crba`, a_exp from `aba`, the solve a float32 Cholesky -- the measure of what the number format
                     costs (the floor of `torque_helpers.bar`).
"""
import numpy as np

from oracle import torque_oracle as to
from tests import contact_reference as cr
from tests import crba_reference as cb
from tests import fd_reference as fr
from tests import push_reference as pr


def foot_jacobians(m, q, dtype=np.float64):
    """(pos [n_feet, 3], J [n_feet, 3, n]): pd = J v is `contact_reference.feet`'s velocity."""
    t = np.dtype(dtype).type
    q = np.asarray(q, t)
    Rw, pw = cr._forward_kinematics(m, q, t)
    nf = len(m.foot_joint)
    pos, J = np.zeros((nf, 3), t), np.zeros((nf, 3, m.n), t)
    for f, j in enumerate(m.foot_joint):
        p = pw[j] + Rw[j] @ m.foot_offset[f].astype(t)
        k = j
        while k >= 0:
            z = Rw[k] @ m.axis[k].astype(t)
            J[f, :, k] = np.cross(z, p - pw[k]) if m.jtype[k] == 0 else z
            k = m.parent[k]
        pos[f] = p
    return pos, J


def mass_matrix(m, q, dtype=np.float64):
    if np.dtype(dtype) == np.float64:
        return to._mass_matrix_and_potential(m, np.asarray(q, np.float64))[0]
    return cb.crba(m, q, dtype=dtype)[0]


def implicit_system(m, g, q, v, dt, tau, a_exp, pd_law, kp, kd, dtype=np.float64, inside=None):
    """(A, rhs) of the substep from (q, v): tau the clamped torque of step 1, a_exp the acceleration of step 2, pd_law: is a PD
    target given.  Every operation in `dtype`.  inside: None, or one entry per foot -- True / False puts the foot on that side
    of the plane whatever the sign of its delta, None leaves it to delta > 0.  The scheme is discontinuous where a foot is at the
    plane (kz jumps from 0 to stiffness g), so a foot whose delta is within rounding of 0 has two references, one per side."""
    t = np.dtype(dtype).type
    q, v, a_exp, dt = np.asarray(q, t), np.asarray(v, t), np.asarray(a_exp, t), t(dt)
    n, nu = m.n, m.nu
    M = mass_matrix(m, q, dtype).astype(t)
    A, rhs = M.copy(), M @ a_exp
    pos, J = foot_jacobians(m, q, dtype)
    k_, c_, mu, slip = t(g.stiffness), t(g.damping), t(g.mu), t(g.slip_velocity)
    for f in range(len(m.foot_joint)):
        delta = t(g.ground_z) - pos[f, 2]
        if not (delta > 0 if inside is None or inside[f] is None else inside[f]):
            continue
        Jf = J[f]
        pd = Jf @ v
        fz = cr.contact_law(g, pos[f], pd)[2]
        gk = max(t(0), t(1) - c_ * pd[2])
        r = np.sqrt(pd[0] * pd[0] + pd[1] * pd[1] + slip * slip)
        C = np.zeros((3, 3), t)
        C[:2, :2] = mu * fz * (np.eye(2, dtype=t) / r - np.outer(pd[:2], pd[:2]) / (r * r * r))
        C[2, 2] = k_ * delta * c_ if gk > 0 else t(0)
        kz = k_ * gk
        Jz = Jf[2]
        A = A + dt * (Jf.T @ C @ Jf) + dt * dt * kz * np.outer(Jz, Jz)
        rhs = rhs - dt * kz * pd[2] * Jz
    if pd_law:
        lim = g.tau_max
        for i in range(nu):
            if lim is None or lim <= 0 or abs(tau[i]) < t(lim):
                j = n - nu + i
                A[j, j] = A[j, j] + dt * t(kd) + dt * dt * t(kp)
                rhs[j] = rhs[j] - dt * t(kp) * v[j]
    assert A.dtype == rhs.dtype == np.dtype(dtype)
    return A, rhs


def cholesky_solve(A, b):
    """A^-1 b of a symmetric positive definite A by L L^T, every operation in A's format"""
    t = A.dtype.type
    n = len(b)
    L = np.zeros_like(A)
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                assert s > 0, "not positive definite"
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n, t)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, t)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    assert x.dtype == A.dtype
    return x


def implicit_step_ref(m, g, q, v, dt, n_sub, tau_ff, q_des, kp, kd, push=None, dtype=np.float64, trace=None, systems=None, first_inside=None):
    """nmpc_contact_step_batch under NMPC_INTEGRATOR_LINEARLY_IMPLICIT for one robot -> (q, v, a, f, tau); a of the implicit solve,
    f and tau of steps 1 and 2 of the last substep.  push: None or a dict F [3], joint, first_substep, n_substeps, s0 (default
    0) with the meaning of `push_reference.pushed_step_ref`.  trace: a list that takes (q, v) after every substep; systems: a
    list that takes (A, rhs, a_exp) of every substep; first_inside: `implicit_system`'s `inside` for the first substep."""
    t = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    q, v = np.array(q, t), np.array(v, t)
    if push is not None:
        m5 = pr.pushed_tree(m, push["joint"])
        F = np.asarray(push["F"], t).reshape(1, 3)
    a = f = tau = None
    for i in range(n_sub):
        tau = cr.pd_torque(m, g, q, v, tau_ff, q_des, kp, kd, t)
        f = cr.contact_law(g, *cr.feet(m, q, v, dtype))
        mm, ff = m, f
        if push is not None and push["first_substep"] <= push.get("s0", 0) + i < push["first_substep"] + push["n_substeps"]:
            mm, ff = m5, np.concatenate([f, F])
        a_exp = np.asarray(fr.fd_ref(mm, q, v, tau, ff), t) if f64 else fr.aba(mm, q, v, tau, ff, dtype)
        A, rhs = implicit_system(m, g, q, v, dt, tau, a_exp, q_des is not None, kp, kd, dtype, inside=first_inside if i == 0 else None)
        if systems is not None:
            systems.append((A, rhs, a_exp))
        a = np.linalg.solve(A, rhs) if f64 else cholesky_solve(A, rhs)
        v = v + t(dt) * a
        q = q + t(dt) * v
        if trace is not None:
            trace.append((q.copy(), v.copy()))
    return q, v, a, f, tau


def tail_speed(trace, fraction=0.2):
    """the largest |v| over the last `fraction` of a trace"""
    k = int(round(len(trace) * (1 - fraction)))
    return max(float(np.abs(v).max()) for _, v in trace[k:])


def ltdl_solve(parent, A, b):
    """A^-1 b by the L^T D L factorisation that eliminates the leaves first (Featherstone, RBDA table 6.3), touching only entries
    of joints on one path to the root -- the kernel's solve, stated on a dense matrix: it is exact only if A has the sparsity of
    the mass matrix.  -> (x, pivots)."""
    H, x = np.array(A), np.array(b)
    n = len(x)
    for k in range(n - 1, -1, -1):
        i = parent[k]
        while i >= 0:
            l = H[k, i] / H[k, k]
            j = i
            while j >= 0:
                H[i, j] -= l * H[k, j]
                j = parent[j]
            H[k, i] = l
            i = parent[i]
    for i in range(n - 1, -1, -1):
        j = parent[i]
        while j >= 0:
            x[j] -= H[i, j] * x[i]
            j = parent[j]
    for i in range(n):
        x[i] /= H[i, i]
        j = parent[i]
        while j >= 0:
            x[i] -= H[i, j] * x[j]
            j = parent[j]
    return x, np.diag(H).copy()
