"""References for the composite-inertia outputs of the torque layer (nmpc_mass_matrix_batch, nmpc_centroidal_batch) -- TEST
INFRASTRUCTURE ONLY (helper module, not collected by pytest), built on oracle/torque_oracle.py without touching it.

  mass_matrix_ref   M(q) in fp64 from forward kinematics and geometric Jacobians (`_mass_matrix_and_potential`): the derivation
                    that shares no step with a recursion over the tree.
  centroidal_ref    com, h, A_g in fp64 from the same per-body world Jacobians Jv_b, Jw_b:
                        com = sum m_b pc_b / sum m_b,   A_g = sum_b [m_b Jv_b ; Iw_b Jw_b + m_b [pc_b - com]x Jv_b],   h = A_g v.
  crba              the composite-rigid-body recursion with the kernel's passes (outward poses and first moment, inward
                    composite inertias, one force per column carried to the root) on 6x6 spatial matrices, in the number format
                    it is asked for: in float64 a second statement of the two above, in float32 the measure of what the
                    recursion itself costs in the kernel's format (another order of operations than the kernel's block form).
"""
import numpy as np

from oracle import torque_oracle as to


def mass_matrix_ref(m, q):
    return to._mass_matrix_and_potential(m, np.asarray(q, np.float64))[0]


def centroidal_ref(m, q, v=None):
    """(com [3], h [6] or None, Ag [6, n]); h = [linear; angular about com], world axes"""
    q = np.asarray(q, np.float64)
    Rw, pw = m.forward_kinematics(q)
    n = m.n
    z = [Rw[i] @ m.axis[i] for i in range(n)]
    pc = [pw[b] + Rw[b] @ m.com[b] for b in range(n)]
    com = sum(m.mass[b] * pc[b] for b in range(n)) / m.mass.sum()
    Ag = np.zeros((6, n))
    for b in range(n):
        Jv, Jw = np.zeros((3, n)), np.zeros((3, n))
        k = b
        while k >= 0:
            if m.jtype[k] == 0:
                Jw[:, k] = z[k]; Jv[:, k] = np.cross(z[k], pc[b] - pw[k])
            else:
                Jv[:, k] = z[k]
            k = m.parent[k]
        Iw = Rw[b] @ to._inertia_matrix(m.inertia[b]) @ Rw[b].T
        Ag[:3] += m.mass[b] * Jv
        Ag[3:] += Iw @ Jw + m.mass[b] * to._skew(pc[b] - com) @ Jv
    return com, (None if v is None else Ag @ np.asarray(v, np.float64)), Ag


def _skew(a, dt):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dt)


def crba(m, q, v=None, dtype=np.float64):
    """(M [n, n], com [3], h [6] or None, Ag [6, n]) by the composite recursion, every operation in `dtype`."""
    dt = np.dtype(dtype).type
    n = m.n
    q = np.asarray(q, dt)
    axis, mass, com_b = m.axis.astype(dt), m.mass.astype(dt), m.com.astype(dt)
    XT, S, Ic, Rw, pw = ([None] * n for _ in range(5))
    first, total = np.zeros(3, dt), dt(0)
    for i in range(n):                                    # outward
        K = _skew(axis[i], dt)
        if m.jtype[i] == 0:
            R = m.R_fix[i].astype(dt) @ (np.eye(3, dtype=dt) + np.sin(q[i]) * K + (dt(1) - np.cos(q[i])) * (K @ K))
            p = m.p_fix[i].astype(dt)
            S[i] = np.concatenate([axis[i], np.zeros(3, dt)])
        else:
            R = m.R_fix[i].astype(dt)
            p = m.p_fix[i].astype(dt) + R @ (axis[i] * q[i])
            S[i] = np.concatenate([np.zeros(3, dt), axis[i]])
        X = np.zeros((6, 6), dt)                          # forces child -> parent: n' = R n + p x (R l), l' = R l
        X[:3, :3] = R; X[3:, 3:] = R; X[:3, 3:] = _skew(p, dt) @ R
        XT[i] = X
        par = m.parent[i]
        Rw[i], pw[i] = (R, p) if par < 0 else (Rw[par] @ R, pw[par] + Rw[par] @ p)
        C = _skew(com_b[i], dt)
        I = np.zeros((6, 6), dt)
        I[:3, :3] = to._inertia_matrix(m.inertia[i]).astype(dt) - mass[i] * (C @ C); I[:3, 3:] = mass[i] * C
        I[3:, :3] = -mass[i] * C; I[3:, 3:] = mass[i] * np.eye(3, dtype=dt)
        Ic[i] = I
        first = first + mass[i] * (pw[i] + Rw[i] @ com_b[i])
        total = total + mass[i]
    com = first / total
    for i in range(n - 1, -1, -1):                        # inward
        if m.parent[i] >= 0:
            Ic[m.parent[i]] = Ic[m.parent[i]] + XT[i] @ Ic[i] @ XT[i].T
    M, Ag = np.zeros((n, n), dt), np.zeros((6, n), dt)
    for i in range(n):                                    # columns
        F = Ic[i] @ S[i]
        l_w = Rw[i] @ F[3:]
        Ag[:3, i] = l_w
        Ag[3:, i] = Rw[i] @ F[:3] + np.cross(pw[i] - com, l_w)
        M[i, i] = S[i] @ F
        j = i
        while m.parent[j] >= 0:
            F = XT[j] @ F
            j = m.parent[j]
            M[i, j] = M[j, i] = S[j] @ F
    h = None
    if v is not None:
        v = np.asarray(v, dt)
        h = np.zeros(6, dt)
        for i in range(n):
            h = h + Ag[:, i] * v[i]
    assert M.dtype == Ag.dtype == com.dtype == np.dtype(dtype)
    return M, com, h, Ag


def mass_matrix_ref_batch(m, q):
    return np.stack([mass_matrix_ref(m, q[b]) for b in range(len(q))])


def centroidal_ref_batch(m, q, v):
    """(com [B, 3], h [B, 6], Ag [B, 6, n])"""
    return tuple(np.stack(x) for x in zip(*(centroidal_ref(m, q[b], v[b]) for b in range(len(q)))))


def crba_batch(m, q, v, dtype=np.float64):
    """(M [B, n, n], com [B, 3], h [B, 6], Ag [B, 6, n])"""
    return tuple(np.stack(x) for x in zip(*(crba(m, q[b], v[b], dtype) for b in range(len(q)))))


def path_mask(parent):
    """[n, n] bool: joints i and j are on one path to the root (i == j included)"""
    n = len(parent)
    mask = np.eye(n, dtype=bool)
    for i in range(n):
        j = parent[i]
        while j >= 0:
            mask[i, j] = mask[j, i] = True
            j = parent[j]
    return mask
