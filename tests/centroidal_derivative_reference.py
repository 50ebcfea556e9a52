"""References for the derivatives of the centroidal momentum of the tree (nmpc_centroidal_derivatives_batch) -- TEST
INFRASTRUCTURE ONLY (helper module, not collected by pytest), built on tests/crba_reference.py and oracle/torque_oracle.py
without touching them.

  centroidal_derivatives_ref   (dh_dq [6, n], dcom_dq [3, n], hdot_bias [6]) by the analytic recursion with the kernel's passes, in
                               the number format it is asked for: in float64 the reference of the device, in float32 the measure
                               of what the recursion itself costs in the kernel's format.  World-frame spatial vectors about a
                               point O at the robot (the origin of the first frame that carries mass; frame positions are
                               accumulated from there, so nothing is ever the size of the base position):
                                   dh_O/dq_j = S_j x* h^c_j - I^c_j (S_j x v_p(j)),
                                   dcom/dq_j = lin(I^c_j S_j) / m,
                                   dk_G/dq_j = dk_O/dq_j - dcom/dq_j x l - (com - O) x dl/dq_j,
                                   hdot_bias = sum_j dh_dq[:, j] v_j   in joint order.
  centroidal_derivatives_fd    the same three by central differences of crba_reference.centroidal_ref's h = A_g(q) v (v fixed) and
                               com in fp64: the judge of the analytic reference, never used against the device.
"""
import numpy as np

from oracle import torque_oracle as to
from tests import crba_reference as cr


def anchor(m):
    """the first joint whose body has mass: the point O of the recursion is the origin of its frame"""
    return int(np.flatnonzero(np.asarray(m.mass) > 0)[0])


def centroidal_derivatives_ref(m, q, v, dtype=np.float64):
    dt = np.dtype(dtype).type
    n = m.n
    q, v = np.asarray(q, dt), np.asarray(v, dt)
    axis, mass, com_b = m.axis.astype(dt), m.mass.astype(dt), m.com.astype(dt)
    zero = np.zeros(3, dt)
    Rw, pl, d = ([None] * n for _ in range(3))
    for i in range(n):                                    # world rotation of every frame, its offset in the parent frame
        K = cr._skew(axis[i], dt)
        if m.jtype[i] == 0:
            R = m.R_fix[i].astype(dt) @ (np.eye(3, dtype=dt) + np.sin(q[i]) * K + (dt(1) - np.cos(q[i])) * (K @ K))
            pl[i] = m.p_fix[i].astype(dt)
        else:
            R = m.R_fix[i].astype(dt)
            pl[i] = m.p_fix[i].astype(dt) + R @ (axis[i] * q[i])
        Rw[i] = R if m.parent[i] < 0 else Rw[m.parent[i]] @ R
    k = anchor(m)                                         # positions about O: back along the path to the root, then outward
    d[k] = zero
    while m.parent[k] >= 0:
        par = m.parent[k]
        d[par] = d[k] - Rw[par] @ pl[k]
        k = par
    O = pl[k] - d[k]
    S, V, A, first, tot, hc = ([None] * n for _ in range(6))
    l_all = zero
    for i in range(n):                                    # outward: velocities, the body's inertia and momentum about O
        par = m.parent[i]
        if d[i] is None:
            d[i] = pl[i] - O if par < 0 else d[par] + Rw[par] @ pl[i]
        z = Rw[i] @ axis[i]
        S[i] = (z, np.cross(d[i], z)) if m.jtype[i] == 0 else (zero, z)
        wp, up = (zero, zero) if par < 0 else V[par]
        w, u = wp + S[i][0] * v[i], up + S[i][1] * v[i]
        V[i] = (w, u)
        c = d[i] + Rw[i] @ com_b[i]
        Ib = Rw[i] @ to._inertia_matrix(m.inertia[i]).astype(dt) @ Rw[i].T
        A[i] = Ib + mass[i] * ((c @ c) * np.eye(3, dtype=dt) - np.outer(c, c))
        first[i], tot[i] = mass[i] * c, mass[i]
        l = mass[i] * (u + np.cross(w, c))
        hc[i] = (Ib @ w + np.cross(c, l), l)
        l_all = l_all + l
    for i in range(n - 1, -1, -1):                        # inward: sums over the subtrees
        par = m.parent[i]
        if par >= 0:
            A[par] = A[par] + A[i]; first[par] = first[par] + first[i]; tot[par] = tot[par] + tot[i]
            hc[par] = (hc[par][0] + hc[i][0], hc[par][1] + hc[i][1])
    total, moment = dt(0), zero
    for i in range(n):
        if m.parent[i] < 0:
            total = total + tot[i]; moment = moment + first[i]
    com = moment / total                                  # com - O
    dh, dcom = np.zeros((6, n), dt), np.zeros((3, n), dt)
    for j in range(n):                                    # columns
        sw, sv = S[j]
        wp, up = (zero, zero) if m.parent[j] < 0 else V[m.parent[j]]
        al, be = np.cross(sw, wp), np.cross(sw, up) + np.cross(sv, wp)
        hn, hl = hc[j]
        dn = np.cross(sw, hn) + np.cross(sv, hl) - (A[j] @ al + np.cross(first[j], be))
        dl = np.cross(sw, hl) - (tot[j] * be - np.cross(first[j], al))
        dc = (tot[j] * sv - np.cross(first[j], sw)) / total
        dh[:3, j] = dl
        dh[3:, j] = dn - np.cross(dc, l_all) - np.cross(com, dl)
        dcom[:, j] = dc
    bias = np.zeros(6, dt)
    for j in range(n):
        bias = bias + dh[:, j] * v[j]
    assert dh.dtype == dcom.dtype == bias.dtype == np.dtype(dtype)
    return dh, dcom, bias


def centroidal_derivatives_fd(m, q, v, eps):
    """(dh_dq [6, n], dcom_dq [3, n], hdot_bias [6]) by central differences of step eps in fp64, v fixed"""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    dh, dcom = np.zeros((6, m.n)), np.zeros((3, m.n))
    for j in range(m.n):
        e = np.zeros(m.n); e[j] = eps
        cp, hp, _ = cr.centroidal_ref(m, q + e, v)
        cm, hm, _ = cr.centroidal_ref(m, q - e, v)
        dh[:, j] = (hp - hm) / (2 * eps)
        dcom[:, j] = (cp - cm) / (2 * eps)
    return dh, dcom, dh @ v


def states(m, B, seed):
    """B float32 states: q of fd_reference.inputs (U(-1, 1)), velocities N(0, 0.3) on the first six joints (the base of the
    quadruped) and N(0, 2.0) on the others"""
    from tests import fd_reference as fr
    q = fr.inputs(m, B, seed)[0]
    rng = np.random.default_rng(seed + 1000)
    v = np.concatenate([rng.normal(0, 0.3, (B, 6)), rng.normal(0, 2.0, (B, m.n - 6))], axis=1).astype(np.float32)
    return q, v


def centroidal_derivatives_ref_batch(m, q, v, dtype=np.float64):
    """(dh_dq [B, 6, n], dcom_dq [B, 3, n], hdot_bias [B, 6])"""
    return tuple(np.stack(x) for x in zip(*(centroidal_derivatives_ref(m, q[b], v[b], dtype) for b in range(len(q)))))
