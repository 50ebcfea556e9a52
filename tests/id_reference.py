"""Inverse-dynamics references for the tests of nmpc_id_torques_batch -- TEST INFRASTRUCTURE ONLY, built on
oracle/torque_oracle.py without touching it.

  id_torques_np  oracle.torque_oracle.id_torques restated with every array and product carried in the number format it is asked
                 for: in float64 a second statement of the oracle (tests/test_id_reference.py holds the two together at 1e-12),
                 in float32 the measure of what the recursion itself costs in the kernel's format -- the model is rounded to
                 float32 as the device's copy is, the order of operations is numpy's, not the kernel's.
  chain, star, single, variant
                 the trees the quadruped and fd_reference.random_tree are not: the deepest tree, the widest, the smallest, and
                 copies of a tree with fewer actuators, massless bodies or another gravity.
  TREES          the trees tests/test_gpu_torque.py runs, by name, for both test files.
  samples        q in U(-1, 1), v in U(-2, 2), a in U(-5, 5), f in U(-40, 80) as float32 (the `batch` of tests/test_gpu_torque.py).
"""
import copy

import numpy as np

from oracle import torque_oracle as to
from tests import fd_reference as fr


def _skew(a, dt):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dt)


def id_torques_np(m, q, v, a, f, dtype=np.float64):
    """All n generalised forces of one sample, every operation in `dtype` (f None: no contact forces)."""
    dt = np.dtype(dtype).type
    n = m.n
    q, v, a = (np.asarray(x, dt) for x in (q, v, a))
    f = np.zeros((len(m.foot_joint), 3), dt) if f is None else np.asarray(f, dt)
    axis, R_fix, p_fix, mass, com = (x.astype(dt) for x in (m.axis, m.R_fix, m.p_fix, m.mass, m.com))
    inertia, foot_offset, gravity = m.inertia.astype(dt), m.foot_offset.astype(dt), m.gravity.astype(dt)
    zero, eye = np.zeros(3, dt), np.eye(3, dtype=dt)
    w, vo, dw, dvo = (np.zeros((n, 3), dt) for _ in range(4))
    Rw, Rl, pl = [None] * n, [None] * n, [None] * n
    fn, fl = np.zeros((n, 3), dt), np.zeros((n, 3), dt)             # moment about the body origin, force
    for i in range(n):
        if m.jtype[i] == 0:
            K = _skew(axis[i], dt)
            R, p = R_fix[i] @ (eye + np.sin(q[i]) * K + (dt(1) - np.cos(q[i])) * (K @ K)), p_fix[i]
        else:
            R, p = R_fix[i], p_fix[i] + R_fix[i] @ (axis[i] * q[i])
        Rl[i], pl[i] = R, p
        par = m.parent[i]
        if par < 0:
            w_p = vo_p = dw_p = zero; dvo_p = -gravity; Rw[i] = R       # gravity as a base acceleration
        else:
            w_p, vo_p, dw_p, dvo_p = w[par], vo[par], dw[par], dvo[par]; Rw[i] = Rw[par] @ R
        w_i = R.T @ w_p; vo_i = R.T @ (vo_p + np.cross(w_p, p))
        dw_i = R.T @ dw_p; dvo_i = R.T @ (dvo_p + np.cross(dw_p, p))
        s_w, s_v = (axis[i], zero) if m.jtype[i] == 0 else (zero, axis[i])
        vj_w, vj_v = s_w * v[i], s_v * v[i]
        dw_i = dw_i + s_w * a[i] + np.cross(w_i, vj_w)
        dvo_i = dvo_i + s_v * a[i] + np.cross(w_i, vj_v) + np.cross(vo_i, vj_w)
        w_i = w_i + vj_w; vo_i = vo_i + vj_v
        w[i], vo[i], dw[i], dvo[i] = w_i, vo_i, dw_i, dvo_i
        xx, xy, xz, yy, yz, zz = inertia[i]
        c, Ic = com[i], np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=dt)
        h_l = mass[i] * (vo_i + np.cross(w_i, c)); h_n = Ic @ w_i + np.cross(c, h_l)
        g_l = mass[i] * (dvo_i + np.cross(dw_i, c)); g_n = Ic @ dw_i + np.cross(c, g_l)
        fn[i] = g_n + np.cross(w_i, h_n) + np.cross(vo_i, h_l)
        fl[i] = g_l + np.cross(w_i, h_l)
    for k, j in enumerate(m.foot_joint):                              # world force at the foot point of body j
        l = Rw[j].T @ f[k]
        fl[j] = fl[j] - l; fn[j] = fn[j] - np.cross(foot_offset[k], l)
    tau = np.zeros(n, dt)
    for i in range(n - 1, -1, -1):
        tau[i] = axis[i] @ (fn[i] if m.jtype[i] == 0 else fl[i])
        par = m.parent[i]
        if par >= 0:
            l_p = Rl[i] @ fl[i]
            fl[par] = fl[par] + l_p; fn[par] = fn[par] + (Rl[i] @ fn[i] + np.cross(pl[i], l_p))
    assert tau.dtype == np.dtype(dtype)
    return tau


def id_torques_np_batch(m, q, v, a, f=None, dtype=np.float64):
    """[B, nu]: the last nu columns, as oracle.torque_oracle.id_torques_batch returns them."""
    out = [id_torques_np(m, q[b], v[b], a[b], None if f is None else f[b], dtype)[m.n - m.nu:] for b in range(len(q))]
    return np.stack(out) if out else np.zeros((0, m.nu), dtype)


def oracle_batch(m, q, v, a, f=None):
    """oracle.torque_oracle.id_torques_batch on the float64 casts of the device's inputs (f None: zero forces)."""
    f = np.zeros((len(q), len(m.foot_joint), 3)) if f is None else f
    return to.id_torques_batch(m, *(np.asarray(x, np.float64) for x in (q, v, a, f)))


def samples(m, B, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1, 1, (B, m.n)); v = rng.uniform(-2, 2, (B, m.n)); a = rng.uniform(-5, 5, (B, m.n))
    f = rng.uniform(-40, 80, (B, len(m.foot_joint), 3))
    return [x.astype(np.float32) for x in (q, v, a, f)]


# ---- trees ------------------------------------------------------------------------------------------------------------------------
def variant(m, n_actuated=None, massless=(), gravity=None):
    """A copy of tree m with the last n_actuated joints actuated, the listed bodies without mass and inertia, another gravity."""
    m = copy.deepcopy(m)
    if n_actuated is not None:
        assert 1 <= n_actuated <= m.n
        m.nu = int(n_actuated)
    for i in massless:
        m.mass[i] = 0.0; m.inertia[i] = 0.0
    if gravity is not None:
        m.gravity = np.asarray(gravity, float)
    return m


def _tree(parent, jtype, seed, feet, n_actuated, massless):
    """Random axes, placements and bodies of the magnitudes of fd_reference.random_tree on a given topology."""
    n = len(parent)
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((n, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    tilt = rng.standard_normal((n, 3)); tilt /= np.linalg.norm(tilt, axis=1, keepdims=True)
    R = np.stack([to._axis_rotation(tilt[i], rng.uniform(-2, 2)) for i in range(n)])
    A = 0.1 * rng.standard_normal((n, 3, 3))
    inertia = np.stack([(A[i] @ A[i].T + np.eye(3))[np.triu_indices(3)] for i in range(n)])
    m = to.TreeModel(parent, jtype, axis, R, 0.3 * rng.standard_normal((n, 3)), rng.uniform(0.1, 3.0, n), 0.1 * rng.standard_normal((n, 3)),
                     inertia, foot_joint=list(feet), foot_offset=0.2 * rng.standard_normal((len(feet), 3)), n_actuated=n,
                     gravity=(0.3, -0.2, -9.7))
    return variant(m, n_actuated, massless)


def chain(n, jtype=None, seed=31, feet=None, n_actuated=None, massless=()):
    """parent[i] = i - 1: every body hangs on the one before it (jtype None: revolute and prismatic joints in turn; feet None:
    one in the middle, one on the last body)."""
    jtype = [i % 2 for i in range(n)] if jtype is None else jtype
    return _tree([i - 1 for i in range(n)], jtype, seed, [n // 2, n - 1] if feet is None else feet, n_actuated, massless)


def star(n, jtype=None, seed=32, feet=None, n_actuated=None, massless=()):
    """every body but the first on joint 0 (jtype None: random types; feet None: one on joint 0, one on the last body)."""
    jtype = np.random.default_rng(seed + 1000).integers(0, 2, n) if jtype is None else jtype
    return _tree([-1] + [0] * (n - 1), jtype, seed, [0, n - 1] if feet is None else feet, n_actuated, massless)


def single(jtype, seed=33, feet=(0,)):
    """n = nu = 1: one body on one joint of the given type, a foot on it."""
    return _tree([-1], [jtype], seed + jtype, feet, None, ())


def inner_and_leaves(m):
    """(bodies other than joint 0 that carry a child, bodies that carry none)"""
    has_child = np.zeros(m.n, bool)
    has_child[m.parent[m.parent >= 0]] = True
    return [i for i in range(1, m.n) if has_child[i]], [i for i in range(m.n) if not has_child[i]]


def eight_feet():
    """The random 10-joint tree with as many feet as the layer takes: four on one inner body, two on joint 0, two on a leaf."""
    inner, leaves = inner_and_leaves(fr.random_tree(n=10, seed=14, feet=()))
    return fr.random_tree(n=10, seed=14, feet=[inner[-1]] * 4 + [0, 0] + [leaves[-1]] * 2)


def massless():
    """The random 10-joint tree with two massless inner bodies and a massless leaf."""
    m = fr.random_tree(n=10, seed=15, feet=(3, 9, 9))
    inner, leaves = inner_and_leaves(m)
    assert len(inner) >= 2
    return variant(m, massless=[inner[0], inner[-1], leaves[-1]])


TREES = {
    "quadruped": lambda: fr.quadruped(0.0),
    "tilted": lambda: fr.quadruped(0.3),
    "random23": fr.random_tree,
    "random32": lambda: fr.random_tree(n=32, seed=16, feet=(5, 31, 31, 17, 0)),
    "chain32": lambda: chain(32),
    "star32": lambda: star(32),
    "single_revolute": lambda: single(0),
    "single_prismatic": lambda: single(1),
    "one_actuator": lambda: variant(fr.random_tree(n=12, seed=17, feet=(2, 11, 7)), n_actuated=1),
    "five_actuators": lambda: variant(fr.random_tree(n=12, seed=17, feet=(2, 11, 7)), n_actuated=5),
    "eight_feet": eight_feet,
    "no_feet": lambda: fr.random_tree(n=10, seed=18, feet=()),
    "massless": massless,
    "no_gravity": lambda: variant(fr.random_tree(), gravity=(0.0, 0.0, 0.0)),
}
