"""Action labels of a whole-body plan, the parts that need no device: the C-ABI declarations, `references.plan_rows` (the
declared meaning of "row j of a plan") against the host loop's own up-sampling, and the label formula on a case with a
known answer.  "Oracle labels" (`torque_helpers.oracle_labels`, used by the GPU tests too): plan_rows in fp64 -> oracle/torque_oracle.py
on the declared tree -> (tau + kd v_j) / kp + q_j in fp64."""
import os
import re

import numpy as np

from iterative_learning_nmpc_amd import references as refs
from iterative_learning_nmpc_amd.workloads import quadruped_tree
from tests.torque_helpers import oracle_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_calls_are_declared_and_bound():
    from iterative_learning_nmpc_amd import _lib
    torque_h = open(os.path.join(ROOT, "include", "nmpc_torque.h")).read()
    nmpc_h = open(os.path.join(ROOT, "include", "nmpc.h")).read()
    assert re.search(r"\bint\s+nmpc_plan_actions_batch\s*\(", torque_h)
    assert re.search(r"\bint\s+nmpc_wb_rollout_set_actions\s*\(", nmpc_h)
    assert "nmpc_plan_actions_batch" in _lib.SIGNATURES and "nmpc_wb_rollout_set_actions" in _lib.SIGNATURES


def test_plan_rows_are_the_host_loops_rows_at_the_default_horizon():
    """N = 25: dt_nodes = 0.04 and the horizon is exactly 1.0 s, so the host's linspace query times and (j + 1) sim_dt coincide
    to rounding.  Same fp64 expressions, different association at most: 1e-12 absolute."""
    rng = np.random.default_rng(0)
    N, n, sim_dt, dt = 25, 40, 1.0e-3, 0.04
    X, U = rng.standard_normal((3, N + 1, 42)), rng.standard_normal((3, N, 30))
    id_repeat = refs.zero_order_hold_index(1000, N)
    q, v, a, f = refs.plan_rows(X, U, id_repeat[:n], dt, sim_dt)
    assert q.shape == v.shape == a.shape == (3, n, 18) and f.shape == (3, n, 4, 3)
    time_traj = np.concatenate(([0.0], np.cumsum(np.full(N, dt))))
    for b in range(3):
        qp, vp = refs.hermite_upsample(time_traj, X[b, :, :18], X[b, :, 18:36], U[b, :, :18], 1000)
        assert np.abs(qp[1:n + 1] - q[b]).max() <= 1e-12 and np.abs(vp[1:n + 1] - v[b]).max() <= 1e-12
        assert np.abs(np.take(U[b, :, :18], id_repeat[:n], axis=0) - a[b]).max() <= 1e-12
        assert np.abs(np.take(U[b, :, 18:].reshape(N, 4, 3), id_repeat[:n], axis=0) - f[b]).max() <= 1e-12
    # one plan without a batch axis is the same rows
    q1, v1, a1, f1 = refs.plan_rows(X[1], U[1], id_repeat[:n], dt, sim_dt)
    assert np.array_equal(q1, q[1]) and np.array_equal(v1, v[1]) and np.array_equal(a1, a[1]) and np.array_equal(f1, f[1])


def test_plan_rows_follow_the_device_clock_at_30_nodes():
    """N = 30: the configured dt_nodes is rounded (0.0333) and the host loop samples every 0.999 ms; plan_rows samples at
    (j + 1) sim_dt on nodes `dt_nodes` apart [decl].  Checked: the hold indices, and continuity with the node values at
    t = k dt_nodes (a Hermite segment passes through its end points)."""
    rng = np.random.default_rng(1)
    N, dt = 30, 1.0 / 30
    X, U = rng.standard_normal((2, N + 1, 42)), rng.standard_normal((2, N, 30))
    zoh = np.sort(rng.integers(0, N, 40))
    _, _, a, f = refs.plan_rows(X, U, zoh, dt, 1.0e-3)
    assert np.array_equal(a, U[:, zoh, :18]) and np.array_equal(f, U[:, zoh, 18:].reshape(2, 40, 4, 3))
    # sim_dt = dt_nodes: row j is node j + 1 (the last sample sits on the end of the last segment)
    q, v, _, _ = refs.plan_rows(X, U, np.zeros(N, int), dt, dt)
    assert np.abs(q - X[:, 1:, :18]).max() <= 1e-12 and np.abs(v - X[:, 1:, 18:36]).max() <= 1e-12
    # approaching a node from either side
    eps = 1e-7
    ql, vl, _, _ = refs.plan_rows(X, U, np.zeros(1, int), dt, 3 * dt - eps)
    qr, vr, _, _ = refs.plan_rows(X, U, np.zeros(1, int), dt, 3 * dt + eps)
    assert np.abs(ql[:, 0] - X[:, 3, :18]).max() < 1e-5 and np.abs(qr[:, 0] - X[:, 3, :18]).max() < 1e-5
    assert np.abs(vl[:, 0] - X[:, 3, 18:36]).max() < 1e-5 and np.abs(vr[:, 0] - X[:, 3, 18:36]).max() < 1e-5


def test_standing_plan_gives_the_statics_labels():
    """A plan that stands still (v = a = 0, four feet sharing the weight): action - q_j = tau / kp with the statics torques of
    tests/test_torque_oracle.py's case, and the base joints of that case carry nothing."""
    from oracle import torque_oracle as to
    m = to.TreeModel.from_arrays(quadruped_tree())
    q = np.zeros(18); q[2] = 0.4
    q[6:] = np.tile([0.0, 0.7, -1.4], 4)
    fz = m.mass.sum() * 9.81 / 4
    N, kp, kd = 25, 20.0, 1.5
    X = np.zeros((N + 1, 42)); X[:, :18] = q
    U = np.zeros((N, 30)); U[:, 18:] = np.tile([0.0, 0.0, fz], 4)
    A, tau, qr, vr = oracle_labels(m, X, U, refs.zero_order_hold_index(1000, N)[:40], 0.04, 1.0e-3, kp, kd)
    tau_all = to.id_torques(m, q, np.zeros(18), np.zeros(18), np.tile([0.0, 0.0, fz], (4, 1)))   # the statics case: all 18 forces
    assert np.abs(tau_all[:3]).max() < 1e-9                                         # net force on the base: zero
    full = tau_all[6:]
    assert np.abs(qr - q).max() < 1e-14 and np.abs(vr).max() == 0.0
    assert np.abs(tau - full).max() < 1e-12 and np.abs(full).max() > 1.0             # the legs do carry the trunk
    assert np.abs((A - q[6:]) - full / kp).max() < 1e-13
