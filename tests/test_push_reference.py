"""The references of the push tests (tests/push_reference.py) are checked before anything is checked against them.  No GPU.

A push F on joint j must move the tree as the generalised force J^T F does, J the Jacobian of the push point -- a statement
about the mass matrix and forward kinematics that shares no step with the recursions the references are built on."""
import numpy as np
import pytest

from oracle import torque_oracle as to
from tests import contact_reference as cr
from tests import fd_reference as fr
from tests import push_reference as pr

KP, KD, DT = 20.0, 1.5, 5e-4
# the random tree is pushed on joint 7, whose path to the root is three revolute joints, and on joint 13, which has prismatic
# joints on it (13, 5): the push point then slides with them
TREES = {"quadruped": (fr.quadruped, 5), "tree23": (fr.random_tree, 7), "tree23 sliding": (fr.random_tree, 13)}


def states(name, seed=31):
    m, joint = TREES[name][0](), TREES[name][1]
    q, v, tau, _ = fr.inputs(m, 3, seed)
    F = np.random.default_rng(seed + 1).uniform(-80, 80, (3, 3))
    return m, joint, q.astype(np.float64), v.astype(np.float64), tau.astype(np.float64), F


def test_the_random_tree_is_pushed_behind_prismatic_joints_too():
    m = fr.random_tree()

    def kinds(k):
        out = []
        while k >= 0:
            out.append(int(m.jtype[k]))
            k = int(m.parent[k])
        return out
    assert kinds(7) == [0, 0, 0] and kinds(13) == [1, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(TREES))
def test_a_push_is_the_generalised_force_of_its_jacobian(name):
    m, joint, q, v, tau, F = states(name)
    m5 = pr.pushed_tree(m, joint)
    for b in range(3):
        f = cr.contact_law(cr.Ground(), *cr.feet(m, q[b], v[b]))
        a_u = fr.fd_ref(m, q[b], v[b], tau[b], f)
        a_p = fr.fd_ref(m5, q[b], v[b], tau[b], np.concatenate([f, F[b:b + 1]]))
        M, _ = to._mass_matrix_and_potential(m, q[b])
        lhs, rhs = M @ (a_p - a_u), pr.push_jacobian(m, joint, q[b]).T @ F[b]
        err = np.abs(lhs - rhs).max() / np.abs(rhs).max()
        print(f"{name} state {b}: |M da - J^T F| / |J^T F| = {err:.2e}")
        assert err < 1e-9


@pytest.mark.parametrize("name", sorted(TREES))
def test_aba_is_fd_ref_on_the_pushed_tree(name):
    m, joint, q, v, tau, F = states(name)
    m5 = pr.pushed_tree(m, joint)
    for b in range(3):
        f = np.concatenate([cr.contact_law(cr.Ground(), *cr.feet(m, q[b], v[b])), F[b:b + 1]])
        ref, got = fr.fd_ref(m5, q[b], v[b], tau[b], f), fr.aba(m5, q[b], v[b], tau[b], f)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{name} state {b}: aba against fd_ref {err:.2e}")
        assert err < 1e-9


def step_args(name):
    m, joint, q, v, tau, F = states(name)
    g = cr.Ground() if name == "quadruped" else pr.general_ground(m, q)
    q_des = q[:, m.n - m.nu:] + 0.05
    return m, joint, g, q, v, tau, q_des, F


@pytest.mark.parametrize("name", sorted(TREES))
def test_a_window_that_misses_is_the_unpushed_step_bit_for_bit(name):
    m, joint, g, q, v, tau, q_des, F = step_args(name)
    for b in range(3):
        plain = cr.contact_step_ref(m, g, q[b], v[b], DT, 4, tau[b], q_des[b], KP, KD)
        for first, count in ((4, 3), (-5, 5), (1, 0)):
            got = pr.pushed_step_ref(m, g, q[b], v[b], DT, 4, tau[b], q_des[b], KP, KD, F[b], joint, first, count)
            assert all(np.array_equal(x, y) for x, y in zip(got, plain)), (b, first, count)
        pushed = pr.pushed_step_ref(m, g, q[b], v[b], DT, 4, tau[b], q_des[b], KP, KD, F[b], joint, 1, 2)
        assert not np.array_equal(pushed[1], plain[1])


@pytest.mark.parametrize("name", sorted(TREES))
def test_two_half_runs_with_the_offset_moved_are_the_long_run(name):
    m, joint, g, q, v, tau, q_des, F = step_args(name)
    for b in range(3):
        kw = dict(F=F[b], joint=joint, first_substep=1, n_substeps=2)
        long = pr.pushed_step_ref(m, g, q[b], v[b], DT, 4, tau[b], q_des[b], KP, KD, **kw)
        half = pr.pushed_step_ref(m, g, q[b], v[b], DT, 2, tau[b], q_des[b], KP, KD, **kw)
        both = pr.pushed_step_ref(m, g, half[0], half[1], DT, 2, tau[b], q_des[b], KP, KD, s0=2, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(both, long)), b
