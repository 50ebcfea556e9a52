"""The forward-dynamics reference of the tests (tests/fd_reference.py): fd_ref = solve(M, S^T tau - h) against the inverse
dynamics it has to invert, against closed forms, and against the articulated-body recursion stated a second time."""
import numpy as np
import pytest

from oracle import torque_oracle as to
from tests import fd_reference as fr

TREES = {"quadruped": lambda: fr.quadruped(0.0), "tilted": lambda: fr.quadruped(0.3), "random23": fr.random_tree}


@pytest.fixture(scope="module", params=list(TREES))
def case(request):
    m = TREES[request.param]()
    q, v, tau, f = (x.astype(np.float64) for x in fr.inputs(m, 64, seed=7))
    return m, q, v, tau, f, fr.fd_ref_batch(m, q, v, tau, f)


def test_inverse_dynamics_of_fd_ref_returns_the_torque(case):
    m, q, v, tau, f, a = case
    res = max(np.abs(to.id_torques(m, q[b], v[b], a[b], f[b]) - fr.generalised(m, tau[b])).max() for b in range(len(q)))
    print(f"round-trip residual {res:.2e}")
    assert res < 1e-9


def test_articulated_body_recursion_equals_fd_ref(case):
    """fp64: the two derivations agree; fp32: the figure the GPU test takes its fallback bar from, printed."""
    m, q, v, tau, f, a = case
    assert fr.rel_err(fr.aba_batch(m, q, v, tau, f), a) < 1e-9
    print(f"float32 recursion vs fd_ref {fr.rel_err(fr.aba_batch(m, q[:16], v[:16], tau[:16], f[:16], np.float32), a[:16]):.2e}")


def test_free_fall_of_the_standing_pose():
    m = fr.quadruped()
    q, _ = fr.standing(m)
    a = fr.fd_ref(m, q, np.zeros(m.n), np.zeros(m.nu), np.zeros((4, 3)))
    expect = np.zeros(m.n); expect[2] = -fr.G
    assert np.abs(a - expect).max() < 1e-12


def test_standing_robot_that_holds_its_static_torques_does_not_move():
    m = fr.quadruped()
    q, f = fr.standing(m)
    tau = to.id_torques(m, q, np.zeros(m.n), np.zeros(m.n), f)[-m.nu:]
    assert np.abs(fr.fd_ref(m, q, np.zeros(m.n), tau, f)).max() < 1e-9


def test_step_ref_is_semi_implicit_euler():
    m = fr.quadruped()
    q0, _ = fr.standing(m)
    K, dt = 20, 1e-3
    q, v, a = fr.step_ref(m, q0, np.zeros(m.n), dt, K, None, None, 0.0, 0.0, np.zeros((4, 3)))
    assert abs(v[2] + fr.G * K * dt) < 1e-12 and abs(q[2] - (q0[2] - fr.G * dt * dt * K * (K + 1) / 2)) < 1e-12
    assert np.abs(q[6:] - q0[6:]).max() < 1e-12 and abs(a[2] + fr.G) < 1e-12
