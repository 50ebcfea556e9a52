"""The reference of an actuator per robot (tests/actuator_reference.py) against the references it is built on and against the
declaration of nmpc_contact_set_actuators in include/nmpc_torque.h -- host only, float64.

  * the row (kp, kd, 0, 0) is the plant without a table: `contact_step_ref` and `implicit_step_ref`, to 1e-12 relative;
  * the acceleration under a row solves (M + D) a + bias = S^T t + J^T f, to 1e-10, on random states;
  * the damping takes exactly damping v_i off the joint torque, after the clamp;
  * in the implicit system the joints the clamp cut and the others get the diagonals the header states."""
import numpy as np
import pytest

from oracle import torque_oracle as to
from tests import actuator_reference as ar
from tests import contact_reference as cr
from tests import fd_reference as fr
from tests import implicit_reference as ir

KP, KD = 20.0, 1.5
ROW = np.array([27.0, 1.1, 0.15, 0.012])                 # every field away from the nominal one


def states(m, n, seed):
    """n states of the quadruped around its standing pose, the feet from 1 cm above the ground to 1 cm inside it"""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, m.n)); q[:, 3:6] = rng.uniform(-0.05, 0.05, (n, 3)); q[:, 6:] = fr.STAND + rng.uniform(-0.1, 0.1, (n, 12))
    q[:, 2] = 0.3
    for b in range(n):
        q[b, 2] += np.linspace(0.01, -0.01, n)[b] - cr.feet(m, q[b])[0][:, 2].min()
    v = rng.uniform(-1, 1, (n, m.n))
    tau = rng.uniform(-2, 2, (n, m.nu))
    q_des = q[:, 6:] + rng.uniform(-0.1, 0.1, (n, m.nu))
    return q, v, tau, q_des


@pytest.fixture(scope="module")
def m():
    return fr.quadruped()


def rel(x, ref):
    return float(np.abs(np.asarray(x) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("tau_max", [None, 3.0])
def test_the_nominal_row_is_the_plant_without_a_table(m, tau_max):
    g = cr.Ground(tau_max=tau_max)
    q, v, tau, q_des = states(m, 4, 1)
    worst = 0.0
    for b in range(4):
        plain = cr.contact_step_ref(m, g, q[b], v[b], 5e-4, 3, tau[b], q_des[b], KP, KD)
        mine = ar.step(m, g, ar.nominal(KP, KD), q[b], v[b], 5e-4, 3, tau[b], q_des[b])
        worst = max([worst] + [rel(x, y) for x, y in zip(mine, plain) if np.abs(y).max() > 0])
        assert all(np.array_equal(x, y) for x, y in zip(mine, plain) if np.abs(y).max() == 0)
        plain = ir.implicit_step_ref(m, g, q[b], v[b], 1e-3, 3, tau[b], q_des[b], KP, KD)
        mine = ar.step(m, g, ar.nominal(KP, KD), q[b], v[b], 1e-3, 3, tau[b], q_des[b], implicit=True)
        worst = max([worst] + [rel(x, y) for x, y in zip(mine, plain) if np.abs(y).max() > 0])
    print(f"nominal row against contact_step_ref and implicit_step_ref, tau_max {tau_max}: worst relative difference {worst:.2e}")
    assert worst <= 1e-12


def test_the_acceleration_solves_the_equation_of_motion_of_m_plus_d(m):
    """(M + D) a + bias = S^T t + J^T f with bias and J^T f from the oracle's inverse dynamics at a = 0"""
    g = cr.Ground()
    q, v, tau, q_des = states(m, 6, 2)
    worst = 0.0
    for b in range(6):
        f = cr.contact_law(g, *cr.feet(m, q[b], v[b]))
        t = ar.joint_torque(m, ar.motor_torque(m, g, q[b], v[b], tau[b], q_des[b], ROW), v[b], ROW)
        a = ar.accel(m, q[b], v[b], t, f, ROW)
        M = to._mass_matrix_and_potential(m, q[b])[0]
        h = to.id_torques(m, q[b], v[b], np.zeros(m.n), f)      # bias - J^T f: the generalised force that holds a = 0
        assert h.shape == (m.n,)
        lhs = (M + np.diag(ar.armature(m, ROW))) @ a + h
        worst = max(worst, np.abs(lhs - fr.generalised(m, t)).max() / max(1.0, np.abs(h).max()))
        # and the rotor does slow the actuated joints down: the solution is not the nominal one
        assert np.abs(a - fr.fd_ref(m, q[b], v[b], t, f)).max() > 1e-3
    print(f"(M + D) a + bias - S^T t - J^T f: worst residual {worst:.2e} of the bias")
    assert worst <= 1e-10


def test_damping_takes_damping_times_v_off_the_joint_torque_after_the_clamp(m):
    g = cr.Ground(tau_max=3.0)
    q, v, tau, q_des = states(m, 4, 3)
    cut = 0
    for b in range(4):
        motor = ar.motor_torque(m, g, q[b], v[b], tau[b], q_des[b], ROW)
        assert np.array_equal(motor, cr.pd_torque(m, g, q[b], v[b], tau[b], q_des[b], ROW[0], ROW[1]))
        assert np.abs(motor).max() <= 3.0
        cut += int((np.abs(motor) == 3.0).sum())
        t = ar.joint_torque(m, motor, v[b], ROW)
        assert np.array_equal(t, motor - ROW[2] * v[b, 6:])      # one product and one difference: nothing else, and not inside the clamp        # tau_out is the motor torque, the dynamics see the damped one
        out = ar.step(m, g, ROW, q[b], v[b], 5e-4, 1, tau[b], q_des[b])
        assert np.array_equal(out[4], motor)
        f = cr.contact_law(g, *cr.feet(m, q[b], v[b]))
        assert np.array_equal(out[2], ar.accel(m, q[b], v[b], t, f, ROW))
    assert cut > 0, "no torque of the fixture reaches the limit"
    assert np.array_equal(ar.armature(m, ROW)[:6], np.zeros(6)) and np.array_equal(ar.armature(m, ROW)[6:], np.full(12, ROW[3]))


def test_the_implicit_system_has_the_stated_diagonals(m):
    g = cr.Ground(tau_max=3.0)
    dt = 1e-3
    q, v, tau, q_des = states(m, 4, 4)
    seen = set()
    for b in range(4):
        motor = ar.motor_torque(m, g, q[b], v[b], tau[b], q_des[b], ROW)
        f = cr.contact_law(g, *cr.feet(m, q[b], v[b]))
        a_exp = ar.accel(m, q[b], v[b], ar.joint_torque(m, motor, v[b], ROW), f, ROW)
        A, rhs = ar.implicit_system(m, g, q[b], v[b], dt, motor, a_exp, True, ROW)
        A0, rhs0 = ir.implicit_system(m, g, q[b], v[b], dt, motor, a_exp, False, 0.0, 0.0)      # M, the feet, M a_exp and the feet's part
        dA, dr = A - A0, rhs - rhs0
        assert np.abs(dA - np.diag(np.diag(dA))).max() == 0.0
        kp, kd, c, arm = ROW
        for j in range(m.n):
            if j < 6:
                want_A, want_r = 0.0, 0.0
            elif abs(motor[j - 6]) < 3.0:
                want_A, want_r = arm + dt * (kd + c) + dt * dt * kp, arm * a_exp[j] - dt * kp * v[b, j]
                seen.add("free")
            else:
                want_A, want_r = arm + dt * c, arm * a_exp[j]
                seen.add("cut")
            assert abs(dA[j, j] - want_A) <= 1e-12 * max(1.0, abs(A[j, j])), (b, j)
            assert abs(dr[j] - want_r) <= 1e-12 * max(1.0, abs(rhs[j])), (b, j)
        # without a PD target nothing counts as free: dt damping on every actuated joint
        A1, _ = ar.implicit_system(m, g, q[b], v[b], dt, motor, a_exp, False, ROW)
        assert np.allclose(np.diag(A1 - A0)[6:], arm + dt * c, rtol=0, atol=1e-12) and np.abs(np.diag(A1 - A0)[:6]).max() == 0.0
    assert seen == {"free", "cut"}
