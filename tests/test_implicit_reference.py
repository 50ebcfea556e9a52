"""The reference of the linearly implicit contact step (tests/implicit_reference.py) checked against what it has to be: first-order
consistent with the explicit acceleration, settling where the explicit step does not, symmetric positive definite, the explicit
step itself where nothing is stiff, and solvable on the tree's sparsity.  No GPU."""
import os

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import crba_reference as cb
from tests import fd_reference as fr
from tests import implicit_reference as ir

KP, KD = 20.0, 1.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "implicit_settle.npz")


@pytest.fixture(scope="module")
def states():
    """8 `fr.inputs` states of the quadruped, the lowest foot 5 mm in the ground, with torques and PD targets"""
    m = fr.quadruped(0.1)
    q, v, tau, _ = fr.inputs(m, 8, 21)
    q = q.astype(np.float64)
    for b in range(len(q)):
        q[b, 2] -= cr.feet(m, q[b])[0][:, 2].min() + 0.005
    q_des = q[:, 6:] + np.random.default_rng(2).uniform(-0.1, 0.1, (8, 12))
    return m, cr.Ground(), q, v.astype(np.float64), tau.astype(np.float64), q_des


def test_the_implicit_acceleration_is_first_order_consistent(states):
    m, g, q, v, tau, q_des = states
    for b in range(len(q)):
        gap = []
        for dt in (1e-5, 5e-6):
            sy = []
            a = ir.implicit_step_ref(m, g, q[b], v[b], dt, 1, tau[b], q_des[b], KP, KD, systems=sy)[2]
            gap.append(np.abs(a - sy[0][2]).max())
        print(f"state {b}: |a_implicit - a_exp| {gap[0]:.3e} at dt = 1e-5, {gap[1]:.3e} at 5e-6, ratio {gap[0] / gap[1]:.3f}")
        assert gap[0] > 0 and 1.7 <= gap[0] / gap[1] <= 2.3


def test_the_system_is_symmetric_positive_definite_and_has_the_sparsity_of_the_mass_matrix(states):
    m, g, q, v, tau, q_des = states
    mask = cb.path_mask(m.parent)
    for b in range(len(q)):
        for target, ground in ((q_des[b], g), (q_des[b], cr.Ground(tau_max=12.0)), (None, g)):
            sy = []
            ir.implicit_step_ref(m, ground, q[b], v[b], 2e-3, 1, tau[b], target, KP, KD, systems=sy)
            A, rhs, _ = sy[0]
            assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max() and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
            assert not np.any(A[~mask])
            x, pivots = ir.ltdl_solve(m.parent, A, rhs)
            assert np.all(pivots > 0) and np.abs(x - np.linalg.solve(A, rhs)).max() <= 1e-9 * np.abs(x).max()
    m23 = fr.random_tree()
    q, v, tau, _ = fr.inputs(m23, 3, 5)
    from tests import push_reference as pr
    for b in range(3):
        sy = []
        ir.implicit_step_ref(m23, pr.general_ground(m23, q), q[b], v[b], 2e-3, 1, tau[b], q[b], KP, KD, systems=sy)
        A, rhs, _ = sy[0]
        assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0 and not np.any(A[~cb.path_mask(m23.parent)])
        assert np.abs(ir.ltdl_solve(m23.parent, A, rhs)[0] - np.linalg.solve(A, rhs)).max() <= 1e-9 * np.abs(rhs).max()


def test_above_the_ground_without_a_target_it_is_the_explicit_step(states):
    m, _, q, v, tau, _ = states
    far = cr.Ground(ground_z=-10.0)
    for dtype, tol in ((np.float64, 1e-11), (np.float32, 2e-4)):
        for b in range(3):
            kw = dict(dtype=dtype) if dtype is np.float64 else dict(dtype=dtype)
            got = ir.implicit_step_ref(m, far, q[b], v[b], 2e-3, 3, tau[b], None, KP, KD, **kw)
            ref = cr.contact_step_ref(m, far, q[b], v[b], 2e-3, 3, tau[b], None, KP, KD, **(dict(fd=fr.aba, dtype=dtype) if dtype is np.float32 else {}))
            for name, x, r in zip("qvaft", got, ref):
                err = np.abs(np.asarray(x, np.float64) - np.asarray(r, np.float64)).max()
                print(f"{np.dtype(dtype).name} state {b} {name}: {err:.2e} of {np.abs(r).max():.2e}")
                assert err <= tol * max(1.0, np.abs(r).max())


def test_the_float32_run_stays_in_float32_and_near_the_reference(states):
    m, g, q, v, tau, q_des = states
    ref = ir.implicit_step_ref(m, g, q[0], v[0], 2e-3, 2, tau[0], q_des[0], KP, KD)
    f32 = ir.implicit_step_ref(m, g, q[0], v[0], 2e-3, 2, tau[0], q_des[0], KP, KD, dtype=np.float32)
    assert all(x.dtype == np.float32 for x in f32)
    assert all(np.abs(x - r).max() <= 1e-3 * max(1.0, np.abs(r).max()) for x, r in zip(f32, ref))


def test_a_push_is_one_more_force_in_its_window(states):
    m, g, q, v, tau, q_des = states
    push = dict(F=[60.0, -30.0, 20.0], joint=5, first_substep=1, n_substeps=1)
    plain = ir.implicit_step_ref(m, g, q[0], v[0], 2e-3, 1, tau[0], q_des[0], KP, KD)
    missed = ir.implicit_step_ref(m, g, q[0], v[0], 2e-3, 1, tau[0], q_des[0], KP, KD, push=push)
    hit = ir.implicit_step_ref(m, g, q[0], v[0], 2e-3, 1, tau[0], q_des[0], KP, KD, push=dict(push, s0=1))
    assert all(np.array_equal(a, b) for a, b in zip(plain, missed))
    assert np.abs(hit[2] - plain[2]).max() > 0.1 and np.array_equal(hit[3], plain[3]) and np.array_equal(hit[4], plain[4])


def test_the_drop_settles_at_two_milliseconds_where_the_explicit_step_does_not():
    """2 ms x 500 on the default ground: the largest |v| over the last 20 % (measured: 9.2e-3 implicit, 8.5 explicit); the run is
    the one tests/golden/implicit_settle.npz stores."""
    d, G = cr.drop(), np.load(GOLDEN)
    args = (d["m"], d["g"], d["q"], d["v"], 2e-3, 500, d["tau_ff"], d["q_des"], d["kp"], d["kd"])
    trace = []
    q, v = ir.implicit_step_ref(*args, trace=trace)[:2]
    tail = ir.tail_speed(trace)
    print(f"implicit: tail |v| {tail:.3e}, z {q[2]:.4f}, pitch {q[4]:.4f}")
    assert tail <= 2e-2
    assert np.allclose(trace[19][0], G["q20"], rtol=0, atol=1e-12) and np.allclose(q, G["q"], rtol=0, atol=1e-9) and np.allclose(v, G["v"], rtol=0, atol=1e-9)
    assert abs(float(G["tail"]) - tail) <= 1e-9 and float(G["tail32"]) <= 2e-2
    trace = []
    with np.errstate(all="ignore"):
        cr.contact_step_ref(*args, trace=trace)
    explicit = ir.tail_speed(trace)
    print(f"explicit: tail |v| {explicit:.3e}")
    assert explicit >= 1.0
