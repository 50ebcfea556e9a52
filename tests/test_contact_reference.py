"""The references of the contact plant (tests/contact_reference.py) against what they can be held to without a GPU: the foot
velocity against differences of the foot position, the law against its declared properties, the step against step_ref, and
the stored settling run (tests/golden/contact_settle.npz) against its first substeps and against standing."""
import os

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_settle.npz")


@pytest.fixture(scope="module")
def settle():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tree", ["quadruped", "tilted", "tree23"])
def test_foot_velocity_is_the_derivative_of_the_foot_position_along_v(tree):
    m = {"quadruped": fr.quadruped, "tilted": lambda: fr.quadruped(perturb=0.3), "tree23": fr.random_tree}[tree]()
    q, v, _, _ = (x.astype(np.float64) for x in fr.inputs(m, 8, seed=3))
    h, worst = 1e-5, 0.0
    for b in range(len(q)):
        pos, vel = cr.feet(m, q[b], v[b])
        diff = (cr.feet(m, q[b] + h * v[b])[0] - cr.feet(m, q[b] - h * v[b])[0]) / (2 * h)
        worst = max(worst, np.abs(vel - diff).max() / np.abs(vel).max())
        assert np.array_equal(pos, cr.feet(m, q[b])[0]) and not np.any(cr.feet(m, q[b])[1])
    print(f"{tree}: {worst:.2e}")
    assert worst < 1e-7


def test_float32_kinematics_are_the_float64_ones_rounded():
    m = fr.random_tree()
    q, v, _, _ = fr.inputs(m, 4, seed=9)
    for b in range(4):
        p32, v32 = cr.feet(m, q[b], v[b], np.float32)
        p64, v64 = cr.feet(m, q[b], v[b])
        assert p32.dtype == np.float32 and v32.dtype == np.float32
        assert np.abs(p32 - p64).max() < 1e-5 * np.abs(p64).max() and np.abs(v32 - v64).max() < 1e-5 * np.abs(v64).max()


def test_the_law_is_continuous_at_touch_down_and_at_the_end_of_the_damping():
    g, eps = cr.Ground(), 1e-9
    vel = np.array([0.3, -0.2, -0.5])
    above, below = (cr.contact_law(g, np.array([0.0, 0.0, z]), vel) for z in (eps, -eps))
    assert not np.any(above)
    assert np.abs(below).max() <= g.stiffness * eps * (1 + g.damping * 0.5)
    pos = np.array([0.0, 0.0, -0.004])
    slow, fast = (cr.contact_law(g, pos, np.array([0.3, -0.2, 1 / g.damping + s * eps])) for s in (-1, 1))
    assert not np.any(fast) and slow[2] > 0
    assert np.abs(slow).max() <= 1.01 * g.stiffness * 0.004 * g.damping * eps
    # never pulls, and pushes harder on the way in
    assert cr.contact_law(g, pos, np.array([0.0, 0.0, 5.0]))[2] == 0
    assert cr.contact_law(g, pos, np.array([0.0, 0.0, -1.0]))[2] == g.stiffness * 0.004 * 4


def test_friction_opposes_the_slip_and_stays_inside_the_cone():
    g, rng = cr.Ground(), np.random.default_rng(1)
    pos = np.concatenate([rng.uniform(-1, 1, (4096, 2)), rng.uniform(-0.01, 0.005, (4096, 1))], axis=1)
    vel = rng.uniform(-1, 1, (4096, 3)) * 10.0 ** rng.uniform(-4, 0.5, (4096, 1))
    f = cr.contact_law(g, pos, vel)
    touching = f[:, 2] > 0
    assert touching.any() and (~touching).any() and np.all(f[:, 2] >= 0)
    assert not np.any(f[~touching])
    assert np.all(np.hypot(f[:, 0], f[:, 1]) <= g.mu * f[:, 2])
    assert np.all(np.sum(f[touching, :2] * vel[touching, :2], axis=1) < 0)
    fast = touching & (np.hypot(vel[:, 0], vel[:, 1]) > 20 * g.slip_velocity)
    assert fast.any() and np.all(np.hypot(f[fast, 0], f[fast, 1]) > 0.998 * g.mu * f[fast, 2])


def test_without_stiffness_the_step_is_step_ref_without_forces():
    m = fr.quadruped(perturb=0.3)
    q, v, tau, _ = fr.inputs(m, 2, seed=4)
    q[:, 2] = 0.0                                               # feet on both sides of the plane
    for b in range(2):
        got = cr.contact_step_ref(m, cr.Ground(stiffness=0.0), q[b], v[b], 1e-3, 3, tau[b], q[b, 6:], 20.0, 1.5)
        ref = fr.step_ref(m, q[b], v[b], 1e-3, 3, tau[b], q[b, 6:], 20.0, 1.5, np.zeros((4, 3)))
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], ref)) and not np.any(got[3])


def test_the_torque_limit_clamps_the_pd_torque():
    m = fr.quadruped()
    q, v, tau, _ = fr.inputs(m, 1, seed=4)
    free = cr.pd_torque(m, cr.Ground(), q[0], v[0], tau[0], None, 0.0, 0.0)
    held = cr.pd_torque(m, cr.Ground(tau_max=5.0), q[0], v[0], tau[0], None, 0.0, 0.0)
    assert np.abs(free).max() > 5 and np.array_equal(held, np.clip(free, -5, 5))
    assert np.array_equal(cr.pd_torque(m, cr.Ground(tau_max=0.0), q[0], v[0], tau[0], None, 0.0, 0.0), free)


def test_the_fixture_reproduces_its_first_fifty_substeps(settle):
    d = cr.drop()
    for k in ("q0", "v0", "tau_ff", "q_des"):
        assert np.array_equal(settle[k], d[{"q0": "q", "v0": "v"}.get(k, k)]), k
    assert (float(settle["dt"]), int(settle["n_sub"]), float(settle["kp"]), float(settle["kd"])) == (d["dt"], d["n_sub"], d["kp"], d["kd"])
    q, v, *_ = cr.contact_step_ref(d["m"], d["g"], d["q"], d["v"], d["dt"], 50, d["tau_ff"], d["q_des"], d["kp"], d["kd"])
    assert np.abs(q - settle["q50"]).max() < 1e-12 and np.abs(v - settle["v50"]).max() < 1e-12
    assert np.abs(cr.feet(d["m"], d["q"])[0][:, 2].min() - 0.02) < 1e-7


def test_the_fixtures_end_state_stands(settle):
    m = fr.quadruped()
    weight = m.mass.sum() * fr.G
    f, v = settle["f"], settle["v"]
    pos, vel = cr.feet(m, settle["q"], v)
    print(f"sum f_z {f[:, 2].sum():.4f} N of {weight:.4f} N, max|v| {np.abs(v).max():.2e}, penetration mm {np.round(-1e3 * pos[:, 2], 2)}")
    assert abs(f[:, 2].sum() - weight) < 1e-3 * weight
    assert np.abs(v).max() < 1e-2
    assert np.all(pos[:, 2] < 0) and np.all(f[:, 2] > 0)
    assert np.allclose(f, cr.contact_law(cr.Ground(), *cr.feet(m, settle["q"] - 5e-4 * v, v - 5e-4 * settle["a"])), rtol=0, atol=1e-6)
