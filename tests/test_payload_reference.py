"""The declaration of a payload per robot, proved on the host: the baked tree of tests/payload_reference.py --
body `joint` with mass m + m_p, centre of mass (m c + m_p r) / (m + m_p) and the parallel-axis inertia -- has the mass matrix
M(q) + m_p J^T J, J the Jacobian of the payload point, which is what "a point mass rigidly attached at r" means.  No GPU.

J is taken by central differences of the point's world position, so the identity holds to the error of that difference.  The bar
is that error measured where it can be known: the same expression m_p J^T J on a foot point of the nominal tree, whose exact
Jacobian tests/implicit_reference.py states, differenced with the same step; times 4.  Both numbers are printed."""
import numpy as np
import pytest

from tests import fd_reference as fr
from tests import implicit_reference as ir
from tests import payload_reference as plr

H = 1e-5                                                  # the step of the central differences
CASES = [("quadruped", lambda: fr.quadruped(perturb=0.3), 5), ("tree32", lambda: fr.random_tree(n=32, seed=21, feet=(4, 31, 31, 17)), 9)]


@pytest.mark.parametrize("name,make,joint", CASES)
def test_the_baked_tree_is_the_nominal_tree_and_a_point_mass(name, make, joint):
    m = make()
    rng = np.random.default_rng(11)
    worst = bar = 0.0
    for _ in range(4):
        q = rng.uniform(-1, 1, m.n)
        r = rng.standard_normal(3); r *= rng.uniform(0.02, 0.15) / np.linalg.norm(r)
        mp = rng.uniform(0.5, 5.0)
        M = plr.mass_matrix(m, q)
        J = plr.central_jacobian(lambda x: plr.payload_point(m, x, r, joint), q, H)
        err = np.abs(plr.mass_matrix(plr.baked(m, [mp, *r], joint), q) - (M + mp * J.T @ J)).max()
        # the error of the same expression where the exact Jacobian is known: every foot point of the nominal tree
        exact = ir.foot_jacobians(m, q)[1]
        fd = 0.0
        for k in range(len(m.foot_joint)):
            Jk = plr.central_jacobian(lambda x: plr.foot_point(m, x, k), q, H)
            fd = max(fd, np.abs(mp * (Jk.T @ Jk - exact[k].T @ exact[k])).max())
        print(f"  {name}: |M_baked - (M + m_p J^T J)| {err:.3e}, finite-difference error of m_p J^T J on a foot point {fd:.3e} (bar {4 * fd:.3e})")
        assert err <= 4 * fd
        worst, bar = max(worst, err), max(bar, 4 * fd)
    assert bar < 1e-6 * np.abs(M).max()                   # and the bar is a tight one: the identity is not held to a loose number


@pytest.mark.parametrize("name,make,joint", CASES)
def test_a_massless_payload_bakes_the_nominal_tree_exactly(name, make, joint):
    m = make()
    b = plr.baked(m, [0.0, 0.1, -0.05, 0.02], joint)
    for field in ("parent", "jtype", "axis", "R_fix", "p_fix", "mass", "com", "inertia", "foot_joint", "foot_offset", "gravity"):
        assert np.array_equal(getattr(b, field), getattr(m, field)), field
    assert b.mass is not m.mass                           # a copy: the nominal tree is never written to
    loaded = plr.baked(m, [2.0, 0.1, -0.05, 0.02], joint)
    assert loaded.mass[joint] == m.mass[joint] + 2.0 and np.array_equal(np.delete(loaded.mass, joint), np.delete(m.mass, joint))
    assert np.array_equal(m.mass, make().mass) and np.array_equal(m.com, make().com) and np.array_equal(m.inertia, make().inertia)


def test_the_references_run_on_the_baked_tree_in_both_formats():
    """one robot, one substep: the float32 loop stays near the float64 one, and the payload moves the answer"""
    from tests import contact_reference as cr
    m = fr.quadruped(perturb=0.3)
    q, v, tau, _ = fr.inputs(m, 2, 5)
    q[:, 2] = 0.3
    q_des = q[:, 6:].copy()
    rows = np.array([[5.0, 0.1, 0.0, 0.05], [0.0, 0.0, 0.0, 0.0]], np.float32)
    g = cr.Ground()
    for implicit in (False, True):
        r64 = plr.step(m, g, rows, 5, q, v, 5e-4, 1, tau, q_des, 20.0, 1.5, np.float64, implicit)
        r32 = plr.step(m, g, rows, 5, q, v, 5e-4, 1, tau, q_des, 20.0, 1.5, np.float32, implicit)
        bare = plr.step(m, g, 0 * rows, 5, q, v, 5e-4, 1, tau, q_des, 20.0, 1.5, np.float64, implicit)
        assert r32[2].dtype == np.float32
        assert np.abs(r32[2] - r64[2]).max() < 1e-3 * np.abs(r64[2]).max()
        assert np.abs(r64[2][0, :6] - bare[2][0, :6]).max() > 1e-2 * np.abs(bare[2][0, :6]).max()      # the trunk that carries 5 kg
        assert np.array_equal(r64[2][1], bare[2][1])      # m_p = 0 is the nominal tree
