"""The inverse-dynamics reference of the tests (tests/id_reference.py): the numpy restatement in float64 against the oracle it
restates, the oracle against Lagrange's equations on the two 32-joint trees that tests/test_torque_oracle.py never ran, and the
float32 run of the restatement, whose deviation is the floor the bars of tests/test_gpu_torque.py are built from."""
import numpy as np
import pytest

from oracle import torque_oracle as to
from tests import id_reference as ir

B = 8


@pytest.fixture(scope="module", params=list(ir.TREES))
def case(request):
    m = ir.TREES[request.param]()
    q, v, a, f = ir.samples(m, B, seed=9)
    return request.param, m, q, v, a, f, ir.oracle_batch(m, q, v, a, f)


def test_the_trees_are_what_their_names_say():
    t = {k: make() for k, make in ir.TREES.items()}
    assert [t[k].n for k in ("random32", "chain32", "star32")] == [32] * 3 and all(t[k].nu == 32 for k in ("random32", "chain32", "star32"))
    assert list(t["chain32"].parent) == list(range(-1, 31)) and list(t["chain32"].jtype) == [i % 2 for i in range(32)]
    assert list(t["star32"].parent) == [-1] + [0] * 31 and set(t["star32"].jtype) == {0, 1}
    assert [(t[k].n, t[k].nu, int(t[k].jtype[0])) for k in ("single_revolute", "single_prismatic")] == [(1, 1, 0), (1, 1, 1)]
    assert [(t[k].n, t[k].nu) for k in ("one_actuator", "five_actuators")] == [(12, 1), (12, 5)]
    m = t["eight_feet"]
    inner, leaves = ir.inner_and_leaves(m)
    feet = list(m.foot_joint)
    assert m.n == 10 and len(feet) == 8 and feet[4:6] == [0, 0]
    assert feet[0] in inner and feet[:4] == [feet[0]] * 4 and feet[6] in leaves and feet[6:] == [feet[6]] * 2
    assert t["no_feet"].n == 10 and len(t["no_feet"].foot_joint) == 0
    m = t["massless"]
    inner, leaves = ir.inner_and_leaves(m)
    gone = [i for i in range(m.n) if m.mass[i] == 0.0 and not m.inertia[i].any()]
    assert len(gone) == 3 and sum(i in inner for i in gone) == 2 and sum(i in leaves for i in gone) == 1
    assert not t["no_gravity"].gravity.any() and t["random23"].gravity.any()
    assert set(t["random23"].jtype) == {0, 1} and t["random23"].n == 23


def test_float64_restatement_equals_the_oracle(case):
    name, m, q, v, a, f, ref = case
    got = ir.id_torques_np_batch(m, q, v, a, f, np.float64)
    assert got.shape == ref.shape == (B, m.nu) and got.dtype == np.float64
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: float64 restatement against the oracle {err:.2e} of the largest torque")
    assert err <= 1e-12
    if len(m.foot_joint) == 0:
        assert np.array_equal(ir.id_torques_np_batch(m, q, v, a, None, np.float64), got)


def test_float32_run_is_float32_and_its_deviation_is_the_floor(case):
    """The figure per tree that the GPU test's bars start from: printed here, asserted nowhere (there is nothing to hold a
    number format's own cost to but itself)."""
    name, m, q, v, a, f, ref = case
    f32 = ir.id_torques_np_batch(m, q, v, a, f, np.float32)
    assert f32.dtype == np.float32 and f32.shape == ref.shape
    dev = np.abs(f32.astype(np.float64) - ref)
    print(f"{name}: float32 floor {dev.max():.2e} N m, {(dev.max(axis=1) / np.abs(ref).max(axis=1)).max():.2e} of a sample's largest torque "
          f"(largest torque {np.abs(ref).max():.1f})")
    assert np.isfinite(f32).all()


@pytest.mark.parametrize("name", ["chain32", "star32"])
def test_oracle_equals_lagrange_on_the_32_joint_trees(name):
    """The tolerance of tests/test_torque_oracle.py, 2e-7 max(1, max |tau|), at the step it uses, h = 1e-6: the central
    differences of M and V lose about eps |M| / h, which grows with the lever arms of a deep chain as the torques do, so the
    relative figure stays where it is on the quadruped and the step needs no change at depth 32: the chain's two samples
    differ by 3.7e-7 and 5.4e-7 N m at torques of 1267 and 1604 N m, the star's by 4.5e-8 and 1.2e-8 at 162 and 105."""
    m = ir.TREES[name]()
    q, v, a, f = (x.astype(np.float64) for x in ir.samples(m, 2, seed=10))
    for b in range(2):
        tau, ref = to.id_torques(m, q[b], v[b], a[b], f[b]), to.lagrangian_torques(m, q[b], v[b], a[b], f[b])
        err = np.abs(tau - ref).max()
        print(f"{name} sample {b}: Newton-Euler against Lagrange {err:.2e} (largest torque {np.abs(ref).max():.1f})")
        assert err <= 2e-7 * max(1.0, np.abs(ref).max())
