"""The analytic reference of the momentum derivatives (tests/centroidal_derivative_reference.py) is held to central differences of
tests/crba_reference.centroidal_ref in fp64, before anything on the device is held to it.  No GPU.

The step of the differences, scanned over decades on the first 8 states of the tilted quadruped (largest |dh_dq| 1.16): the
largest |fd - analytic| of dh_dq is
    eps    1e-1     1e-2     1e-3     1e-4     1e-5     1e-6     1e-7     1e-8     1e-9
    error  1.6e-3   1.6e-5   1.6e-7   1.6e-9   1.6e-10  1.7e-9   2.3e-8   1.7e-7   1.8e-6
truncation (eps^2) down to 1e-4, round-off (1 / eps) from 1e-6 on: the bottom is eps = 1e-5 with 1.40e-10 of the largest |dh_dq|.
Agreement is asserted at ten times that, 1.4e-9 of the largest |reference| of each set (measured over the whole sets: 1.8e-10
on the 33 states of the quadruped, 5.3e-11 on the 23-joint and 3.8e-11 on the 32-joint tree)."""
import numpy as np
import pytest

from tests import centroidal_derivative_reference as cd
from tests import fd_reference as fr
from tests.torque_helpers import bar

EPS = 1e-5
FD_BOUND = 1.4e-9                       # ten times the error at the bottom of the curve, relative to the largest |reference|
NAMES = ("dh_dq", "dcom_dq", "hdot_bias")

TREES = {"quad": (lambda: fr.quadruped(0.1), 33, 41), "tree23": (fr.random_tree, 5, 42),
         "tree32": (lambda: fr.random_tree(n=32, feet=(5,)), 3, 43)}


@pytest.fixture(scope="module", params=sorted(TREES))
def case(request):
    make, B, seed = TREES[request.param]
    m = make()
    q, v = cd.states(m, B, seed)
    ref = cd.centroidal_derivatives_ref_batch(m, q, v)
    for x in (q, v, *ref):
        x.setflags(write=False)
    return request.param, m, q, v, ref


def test_analytic_reference_agrees_with_central_differences(case):
    name, m, q, v, ref = case
    fd = [cd.centroidal_derivatives_fd(m, q[b], v[b], EPS) for b in range(len(q))]
    for k, out in enumerate(NAMES):
        got = np.stack([f[k] for f in fd])
        scale = np.abs(ref[k]).max()
        err = np.abs(got - ref[k]).max() / scale
        print(f"  {name} {out}: {err:.2e} of the largest |reference| {scale:.2e} (bound {FD_BOUND:.1e})")
        assert err <= FD_BOUND, (name, out)


def test_the_step_sits_at_the_bottom_of_the_curve():
    m = fr.quadruped(0.1)
    q, v = cd.states(m, 2, 41)
    ref = [cd.centroidal_derivatives_ref(m, q[b], v[b])[0] for b in range(2)]
    err = {e: max(np.abs(cd.centroidal_derivatives_fd(m, q[b], v[b], e)[0] - ref[b]).max() for b in range(2)) for e in (1e-3, EPS, 1e-7)}
    print("  ", err)
    assert err[EPS] < err[1e-3] and err[EPS] < err[1e-7]


def test_bias_is_the_joint_order_sum_of_the_columns_bit_for_bit(case):
    _, m, q, v, (dh, _, bias) = case
    for b in range(len(q)):
        acc = np.zeros(6)
        for j in range(m.n):
            acc = acc + dh[b][:, j] * np.float64(v[b, j])
        assert np.array_equal(acc, bias[b])


def test_the_float32_run_is_float32_and_close():
    m = fr.quadruped(0.1)
    q, v = cd.states(m, 3, 41)
    out = cd.centroidal_derivatives_ref(m, q[0], v[0], np.float32)
    ref = cd.centroidal_derivatives_ref(m, q[0], v[0])
    assert all(x.dtype == np.float32 for x in out)
    assert all(np.abs(x - r).max() <= 1e-5 * np.abs(r).max() for x, r in zip(out, ref))


def test_a_base_100_m_away_changes_nothing_at_the_size_of_the_robot():
    """The base coordinates of the quadruped do not enter the derivatives.  In fp64 the translated reference is the untranslated
    one to rounding (1e-12 of the scale: 100 m x 2^-52 = 2e-14 m of position, in products of order 10); in float32 the translated
    run stays within the layer's bar of the untranslated states -- the property the kernel has to keep."""
    m = fr.quadruped(0.1)
    assert m.jtype[0] == 1 and m.jtype[1] == 1
    q, v = cd.states(m, 33, 41)
    far = q.copy()
    far[:, 0] += 100.0; far[:, 1] += 100.0
    assert far.dtype == np.float32
    ref = cd.centroidal_derivatives_ref_batch(m, q, v)
    ref_far = cd.centroidal_derivatives_ref_batch(m, far, v)
    f32 = cd.centroidal_derivatives_ref_batch(m, q, v, np.float32)
    f32_far = cd.centroidal_derivatives_ref_batch(m, far, v, np.float32)
    for k, out in enumerate(NAMES):
        scale = np.abs(ref[k]).max()
        moved, err, b_ = np.abs(ref_far[k] - ref[k]).max(), np.abs(f32_far[k] - ref[k]).max(), bar(ref[k], f32[k])
        print(f"  {out}: fp64 moved by {moved:.2e}, float32 at 100 m {err:.2e} (bar {b_:.2e}, float32 at home {np.abs(f32[k] - ref[k]).max():.2e})")
        assert moved <= 1e-12 * scale, out
        assert err <= b_, out
