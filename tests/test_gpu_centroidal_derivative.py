"""GPU checks of nmpc_centroidal_derivatives_batch (dh_dq = d(A_g v)/dq, dcom_dq, hdot_bias) against the fp64 analytic reference
of tests/centroidal_derivative_reference.py, itself held to finite differences in tests/test_centroidal_derivative_reference.py.
The bar is the layer's own (torque_helpers.held): max(1e-5 of the largest |reference|, 4 x the deviation of the float32 numpy
recursion); bit-for-bit claims are equality of bit patterns.  Every output buffer starts as a sentinel, so an entry the kernel
does not write shows.  Every figure is printed before it is asserted."""
import copy

import numpy as np
import pytest

from tests import centroidal_derivative_reference as cd
from tests import contact_reference as ct
from tests import crba_reference as cr
from tests import fd_reference as fr
from tests.torque_helpers import bar, held, host, layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -7.25e33
E_ARG = -1
NAMES = ("dh", "dcom", "bias")


def call(L, q, v, want=NAMES, B=None, null=()):
    """The C call on sentinel-filled outputs: ({name: tensor}, return code).  `want`: the outputs handed over; `null`: inputs
    replaced by NULL; B: the batch size handed over instead of the tensors' own."""
    from iterative_learning_nmpc_amd._lib import ptr, stream
    t32 = lambda x: torch.as_tensor(np.array(x, np.float32), device=L.device).contiguous()      # noqa: E731
    q, v = t32(q), t32(v)
    rows, n = q.shape[0], L.n
    out = {k: torch.full((rows,) + s, SENTINEL, dtype=torch.float32, device=L.device) for k, s in (("dh", (6, n)), ("dcom", (3, n)), ("bias", (6,)))}
    o = lambda k: ptr(out[k]) if k in want else None      # noqa: E731
    rc = L.lib.nmpc_centroidal_derivatives_batch(L._h, rows if B is None else B, None if "q" in null else ptr(q), None if "v" in null else ptr(v),
                                                 o("dh"), o("dcom"), o("bias"), stream(L.device))
    torch.cuda.synchronize()
    return out, rc


def untouched(t):
    return same(t, torch.full_like(t, SENTINEL))


class Case:
    """A tree, its device layer, B float32 states (base velocity N(0, 0.3), joint rates N(0, 2.0)), their fp64 reference and
    float32 numpy recursion, and the device outputs on sentinel-filled buffers: computed once, never written to."""
    def __init__(self, m, B, seed):
        self.m, self.L = m, layer(m)
        self.q, self.v = cd.states(m, B, seed)
        self.ref = dict(zip(NAMES, cd.centroidal_derivatives_ref_batch(m, self.q, self.v)))
        self.f32 = dict(zip(NAMES, cd.centroidal_derivatives_ref_batch(m, self.q, self.v, np.float32)))
        self.dev, rc = call(self.L, self.q, self.v)
        assert rc == 0, rc
        for x in (self.q, self.v, *self.ref.values(), *self.f32.values()):
            x.setflags(write=False)


@pytest.fixture(scope="module")
def quad():
    return Case(fr.quadruped(0.1), 33, seed=41)


@pytest.fixture(scope="module")
def tree23():
    return Case(fr.random_tree(), 5, seed=42)


@pytest.fixture(scope="module")
def tree32():
    return Case(fr.random_tree(n=32, feet=(5,)), 3, seed=43)


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["quad", "tree23", "tree32"])
def test_outputs_match_the_reference(which, request):
    """The tilted quadruped at B = 33 (the edge of a 32-robot block lies inside the batch), the 23-joint tree with prismatic joints
    behind revolute ones, and 32 joints: the largest tree, the slice of the block at its largest (139 264 B)."""
    c = request.getfixturevalue(which)
    ok = True
    for k in NAMES:
        got, = host(c.dev[k])
        assert got.shape == c.ref[k].shape and not (got == np.float32(SENTINEL)).any(), k
        ok = held(f"{which} {k}", got.astype(np.float64), c.ref[k], c.f32[k]) and ok
    assert ok


# ---- 2. time variation --------------------------------------------------------------------------------------------------------------
def test_dcom_is_the_linear_map_over_the_mass_and_bias_is_the_columns_times_v(quad):
    """dcom_dq against the linear rows of the same handle's A_g over the total mass, at the bar of dcom_dq; hdot_bias against
    dh_dq @ v in fp64 from the device's own dh_dq, at the bar of hdot_bias (the layer's bar of the array that is compared)."""
    c = quad
    _, _, Ag = c.L.centroidal(c.q.copy(), c.v.copy(), jacobian=True)
    Ag, dh, dcom, bias = (x.astype(np.float64) for x in host(Ag, c.dev["dh"], c.dev["dcom"], c.dev["bias"]))
    total = c.m.mass.astype(np.float32).astype(np.float64).sum()
    e1, b1 = np.abs(dcom - Ag[:, :3] / total).max(), bar(c.ref["dcom"], c.f32["dcom"])
    e2, b2 = np.abs(bias - np.einsum("bij,bj->bi", dh, c.v.astype(np.float64))).max(), bar(c.ref["bias"], c.f32["bias"])
    print(f"  dcom_dq - Ag_lin / m: {e1:.2e} (bar {b1:.2e});  hdot_bias - dh_dq v: {e2:.2e} (bar {b2:.2e}, scale {np.abs(c.ref['bias']).max():.2e})")
    assert e1 <= b1 and e2 <= b2


# ---- 3. Newton-Euler of the whole tree ------------------------------------------------------------------------------------------------
def wrench_residual(m, a, p, com, Ag, bias, f):
    """the largest |A_g a + hdot_bias - [sum f + m g; sum (p_i - com) x f_i]| and the largest |right-hand side|, combined in fp64"""
    a, p, com, Ag, bias, f = (np.asarray(x, np.float64) for x in (a, p, com, Ag, bias, f))
    total = m.mass.astype(np.float32).astype(np.float64).sum()
    rhs = np.concatenate([f.sum(axis=1) + total * m.gravity, np.cross(p - com[:, None], f).sum(axis=1)], axis=1)
    return np.abs(np.einsum("bij,bj->bi", Ag, a) + bias - rhs).max(), np.abs(rhs).max()


def test_momentum_rate_is_the_wrench_on_the_tree(quad):
    """h_dot = A_g a + hdot_bias is the sum of the external forces and of their moments about the centre of mass: the new call
    against forward_dynamics, foot_kinematics and centroidal, which share no code with it.  The identity goes through M^-1 in
    float32, so its floor is the same identity on the float32 numpy references; 4 x that, at least 1e-5 of the right-hand side."""
    c, B = quad, 33
    _, _, tau, f = fr.inputs(c.m, B, seed=45)
    q, v = c.q.copy(), c.v.copy()                         # the layer takes writable arrays
    a = c.L.forward_dynamics(q, v, tau, f)
    p, _ = c.L.foot_kinematics(q)
    com, _, Ag = c.L.centroidal(q, v, jacobian=True)
    res, scale = wrench_residual(c.m, *host(a, p, com, Ag, c.dev["bias"]), f)
    a32 = fr.aba_batch(c.m, c.q, c.v, tau, f, np.float32)
    p32 = np.stack([ct.feet(c.m, c.q[b], None, np.float32)[0] for b in range(B)])
    _, com32, _, Ag32 = cr.crba_batch(c.m, c.q, c.v, np.float32)
    res32, _ = wrench_residual(c.m, a32, p32, com32, Ag32, c.f32["bias"], f)
    bound = max(4 * res32, 1e-5 * scale)
    print(f"  A_g a + hdot_bias - wrench: {res:.2e} (bound {bound:.2e}: float32 references {res32:.2e}, largest right-hand side {scale:.2e}, "
          f"largest |a| {np.abs(a32).max():.2e})")
    assert res <= bound


# ---- 4. rows and outputs ------------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_batch_and_an_output_not_on_its_neighbours():
    """B = 65: two full blocks of 32 and a ragged one."""
    m = fr.quadruped(0.1)
    L = layer(m)
    q, v = cd.states(m, 65, seed=44)
    whole, rc = call(L, q, v)
    assert rc == 0 and not any((host(t)[0] == np.float32(SENTINEL)).any() for t in whole.values())
    for b in (0, 31, 32, 64):
        row, rc = call(L, q[b:b + 1], v[b:b + 1])
        assert rc == 0
        for k in NAMES:
            assert same(row[k][0], whole[k][b]), (k, b)
    for k in NAMES:
        alone, rc = call(L, q, v, want=(k,))
        assert rc == 0 and same(alone[k], whole[k]), k
        assert all(untouched(alone[o]) for o in NAMES if o != k), k
    # the Python layer hands the same buffers over
    dh, dcom, bias = L.centroidal_derivatives(q, v, com_jacobian=True, bias=True)
    assert same(dh, whole["dh"]) and same(dcom, whole["dcom"]) and same(bias, whole["bias"])
    assert same(L.centroidal_derivatives(q, v), whole["dh"])
    dh, bias = L.centroidal_derivatives(q, v, bias=True)
    assert same(dh, whole["dh"]) and same(bias, whole["bias"])


# ---- 5. refusals and edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kw", [
    ("B < 0", dict(B=-1)),
    ("q NULL", dict(null=("q",))),
    ("v NULL", dict(null=("v",))),
    ("all outputs NULL", dict(want=())),
])
def test_bad_arguments_are_refused_before_any_launch(quad, name, kw):
    out, rc = call(quad.L, quad.q[:3], quad.v[:3], **kw)
    assert rc == E_ARG, (name, rc)
    assert quad.L.lib.nmpc_torque_last_error(quad.L._h)
    assert all(untouched(t) for t in out.values()), name


def test_the_empty_batch_is_ok_and_launches_nothing(quad):
    out, rc = call(quad.L, quad.q[:3], quad.v[:3], B=0)
    assert rc == 0 and all(untouched(t) for t in out.values())
    dh, dcom, bias = quad.L.centroidal_derivatives(quad.q[:0], quad.v[:0], com_jacobian=True, bias=True)
    assert (tuple(dh.shape), tuple(dcom.shape), tuple(bias.shape)) == ((0, 6, 18), (0, 3, 18), (0, 6))


def test_a_massless_tree_is_refused(quad):
    from iterative_learning_nmpc_amd._lib import NmpcError
    bad = copy.deepcopy(quad.m)
    bad.mass[:] = 0.0; bad.inertia[:] = 0.0
    L = layer(bad)
    out, rc = call(L, quad.q[:3], quad.v[:3])
    assert rc == E_ARG and b"mass" in L.lib.nmpc_torque_last_error(L._h)
    assert all(untouched(t) for t in out.values())
    with pytest.raises(NmpcError, match="mass"):
        L.centroidal_derivatives(quad.q[:3], quad.v[:3])


def test_a_massless_leaf_among_massive_bodies_gives_finite_outputs(quad):
    """Nothing is inverted: the forward dynamics has no pivot for such a body, this call has no use for one."""
    m = copy.deepcopy(quad.m)
    leaf = m.n - 1
    assert leaf not in list(m.parent)
    m.mass[leaf] = 0.0; m.inertia[leaf] = 0.0
    out, rc = call(layer(m), quad.q[:5], quad.v[:5])
    assert rc == 0
    ref = dict(zip(NAMES, cd.centroidal_derivatives_ref_batch(m, quad.q[:5], quad.v[:5])))
    f32 = dict(zip(NAMES, cd.centroidal_derivatives_ref_batch(m, quad.q[:5], quad.v[:5], np.float32)))
    for k in NAMES:
        got, = host(out[k])
        assert np.isfinite(got).all(), k
        assert held(f"massless leaf {k}", got.astype(np.float64), ref[k], f32[k])


def test_shapes_are_checked_in_python(quad):
    with pytest.raises(ValueError, match="expected"):
        quad.L.centroidal_derivatives(quad.q[:2, :17], quad.v[:2])
    with pytest.raises(ValueError, match="batch sizes"):
        quad.L.centroidal_derivatives(quad.q[:2], quad.v[:3])


@pytest.mark.parametrize("where", ["q", "v"])
def test_a_row_that_is_not_finite_stays_in_its_row(quad, where):
    q, v = quad.q.copy(), quad.v.copy()
    (q if where == "q" else v)[7, 9] = np.nan
    out, rc = call(quad.L, q, v)
    assert rc == 0
    for k in NAMES:
        got, = host(out[k])
        if where == "q" or k != "dcom":                   # the centre of mass does not move with v
            assert not np.isfinite(got[7]).all(), k
        keep = torch.arange(33, device=out[k].device) != 7
        assert same(out[k][keep], quad.dev[k][keep]), k


# ---- 6. base position ---------------------------------------------------------------------------------------------------------------
def test_a_base_100_m_away_is_held_to_the_bar_of_the_states_at_home(quad):
    """The reference does not move with the base position (asserted in tests/test_centroidal_derivative_reference.py), so the
    reference and the bar of the untranslated states are used."""
    far = quad.q.copy()
    far[:, 0] += 100.0; far[:, 1] += 100.0
    out, rc = call(quad.L, far, quad.v)
    assert rc == 0
    ok = True
    for k in NAMES:
        got, = host(out[k])
        ok = held(f"at 100 m {k}", got.astype(np.float64), quad.ref[k], quad.f32[k]) and ok
    assert ok
