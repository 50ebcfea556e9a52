"""GPU checks of the composite-inertia outputs of the torque layer (nmpc_mass_matrix_batch, nmpc_centroidal_batch) against the
fp64 references of tests/crba_reference.py (themselves checked in tests/test_crba_reference.py): M against the Jacobian
derivation of the oracle, com, h, A_g against the same per-body Jacobians.  The bar is the layer's own (torque_helpers.held):
max(1e-5 of the largest |reference|, 4 x the deviation of the float32 numpy recursion); bit-for-bit claims are equality of bit
patterns.  Every output buffer starts as a sentinel, so an entry the kernel does not write shows.  Every figure is printed
before it is asserted."""
import copy

import numpy as np
import pytest

from tests import crba_reference as cr
from tests import fd_reference as fr
from tests.torque_helpers import bar, held, host, layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -7.25e33
E_ARG = -1


def call(L, q, v=None, want=("M", "com", "h", "Ag"), B=None, null=()):
    """The two C calls on sentinel-filled outputs: ({name: tensor}, {call: return code}).  `want`: the outputs handed over;
    `null`: inputs replaced by NULL; B: the batch size handed over instead of the tensors' own."""
    from iterative_learning_nmpc_amd._lib import ptr, stream
    t32 = lambda x: None if x is None else torch.as_tensor(np.array(x, np.float32), device=L.device).contiguous()      # noqa: E731
    q, v = t32(q), t32(v)
    rows, n = q.shape[0], L.n
    out = {k: torch.full((rows,) + s, SENTINEL, dtype=torch.float32, device=L.device)
           for k, s in (("M", (n, n)), ("com", (3,)), ("h", (6,)), ("Ag", (6, n)))}
    o = lambda k: ptr(out[k]) if k in want else None      # noqa: E731
    B = rows if B is None else B
    qp, vp = (None if "q" in null else ptr(q)), (None if "v" in null else ptr(v))
    rc = {}
    if "M" in want or want == ():
        rc["M"] = L.lib.nmpc_mass_matrix_batch(L._h, B, qp, o("M"), stream(L.device))
    if set(want) - {"M"} or want == ():
        rc["c"] = L.lib.nmpc_centroidal_batch(L._h, B, qp, vp, o("com"), o("h"), o("Ag"), stream(L.device))
    torch.cuda.synchronize()
    return out, rc


def untouched(t):
    return same(t, torch.full_like(t, SENTINEL))


class Case:
    """A tree, its device layer, B float32 states, their fp64 references and float32 numpy recursion, and the device outputs on
    sentinel-filled buffers: computed once, never written to."""
    def __init__(self, m, B, seed):
        self.m, self.L = m, layer(m)
        self.q, self.v, _, _ = fr.inputs(m, B, seed)
        self.ref = dict(zip(("com", "h", "Ag"), cr.centroidal_ref_batch(m, self.q, self.v)), M=cr.mass_matrix_ref_batch(m, self.q))
        self.f32 = dict(zip(("M", "com", "h", "Ag"), cr.crba_batch(m, self.q, self.v, np.float32)))
        self.dev, rc = call(self.L, self.q, self.v)
        assert rc == {"M": 0, "c": 0}, rc
        for x in (self.q, self.v, *self.ref.values(), *self.f32.values()):
            x.setflags(write=False)


@pytest.fixture(scope="module")
def quad():
    return Case(fr.quadruped(0.1), 33, seed=41)


@pytest.fixture(scope="module")
def tree23():
    return Case(fr.random_tree(), 5, seed=42)


def accurate(c):
    ok = True
    for k in ("M", "com", "h", "Ag"):
        got, = host(c.dev[k])
        assert got.shape == c.ref[k].shape and not (got == np.float32(SENTINEL)).any(), k
        ok = held(k, got.astype(np.float64), c.ref[k], c.f32[k]) and ok
    return ok


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------
def test_quadruped_matches_the_references(quad):
    """B = 33: the edge of a 32-robot block lies inside the batch."""
    assert accurate(quad)


def test_general_tree_matches_the_references(tree23):
    """23 joints, prismatic joints behind revolute ones, two feet on one body."""
    assert accurate(tree23)


def test_the_largest_tree_matches_the_reference():
    """32 joints: the largest tree the handle takes, the slice of the block at its largest (139 264 B); B = 17."""
    m = fr.random_tree(n=32, feet=(5,))
    q, v, _, _ = fr.inputs(m, 17, seed=43)
    out, rc = call(layer(m), q, want=("M",))
    assert rc == {"M": 0}
    M, = host(out["M"])
    assert not (M == np.float32(SENTINEL)).any()
    assert held("M (32 joints)", M.astype(np.float64), cr.mass_matrix_ref_batch(m, q), cr.crba_batch(m, q, v, np.float32)[0])


# ---- 2. structure -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["quad", "tree23"])
def test_mass_matrix_is_symmetric_and_zero_off_the_paths_bit_for_bit(which, request):
    c = request.getfixturevalue(which)
    M = c.dev["M"]
    assert same(M, M.transpose(1, 2).contiguous())
    off = torch.as_tensor(~cr.path_mask(c.m.parent), device=M.device)
    assert bool(off.any())
    zeros = M[:, off]
    assert same(zeros, torch.zeros_like(zeros))           # +0.0, not -0.0 and not a small number


# ---- 3. batch independence ----------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_batch_and_ag_changes_no_bits():
    """B = 65: two full blocks of 32 and a ragged one."""
    m = fr.quadruped(0.1)
    L = layer(m)
    q, v, _, _ = fr.inputs(m, 65, seed=44)
    whole, rc = call(L, q, v)
    assert rc == {"M": 0, "c": 0}
    for b in (0, 31, 32, 64):
        row, rc = call(L, q[b:b + 1], v[b:b + 1])
        assert rc == {"M": 0, "c": 0}
        for k in ("M", "com", "h", "Ag"):
            assert same(row[k][0], whole[k][b]), (k, b)
    bare, rc = call(L, q, v, want=("com", "h"))
    assert rc == {"c": 0} and same(bare["com"], whole["com"]) and same(bare["h"], whole["h"]) and untouched(bare["Ag"])
    only_com, rc = call(L, q, None, want=("com",))
    assert rc == {"c": 0} and same(only_com["com"], whole["com"]) and untouched(only_com["h"])
    # the Python layer hands the same buffers over
    com, h, Ag = L.centroidal(q, v, jacobian=True)
    com2, none = L.centroidal(q)
    assert same(com, whole["com"]) and same(h, whole["h"]) and same(Ag, whole["Ag"]) and same(com2, com) and none is None
    assert same(L.mass_matrix(q), whole["M"])


# ---- 4. against the layer's own inverse dynamics ------------------------------------------------------------------------------------
def test_columns_are_the_inverse_dynamics_of_unit_accelerations(tree23):
    """Column j of M is id_torques(q, 0, e_j) - id_torques(q, 0, 0) on a handle with every joint actuated.  Both sides are fp32
    evaluations, so neither is the other's reference: the difference is held to the bar of M, the fp64 M as its scale."""
    c, n, B = tree23, tree23.m.n, 3
    assert c.m.nu == n
    q = np.repeat(c.q[:B], n + 1, axis=0)                 # per state: n unit accelerations and the zero one
    a = np.tile(np.concatenate([np.eye(n), np.zeros((1, n))]), (B, 1)).astype(np.float32)
    tau, = host(c.L.id_torques(q, np.zeros_like(q), a))
    tau = tau.reshape(B, n + 1, n).astype(np.float64)
    cols = (tau[:, :n] - tau[:, n:]).transpose(0, 2, 1)   # [b][:, j] = column j
    M, = host(c.dev["M"][:B])
    err, b_ = np.abs(M - cols).max(), bar(c.ref["M"][:B], c.f32["M"][:B])
    print(f"  M - (id(e_j) - id(0)): {err:.2e} (bar {b_:.2e}, scale {np.abs(c.ref['M'][:B]).max():.2e}, largest |tau| {np.abs(tau).max():.2e})")
    assert err <= b_


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def massless(m):
    bad = copy.deepcopy(m)
    bad.mass[:] = 0.0; bad.inertia[:] = 0.0
    return bad


@pytest.mark.parametrize("name, kw", [
    ("B < 0", dict(B=-1)),
    ("q NULL", dict(null=("q",))),
    ("M NULL / all outputs NULL", dict(want=())),
    ("h without v", dict(want=("h",), null=("v",))),
])
def test_bad_arguments_are_refused_before_any_launch(quad, name, kw):
    out, rc = call(quad.L, quad.q[:3], quad.v[:3], **kw)
    assert rc and all(r == E_ARG for r in rc.values()), (name, rc)
    assert quad.L.lib.nmpc_torque_last_error(quad.L._h)
    assert all(untouched(t) for t in out.values()), name


def test_the_empty_batch_is_ok_and_launches_nothing(quad):
    out, rc = call(quad.L, quad.q[:3], quad.v[:3], B=0)
    assert rc == {"M": 0, "c": 0} and all(untouched(t) for t in out.values())
    assert quad.L.mass_matrix(quad.q[:0]).shape == (0, 18) + (18,)
    com, h, Ag = quad.L.centroidal(quad.q[:0], quad.v[:0], jacobian=True)
    assert (tuple(com.shape), tuple(h.shape), tuple(Ag.shape)) == ((0, 3), (0, 6), (0, 6, 18))


def test_a_massless_tree_has_a_zero_mass_matrix_and_no_centre_of_mass(quad):
    from iterative_learning_nmpc_amd._lib import NmpcError
    L = layer(massless(quad.m))
    out, rc = call(L, quad.q[:3], quad.v[:3])
    assert rc == {"M": 0, "c": E_ARG}
    assert b"mass" in L.lib.nmpc_torque_last_error(L._h)
    assert all(untouched(out[k]) for k in ("com", "h", "Ag"))
    M, = host(out["M"])
    assert np.array_equal(M, np.zeros_like(M))
    with pytest.raises(NmpcError, match="mass"):
        L.centroidal(quad.q[:3])


def test_shapes_are_checked_in_python(quad):
    with pytest.raises(ValueError, match="expected"):
        quad.L.mass_matrix(quad.q[:2, :17])
    with pytest.raises(ValueError, match="batch sizes"):
        quad.L.centroidal(quad.q[:2], quad.v[:3])


def test_a_row_that_is_not_finite_stays_in_its_row(quad):
    q = quad.q[:33].copy()
    q[7, 9] = np.nan
    out, rc = call(quad.L, q, quad.v[:33])
    assert rc == {"M": 0, "c": 0}
    for k in ("M", "com", "h", "Ag"):
        got, = host(out[k])
        assert not np.isfinite(got[7]).all(), k
        keep = torch.arange(33, device=out[k].device) != 7
        assert same(out[k][keep], quad.dev[k][keep]), k
