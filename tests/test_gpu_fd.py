"""GPU checks of the forward dynamics of the torque layer (nmpc_fd_accel_batch, nmpc_fd_step_batch) against fd_ref, the fp64
solve with the mass matrix (tests/fd_reference.py, itself checked in tests/test_fd_reference.py), against the shipped inverse
dynamics and against closed forms.  The bar of the accelerations is the torque layer's own, 1e-5 of the largest |a| of a
sample (tests/test_gpu_torque.py); bit-for-bit claims are array equality.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from tests import fd_reference as fr
from tests.torque_helpers import host, layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BAR = 1e-5
ZERO3 = (0.0, 0.0, 0.0)


class Case:
    """A tree, its device layer, B float32 samples and their fp64 accelerations: computed once, never written to."""
    def __init__(self, m, B, seed):
        self.m, self.L = m, layer(m)
        self.q, self.v, self.tau, self.f = fr.inputs(m, B, seed)
        self.a = fr.fd_ref_batch(m, self.q, self.v, self.tau, self.f)
        for x in (self.q, self.v, self.tau, self.f, self.a):
            x.setflags(write=False)


class QuadrupedCases(dict):
    """perturb -> the quadruped tree's case, built when first asked for"""
    def __missing__(self, perturb):
        self[perturb] = Case(fr.quadruped(perturb), 257, seed=257)
        return self[perturb]


@pytest.fixture(scope="module")
def quad():
    return QuadrupedCases()


@pytest.fixture(scope="module")
def tree23():
    return Case(fr.random_tree(), 96, seed=5)


# ---- 1. parity with fd_ref ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 33, 257])
@pytest.mark.parametrize("perturb", [0.0, 0.3])
def test_accelerations_match_fd_ref(quad, perturb, B):
    """B = 33: the edge of a 32-robot block lies inside the batch; B = 1: all lanes but one idle."""
    c = quad[perturb]
    a, = host(c.L.forward_dynamics(c.q[:B], c.v[:B], c.tau[:B], c.f[:B]))
    assert a.shape == (B, 18)
    err = fr.rel_err(a, c.a[:B])
    print(f"perturb {perturb} B {B}: {err:.2e}")
    assert err < BAR


def test_general_tree_matches_fd_ref(tree23):
    """23 joints, all actuated, prismatic joints inside the tree, two feet on one body, a foot on joint 0."""
    c = tree23
    a, = host(c.L.forward_dynamics(c.q, c.v, c.tau, c.f))
    err = fr.rel_err(a, c.a)
    print(f"random 23-joint tree: {err:.2e}")
    assert err < BAR


def test_tree_too_large_for_the_wide_block_matches_fd_ref():
    """30 joints: the slice of 32 robots does not fit a CU's LDS, the 16-robot block runs; B = 40 is two and a half of them."""
    m = fr.random_tree(n=30, seed=13, feet=(4, 29, 29, 17))
    c = Case(m, 40, seed=6)
    a, = host(c.L.forward_dynamics(c.q, c.v, c.tau, c.f))
    err = fr.rel_err(a, c.a)
    print(f"random 30-joint tree: {err:.2e}")
    assert err < BAR


# ---- 2. inverse of the shipped inverse dynamics ---------------------------------------------------------------------------------
def test_forward_dynamics_inverts_id_torques_on_the_device(tree23):
    """The kernel does not hold 1e-5 here (1.16e-5 measured), and neither does the format: the torques of this tree reach
    870 N m, their float32 rounding alone moves the accelerations by 3.0e-6 of the largest |a| (fp64 recursion on the rounded
    exact torques), and the float32 numpy recursion on them is 1.04e-5 away.  So the bar is, as for check 1, 4x the error of
    that float32 run, computed here: 4.1e-5."""
    from oracle import torque_oracle as to
    c = tree23
    a = np.random.default_rng(8).uniform(-5, 5, c.q.shape).astype(np.float32)
    exact = np.stack([to.id_torques(c.m, *(x[b].astype(np.float64) for x in (c.q, c.v, a, c.f))) for b in range(len(a))])
    floor = fr.rel_err(fr.aba_batch(c.m, c.q, c.v, exact.astype(np.float32), c.f, np.float32), a.astype(np.float64))
    tau = c.L.id_torques(c.q, c.v, a, c.f)
    back, = host(c.L.forward_dynamics(c.q, c.v, tau, c.f))
    err = fr.rel_err(back, a.astype(np.float64))
    print(f"fd(id(a)) - a: {err:.2e}; float32 numpy recursion on the exact torques: {floor:.2e}")
    assert err < max(BAR, 4 * floor)


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------------
def test_free_fall_and_statics(quad):
    from oracle import torque_oracle as to
    m, L = quad[0.0].m, quad[0.0].L
    q, f = fr.standing(m)
    z = np.zeros((1, 18), np.float32)
    a, = host(L.forward_dynamics(q[None], z))
    expect = np.zeros(18); expect[2] = -fr.G
    print(f"free fall: {np.abs(a[0] - expect).max():.2e}")
    assert np.abs(a[0] - expect).max() < BAR * fr.G
    tau = to.id_torques(m, q, np.zeros(18), np.zeros(18), f)[-12:]
    a, = host(L.forward_dynamics(q[None], z, tau[None], f[None]))
    print(f"statics: {np.abs(a).max():.2e}")
    assert np.abs(a).max() < BAR * fr.G


def test_nothing_moves_without_gravity_velocity_torque_and_force(quad):
    c = quad[0.3]
    a, = host(layer(c.m, gravity=ZERO3).forward_dynamics(c.q[:33], np.zeros((33, 18), np.float32)))
    assert np.array_equal(a, np.zeros((33, 18), np.float32))


# ---- 4. NULL arguments, 5. batch independence ---------------------------------------------------------------------------------
def test_omitted_torques_and_forces_are_zeros(quad):
    c, B = quad[0.3], 33
    q, v, tau, f = c.q[:B], c.v[:B], c.tau[:B], c.f[:B]
    no_tau, zero_tau, no_f, zero_f = host(c.L.forward_dynamics(q, v, None, f), c.L.forward_dynamics(q, v, 0 * tau, f),
                                          c.L.forward_dynamics(q, v, tau), c.L.forward_dynamics(q, v, tau, 0 * f))
    assert np.array_equal(no_tau, zero_tau) and np.array_equal(no_f, zero_f)
    assert not np.array_equal(no_tau, no_f)


def test_a_row_does_not_depend_on_its_batch(quad):
    c = quad[0.3]
    whole, = host(c.L.forward_dynamics(c.q[:33], c.v[:33], c.tau[:33], c.f[:33]))
    for b in (0, 15, 16, 31, 32):
        row, = host(c.L.forward_dynamics(c.q[b:b + 1], c.v[b:b + 1], c.tau[b:b + 1], c.f[b:b + 1]))
        assert np.array_equal(row[0], whole[b]), b


# ---- 6. step --------------------------------------------------------------------------------------------------------------------
def test_one_substep_is_semi_implicit_euler_of_the_reference(quad):
    c, B, dt = quad[0.3], 33, 1e-3
    q, v, a = host(*c.L.step(c.q[:B], c.v[:B], dt, 1, tau_ff=c.tau[:B], f=c.f[:B], kp=0.0, kd=0.0))
    v_ref = c.v[:B] + dt * c.a[:B]
    q_ref = c.q[:B] + dt * v_ref
    print(f"one substep: a {fr.rel_err(a, c.a[:B]):.2e} v {fr.rel_err(v, v_ref):.2e} q {fr.rel_err(q, q_ref):.2e}")
    assert fr.rel_err(a, c.a[:B]) < BAR and fr.rel_err(v, v_ref) < BAR and fr.rel_err(q, q_ref) < BAR


def test_free_fall_over_twenty_substeps(quad):
    m, L = quad[0.0].m, quad[0.0].L
    q0, _ = fr.standing(m)
    K, dt = 20, 1e-3
    q, v, a = host(*L.step(q0[None], np.zeros((1, 18), np.float32), dt, K, kp=0.0, kd=0.0))
    vz, z = -fr.G * K * dt, q0[2] - fr.G * dt * dt * K * (K + 1) / 2
    print(f"free fall, {K} substeps: v_z {abs(v[0, 2] - vz) / abs(vz):.2e} z {abs(q[0, 2] - z) / z:.2e} joints {np.abs(q[0, 6:] - q0[6:]).max():.2e}")
    assert abs(v[0, 2] - vz) < BAR * abs(vz) and abs(q[0, 2] - z) < BAR * z
    assert np.abs(q[0, 6:] - np.float32(q0[6:])).max() < 1e-6


def test_pd_hold_without_gravity_returns_the_state_unchanged(quad):
    c, B = quad[0.3], 33
    q0 = c.q[:B]
    q, v, a = host(*layer(c.m, gravity=ZERO3).step(q0, np.zeros((B, 18), np.float32), 1e-3, 5, q_des=q0[:, 6:], kp=20.0, kd=1.5))
    assert np.array_equal(q, q0) and np.array_equal(v, np.zeros_like(v)) and np.array_equal(a, np.zeros_like(a))


@pytest.fixture(scope="module")
def pd_run(quad):
    """Eight substeps of 1 ms under the PD law with the feet carrying the weight: inputs, the fp64 loop over fd_ref and the
    deviation from it of the same loop over the float32 recursion."""
    m, B, K, dt, kp, kd = quad[0.0].m, 8, 8, 1e-3, 20.0, 1.5
    rng = np.random.default_rng(21)
    q = np.tile(fr.standing(m)[0], (B, 1)) + np.concatenate([np.zeros((B, 6)), rng.uniform(-0.2, 0.2, (B, 12))], axis=1)
    v = rng.uniform(-0.5, 0.5, (B, 18))
    q_des = q[:, 6:] + rng.uniform(-0.1, 0.1, (B, 12))
    f = np.tile([0.0, 0.0, m.mass.sum() * fr.G / 4], (B, 4, 1))
    q, v, q_des, f = (x.astype(np.float32) for x in (q, v, q_des, f))
    ref = [fr.step_ref(m, q[b], v[b], dt, K, None, q_des[b], kp, kd, f[b]) for b in range(B)]
    f32 = [fr.step_ref(m, q[b], v[b], dt, K, None, q_des[b], kp, kd, f[b], fd=fr.aba, dtype=np.float32) for b in range(B)]
    q_ref, v_ref = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    dev_q = np.abs(np.stack([r[0] for r in f32]) - q_ref).max()
    dev_v = np.abs(np.stack([r[1] for r in f32]) - v_ref).max()
    return dict(q=q, v=v, q_des=q_des, f=f, K=K, dt=dt, kp=kp, kd=kd, q_ref=q_ref, v_ref=v_ref, dev_q=dev_q, dev_v=dev_v)


def test_eight_substeps_under_the_pd_law(quad, pd_run):
    r = pd_run
    q, v, _ = host(*quad[0.0].L.step(r["q"], r["v"], r["dt"], r["K"], q_des=r["q_des"], kp=r["kp"], kd=r["kd"], f=r["f"]))
    bar_v = max(BAR * np.abs(r["v_ref"]).max(), 4 * r["dev_v"])
    bar_q = max(BAR * np.abs(r["q_ref"]).max(), 4 * r["dev_q"])
    err_v, err_q = np.abs(v - r["v_ref"]).max(), np.abs(q - r["q_ref"]).max()
    print(f"eight PD substeps: v {err_v:.2e} (bar {bar_v:.2e}, float32 loop {r['dev_v']:.2e}) q {err_q:.2e} (bar {bar_q:.2e}, float32 loop {r['dev_q']:.2e})")
    assert err_v < bar_v and err_q < bar_q


def test_outputs_may_alias_the_inputs(quad, pd_run):
    from iterative_learning_nmpc_amd import _lib
    r, L = pd_run, quad[0.0].L
    apart = L.step(r["q"], r["v"], r["dt"], r["K"], q_des=r["q_des"], kp=r["kp"], kd=r["kd"], f=r["f"])
    q, v, q_des, f = (torch.as_tensor(r[k], device=L.device).contiguous() for k in ("q", "v", "q_des", "f"))
    a = torch.empty_like(q)
    ptr = _lib.ptr
    _lib.check(L.lib.nmpc_fd_step_batch(L._h, q.shape[0], r["K"], r["dt"], ptr(q), ptr(v), None, ptr(q_des), r["kp"], r["kd"], ptr(f),
                                        ptr(q), ptr(v), ptr(a), _lib.stream(L.device)), L._h, "nmpc_fd_step_batch", "torque")
    assert all(torch.equal(x, y) for x, y in zip((q, v, a), apart))


def test_twenty_substeps_are_twenty_calls_of_one(quad, pd_run):
    r, L = pd_run, quad[0.0].L
    kw = dict(q_des=r["q_des"], kp=r["kp"], kd=r["kd"], f=r["f"])
    once = L.step(r["q"], r["v"], r["dt"], 20, **kw)
    q, v, a = r["q"], r["v"], None
    for _ in range(20):
        q, v, a = L.step(q, v, r["dt"], 1, **kw)
    assert all(torch.equal(x, y) for x, y in zip((q, v, a), once))


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_batch(quad):
    from iterative_learning_nmpc_amd._lib import NmpcError
    c = quad[0.0]
    q, v = c.q[:2], c.v[:2]
    with pytest.raises(NmpcError, match="n_sub must be at least 1"):
        c.L.step(q, v, 1e-3, 0)
    with pytest.raises(NmpcError, match="dt must be positive"):
        c.L.step(q, v, 0.0, 1)
    with pytest.raises(ValueError, match="expected"):
        c.L.forward_dynamics(q[:, :17], v)
    with pytest.raises(ValueError, match="expected"):
        c.L.step(q, v, 1e-3, q_des=np.zeros((2, 18), np.float32))
    with pytest.raises(ValueError, match="batch sizes"):
        c.L.forward_dynamics(q, v, c.tau[:3])
    assert c.L.forward_dynamics(q[:0], v[:0]).shape == (0, 18)
    assert [tuple(x.shape) for x in c.L.step(q[:0], v[:0], 1e-3, 3)] == [(0, 18)] * 3


def test_massless_leaf_gives_nan_rows_and_the_next_call_is_sound(quad):
    import copy
    c, B = quad[0.0], 33
    bad = copy.deepcopy(c.m)
    bad.mass[17] = 0.0; bad.inertia[17] = 0.0
    Lb = layer(bad)
    a, = host(Lb.forward_dynamics(c.q[:B], c.v[:B], c.tau[:B], c.f[:B]))
    assert a.shape == (B, 18) and np.isnan(a).all()
    assert all(np.isnan(x).all() for x in host(*Lb.step(c.q[:B], c.v[:B], 1e-3, 2)))
    a, = host(c.L.forward_dynamics(c.q[:B], c.v[:B], c.tau[:B], c.f[:B]))
    assert fr.rel_err(a, c.a[:B]) < BAR
