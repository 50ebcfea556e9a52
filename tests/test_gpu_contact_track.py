"""GPU checks of nmpc_contact_track_batch and nmpc_observe_rows_batch: each is held bit for bit to the chain of public calls it
replaces (nmpc_contact_step_batch per control step, nmpc_observe_batch per row), so the reference of every comparison is the
project's own, separately tested, single-step call and the bar is array equality of the bit patterns (NaN rows included).

The world is the standing world of tests/test_gpu_policy_rollout.py, built again here: the tilted quadruped with 257 states
whose lowest foot is at -3 mm / 0 / +2 cm in turn, a small feed-forward torque, and PD targets within 0.05 rad of STAND."""
import copy
import ctypes

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr
from tests.torque_helpers import ground, layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KP, KD, DT = 20.0, 1.5, 5e-4
N_STEPS, N_SUB, A_ROWS, QV_ROWS = 3, 2, 5, 4          # the tables are longer than the steps taken: strides differ from counts
PERIOD, T0, DT_ROW, HEIGHT = 0.5, 0.37, 1e-3, 0.08
COLLISION, JOINT_LIMIT, TERM_SHIFT = 32, 64, 8
KEPT = 16                                              # the velocity-tracking bit: no observation raises it
SENTINEL = -77.0


class World:
    B = 257

    def __init__(self):
        self.m = m = fr.quadruped(perturb=0.3)
        self.L = layer(m)
        B = self.B
        q, v, tau, _ = fr.inputs(m, B, 258)
        lowest = lambda: np.array([cr.feet(m, q[b])[0][:, 2].min() for b in range(B)])      # noqa: E731
        want = np.array([-0.003, 0.0, 0.02])[np.arange(B) % 3]
        lift = (m.forward_kinematics(q[0])[0][2] @ m.axis[2])[2]                              # world z per unit of q[2]
        assert m.jtype[2] == 1 and lift > 0.5
        q[:, 2] += ((want - lowest()) / lift).astype(np.float32)
        assert np.abs(lowest() - want).max() < 1e-6
        rng = np.random.default_rng(11)
        self.q, self.v = q.astype(np.float32), v.astype(np.float32)
        self.tau = (0.1 * tau).astype(np.float32)
        self.A = (fr.STAND[None, None, :] + rng.uniform(-0.05, 0.05, (B, A_ROWS, 12))).astype(np.float32)
        for x in (self.q, self.v, self.tau, self.A):
            x.setflags(write=False)

    def dev(self, x, dtype=torch.float32):
        return torch.as_tensor(np.array(x), dtype=dtype, device=self.L.device)

    def chain(self, rows, tau=True, tau_max=None, L=None):
        """n_steps public contact steps -> (q, v, Q, V, tau_out of every step)"""
        L = L or self.L
        q, v, A = self.dev(self.q[rows]), self.dev(self.v[rows]), self.dev(self.A[rows])
        tau_ff = self.dev(self.tau[rows]) if tau else None
        Q, V, T = [], [], []
        for k in range(N_STEPS):
            Q.append(q); V.append(v)
            q, v, _, _, t = L.contact_step(q, v, DT, N_SUB, tau_ff=tau_ff, q_des=A[:, k].contiguous(), kp=KP, kd=KD, ground=ground(tau_max=tau_max))
            T.append(t)
        return q, v, torch.stack(Q, 1), torch.stack(V, 1), torch.stack(T, 1)

    def track(self, rows, tau=True, tau_max=None, L=None, skip=None, skip_mask=0, fill=None):
        """one nmpc_contact_track_batch on tables of A_ROWS / QV_ROWS rows -> (q, v, Q, V, the whole Q, V tables)"""
        L = L or self.L
        q, v, A = self.dev(self.q[rows]), self.dev(self.v[rows]), self.dev(self.A[rows])
        B = q.shape[0]
        Qt, Vt = (torch.full((B, QV_ROWS, 18), SENTINEL if fill is None else fill, dtype=torch.float32, device=L.device) for _ in range(2))
        tau_ff = self.dev(self.tau[rows]) if tau else None
        q2, v2, Q, V = L.contact_track(q, v, A[:, :N_STEPS], DT, N_SUB, tau_ff=tau_ff, kp=KP, kd=KD, ground=ground(tau_max=tau_max),
                                       Q=Qt[:, :N_STEPS], V=Vt[:, :N_STEPS], skip=skip, skip_mask=skip_mask)
        assert q2.data_ptr() == q.data_ptr() and v2.data_ptr() == v.data_ptr()        # in place on q, v
        return q, v, Q, V, Qt, Vt


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def chain33(world):
    """the chain of B = 33 with the feed-forward torque, shared by the tests that compare with it"""
    return world.chain(slice(0, 33))


# ---- 1. the track is the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [True, False])
@pytest.mark.parametrize("B", [1, 33, 257])
def test_track_equals_the_chain_bit_for_bit(world, B, tau):
    r = slice(0, B)
    ref = world.chain(r, tau=tau)
    q, v, Q, V, Qt, Vt = world.track(r, tau=tau)
    diff = [float((a - b).abs().max()) for a, b in zip((q, v, Q, V), ref[:4])]
    print(f"B = {B}, tau_ff {tau}: largest |track - chain| of q, v, Q, V: {diff}")
    assert all(same(a, b) for a, b in zip((q, v, Q, V), ref[:4]))
    assert same(Q[:, 0], world.dev(world.q[r])) and same(V[:, 0], world.dev(world.v[r]))
    assert not same(q, world.dev(world.q[r]))                                          # the plant has moved
    assert bool((Qt[:, N_STEPS:] == SENTINEL).all()) and bool((Vt[:, N_STEPS:] == SENTINEL).all())    # rows past n_steps are not written


def test_track_equals_the_chain_under_a_torque_limit_that_clamps(world):
    r, lim = slice(0, 33), 5.0
    free, ref = world.chain(r)[4], world.chain(r, tau_max=lim)
    clamped = int((free.abs() > lim).sum())
    print(f"torque limit {lim}: {clamped} of {free.numel()} unclamped last-substep torques beyond it; largest clamped |tau| {float(ref[4].abs().max())}")
    assert clamped > 0 and float(ref[4].abs().max()) == lim and bool((ref[4].abs() == lim).any())
    got = world.track(r, tau_max=lim)
    assert all(same(a, b) for a, b in zip(got[:4], ref[:4]))
    assert not same(got[0], world.chain(r)[0])                                         # and the limit matters


# ---- 2. skip, independence ----------------------------------------------------------------------------------------------------------
def test_skipped_robots_are_untouched_and_the_others_unchanged(world, chain33):
    B, r = 33, slice(0, 33)
    skip = torch.zeros(B, dtype=torch.int32, device=world.L.device)
    skip[::3] = 4 | 1
    skip[1::3] = 1                                                                     # a bit outside the mask does not skip
    q, v, Q, V, Qt, Vt = world.track(r, skip=skip, skip_mask=4)
    out, kept = torch.arange(B, device=q.device) % 3 == 0, torch.arange(B, device=q.device) % 3 != 0
    assert same(q[out], world.dev(world.q[r])[out]) and same(v[out], world.dev(world.v[r])[out])
    assert bool((Qt[out] == SENTINEL).all()) and bool((Vt[out] == SENTINEL).all())
    assert all(same(a[kept], b[kept]) for a, b in zip((q, v, Q, V), chain33[:4]))
    # a mask of zero skips nobody
    assert all(same(a, b) for a, b in zip(world.track(r, skip=skip, skip_mask=0)[:4], chain33[:4]))


def test_a_robot_does_not_depend_on_its_batch(world, chain33):
    alone = world.track(slice(5, 6))
    full = world.track(slice(0, 33))
    assert all(same(a, b[5:6]) for a, b in zip(alone[:4], full[:4]))
    assert all(same(a, b[5:6]) for a, b in zip(alone[:4], chain33[:4]))


# ---- 3. the rows of a table of states -------------------------------------------------------------------------------------------------
def test_rows_equal_the_calls(world, chain33):
    L, B = world.L, 33
    Qt, Vt = (torch.full((B, QV_ROWS, 18), SENTINEL, dtype=torch.float32, device=L.device) for _ in range(2))
    Qt[:, :N_STEPS], Vt[:, :N_STEPS] = chain33[2], chain33[3]
    Qt[:, :N_STEPS, 6:] = world.dev(fr.STAND)                                          # joints inside their limits (the world's are random),
    Qt[:2, :N_STEPS, 2] = 0.3                                                          # the first two robots well above the ground
    Qt[0, 1, 2] = 0.05                                                                 # robot 0 lies on the ground in row 1 only
    Qt[1, 2, 6] = 2.0                                                                  # robot 1: a hip at 115 degrees in row 2 only
    Q, V = Qt[:, :N_STEPS], Vt[:, :N_STEPS]
    goal = torch.zeros(B, 0, dtype=torch.float32, device=L.device)
    for mask in (0, COLLISION):
        start = torch.zeros(B, dtype=torch.int32, device=L.device)
        start[7] = KEPT                                                                # flags the robot came with are kept
        ref_failed, per_row, ref_S = start.clone(), [], []
        for k in range(N_STEPS):
            s, _ = L.observe(Q[:, k].contiguous(), V[:, k].contiguous(), T0 + k * DT_ROW, PERIOD, goal, collision_height=HEIGHT, failed=ref_failed,
                             step_index=4, term_mask=mask)
            own = torch.zeros(B, dtype=torch.int32, device=L.device)
            L.observe(Q[:, k].contiguous(), V[:, k].contiguous(), T0 + k * DT_ROW, PERIOD, goal, collision_height=HEIGHT, failed=own)
            ref_S.append(s); per_row.append(own)
        ref_S, per_row = torch.stack(ref_S, 1), torch.stack(per_row, 1).cpu().numpy()
        # the table is what it is meant to be
        assert [bool(x & COLLISION) for x in per_row[0]] == [False, True, False] and not (per_row[1] & COLLISION).any()
        assert [bool(x & JOINT_LIMIT) for x in per_row[1]] == [False, False, True]
        St = torch.full((B, A_ROWS, 44), SENTINEL, dtype=torch.float32, device=L.device)
        failed = start.clone()
        S = L.observe_rows(Q, V, T0, DT_ROW, PERIOD, collision_height=HEIGHT, S=St[:, :N_STEPS], failed=failed, step_index=4, term_mask=mask)
        print(f"term_mask {mask}: failed[:3] = {failed[:3].tolist()}, largest |S - calls| = {float((S - ref_S).abs().max())}")
        assert same(S, ref_S) and torch.equal(failed, ref_failed)
        assert bool((St[:, N_STEPS:] == SENTINEL).all())
        f = failed.cpu().numpy()
        assert f[0] & COLLISION and f[1] & JOINT_LIMIT and f[7] & KEPT
        assert (f[0] >> TERM_SHIFT) == (5 if mask else 0) and (f[1] >> TERM_SHIFT) == 0
    # skipped robots: rows and flags untouched, the others as before
    skip = torch.zeros(B, dtype=torch.int32, device=L.device)
    skip[::3] = COLLISION
    St2 = torch.full((B, A_ROWS, 44), SENTINEL, dtype=torch.float32, device=L.device)
    failed2 = skip.clone()
    L.observe_rows(Q, V, T0, DT_ROW, PERIOD, collision_height=HEIGHT, S=St2[:, :N_STEPS], failed=failed2, step_index=4, term_mask=COLLISION,
                   skip=skip, skip_mask=COLLISION)
    out = torch.arange(B, device=L.device) % 3 == 0
    assert bool((St2[out] == SENTINEL).all()) and torch.equal(failed2[out], skip[out])
    expected = ref_failed.clone()
    expected[7] -= KEPT                                                                # this run starts from clean flags
    assert same(St2[~out][:, :N_STEPS], ref_S[~out]) and torch.equal(failed2[~out], expected[~out])
    # flags alone: no rows asked for
    only = torch.zeros(B, dtype=torch.int32, device=L.device)
    from iterative_learning_nmpc_amd import _lib
    assert L.lib.nmpc_observe_rows_batch(L._h, B, N_STEPS, _lib.ptr(Qt), _lib.ptr(Vt), QV_ROWS, T0, DT_ROW, PERIOD, HEIGHT, None, 0, _lib.ptr(only), 4,
                                         COLLISION, None, 0, _lib.stream(L.device)) == 0
    start = torch.zeros(B, dtype=torch.int32, device=L.device); start[7] = KEPT
    assert torch.equal(only | start, ref_failed)


def test_one_row_equals_the_call(world, chain33):
    """n_rows = 1 is nmpc_observe_batch of the same state, in S and in failed: one robot skipped, one that comes with a stamp"""
    L, B = world.L, 33
    Q, V = chain33[2][:, 1:2].clone(), chain33[3][:, 1:2].clone()
    Q[:, 0, 6:] = world.dev(fr.STAND)
    Q[:, 0, 2] = 0.3
    Q[::4, 0, 2] = 0.05                                                                # every fourth robot lies on the ground
    Q[2, 0, 6] = 2.0                                                                   # robot 2: a hip beyond its limit
    goal = torch.zeros(B, 0, dtype=torch.float32, device=L.device)
    start = torch.zeros(B, dtype=torch.int32, device=L.device)
    start[4] = (3 << TERM_SHIFT) | COLLISION                                           # stamped by an earlier step: the stamp stays
    start[7] = KEPT
    ref_failed = start.clone()
    ref_S, _ = L.observe(Q[:, 0].contiguous(), V[:, 0].contiguous(), T0, PERIOD, goal, collision_height=HEIGHT, failed=ref_failed, step_index=6,
                         term_mask=COLLISION)
    skip = torch.zeros(B, dtype=torch.int32, device=L.device)
    skip[8] = 1
    St = torch.full((B, 1, 44), SENTINEL, dtype=torch.float32, device=L.device)
    failed = start.clone()
    S = L.observe_rows(Q, V, T0, DT_ROW, PERIOD, collision_height=HEIGHT, S=St, failed=failed, step_index=6, term_mask=COLLISION, skip=skip,
                       skip_mask=1)
    kept = torch.arange(B, device=L.device) != 8
    print(f"largest |S - call| = {float((S[kept, 0] - ref_S[kept]).abs().max())}, failed[:9] = {failed[:9].tolist()}")
    assert same(S[kept, 0], ref_S[kept]) and torch.equal(failed[kept], ref_failed[kept])
    assert bool((St[8] == SENTINEL).all()) and int(failed[8]) == 0 and int(ref_failed[8]) != 0
    f = failed.cpu().numpy()
    assert (f[0] >> TERM_SHIFT) == 7 and (f[4] >> TERM_SHIFT) == 3 and f[2] & JOINT_LIMIT and (f[2] >> TERM_SHIFT) == 0 and f[7] & KEPT


# ---- 4. NaN containment -------------------------------------------------------------------------------------------------------------
def test_massless_leaf_gives_nan_rows_where_the_chain_has_them_and_the_next_call_is_sound(world, chain33):
    r = slice(0, 33)
    bad = copy.deepcopy(world.m)
    bad.mass[17] = 0.0; bad.inertia[17] = 0.0
    Lb = layer(bad)
    ref = world.chain(r, L=Lb)
    got = world.track(r, L=Lb)
    assert same(ref[2][:, 0], world.dev(world.q[r])) and bool(torch.isnan(ref[2][:, 1:]).all()) and bool(torch.isnan(ref[0]).all())
    nan_like = [torch.equal(torch.isnan(a), torch.isnan(b)) for a, b in zip(got[:4], ref[:4])]
    print(f"NaN rows where the chain has them: {nan_like}; bit for bit: {[same(a, b) for a, b in zip(got[:4], ref[:4])]}")
    assert all(nan_like)
    assert all(same(a, b) for a, b in zip(got[:4], ref[:4]))
    # the next call on a sound handle is sound
    assert all(same(a, b) for a, b in zip(world.track(r)[:4], chain33[:4]))


# ---- 5. errors, the empty batch -----------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_batch(world):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import NmpcError
    from iterative_learning_nmpc_amd.torque import GroundContact
    L, B = world.L, 2
    ptr, st = _lib.ptr, _lib.stream(L.device)
    q, v, A = world.dev(world.q[:B]), world.dev(world.v[:B]), world.dev(world.A[:B])
    Q, V = (torch.full((B, QV_ROWS, 18), SENTINEL, dtype=torch.float32, device=L.device) for _ in range(2))
    S = torch.full((B, QV_ROWS, 44), SENTINEL, dtype=torch.float32, device=L.device)
    q0 = q.clone()
    good = GroundContact().cfg()

    def track(n_steps=N_STEPS, n_sub=N_SUB, dt=DT, cfg=good, q=q, v=v, A=A, a_rows=A_ROWS, Q=Q, V=V, qv_rows=QV_ROWS, h=L):
        return h.lib.nmpc_contact_track_batch(h._h, B, n_steps, n_sub, dt, ctypes.byref(cfg) if cfg is not None else None, ptr(q), ptr(v), None, ptr(A),
                                              a_rows, KP, KD, ptr(Q), ptr(V), qv_rows, None, 0, st)

    def rows(n_rows=N_STEPS, Q=Q, V=V, qv_rows=QV_ROWS, period=PERIOD, S=S, s_rows=QV_ROWS, h=L):
        return h.lib.nmpc_observe_rows_batch(h._h, B, n_rows, ptr(Q), ptr(V), qv_rows, T0, DT_ROW, period, HEIGHT, ptr(S), s_rows, None, 0, 0, None, 0, st)

    def refused(rc, text, h=L):
        return rc == -1 and text in h.lib.nmpc_torque_last_error(h._h).decode()

    assert refused(track(n_steps=0), "n_steps must be at least 1")
    assert refused(track(n_sub=0), "n_sub must be at least 1")
    assert refused(track(dt=0.0), "dt must be positive")
    assert refused(track(cfg=None), "cfg is NULL")
    assert refused(track(cfg=GroundContact(slip_velocity=0.0).cfg()), "slip_velocity must be positive")
    assert refused(track(cfg=GroundContact(stiffness=float("inf")).cfg()), "must be finite")
    assert refused(track(q=None), "need B >= 0 and q, v") and refused(track(v=None), "need B >= 0 and q, v")
    assert refused(track(A=None), "A is NULL")
    assert refused(track(a_rows=N_STEPS - 1), "a_rows must be at least n_steps")
    assert refused(track(Q=None), "Q and V come together") and refused(track(V=None), "Q and V come together")
    assert refused(track(qv_rows=N_STEPS - 1), "qv_rows must be at least n_steps")
    small = fr.random_tree()                                                           # 23 joints: no rows of 18
    Ls = layer(small)
    assert refused(track(h=Ls), "whole-body tree", Ls)
    assert refused(rows(h=Ls), "whole-body tree", Ls)
    assert refused(rows(n_rows=0), "n_rows must be at least 1")
    assert refused(rows(Q=None), "need B >= 0 and q, v") and refused(rows(V=None), "need B >= 0 and q, v")
    assert refused(rows(qv_rows=N_STEPS - 1), "qv_rows must be at least n_rows")
    assert refused(rows(s_rows=N_STEPS - 1), "s_rows must be at least n_rows")
    assert refused(rows(period=0.0), "period must be positive")
    # nothing was launched by a refused call
    assert same(q, q0) and bool((Q == SENTINEL).all()) and bool((S == SENTINEL).all())
    # the layer's own checks
    with pytest.raises(ValueError, match="in place"):
        L.contact_track(world.q[:B], v, A[:, :N_STEPS], DT)
    with pytest.raises(ValueError, match="come together"):
        L.contact_track(q, v, A[:, :N_STEPS], DT, Q=Q[:, :N_STEPS])
    with pytest.raises(NmpcError, match="n_steps must be at least 1"):
        L.contact_track(q, v, A[:, :0], DT)
    # B = 0 is a no-op
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=L.device)             # noqa: E731
    out = L.contact_track(e(0, 18), e(0, 18), e(0, N_STEPS, 12), DT, N_SUB)
    assert [tuple(x.shape) for x in out] == [(0, 18), (0, 18), (0, N_STEPS, 18), (0, N_STEPS, 18)]
    assert L.observe_rows(e(0, N_STEPS, 18), e(0, N_STEPS, 18), T0, DT_ROW).shape == (0, N_STEPS, 44)
