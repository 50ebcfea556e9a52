"""GPU checks of the push in nmpc_policy_rollout_batch and learning.evaluate_policy: the pushed rollout is held bit for bit to
the chain observe -> policy.forward -> pushed contact step with the window moved by n_sub per control step (the pushed step
itself is held to the fp64 reference in tests/test_gpu_push_step.py).  B = 1 and 33, K = 6 control steps of 2 substeps, the
window [3, 8): it starts inside control step 1 and ends after control step 3."""
import numpy as np
import pytest

from tests import fd_reference as fr
from tests.solve_helpers import policy_pair
from tests.torque_helpers import Case, ground, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KP, KD, DT = 20.0, 1.5, 5e-4
DT32 = float(np.float32(DT))
K, N_SUB, FIRST, COUNT = 6, 2, 3, 5
PERIOD, T0, HEIGHT, MASK = 0.5, 0.37, 0.08, 2 | 4 | 8 | 32


class World:
    B = 33

    def __init__(self):
        self.c = c = Case(fr.quadruped(perturb=0.3), self.B, seed=258)
        self.L, self.g = c.L, c.g
        rng = np.random.default_rng(21)
        dev = lambda x: torch.as_tensor(np.asarray(x, np.float32), device=self.L.device)      # noqa: E731
        self.q, self.v, self.tau = dev(c.q), dev(c.v), dev(0.1 * c.tau)
        self.goal = dev(rng.uniform(-0.5, 0.5, (self.B, 3)))
        self.F = dev(rng.uniform(-80, 80, (self.B, 3)))
        self.s_mean, self.s_std = rng.uniform(-0.5, 0.5, 44), rng.uniform(0.5, 2.0, 44)
        self.policy = policy_pair(47, 12, 2, 64, True, 64, seed=5)[0]

    def chain(self, B, pushed=True):
        """the Python loop of the three public calls -> (q, v, S, A, failed, Q, V)"""
        L = self.L
        q, v, goal, tau = self.q[:B], self.v[:B], self.goal[:B], self.tau[:B]
        failed = torch.zeros(B, dtype=torch.int32, device=L.device)
        kw = dict(s_mean=self.s_mean, s_std=self.s_std, collision_height=HEIGHT, failed=failed, term_mask=MASK)
        S, A, Q, V = [], [], [], []
        for k in range(K):
            s, x = L.observe(q, v, T0 + (k * N_SUB) * DT32, PERIOD, goal, step_index=k, **kw)
            a = self.policy.forward(x)
            Q.append(q); V.append(v)
            if pushed:
                L.set_push(self.F[:B], FIRST - k * N_SUB, COUNT)
            q, v = L.contact_step(q, v, DT, N_SUB, tau_ff=tau, q_des=a, kp=KP, kd=KD, ground=ground(self.g))[:2]
            S.append(s); A.append(a)
        L.set_push(None)
        L.observe(q, v, T0 + (K * N_SUB) * DT32, PERIOD, goal, step_index=K, **kw)
        return q, v, torch.stack(S, 1), torch.stack(A, 1), failed, torch.stack(Q, 1), torch.stack(V, 1)

    def rollout(self, B, pushed=True):
        L = self.L
        Q, V = (torch.full((B, K, 18), -77.0, device=L.device) for _ in range(2))
        L.set_rollout_states(Q, V)
        if pushed:
            L.set_push(self.F[:B], FIRST, COUNT)
        try:
            out = L.policy_rollout(self.policy, self.q[:B], self.v[:B], K, DT, N_SUB, self.goal[:B], tau_ff=self.tau[:B], kp=KP, kd=KD,
                                   ground=ground(self.g), t0=T0, period=PERIOD, s_mean=self.s_mean, s_std=self.s_std, terminate_mask=MASK,
                                   collision_height=HEIGHT)
        finally:
            L.set_push(None)
            L.set_rollout_states(None)
        return (*out, Q, V)

    def evaluate(self, B, push):
        from iterative_learning_nmpc_amd import learning
        # evaluate_policy normalises with a database or not at all: raw here, as the chain below it is compared with
        return learning.evaluate_policy(self.L, self.policy, None, self.q[:B], self.v[:B], self.goal[:B], K * N_SUB * DT, dt=DT, n_sub=N_SUB,
                                        tau_ff=self.tau[:B], kp=KP, kd=KD, ground=ground(self.g), t0=T0, period=PERIOD, terminate_mask=MASK,
                                        collision_height=HEIGHT, record_states=True, push=push)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("B", [1, 33])
def test_the_pushed_rollout_is_the_chain_bit_for_bit(world, B):
    ref, got, plain = world.chain(B), world.rollout(B), world.rollout(B, pushed=False)
    names = ("q", "v", "S", "A", "failed", "Q", "V")
    for name, a, b in zip(names, got, ref):
        print(f"B = {B}: {name} largest |rollout - chain| {float((a.double() - b.double()).abs().nan_to_num().max()):.3e}")
    assert all(torch.equal(a, b) if a.dtype == torch.int32 else same(a, b) for a, b in zip(got, ref))
    # the first pushed substep is substep 1 of control step 1: rows 0 and 1 are the un-pushed rollout's, the final v is not
    for i in (2, 3, 5, 6):
        assert same(got[i][:, :2], plain[i][:, :2]), names[i]
    assert not same(got[1], plain[1]) and not same(got[6][:, 2], plain[6][:, 2])


@pytest.mark.parametrize("B", [1, 33])
def test_evaluate_policy_pushes_for_the_one_rollout(world, B):
    w, L = world, world.L
    step = lambda: L.contact_step(w.q[:B], w.v[:B], DT, 4, tau_ff=w.tau[:B], kp=KP, kd=KD, ground=ground(w.g))      # noqa: E731
    before = step()
    push = dict(start=FIRST * DT, duration=COUNT * DT, force=w.F[:B].cpu().numpy())
    out = w.evaluate(B, push)
    after = step()
    assert all(same(a, b) for a, b in zip(before, after))                       # nothing is left attached
    assert L._push is None
    # it is the rollout under set_push, here without column statistics
    Q, V = (torch.empty(B, K, 18, device=L.device) for _ in range(2))
    L.set_rollout_states(Q, V)
    L.set_push(w.F[:B], FIRST, COUNT)
    try:
        q, v, S, A, failed = L.policy_rollout(w.policy, w.q[:B], w.v[:B], K, DT, N_SUB, w.goal[:B], tau_ff=w.tau[:B], kp=KP, kd=KD,
                                              ground=ground(w.g), t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)
    finally:
        L.set_push(None)
        L.set_rollout_states(None)
    assert all(same(out[k], x) for k, x in (("q", q), ("v", v), ("S", S), ("A", A), ("Q", Q), ("V", V))) and torch.equal(out["failed"], failed)
    none = w.evaluate(B, None)
    assert not same(out["v"], none["v"])
    # a push of no duration is no push
    zero = w.evaluate(B, dict(push, duration=0.0))
    assert all(same(zero[k], none[k]) for k in ("q", "v", "S", "A", "Q", "V")) and torch.equal(zero["failed"], none["failed"])


def test_a_rollout_of_more_robots_than_the_push_has_rows_is_refused_before_any_launch(world):
    import ctypes

    from iterative_learning_nmpc_amd import _lib
    w, L, B = world, world.L, 8
    q, v = w.q[:B].clone(), w.v[:B].clone()
    S, A = torch.full((B, K, 44), -77.0, device=L.device), torch.full((B, K, 12), -77.0, device=L.device)
    X = torch.full((B, 47), -77.0, device=L.device)
    failed = torch.zeros(B, dtype=torch.int32, device=L.device)
    cfg = _lib.NmpcPolicyRolloutCfg(K, N_SUB, DT, KP, KD, T0, PERIOD, HEIGHT, MASK, 3, 1)
    g, ptr = ground(w.g).cfg(), _lib.ptr
    L.set_push(w.F[:4], FIRST, COUNT)
    try:
        rc = L.lib.nmpc_policy_rollout_batch(L._h, w.policy._h, B, ctypes.byref(cfg), ctypes.byref(g), ptr(q), ptr(v), ptr(w.tau[:B].contiguous()),
                                             ptr(w.goal[:B].contiguous()), None, None, ptr(S), ptr(A), ptr(X), ptr(failed), _lib.stream(L.device))
        assert rc == -1 and "B exceeds force_rows" in L.lib.nmpc_torque_last_error(L._h).decode()
        torch.cuda.synchronize()
        assert same(q, w.q[:B]) and same(v, w.v[:B]) and not bool(failed.any())
        assert all(bool((x == -77.0).all()) for x in (S, A, X))
        # four robots fit the four rows
        assert L.lib.nmpc_policy_rollout_batch(L._h, w.policy._h, 4, ctypes.byref(cfg), ctypes.byref(g), ptr(q), ptr(v), ptr(w.tau[:4].contiguous()),
                                               ptr(w.goal[:4].contiguous()), None, None, ptr(S), ptr(A), ptr(X), ptr(failed), _lib.stream(L.device)) == 0
    finally:
        L.set_push(None)
