"""GPU checks of the observation and action history on the policy input (nmpc_history_push_batch, nmpc_history_push_actions_batch,
nmpc_policy_rollout_set_history behind `BatchedTorqueLayer.set_history`, `history_push`, `history_push_actions`, `set_rollout_wide`,
`history_table`; `learning.evaluate_policy(history=...)`, `learning.dagger_iteration(history=...)`).

Every word of a wide row and of the registers is a copy, and the policy input is the database's fp64 expression rounded once, so
every comparison is equality of the bit patterns: the kernels against the numpy restatement (tests/history_reference.py), the rollout
against the chain of the public calls, and the rollout at (n_obs, n_act) = (1, 0) against the rollout with nothing attached.

Shapes: the quadruped tree.  The push runs 256 threads per block over B x (44 + 12 + 3) (robot, column) pairs: B = 3 (177 pairs, one
block that is not full) and B = 7 (413 pairs, a second block that starts inside robot 4); depths (1, 0), (3, 2) and the deepest
(16, 16); rollouts of 4 control steps of 2 substeps with a policy of one hidden layer of 16."""
import ctypes

import numpy as np
import pytest

from tests import fd_reference as fr
from tests import history_reference as hr
from tests import plant_helpers as ph
from tests.plant_helpers import DT, HEIGHT, KD, KP, MASK, N_SUB, PERIOD, T0
from tests.plant_helpers import error_text, start_states
from tests.solve_helpers import dev, policy_pair  # noqa: F401
from tests.torque_helpers import same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, K, NU, NS, NG = 7, 4, 12, 44, 3
SIZES = (3, 7)
DEPTHS = ((1, 0), (3, 2), (16, 16))
DT32 = float(np.float32(DT))
SENTINEL = -77.0
SEED, STEP0 = 0x9E3779B97F4A7C15, 70000


class Fixture(ph.Fixture):
    def __init__(self):
        self.m = m = fr.quadruped()
        rng = np.random.default_rng(89)
        self.q, self.v = start_states(m, B, rng)
        self.tau = rng.uniform(-2, 2, (B, NU)).astype(np.float32)
        self.goal = rng.uniform(-0.5, 0.5, (B, NG)).astype(np.float32)
        wide = hr.width(16, 16)
        self.s_mean, self.s_std = rng.normal(0.0, 0.1, wide), rng.uniform(0.5, 2.0, wide)
        self.S0 = rng.normal(0.0, 1.5, (B, NS)).astype(np.float32)      # a fill that no row of a rollout equals
        sigma, bias = rng.uniform(0.0, 0.2, (B, NS)), rng.uniform(-0.05, 0.05, (B, NS))
        sigma[:, [0, 5, 30]], bias[:, [0, 5, 30]] = 0.0, 0.0
        self.noise = np.concatenate([sigma, bias], axis=1).astype(np.float32)
        self.delays = np.array([0, 1, 2, 1, 0, 2, 1], np.int32)
        self.freeze()

    def stats(self, depths, on=True):
        n_wide = hr.width(*depths)
        return (self.s_mean[:n_wide], self.s_std[:n_wide]) if on else (None, None)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(scope="module")
def world(fx):
    return ph.World(fx.m, B, q=fx.q, v=fx.v, tau=fx.tau, goal=fx.goal)


@pytest.fixture(scope="module")
def policies(dev):
    """one policy per depth, of n_wide + 3 inputs; (1, 0) is the memoryless policy of 47 inputs"""
    return {d: policy_pair(hr.width(*d) + NG, 12, 1, 16, True, 8, seed=5)[0] for d in DEPTHS}


@pytest.fixture()
def clean(world):
    """whatever a test attaches is gone after it, the history included"""
    yield
    world.L.set_history(None)
    ph.detach(world.L)


def rollout(w, policy, n, s_mean=None, s_std=None, n_steps=K, q=None, v=None, t0=T0):
    return w.L.policy_rollout(policy, w.q[:n] if q is None else q, w.v[:n] if v is None else v, n_steps, DT, N_SUB, w.goal[:n], tau_ff=w.tau[:n],
                              kp=KP, kd=KD, t0=t0, period=PERIOD, s_mean=s_mean, s_std=s_std, terminate_mask=MASK, collision_height=HEIGHT)


def rollouts_equal(a, b):
    return all(same(x, y) for x, y in zip(a[:4], b[:4])) and torch.equal(a[4], b[4])


def setup(w, fx, n, depths, noise=False, delays=False, wide_rows=K, observed_rows=0):
    """noise, delays and a history of `depths` on the layer, every register reset -> (W, O), the tables the rollout writes (or None)"""
    L = w.L
    L.set_history(None)
    ph.detach(L)
    if noise:
        L.set_noise(w.d(fx.noise[:n]), seed=SEED, first_robot=2, step0=STEP0)
    if delays:
        L.set_delays(fx.delays[:n], depth=2)
        L.reset_delay_history(w.q[:n])
    L.set_history(*depths, batch=n)
    L.reset_history(w.d(fx.S0[:n]), w.q[:n])
    W = O = None
    if wide_rows:
        W = torch.full((n, wide_rows, hr.width(*depths)), SENTINEL, device=L.device)
        L.set_rollout_wide(W)
    if observed_rows:
        O = torch.full((n, observed_rows, NS), SENTINEL, device=L.device)
        L.set_rollout_observed(O)
    return W, O


def registers(L):
    """copies of what moves with a rollout: both history registers, the delay register, the noise step"""
    return (L.history.clone(), None if L.action_history is None else L.action_history.clone(),
            None if L.delay_history is None else L.delay_history.clone(), L.noise_step)


def registers_equal(a, b):
    return all((x is None and y is None) or same(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def chain(w, policy, n, s_mean, s_std, n_steps=K):
    """the control steps of a rollout with a history as the chain of the public calls -> (q, v, S, A, failed), O, W, X"""
    L = w.L
    q, v, goal, tau = w.q[:n], w.v[:n], w.goal[:n], w.tau[:n]
    narrow = dict(s_mean=None if s_mean is None else s_mean[:NS], s_std=None if s_std is None else s_std[:NS])
    n_wide = L._history.n_wide
    failed = torch.zeros(n, dtype=torch.int32, device=L.device)
    S, A, O, W, X = [], [], [], [], []
    for k in range(n_steps):
        step = L.noise_step
        s, _ = L.observe(q, v, T0 + (k * N_SUB) * DT32, PERIOD, goal, collision_height=HEIGHT, failed=failed, step_index=k, term_mask=MASK, **narrow)
        assert L.noise_step == (None if step is None else step + 1)
        L.observed_rows(s, step or 0, out=L.history[:n, 0])
        Wk = torch.full((n, n_wide), SENTINEL, device=L.device)
        x = L.history_push(goal, s_mean, s_std, 1, W=Wk)
        a = policy.forward(x)
        q, v = L.contact_step(q, v, DT, N_SUB, tau_ff=tau, q_des=a, kp=KP, kd=KD)[:2]
        if L.action_history is not None:
            L.history_push_actions(a)
        S.append(s); A.append(a); O.append(L.history[:n, 0].clone()); W.append(Wk); X.append(x)
    # the last, flags-only observation: `observe` always makes an X and would draw, so the same flags through the rows call
    L.observe_rows(q[:, None], v[:, None], T0 + (n_steps * N_SUB) * DT32, DT32, PERIOD, collision_height=HEIGHT, failed=failed, step_index=n_steps,
                   term_mask=MASK)
    return (q, v, torch.stack(S, 1), torch.stack(A, 1), failed), torch.stack(O, 1), torch.stack(W, 1), torch.stack(X, 1)


# ---- 1. the two kernels against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("depths", DEPTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_pushes_are_the_reference(fx, world, clean, n, depths, stats):
    L, (n_obs, n_act) = world.L, depths
    n_wide = hr.width(*depths)
    rng = np.random.default_rng(n + n_wide)
    hist = rng.normal(0.0, 1.5, (n, n_obs, NS)).astype(np.float32)
    hist[:, :, 5] = -0.0
    act = rng.uniform(-1, 1, (n, n_act, NU)).astype(np.float32)
    s_mean, s_std = fx.stats(depths, stats)
    L.set_history(n_obs, n_act, batch=n + 1)              # more rows than robots is fine; the spare robot's registers stay zero
    assert L.history.shape == (n + 1, n_obs, NS) and (L.action_history is None if n_act == 0 else L.action_history.shape == (n + 1, n_act, NU))
    L.history[:n] = world.d(hist)
    if n_act:
        L.action_history[:n] = world.d(act)
    want_W, want_X = hr.push(hist, act, fx.goal[:n], s_mean, s_std, 1)      # ages `hist` in place
    W = torch.full((n, n_wide + 5), SENTINEL, device=L.device)      # w_stride > n_wide: the padding stays
    X = L.history_push(world.goal[:n], s_mean, s_std, 1, W=W)
    assert X.shape == (n, n_wide + NG) and same(X, world.d(want_X)) and same(W[:, :n_wide].contiguous(), world.d(want_W))
    assert bool((W[:, n_wide:] == SENTINEL).all())
    assert same(L.history[:n], world.d(hist)) and not bool(L.history[n:].any())
    if n_act:
        assert same(L.action_history[:n], world.d(act))   # the push moves no action
        A = rng.uniform(-1, 1, (n, K, NU)).astype(np.float32)
        for k in range(2):                                 # a row of a table is taken with its stride
            hr.push_actions(act, A[:, k])
            L.history_push_actions(world.d(A)[:, k])
            assert same(L.action_history[:n], world.d(act)) and not bool(L.action_history[n:].any())
    # a second push shows the aged rows; without a W the input alone is written
    assert same(L.history_push(world.goal[:n], s_mean, s_std, 1), world.d(hr.push(hist, act, fx.goal[:n], s_mean, s_std, 1)[1]))
    assert same(L.history[:n], world.d(hist))


# ---- 2. the rollout is its chain of public calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("delays", [False, True])
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("depths", DEPTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_rollout_is_its_chain_of_public_calls(fx, world, clean, policies, n, depths, noise, delays):
    L, policy = world.L, policies[depths]
    s_mean, s_std = fx.stats(depths)
    W, O = setup(world, fx, n, depths, noise, delays, wide_rows=K + 2, observed_rows=K)      # w_rows = 6: rows 4 and 5 stay
    got = rollout(world, policy, n, s_mean, s_std)
    after = registers(L)
    assert L.noise_step == (STEP0 + K if noise else None)
    setup(world, fx, n, depths, noise, delays, wide_rows=0)
    want, want_O, want_W, _ = chain(world, policy, n, s_mean, s_std)
    assert rollouts_equal(got, want) and same(O, want_O) and same(W[:, :K].contiguous(), want_W) and bool((W[:, K:] == SENTINEL).all())
    assert registers_equal(after, registers(L))
    # the wide row is the closed form on the rollout's own O and A, the fill where the rollout had not begun
    closed = hr.closed_form(O.cpu().numpy(), got[3].cpu().numpy(), fx.S0[:n], fx.q[:n, 6:], *depths)
    assert same(want_W, world.d(closed))
    assert same(O, got[2]) != noise                        # the sensors show the state exactly without a table of noise
    # S, failed, O, the delay register and the noise step do not depend on the history beyond what the policy was fed: with W and
    # O taken off, the same rollout
    setup(world, fx, n, depths, noise, delays, wide_rows=0)
    assert rollouts_equal(rollout(world, policy, n, s_mean, s_std), got) and registers_equal(after, registers(L))


def raw_rollout(L, policy, w, n, s_mean, s_std, S, A, failed, x_width, n_steps=K):
    """nmpc_policy_rollout_batch as the library has it: S and A may be None -> (rc, q, v)"""
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import ptr, stream
    from iterative_learning_nmpc_amd.torque import GroundContact
    q, v, goal, tau = w.q[:n].clone(), w.v[:n].clone(), w.goal[:n].contiguous(), w.tau[:n].contiguous()
    X = torch.empty(n, x_width, device=L.device)
    mean, std = (None, None) if s_mean is None else (torch.as_tensor(s_mean, device=L.device), torch.as_tensor(s_std, device=L.device))
    cfg = _lib.NmpcPolicyRolloutCfg(n_steps, N_SUB, DT, KP, KD, T0, PERIOD, HEIGHT, MASK, NG, 1)
    g = GroundContact().cfg()
    rc = L.lib.nmpc_policy_rollout_batch(L._h, policy._h, n, ctypes.byref(cfg), ctypes.byref(g), ptr(q), ptr(v), ptr(tau), ptr(goal), ptr(mean),
                                         ptr(std), ptr(S), ptr(A), ptr(X), ptr(failed), stream(L.device))
    torch.cuda.synchronize()
    return rc, q, v


@pytest.mark.parametrize("with_o", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_without_s_and_a_the_rollout_is_the_same(fx, world, clean, policies, n, with_o):
    L, depths = world.L, (3, 2)
    s_mean, s_std = fx.stats(depths)
    W, O = setup(world, fx, n, depths, True, True, observed_rows=K)
    want = rollout(world, policies[depths], n, s_mean, s_std)
    want_W, want_O, after = W.clone(), O.clone(), registers(L)
    W, O = setup(world, fx, n, depths, True, True, observed_rows=K if with_o else 0)
    failed = torch.zeros(n, dtype=torch.int32, device=L.device)
    rc, q, v = raw_rollout(L, policies[depths], world, n, s_mean, s_std, None, None, failed, hr.width(*depths) + NG)
    assert rc == 0 and same(q, want[0]) and same(v, want[1]) and torch.equal(failed, want[4]) and same(W, want_W)
    assert registers_equal(after, registers(L)) and (not with_o or same(O, want_O))


# ---- 3. (1, 0) is the memoryless rollout; attach and detach; two rollouts are the long one --------------------------------------------
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_one_row_and_no_action_is_the_rollout_without_a_history(fx, world, clean, policies, n, stats):
    L, policy = world.L, policies[(1, 0)]
    s_mean, s_std = fx.stats((1, 0), stats)
    bare = rollout(world, policy, n, s_mean, s_std)
    Q, V = (torch.empty(n, K, 18, device=L.device) for _ in range(2))
    L.set_rollout_states(Q, V)
    bare_QV = (rollouts_equal(rollout(world, policy, n, s_mean, s_std), bare), Q.clone(), V.clone())
    W, O = setup(world, fx, n, (1, 0), observed_rows=K)
    L.set_rollout_states(Q, V)
    got = rollout(world, policy, n, s_mean, s_std)
    assert bare_QV[0] and rollouts_equal(got, bare) and same(W, got[2]) and same(O, got[2]) and same(Q, bare_QV[1]) and same(V, bare_QV[2])
    assert same(L.history[:, 0], got[2][:, K - 1]) and L.action_history is None
    # attached then detached: a rollout is the never-attached one, and a 47-input policy is what it takes again
    L.set_history(None)
    L.set_rollout_observed(None); L.set_rollout_states(None)
    assert L.history is None and rollouts_equal(rollout(world, policy, n, s_mean, s_std), bare)


@pytest.mark.parametrize("depths", [(3, 2), (16, 16)])
def test_two_rollouts_are_the_long_rollout(fx, world, clean, policies, depths):
    L, n, policy = world.L, B, policies[depths]
    s_mean, s_std = fx.stats(depths)
    W, _ = setup(world, fx, n, depths, True, True, wide_rows=2 * K)
    long = rollout(world, policy, n, s_mean, s_std, n_steps=2 * K)
    after = registers(L)
    W1, _ = setup(world, fx, n, depths, True, True)
    one = rollout(world, policy, n, s_mean, s_std)
    W2 = torch.full_like(W1, SENTINEL)
    L.set_rollout_wide(W2)
    two = rollout(world, policy, n, s_mean, s_std, q=one[0], v=one[1], t0=T0 + (K * N_SUB) * DT32)
    assert same(two[0], long[0]) and same(two[1], long[1])
    assert same(torch.cat([one[2], two[2]], 1), long[2]) and same(torch.cat([one[3], two[3]], 1), long[3]) and same(torch.cat([W1, W2], 1), W)
    assert torch.equal((one[4] | two[4]) & 0xFF, long[4] & 0xFF)      # the flag bits; the stamps count each call's own steps
    assert registers_equal(after, registers(L))


# ---- 4. refusals leave what was attached in force --------------------------------------------------------------------------------------
def test_refusals_return_their_text_and_leave_the_attachment(fx, world, clean, policies):
    from iterative_learning_nmpc_amd._lib import ptr
    L, n, depths = world.L, 3, (3, 2)
    n_wide = hr.width(*depths)
    s_mean, s_std = fx.stats(depths)
    setup(world, fx, n, depths)
    want = rollout(world, policies[depths], n, s_mean, s_std)
    W, _ = setup(world, fx, n, depths)
    hist, act = L.history, L.action_history
    set_history = L.lib.nmpc_policy_rollout_set_history
    for args, text in (((ptr(hist), 0, ptr(act), 2, None, 0, n), "n_obs must be in [1, NMPC_HISTORY_MAX]"),
                       ((ptr(hist), 17, ptr(act), 2, None, 0, n), "n_obs must be in [1, NMPC_HISTORY_MAX]"),
                       ((ptr(hist), 3, ptr(act), -1, None, 0, n), "n_act must be in [0, NMPC_HISTORY_MAX]"),
                       ((ptr(hist), 3, ptr(act), 17, None, 0, n), "n_act must be in [0, NMPC_HISTORY_MAX]"),
                       ((ptr(hist), 3, None, 2, None, 0, n), "act is needed with n_act > 0"),
                       ((ptr(hist), 3, ptr(act), 2, None, 0, 0), "rows must be at least 1"),
                       ((ptr(hist), 3, ptr(act), 2, ptr(W), 0, n), "w_rows must be at least 1")):
        assert set_history(L._h, *args) == -1 and "history: " + text in error_text(L), text
    got = rollout(world, policies[depths], n, s_mean, s_std)      # what was attached stayed, W included
    assert rollouts_equal(got, want) and not bool((W == SENTINEL).any())
    # the pushes
    goal, X, Wk = world.goal[:n].contiguous(), torch.full((n, n_wide + NG), SENTINEL, device=L.device), torch.full((n, n_wide), SENTINEL, device=L.device)
    mean, std = world.d(s_mean), world.d(s_std)
    ok = dict(B=n, hist=ptr(hist), n_obs=3, act=ptr(act), n_act=2, goal=ptr(goal), n_goal=NG, s_mean=ptr(mean), s_std=ptr(std), s_first=1, W=ptr(Wk),
              w_stride=n_wide, X=ptr(X))
    kept = registers(L)
    for change, text in ((dict(hist=None), "hist is needed"), (dict(act=None), "act is needed with n_act > 0"), (dict(B=0), "need B >= 1"),
                         (dict(B=-2), "need B >= 1"), (dict(w_stride=n_wide - 1), "w_stride must be at least n_wide"),
                         (dict(s_mean=None), "s_mean and s_std come together"), (dict(s_std=None), "s_mean and s_std come together"),
                         (dict(s_first=-1), "s_first must be in [0, n_wide]"), (dict(s_first=n_wide + 1), "s_first must be in [0, n_wide]"),
                         (dict(goal=None), "X needs goal"), (dict(W=None, X=None), "W or X is needed"), (dict(n_obs=0), "n_obs must be in"),
                         (dict(n_act=17), "n_act must be in")):
        assert L.lib.nmpc_history_push_batch(L._h, *{**ok, **change}.values(), None) == -1 and "history: " + text in error_text(L), text
    A = torch.zeros(n, NU, device=L.device)
    for args, text in (((n, None, 2, ptr(A), NU), "act and A are needed"), ((n, ptr(act), 2, None, NU), "act and A are needed"),
                       ((0, ptr(act), 2, ptr(A), NU), "need B >= 1"), ((n, ptr(act), 0, ptr(A), NU), "n_act must be in [1, NMPC_HISTORY_MAX]"),
                       ((n, ptr(act), 2, ptr(A), NU - 1), "a_stride must be at least 12")):
        assert L.lib.nmpc_history_push_actions_batch(L._h, *args, None) == -1 and "history: " + text in error_text(L), text
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all()) and bool((Wk == SENTINEL).all()) and registers_equal(kept, registers(L))
    # the rollout, before any launch
    S, A = torch.full((n + 1, K, NS), SENTINEL, device=L.device), torch.full((n + 1, K, NU), SENTINEL, device=L.device)
    failed = torch.full((n + 1,), 0x55, dtype=torch.int32, device=L.device)
    cases = [(lambda: raw_rollout(L, policies[depths], world, n + 1, s_mean, s_std, S, A, failed, n_wide + NG), "B exceeds rows"),
             (lambda: raw_rollout(L, policies[depths], world, n, s_mean, s_std, S, A, failed, n_wide + NG, n_steps=K + 1), "w_rows must be at least n_steps"),
             (lambda: raw_rollout(L, policies[(1, 0)], world, n, s_mean, s_std, S, A, failed, n_wide + NG), "the policy must map n_wide + n_goal inputs")]
    for call, text in cases:
        rc, q, v = call()
        assert rc == -1 and "history: " + text in error_text(L), text
        assert same(q, world.q[:q.shape[0]]) and bool((failed == 0x55).all()) and bool((S == SENTINEL).all()) and bool((A == SENTINEL).all())
    assert registers_equal(kept, registers(L))
    # and the Python layer
    with pytest.raises(ValueError, match="set_rollout_wide"):
        rollout(world, policies[depths], n, s_mean, s_std, n_steps=K + 1)
    with pytest.raises(ValueError, match=r"expected \[156\]"):
        rollout(world, policies[depths], n, s_mean[:NS], s_std[:NS])
    L.set_history(None)
    with pytest.raises(ValueError, match="nothing is attached"):
        L.history_push(goal)


# ---- 5. through evaluate_policy and dagger_iteration ------------------------------------------------------------------------------------
def test_evaluate_policy_returns_the_wide_rows_of_history_table(fx, world, clean, policies):
    from iterative_learning_nmpc_amd.learning import evaluate_policy
    L, n, depths = world.L, 3, (3, 2)
    q, v, goal, tau = world.q[:n], world.v[:n], world.goal[:n], world.tau[:n]
    kw = dict(dt=DT, n_sub=N_SUB, tau_ff=tau, kp=KP, kd=KD, t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)
    run = lambda **more: evaluate_policy(L, policies[depths], None, q, v, goal, K * N_SUB * DT, **kw, **more)      # noqa: E731
    out = run(history=depths, noise=fx.noise[:n], noise_seed=5, delays=fx.delays[:n], record_observed=True)
    assert L._history is None and L._noise is None and L._observed is None and L._delays is None
    assert out["W"].shape == (n, K, hr.width(*depths)) and not same(out["O"], out["S"])
    # the registers started from the true row of (q0, v0, t0), which is row 0 of S, and the posture of q0
    table = L.history_table(out["O"], out["A"], out["S"][:, 0], q, n_obs=3, n_act=2)
    assert same(out["W"], table) and L._history is None
    assert same(table, world.d(hr.closed_form(out["O"].cpu().numpy(), out["A"].cpu().numpy(), out["S"][:, 0].cpu().numpy(), fx.q[:n, 6:], *depths)))
    # without the keyword the policy of 159 inputs is refused by the memoryless rollout, and a history of the caller's is not replaced
    with pytest.raises(Exception, match="44 \\+ n_goal"):
        run()
    L.set_history(*depths, batch=n)
    mine = L.history
    assert same(L.history_table(out["O"], out["A"], out["S"][:, 0], q), table) and L.history is mine and not bool(mine.any())
    with pytest.raises(ValueError, match="history attached already"):
        run(history=depths)
    assert L.history is mine
    with pytest.raises(ValueError, match="n_obs must be in"):
        run(history=(0, 0))


class Dagger(ph.Dagger):
    """the fixtures of tests/test_gpu_dagger_iteration.py at B = 2 robots and 3 control steps"""
    B, K = 2, 3
    T = K * ph.Dagger.N_SUB * ph.Dagger.DT


def test_dagger_stores_the_wide_rows_the_learner_was_shown(dev):
    from iterative_learning_nmpc_amd import _lib, learning
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    n, depths = Dagger.B, (3, 2)
    n_wide = hr.width(*depths)
    rng = np.random.default_rng(2)
    q0 = ph.standing_start(n)[0]; q0[:, 6:] += rng.normal(0, 0.03, (n, 12))
    v0, goal = np.zeros((n, 18)), np.tile(np.float32([0.2, 0.0, 0.0]), (n, 1))
    mpc = ph.expert(dev, n, n_nodes=30)
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    L = BatchedTorqueLayer(**quadruped_tree(), device=dev)
    policy = policy_pair(n_wide + NG, 12, 2, 64, False, 64, seed=3)[0]
    noise = np.zeros((n, 2 * NS), np.float32)
    noise[:, 1:NS] = 0.02
    run = lambda db, **kw: learning.dagger_iteration(mpc, L, db, policy, q0, v0, goal, Dagger.T, dt=Dagger.DT, n_sub=Dagger.N_SUB, n_epoch=1,      # noqa: E731
                                                     batch_size=Dagger.BATCH, lr=1e-3, seed=Dagger.SEED, noise=noise, noise_seed=5, **kw)
    with pytest.raises(ValueError, match="the database stores states of width 44"):
        run(DeviceDatabase(limit=64, norm_input=False, device=dev), history=depths)
    assert L._history is None and L._noise is None
    # a database of wide rows that has statistics before the learner drives: eight rows of the expert's kind
    db = DeviceDatabase(limit=64, n_state=n_wide, norm_input=True, device=dev)
    db.append(rng.normal(0.0, 1.0, (8, n_wide)).astype(np.float32), rng.uniform(-1, 1, (8, 12)).astype(np.float32), goal[:1].repeat(8, 0))
    mean0, std0 = db.states_mean.clone(), db.states_std.clone()
    out = run(db, history=depths)
    torch.cuda.synchronize()
    st, alive = out["status"].cpu().numpy(), out["steps_survived"].cpu().numpy()
    idx = [(b, k) for b in range(n) for k in range(Dagger.K) if k < alive[b] and st[b, k] not in (_lib.NMPC_STATUS_NAN, _lib.NMPC_STATUS_QP)]
    print("steps survived", alive.tolist(), "rows", out["n_rows"])
    assert out["n_rows"] == len(idx) == len(db) - 8 > 0 and L._history is None and "O" not in out
    bs, ks = (torch.as_tensor(x, device=dev) for x in zip(*idx))
    assert same(db.tables["states"][8:len(db)], out["W"][bs, ks]) and same(db.tables["actions"][8:len(db)], out["A_star"][bs, ks])
    # the chain of the public calls from the visited states, under the statistics the rollout used
    L.set_noise(noise, seed=5)
    L.set_history(*depths, batch=n)
    q = torch.as_tensor(q0, dtype=torch.float32, device=dev)
    L.reset_history(out["S"][:, 0], q)
    g = torch.as_tensor(goal, device=dev)
    X = []
    for k in range(Dagger.K):
        L.observed_rows(out["S"][:, k], k, out=L.history[:, 0])      # the true row of step k under the draw of noise step k
        X.append(L.history_push(g, mean0, std0, 1))
        L.history_push_actions(out["A"][:, k])
    X = torch.stack(X, 1)
    # what the database makes of the stored rows under those statistics is what the policy was shown, to the bit
    db.states_mean, db.states_std = mean0, std0
    x, y = db.batch(torch.arange(8, len(db), dtype=torch.int32, device=dev))
    assert same(x, X[bs, ks]) and same(y, out["A_star"][bs, ks])
