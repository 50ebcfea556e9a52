"""GPU checks of sensor noise and bias per robot on the policy input of the contact plant (nmpc_contact_set_noise,
nmpc_contact_noise_step and nmpc_observe_noise_batch behind `BatchedTorqueLayer.set_noise`, `noise_step`, `observe_noise`).

The rule is an exact integer, one fp32 product and a handful of fp64 operations that are each rounded once, so every comparison is
equality of the bit patterns: the kernel against the numpy restatement of the rule (tests/noise_reference.py), an attached call
against the detached call of the same build followed by `observe_noise`, a rollout against the chain of the public calls.

Shapes: the quadruped tree.  The noise kernel runs 256 threads per block over B x 44 (robot, slot) pairs: B = 1, B = 5 (220 pairs,
a block that is not full) and B = 13 (572 pairs, three blocks, the second starting inside robot 5's row); rollouts at B = 5 over 3
control steps of 2 substeps.  A control step of 2 substeps keeps the times of `observe_rows` (t0 + k (2 dt)) and of the rollout
(t0 + (2 k) dt) the same doubles: the factor 2 is exact."""
import ctypes

import numpy as np
import pytest

from tests import fd_reference as fr
from tests import noise_reference as nr
from tests import plant_helpers as ph
from tests.plant_helpers import DT, HEIGHT, KD, KP, MASK, N_SUB, PERIOD, T0
from tests.plant_helpers import default_policy, detached, error_text, start_states  # noqa: F401
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, N, K, NU, NS = 13, 5, 3, 12, 44
DT32 = float(np.float32(DT))
SENTINEL = -77.0
SEED = 0x9E3779B97F4A7C15                                 # above 2^63: all 64 bits of the key are carried
QUIET = (0, 5, 30)                                        # slots without noise on every robot; robot b also has slot 8 + b quiet


class Fixture(ph.Fixture):
    def __init__(self):
        self.m = m = fr.quadruped()
        rng = np.random.default_rng(71)
        self.q, self.v = start_states(m, B, rng)
        self.tau = rng.uniform(-2, 2, (B, NU)).astype(np.float32)
        self.goal = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
        self.s_mean, self.s_std = rng.normal(0.0, 0.1, NS), rng.uniform(0.5, 2.0, NS)
        sigma, bias = rng.uniform(0.0, 0.2, (B, NS)), rng.uniform(-0.05, 0.05, (B, NS))
        sigma[:, 40], bias[:, 41] = 0.0, 0.0              # a bias alone, a sigma alone
        for b in range(B):
            sigma[b, list(QUIET) + [8 + b]] = 0.0
            bias[b, list(QUIET) + [8 + b]] = 0.0
        self.noise = np.concatenate([sigma, bias], axis=1).astype(np.float32)
        self.quiet = (self.noise[:, :NS] == 0) & (self.noise[:, NS:] == 0)
        self.delays = (np.arange(B) % 3).astype(np.int32)
        self.freeze()


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    assert int(f.quiet.sum()) == 4 * B and not f.quiet[:, [40, 41]].any()
    return f


@pytest.fixture(scope="module")
def world(fx):
    return ph.World(fx.m, B, q=fx.q, v=fx.v, tau=fx.tau, goal=fx.goal)


@pytest.fixture(scope="module")
def policy(dev):
    return default_policy()


def stats_of(fx, stats):
    return (fx.s_mean, fx.s_std) if stats else (None, None)


def rollout(w, policy, fx, rows=slice(0, N), n_steps=K, t0=T0, q=None, v=None, stats=True):
    """`policy_rollout` of the robots `rows` from the fixture's states, or from q, v given for them"""
    s_mean, s_std = stats_of(fx, stats)
    return w.L.policy_rollout(policy, w.q[rows] if q is None else q, w.v[rows] if v is None else v, n_steps, DT, N_SUB, w.goal[rows],
                              tau_ff=w.tau[rows], kp=KP, kd=KD, t0=t0, period=PERIOD, s_mean=s_mean, s_std=s_std, terminate_mask=MASK,
                              collision_height=HEIGHT)


def rollouts_equal(a, b):
    return all(same(x, y) for x, y in zip(a[:4], b[:4])) and torch.equal(a[4], b[4])


# ---- 1. the kernel against the restatement of its rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("stats,s_first", [(False, 1), (True, 0), (True, 1)])
@pytest.mark.parametrize("n_goal", [0, 3])
@pytest.mark.parametrize("n", [1, 5, B])
def test_observe_noise_is_the_reference(fx, world, detached, n, n_goal, stats, s_first):
    L = world.L
    rng = np.random.default_rng(1000 * n + 10 * n_goal + s_first)
    X = rng.normal(0.0, 1.5, (n, NS + n_goal)).astype(np.float32)
    X[:, NS:] = SENTINEL
    X[:, :NS][fx.quiet[:n]] = SENTINEL
    s_std = fx.s_std if stats else None
    # a step above 2^16 with a population index that wraps past 2^32 inside the batch, the plain case, and both counters past 2^32
    for step, first_robot in ((2 ** 16 + 4465, 2 ** 32 - 3), (0, 0), (2 ** 32 + 7, 2 ** 33 + 2)):
        L.set_noise(world.d(fx.noise), seed=SEED, first_robot=first_robot, step0=11)
        got = L.observe_noise(world.d(X), step, s_std=s_std, s_first=s_first)
        want = nr.observe_noise(X, fx.noise, SEED, first_robot, step, s_std, s_first)
        diff = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"  B = {n}, n_goal = {n_goal}, stats = {stats}, s_first = {s_first}, step = {step}, first_robot = {first_robot}: "
              f"largest |gpu - numpy| = {diff.max():.3e}, moved {int((want != X).sum())} of {X.size}")
        assert same(got, world.d(want))
        assert bool((got[:, NS:] == SENTINEL).all()) and bool((got[:, :NS][world.d(fx.quiet[:n])] == SENTINEL).all())
        assert int((want[:, :NS] != X[:, :NS]).sum()) >= (NS - 5) * n      # and everything else did move
        assert L.noise_step == 11                          # the rule alone leaves the layer's step where it is
    # the host-validated table is the same table
    L.set_noise(fx.noise, seed=SEED)
    assert same(L.observe_noise(world.d(X), 3, s_std=s_std, s_first=s_first), world.d(nr.observe_noise(X, fx.noise, SEED, 0, 3, s_std, s_first)))


def test_a_robot_draws_by_its_place_in_the_population_not_in_the_batch(fx, world, detached):
    L = world.L
    X = np.random.default_rng(5).normal(0.0, 1.0, (B, NS + 3)).astype(np.float32)
    L.set_noise(world.d(fx.noise), seed=SEED)
    whole = L.observe_noise(world.d(X), 9, s_std=fx.s_std)
    for b in (0, 5, B - 1):                                # 5: the robot whose row straddles the first block boundary
        L.set_noise(world.d(fx.noise[b:b + 1]), seed=SEED, first_robot=b)
        assert same(L.observe_noise(world.d(X[b:b + 1]), 9, s_std=fx.s_std), whole[b:b + 1]), b
    L.set_noise(world.d(fx.noise), seed=SEED + 1)
    other = L.observe_noise(world.d(X), 9, s_std=fx.s_std)
    assert not same(other[:, 1:4], whole[:, 1:4])          # the key is read


# ---- 2. an attached observation is the detached one followed by the rule -------------------------------------------------------------
def observe_raw(L, w, fx, n, t, S, X, failed, step_index, stats=True):
    """nmpc_observe_batch as the library has it, for the outputs the Python layer always asks for: S, X may be None"""
    from iterative_learning_nmpc_amd._lib import ptr, stream
    s_mean, s_std = (None, None) if not stats else (w.d(fx.s_mean), w.d(fx.s_std))
    q, v, goal = w.q[:n].contiguous(), w.v[:n].contiguous(), w.goal[:n].contiguous()
    rc = L.lib.nmpc_observe_batch(L._h, n, ptr(q), ptr(v), t, PERIOD, ptr(goal), 3, ptr(s_mean), ptr(s_std), 1, HEIGHT, ptr(S), NS, ptr(X),
                                  ptr(failed), step_index, MASK, stream(L.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("stats", [False, True])
def test_the_attached_observation_is_the_detached_one_then_the_rule(fx, world, detached, stats):
    L, n = world.L, B
    s_mean, s_std = stats_of(fx, stats)
    flags = lambda: torch.zeros(n, dtype=torch.int32, device=L.device)      # noqa: E731
    f0 = flags()
    S0, X0 = L.observe(world.q, world.v, T0, PERIOD, world.goal, s_mean=s_mean, s_std=s_std, collision_height=HEIGHT, failed=f0, step_index=2,
                       term_mask=MASK)
    assert L.noise_step is None
    L.set_noise(world.d(fx.noise), seed=SEED, first_robot=4, step0=70000)
    assert L.noise_step == 70000
    f1 = flags()
    S1, X1 = L.observe(world.q, world.v, T0, PERIOD, world.goal, s_mean=s_mean, s_std=s_std, collision_height=HEIGHT, failed=f1, step_index=2,
                       term_mask=MASK)
    assert L.noise_step == 70001                           # one observation with an X: one step
    want = L.observe_noise(X0.clone(), 70000, s_std=s_std)
    assert same(X1, want) and not same(X1, X0)
    assert same(X1, world.d(nr.observe_noise(X0.cpu().numpy(), fx.noise, SEED, 4, 70000, s_std)))
    assert same(S1, S0) and torch.equal(f1, f0)            # the row and the flags are the true state's
    assert same(X1[:, NS:], world.goal)
    # the next one draws at the next step
    _, X2 = L.observe(world.q, world.v, T0, PERIOD, world.goal, s_mean=s_mean, s_std=s_std, collision_height=HEIGHT)
    assert L.noise_step == 70002 and same(X2, L.observe_noise(X0.clone(), 70001, s_std=s_std)) and not same(X2, X1)
    # without an X nothing is drawn and nothing advances: the row alone, then the flags alone
    S3, f3 = torch.full((n, NS), SENTINEL, device=L.device), flags()
    assert observe_raw(L, world, fx, n, T0, S3, None, f3, 2, stats) == 0
    assert L.noise_step == 70002 and same(S3, S0) and torch.equal(f3, f0)
    assert observe_raw(L, world, fx, n, T0, None, None, f3, 2, stats) == 0 and L.noise_step == 70002
    # and with one it is the library that counts, whoever calls
    X4 = torch.empty(n, NS + 3, device=L.device)
    assert observe_raw(L, world, fx, n, T0, None, X4, None, 2, stats) == 0
    assert L.noise_step == 70003 and same(X4, L.observe_noise(X0.clone(), 70002, s_std=s_std))


# ---- 3. the policy rollout ------------------------------------------------------------------------------------------------------------
def chain(w, policy, fx, perturb, n_steps=K, stats=True):
    """observe -> [perturb(X, k)] -> forward -> contact_step through the Python layer, and the last observation"""
    L = w.L
    s_mean, s_std = stats_of(fx, stats)
    q, v, goal, tau = w.q[:N], w.v[:N], w.goal[:N], w.tau[:N]
    failed = torch.zeros(N, dtype=torch.int32, device=L.device)
    S, A = [], []
    for k in range(n_steps):
        s, x = L.observe(q, v, T0 + (k * N_SUB) * DT32, PERIOD, goal, s_mean=s_mean, s_std=s_std, collision_height=HEIGHT, failed=failed,
                         step_index=k, term_mask=MASK)
        a = policy.forward(perturb(x, k)).clone()
        S.append(s); A.append(a)
        q, v = L.contact_step(q, v, DT, N_SUB, tau_ff=tau, q_des=a, kp=KP, kd=KD)[:2]
    L.observe(q, v, T0 + (n_steps * N_SUB) * DT32, PERIOD, goal, s_mean=s_mean, s_std=s_std, collision_height=HEIGHT, failed=failed,
              step_index=n_steps, term_mask=MASK)
    return q, v, torch.stack(S, 1), torch.stack(A, 1), failed


@pytest.mark.parametrize("stats", [False, True])
def test_the_policy_rollout_is_its_chain_of_public_calls(fx, world, detached, policy, stats):
    L = world.L
    s_std = fx.s_std if stats else None
    bare = rollout(world, policy, fx, stats=stats)
    assert rollouts_equal(bare, chain(world, policy, fx, lambda x, k: x, stats=stats))
    attach = lambda **kw: L.set_noise(world.d(fx.noise), seed=SEED, **kw)      # noqa: E731
    attach(step0=40)
    got = rollout(world, policy, fx, stats=stats)
    assert L.noise_step == 40 + K                          # K observations with an X; the last one has none
    # the chain with the table attached: every observe perturbs its own X
    attach(step0=40)
    assert rollouts_equal(got, chain(world, policy, fx, lambda x, k: x, stats=stats))
    assert L.noise_step == 40 + K + 1                      # the Python `observe` always asks for an X, the chain's last one too
    # the chain with the table on a second layer: the observation is the detached one, the rule is applied by hand
    L.set_noise(None)
    other = layer(fx.m)
    other.set_noise(world.d(fx.noise), seed=SEED)
    by_hand = chain(world, policy, fx, lambda x, k: other.observe_noise(x, 40 + k, s_std=s_std), stats=stats)
    assert rollouts_equal(got, by_hand)
    # what moved and what did not: the first row of S is the start state's, the actions differ from the first step on
    assert same(got[2][:, 0], bare[2][:, 0]) and not same(got[3][:, 0], bare[3][:, 0]) and not same(got[0], bare[0])
    assert same(rollout(world, policy, fx, stats=stats)[3], bare[3])      # detached: the un-noised bits again


def test_robot_b_of_a_rollout_is_the_batch_of_one_of_its_row(fx, world, detached, policy):
    L = world.L
    L.set_noise(world.d(fx.noise), seed=SEED, step0=7)
    got = rollout(world, policy, fx)
    for b in (0, 3, N - 1):
        L.set_noise(world.d(fx.noise[b:b + 1]), seed=SEED, first_robot=b, step0=7)
        one = rollout(world, policy, fx, rows=slice(b, b + 1))
        assert all(same(x[b:b + 1], y) for x, y in zip(got[:4], one[:4])) and torch.equal(got[4][b:b + 1], one[4]), b
    # spare rows change nothing, a robot without noise is the robot of the un-noised call, and its neighbours are not
    table = fx.noise.copy()
    table[2] = 0.0
    L.set_noise(world.d(table), seed=SEED, step0=7)
    mixed = rollout(world, policy, fx)
    L.set_noise(None)
    bare = rollout(world, policy, fx)
    assert all(same(x[2], y[2]) for x, y in zip(mixed[:4], bare[:4]))
    assert all(same(x[b], y[b]) for x, y in zip(mixed[:4], got[:4]) for b in (0, 1, 3, 4))
    assert not same(mixed[3][1], bare[3][1])


def test_a_table_of_zeros_is_no_table_and_a_detach_restores_the_bits(fx, world, detached, policy):
    L = world.L
    bare = rollout(world, policy, fx)
    L.set_noise(np.zeros((N, 2 * NS), np.float32), seed=SEED)
    assert rollouts_equal(rollout(world, policy, fx), bare) and L.noise_step == K      # nothing is written, the step still counts
    L.set_noise(world.d(fx.noise), seed=SEED)
    noisy = rollout(world, policy, fx)
    assert not same(noisy[3], bare[3])                     # non-zero sigma changes the actions
    L.set_noise(None)
    assert L.noise_step is None and rollouts_equal(rollout(world, policy, fx), bare)


# ---- 4. two rollouts of K are the rollout of 2 K ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delayed", [False, True])
def test_two_rollouts_are_the_long_rollout(fx, world, detached, policy, delayed):
    L = world.L

    def start():
        L.set_noise(world.d(fx.noise), seed=SEED, step0=3)
        if delayed:
            L.set_delays(fx.delays[:N], depth=2)
            L.reset_delay_history(world.q[:N])

    start()
    long = rollout(world, policy, fx, n_steps=2 * K)
    H = L.delay_history.clone() if delayed else None
    assert L.noise_step == 3 + 2 * K
    start()
    one = rollout(world, policy, fx)
    assert L.noise_step == 3 + K
    two = rollout(world, policy, fx, q=one[0], v=one[1], t0=T0 + (K * N_SUB) * DT32)
    assert L.noise_step == 3 + 2 * K
    assert same(two[0], long[0]) and same(two[1], long[1])
    assert same(torch.cat([one[2], two[2]], 1), long[2]) and same(torch.cat([one[3], two[3]], 1), long[3])
    assert torch.equal((one[4] | two[4]) & 0xFF, long[4] & 0xFF)      # the flag bits; the stamps count each call's own steps
    if delayed:                                            # the two tables compose: the register went through the same six steps
        assert same(L.delay_history, H)
        L.set_delays(None)
        L.set_noise(world.d(fx.noise), seed=SEED, step0=3)
        assert not same(rollout(world, policy, fx, n_steps=2 * K)[0], long[0])      # and the delay was not idle


# ---- 5. refusals leave what was attached in force --------------------------------------------------------------------------------------
def test_refusals_leave_the_attached_table_in_force(fx, world, detached, policy):
    from iterative_learning_nmpc_amd._lib import NmpcError, ptr
    L, lib = world.L, world.L.lib
    X = torch.full((N, NS + 3), SENTINEL, device=L.device)
    with pytest.raises(NmpcError, match="noise: no table is attached"):
        L.observe_noise(X, 0)
    step = ctypes.c_longlong(-5)
    assert lib.nmpc_contact_noise_step(L._h, ctypes.byref(step)) == -1 and "no table is attached" in error_text(L) and step.value == -5
    L.set_noise(world.d(fx.noise[:4]), seed=SEED, step0=21)
    want = rollout(world, policy, fx, rows=slice(0, 4))
    L.set_noise(world.d(fx.noise[:4]), seed=SEED, step0=21)
    # more robots than rows: at the rollout, at the observation, at the rule alone -- before any launch
    with pytest.raises(NmpcError, match="noise: B exceeds rows"):
        rollout(world, policy, fx)
    with pytest.raises(NmpcError, match="noise: B exceeds rows"):
        L.observe(world.q[:N], world.v[:N], T0, PERIOD, world.goal[:N])
    with pytest.raises(NmpcError, match="noise: B exceeds rows"):
        L.observe_noise(X, 0)
    # rows < 1: refused, and neither the table nor its step is replaced
    bigger = world.d(fx.noise)
    for rows in (0, -3):
        assert lib.nmpc_contact_set_noise(L._h, ptr(bigger), rows, 1, 2, 3) == -1 and "rows must be at least 1" in error_text(L)
    # what the rule alone does not take
    X4 = X[:4].contiguous()
    for args, text in (((4, None, NS + 3, None, 1, 0), "X is needed"), ((4, ptr(X4), NS - 1, None, 1, 0), "x_stride must be at least 44"),
                       ((4, ptr(X4), NS + 3, None, -1, 0), "s_first must be in"), ((4, ptr(X4), NS + 3, None, NS + 1, 0), "s_first must be in"),
                       ((-1, ptr(X4), NS + 3, None, 1, 0), "B >= 0")):
        assert lib.nmpc_observe_noise_batch(L._h, *args, None) == -1 and text in error_text(L), text
    assert lib.nmpc_observe_noise_batch(L._h, 0, None, 0, None, 1, 0, None) == 0      # an empty batch is no error
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all())
    assert L.noise_step == 21                              # nothing above drew or counted
    assert rollouts_equal(rollout(world, policy, fx, rows=slice(0, 4)), want)
    # the calls that do not read the table are not refused for it
    L.set_noise(world.d(fx.noise[:4]), seed=SEED)
    bare = L.contact_step(world.q, world.v, DT, N_SUB, tau_ff=world.tau, q_des=world.q[:, 6:].contiguous(), kp=KP, kd=KD)[:2]
    L.set_noise(None)
    again = L.contact_step(world.q, world.v, DT, N_SUB, tau_ff=world.tau, q_des=world.q[:, 6:].contiguous(), kp=KP, kd=KD)[:2]
    assert same(bare[0], again[0]) and same(bare[1], again[1])


# ---- 6. through evaluate_policy ------------------------------------------------------------------------------------------------------
def test_evaluate_policy_attaches_and_detaches_the_table(fx, world, detached, policy):
    from iterative_learning_nmpc_amd.learning import evaluate_policy
    L = world.L
    q, v, goal, tau = world.q[:N], world.v[:N], world.goal[:N], world.tau[:N]
    kw = dict(dt=DT, n_sub=N_SUB, tau_ff=tau, kp=KP, kd=KD, t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)
    T = K * N_SUB * DT
    run = lambda **more: evaluate_policy(L, policy, None, q, v, goal, T, **kw, **more)      # noqa: E731
    bare = run()
    L.set_noise(fx.noise[:N], seed=5)
    want = rollout(world, policy, fx, stats=False)
    L.set_noise(None)
    out = run(noise=fx.noise[:N], noise_seed=5, record_states=True)
    assert L._noise is None and L.noise_step is None
    assert all(same(out[k], x) for k, x in zip(("q", "v", "S", "A"), want)) and torch.equal(out["failed"], want[4])
    assert not same(out["A"], bare["A"]) and not same(run(noise=fx.noise[:N], noise_seed=6)["A"], out["A"])
    # Q, V are the true plant states: the rows rebuilt from them are the rows returned (2 substeps: the times are the same doubles)
    assert out["Q"].shape == (N, K, 18) and same(out["Q"][:, 0], q) and same(out["V"][:, 0], v)
    rebuilt = L.observe_rows(out["Q"], out["V"], T0, N_SUB * DT32, PERIOD, collision_height=HEIGHT)
    assert same(rebuilt, out["S"])
    assert same(run()["A"], bare["A"])                     # nothing is left behind
    with pytest.raises(Exception):                         # also when the rollout raises
        evaluate_policy(L, policy, None, q, v, goal[:3], T, noise=fx.noise[:N], **kw)
    assert L._noise is None
    bad = fx.noise[:N].copy()
    bad[1, 3] = -1.0
    with pytest.raises(ValueError, match="noise: row 1: sigma must not be negative"):      # host input is validated on its way in
        run(noise=bad)
    assert L._noise is None
    # a table of the caller's stays, is used, keeps counting, and is not replaced
    L.set_noise(fx.noise[:N], seed=5)
    mine = L._noise
    again = run()
    assert L._noise is mine and L.noise_step == K and same(again["A"], out["A"])
    with pytest.raises(ValueError, match="attached already"):
        run(noise=fx.noise[:N])
    assert L._noise is mine
