"""GPU checks of the rows the sensors showed (nmpc_observed_rows_batch, nmpc_policy_rollout_set_observed behind
`BatchedTorqueLayer.observed_rows`, `set_rollout_observed`; `learning.evaluate_policy(record_observed=True)`,
`learning.dagger_iteration(store="observed")`).

The rule is the sensor rule's draw added to the true row in fp64 and rounded once, so every comparison is equality of the bit
patterns: the kernel against the numpy restatement (tests/input_noise_reference.py), the rollout's O against the chain of the
public calls, and every other output of a rollout with O attached against the rollout without.

Shapes: the quadruped tree.  The kernel runs 256 threads per block over B x 44 (robot, slot) pairs: B = 3 (132 pairs, a block
that is not full) and B = 7 (308 pairs, a second block that starts inside robot 5's row); rollouts of 4 control steps of 2
substeps with a policy of one hidden layer of 16."""
import ctypes

import numpy as np
import pytest

from tests import fd_reference as fr
from tests import input_noise_reference as ir
from tests import plant_helpers as ph
from tests.plant_helpers import DT, HEIGHT, KD, KP, MASK, N_SUB, PERIOD, T0
from tests.plant_helpers import detached, error_text, start_states  # noqa: F401
from tests.solve_helpers import dev, policy_pair  # noqa: F401
from tests.torque_helpers import same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, K, NU, NS = 7, 4, 12, 44
SIZES = (3, 7)
DT32 = float(np.float32(DT))
SENTINEL = -77.0
SEED = 0x9E3779B97F4A7C15                                 # above 2^63: all 64 bits of the key are carried
FIRST, STEP0 = 2 ** 32 - 2, 70000                          # a population index that wraps past 2^32 inside the batch
QUIET = (0, 5, 30)                                        # slots without noise on every robot


class Fixture(ph.Fixture):
    def __init__(self):
        self.m = m = fr.quadruped()
        rng = np.random.default_rng(83)
        self.q, self.v = start_states(m, B, rng)
        self.tau = rng.uniform(-2, 2, (B, NU)).astype(np.float32)
        self.goal = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
        self.s_mean, self.s_std = rng.normal(0.0, 0.1, NS), rng.uniform(0.5, 2.0, NS)
        sigma, bias = rng.uniform(0.0, 0.2, (B, NS)), rng.uniform(-0.05, 0.05, (B, NS))
        sigma[:, 40], bias[:, 41] = 0.0, 0.0              # a bias alone, a sigma alone
        sigma[:, list(QUIET)], bias[:, list(QUIET)] = 0.0, 0.0
        self.noise = np.concatenate([sigma, bias], axis=1).astype(np.float32)
        self.quiet = (self.noise[:, :NS] == 0) & (self.noise[:, NS:] == 0)
        self.freeze()


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    assert int(f.quiet.sum()) == len(QUIET) * B
    return f


@pytest.fixture(scope="module")
def world(fx):
    return ph.World(fx.m, B, q=fx.q, v=fx.v, tau=fx.tau, goal=fx.goal)


@pytest.fixture(scope="module")
def policy(dev):
    return policy_pair(47, 12, 1, 16, True, 8, seed=5)[0]


def rollout(w, policy, fx, n, stats, n_steps=K):
    s_mean, s_std = (fx.s_mean, fx.s_std) if stats else (None, None)
    return w.L.policy_rollout(policy, w.q[:n], w.v[:n], n_steps, DT, N_SUB, w.goal[:n], tau_ff=w.tau[:n], kp=KP, kd=KD, t0=T0, period=PERIOD,
                              s_mean=s_mean, s_std=s_std, terminate_mask=MASK, collision_height=HEIGHT)


def rollouts_equal(a, b):
    return all(same(x, y) for x, y in zip(a[:4], b[:4])) and torch.equal(a[4], b[4])


def attach(w, fx, n, **kw):
    w.L.set_noise(w.d(fx.noise[:n]), seed=SEED, first_robot=FIRST, **kw)


def observed(L, n, rows=K, fill=SENTINEL):
    O = torch.full((n, rows, NS), fill, device=L.device)
    L.set_rollout_observed(O)
    return O


# ---- 1. the kernel against the restatement of its rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_observed_rows_is_the_reference(fx, world, detached, n):
    L = world.L
    S = np.random.default_rng(n).normal(0.0, 1.5, (n, NS)).astype(np.float32)
    S[:, 5] = -0.0
    for step, first_robot in ((0, 0), (2 ** 16 + 4465, 2 ** 32 - 3), (2 ** 32 + 7, 2 ** 33 + 2)):
        L.set_noise(world.d(fx.noise), seed=SEED, first_robot=first_robot, step0=11)       # more rows than robots is fine
        want = ir.observed_rows(S, fx.noise, SEED, first_robot, step)
        got = L.observed_rows(world.d(S), step)
        assert got.shape == (n, NS) and same(got, world.d(want))
        assert same(got[world.d(fx.quiet[:n])], world.d(S[fx.quiet[:n]])) and int((want != S).sum()) == n * (NS - len(QUIET))
        # strides larger than 44 on either side: the columns behind slot 43 are neither read nor written
        wide = torch.full((n, NS + 3), SENTINEL, device=L.device)
        wide[:, :NS] = world.d(S)
        out = torch.full((n, NS + 6), SENTINEL, device=L.device)
        assert L.observed_rows(wide, step, out=out) is out
        assert same(out[:, :NS].contiguous(), world.d(want)) and bool((out[:, NS:] == SENTINEL).all()) and bool((wide[:, NS:] == SENTINEL).all())
        # in place, and the row is what the sensor rule makes of a raw policy input
        assert same(L.observed_rows(wide, step, out=wide)[:, :NS].contiguous(), world.d(want))
        X = torch.cat([world.d(S), torch.full((n, 3), SENTINEL, device=L.device)], 1).contiguous()
        assert same(L.observe_noise(X, step)[:, :NS].contiguous(), got)
        assert L.noise_step == 11                          # the rule alone leaves the layer's step where it is
    L.set_noise(world.d(fx.noise), seed=SEED + 1)
    assert not same(L.observed_rows(world.d(S), 0)[:, 1:4], world.d(ir.observed_rows(S, fx.noise, SEED, 0, 0))[:, 1:4])      # the key is read


@pytest.mark.parametrize("n", SIZES)
def test_without_a_table_the_observed_rows_are_the_rows(fx, world, detached, policy, n):
    L = world.L
    S = np.random.default_rng(n).normal(0.0, 1.5, (n, NS)).astype(np.float32)
    S[:, 5] = -0.0
    assert L.noise_step is None and same(L.observed_rows(world.d(S), 9), world.d(S))
    L.set_noise(np.zeros((n, 2 * NS), np.float32), seed=SEED)
    assert same(L.observed_rows(world.d(S), 9), world.d(S))
    L.set_noise(None)
    O = observed(L, n)
    got = rollout(world, policy, fx, n, True)
    assert same(O, got[2])


# ---- 2. the policy rollout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_the_rollouts_observed_rows_are_the_rule_and_the_chain(fx, world, detached, policy, n, stats):
    L = world.L
    s_mean, s_std = (fx.s_mean, fx.s_std) if stats else (None, None)
    attach(world, fx, n, step0=STEP0)
    bare = rollout(world, policy, fx, n, stats)
    assert L.noise_step == STEP0 + K
    attach(world, fx, n, step0=STEP0)
    Q, V = (torch.empty(n, K, 18, device=L.device) for _ in range(2))
    L.set_rollout_states(Q, V)
    plain = rollout(world, policy, fx, n, stats)
    plain_QV = (Q.clone(), V.clone())
    attach(world, fx, n, step0=STEP0)
    O = observed(L, n)
    got = rollout(world, policy, fx, n, stats)
    # S, A, q, v, failed, Q, V and the final noise step are what they are without O
    assert rollouts_equal(got, plain) and rollouts_equal(got, bare) and same(Q, plain_QV[0]) and same(V, plain_QV[1])
    assert L.noise_step == STEP0 + K
    # O is the rule on the rollout's own S at the steps step0 .. step0 + K - 1
    S = got[2].cpu().numpy()
    for k in range(K):
        assert same(O[:, k], world.d(ir.observed_rows(S[:, k], fx.noise[:n], SEED, FIRST, STEP0 + k))), k
    assert not same(O, got[2]) and same(O[:, :, list(QUIET)], got[2][:, :, list(QUIET)])
    # and the chain of the public calls: the noise step, the observation, the observed rows at the step read
    L.set_rollout_observed(None)
    L.set_rollout_states(None)
    attach(world, fx, n, step0=STEP0)
    for k in range(K):
        step = L.noise_step
        s, x = L.observe(Q[:, k], V[:, k], T0 + (k * N_SUB) * DT32, PERIOD, world.goal[:n], s_mean=s_mean, s_std=s_std, collision_height=HEIGHT)
        o = L.observed_rows(s, step)
        assert step == STEP0 + k and same(s, got[2][:, k]) and same(o, O[:, k]), k
        assert same(policy.forward(x), got[3][:, k])       # the input the policy acted on in step k is this draw
        if not stats:                                      # raw inputs: what the policy was shown is the observed row to the bit
            assert same(x[:, :NS].contiguous(), O[:, k]), k


def raw_rollout(L, policy, w, fx, n, S, A, failed, n_steps=K):
    """nmpc_policy_rollout_batch as the library has it, with raw inputs: S and A may be None -> (rc, q, v)"""
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import ptr, stream
    from iterative_learning_nmpc_amd.torque import GroundContact
    q, v, goal, tau = w.q[:n].clone(), w.v[:n].clone(), w.goal[:n].contiguous(), w.tau[:n].contiguous()
    X = torch.empty(n, NS + 3, device=L.device)
    cfg = _lib.NmpcPolicyRolloutCfg(n_steps, N_SUB, DT, KP, KD, T0, PERIOD, HEIGHT, MASK, 3, 1)
    g = GroundContact().cfg()
    rc = L.lib.nmpc_policy_rollout_batch(L._h, policy._h, n, ctypes.byref(cfg), ctypes.byref(g), ptr(q), ptr(v), ptr(tau), ptr(goal), None, None,
                                         ptr(S), ptr(A), ptr(X), ptr(failed), stream(L.device))
    torch.cuda.synchronize()
    return rc, q, v


@pytest.mark.parametrize("n", SIZES)
def test_without_an_s_the_rollout_still_writes_the_observed_rows(fx, world, detached, policy, n):
    L = world.L
    attach(world, fx, n, step0=STEP0)
    O = observed(L, n, rows=6)                             # o_rows = 6: rows 4 and 5 of every robot stay as they are
    want = rollout(world, policy, fx, n, False)
    with_s = O.clone()
    assert same(O[:, :K], world.d(np.stack([ir.observed_rows(want[2][:, k].cpu().numpy(), fx.noise[:n], SEED, FIRST, STEP0 + k) for k in range(K)], 1)))
    assert bool((O[:, K:] == SENTINEL).all())
    attach(world, fx, n, step0=STEP0)
    O.fill_(SENTINEL)
    failed = torch.zeros(n, dtype=torch.int32, device=L.device)
    rc, q, v = raw_rollout(L, policy, world, fx, n, None, None, failed)
    assert rc == 0 and same(O, with_s) and same(q, want[0]) and same(v, want[1]) and torch.equal(failed, want[4])
    assert L.noise_step == STEP0 + K
    # a slice [:, :K] of the longer table is taken with its stride
    attach(world, fx, n, step0=STEP0)
    O.fill_(SENTINEL)
    L.set_rollout_observed(O[:, :K])
    assert rollouts_equal(rollout(world, policy, fx, n, False), want) and same(O, with_s)


def test_too_few_rows_are_refused_before_any_launch(fx, world, detached, policy):
    from iterative_learning_nmpc_amd._lib import NmpcError, ptr
    L, n = world.L, 3
    attach(world, fx, n, step0=STEP0)
    O = observed(L, n, rows=3)
    with pytest.raises(ValueError, match="set_rollout_observed"):      # the Python layer sees it first
        rollout(world, policy, fx, n, False)
    S, A = torch.full((n, K, NS), SENTINEL, device=L.device), torch.full((n, K, NU), SENTINEL, device=L.device)
    failed = torch.full((n,), 0x55, dtype=torch.int32, device=L.device)
    rc, q, v = raw_rollout(L, policy, world, fx, n, S, A, failed)
    assert rc == -1 and "observed: o_rows must be at least n_steps" in error_text(L)
    assert bool((failed == 0x55).all()) and bool((S == SENTINEL).all()) and bool((A == SENTINEL).all()) and bool((O == SENTINEL).all())
    assert same(q, world.q[:n]) and same(v, world.v[:n]) and L.noise_step == STEP0
    assert raw_rollout(L, policy, world, fx, n, S, A, failed, n_steps=3)[0] == 0      # three steps fit
    assert not bool((O == SENTINEL).any())
    # what the rule alone does not take
    s, o = torch.zeros(n, NS, device=L.device), torch.full((n, NS), SENTINEL, device=L.device)
    for args, text in (((n, None, NS, ptr(o), NS, 0), "S and O are needed"), ((n, ptr(s), NS, None, NS, 0), "S and O are needed"),
                       ((n, ptr(s), NS - 1, ptr(o), NS, 0), "must be at least 44"), ((n, ptr(s), NS, ptr(o), NS - 1, 0), "must be at least 44"),
                       ((n + 1, ptr(s), NS, ptr(o), NS, 0), "B exceeds the rows"), ((-1, ptr(s), NS, ptr(o), NS, 0), "B >= 0")):
        assert L.lib.nmpc_observed_rows_batch(L._h, *args, None) == -1 and text in error_text(L), text
    assert L.lib.nmpc_observed_rows_batch(L._h, 0, None, 0, None, 0, 0, None) == 0      # an empty batch is no error
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())
    with pytest.raises(NmpcError, match="B exceeds the rows"):
        L.observed_rows(torch.zeros(n + 1, NS, device=L.device), 0)
    with pytest.raises(ValueError, match="O: need a float32"):
        L.set_rollout_observed(torch.zeros(n, K, NS + 1, device=L.device))


# ---- 3. through evaluate_policy and dagger_iteration ------------------------------------------------------------------------------------
def test_evaluate_policy_returns_the_observed_rows_and_leaves_nothing_attached(fx, world, detached, policy):
    from iterative_learning_nmpc_amd.learning import evaluate_policy
    L, n = world.L, 3
    q, v, goal, tau = world.q[:n], world.v[:n], world.goal[:n], world.tau[:n]
    kw = dict(dt=DT, n_sub=N_SUB, tau_ff=tau, kp=KP, kd=KD, t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)
    T = K * N_SUB * DT
    run = lambda **more: evaluate_policy(L, policy, None, q, v, goal, T, **kw, **more)      # noqa: E731
    plain = run(noise=fx.noise[:n], noise_seed=5)
    assert "O" not in plain
    out = run(noise=fx.noise[:n], noise_seed=5, record_observed=True, record_states=True)
    assert L._observed is None and L._noise is None and L._states is None
    assert out["O"].shape == (n, K, NS) and all(same(out[k], plain[k]) for k in ("q", "v", "S", "A")) and torch.equal(out["failed"], plain["failed"])
    S = out["S"].cpu().numpy()
    for k in range(K):                                     # evaluate_policy attaches with first_robot = 0 and the noise step 0
        assert same(out["O"][:, k], world.d(ir.observed_rows(S[:, k], fx.noise[:n], 5, 0, k))), k
    assert same(run(record_observed=True)["O"], run()["S"])      # without noise the sensors show the state
    with pytest.raises(Exception):                         # detached also when the rollout raises
        evaluate_policy(L, policy, None, q, v, goal[:2], T, record_observed=True, **kw)
    assert L._observed is None
    mine = observed(L, n)
    with pytest.raises(ValueError, match="observed rows attached already"):
        run(record_observed=True)
    assert L._observed is mine
    assert same(run()["S"], mine)                          # rows of the caller's stay attached and are written


class Dagger(ph.Dagger):
    """the fixtures of tests/test_gpu_dagger_iteration.py at B = 2 robots and 3 control steps"""
    B, K = 2, 3
    T = K * ph.Dagger.N_SUB * ph.Dagger.DT


@pytest.fixture(scope="module")
def expert(dev):
    """the controller, the layer and the start states, made once: a run leaves nothing on either (the labels of a set of states
    are the same bits whatever was labelled before, tests/test_gpu_dagger_iteration.py)"""
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    n = Dagger.B
    rng = np.random.default_rng(2)
    q0 = ph.standing_start(n)[0]; q0[:, 6:] += rng.normal(0, 0.03, (n, 12))
    mpc = ph.expert(dev, n, n_nodes=30)
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    return dict(mpc=mpc, layer=BatchedTorqueLayer(**quadruped_tree(), device=dev), q0=q0, v0=np.zeros((n, 18)),
                goal=np.tile(np.float32([0.2, 0.0, 0.0]), (n, 1)))


def fresh(expert, dev):
    """the expert's world with an empty database and an untrained policy"""
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    return dict(expert, db=DeviceDatabase(limit=64, norm_input=False, device=dev), policy=policy_pair(47, 12, 2, 64, False, 64, seed=3)[0])


def dagger(w, **kw):
    from iterative_learning_nmpc_amd import learning
    out = learning.dagger_iteration(w["mpc"], w["layer"], w["db"], w["policy"], w["q0"], w["v0"], w["goal"], Dagger.T, dt=Dagger.DT, n_sub=Dagger.N_SUB,
                                    n_epoch=1, batch_size=Dagger.BATCH, lr=1e-3, seed=Dagger.SEED, val_fraction=0.0, **kw)
    torch.cuda.synchronize()
    return out


def kept(out):
    """host copy of the selection of `dagger_iteration`: k < steps_survived[b] and a status that is neither NaN nor a QP failure"""
    from iterative_learning_nmpc_amd import _lib
    st, alive = out["status"].cpu().numpy(), out["steps_survived"].cpu().numpy()
    return [(b, k) for b in range(Dagger.B) for k in range(Dagger.K) if k < alive[b] and st[b, k] not in (_lib.NMPC_STATUS_NAN, _lib.NMPC_STATUS_QP)]


def tables(db):
    return [db.tables[f][:len(db)] for f in ("states", "actions", "vc_goals")] + [db.weights[:len(db)]]


def test_a_bad_store_raises_before_anything_runs(expert, dev):
    w = fresh(expert, dev)
    for store in ("noisy", "Observed", ""):
        with pytest.raises(ValueError, match="store: expected"):
            dagger(w, store=store)
    assert len(w["db"]) == 0 and w["layer"]._observed is None and w["layer"]._states is None


def test_under_a_table_of_zeros_the_two_stores_leave_the_same_database(expert, dev):
    zero = np.zeros((Dagger.B, 2 * NS), np.float32)
    w, w2 = fresh(expert, dev), fresh(expert, dev)
    true = dagger(w, noise=zero, store="true")
    seen = dagger(w2, noise=zero, store="observed")
    assert "O" not in true and same(seen["O"], seen["S"]) and same(seen["S"], true["S"])
    assert len(w["db"]) == len(w2["db"]) == true["n_rows"] > 0 and all(same(a, b) for a, b in zip(tables(w["db"]), tables(w2["db"])))
    assert same(true["train_loss"], seen["train_loss"]) and same(w["policy"].get_parameters()[0], w2["policy"].get_parameters()[0])


def test_dagger_stores_what_the_learner_saw_with_the_experts_labels(expert, dev):
    noise = np.zeros((Dagger.B, 2 * NS), np.float32)
    noise[:, 1:NS] = 0.02                                  # every sensor but the phase
    noise[1, NS + 19] = 0.01
    w = fresh(expert, dev)
    out = dagger(w, noise=noise, noise_seed=5, store="observed")
    idx = kept(out)
    print("steps survived", out["steps_survived"].tolist(), "statuses", out["status"].tolist(), "rows", out["n_rows"])
    assert out["n_rows"] == len(idx) == len(w["db"]) > 0 and w["layer"]._observed is None and w["layer"]._noise is None
    bs, ks = (torch.as_tensor(x, device=dev) for x in zip(*idx))
    states, actions, goals, weights = tables(w["db"])
    assert same(states, out["O"][bs, ks]) and not same(states, out["S"][bs, ks]) and same(states[:, 0], out["S"][bs, ks][:, 0])
    assert same(actions, out["A_star"][bs, ks]) and same(goals, torch.as_tensor(w["goal"], device=dev)[bs]) and bool((weights == 1.0).all())
    S = out["S"].cpu().numpy()
    for k in range(Dagger.K):                              # the rows the sensors showed: first_robot = 0, noise step k
        assert same(out["O"][:, k], torch.as_tensor(ir.observed_rows(S[:, k], noise, 5, 0, k), device=dev)), k
    # the labels are the expert's from the TRUE states
    A_ref, st_ref = w["mpc"].label_states(out["Q"], out["V"], w["layer"], dt_row=Dagger.N_SUB * Dagger.DT, failed=out["failed"])
    assert same(A_ref, out["A_star"]) and torch.equal(st_ref, out["status"])
