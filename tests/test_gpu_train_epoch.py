"""Device-resident policy training (include/nmpc_policy.h: nmpc_policy_train_epoch, nmpc_policy_loss; database weights;
learning.train_network / learning_iteration).

The bar of the epoch call is BIT IDENTITY with the chain of the entry points it fuses -- weighted_sample -> db.batch ->
train_step -- since it runs the same device functions on the same numbers in the same order.  Against the numpy oracles
the bars are the ones tests/test_gpu_policy.py holds the single step to (its measured fp32 floors)."""
import numpy as np
import pytest

from iterative_learning_nmpc_amd.workloads import quadruped_tree
from tests.plant_helpers import expert, standing_start
from tests.solve_helpers import policy_pair, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LR = 1e-3
NET_A = (47, 12, 3, 512, True)              # the reference's network (cfgs/iter_locosafedagger.yaml)

# name -> (network, database widths (n_state, n_vc, n_cc, n_action), goal type, norm_input, n_rows, batch, n_batches)
CASES = {
    "A": (NET_A, (44, 3, 8, 12), "vc", True, 300, 64, 3),
    "B": ((9, 4, 2, 65, False), (6, 3, 8, 4), "vc", False, 100, 33, 4),             # tile remainders, no BatchNorm, raw rows
    "C": (NET_A, (39, 3, 8, 12), "cc", True, 2048 + 77, 1000, 2),                   # normalised goals; the CDF crosses a scan chunk
}
_made = {}


def case(name):
    """(network dims, DeviceDatabase, the arrays it was filled with, weights on the device and as numpy, batch, n_batches);
    made once per module, never changed by a test"""
    if name not in _made:
        from iterative_learning_nmpc_amd.database import DeviceDatabase
        net, (n_state, n_vc, n_cc, n_action), goal_type, norm, n, batch, n_batches = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        s = (rng.normal(0, 2, n_state) + np.exp(rng.uniform(-2, 1, n_state)) * rng.standard_normal((n, n_state))).astype(np.float32)
        s[:, 0] = np.round(rng.uniform(0, 1, n), 4)
        rows = dict(states=s, actions=rng.standard_normal((n, n_action)).astype(np.float32),
                    vc_goals=rng.uniform(-0.5, 0.5, (n, n_vc)).astype(np.float32),
                    cc_goals=rng.uniform(-0.3, 0.3, (n, n_cc)).astype(np.float32))
        db = DeviceDatabase(n + 5, n_state=n_state, n_action=n_action, n_vc_goal=n_vc, n_cc_goal=n_cc, norm_input=norm,
                            goal_type=goal_type)
        db.append(rows["states"], rows["actions"], vc_goals=rows["vc_goals"], cc_goals=rows["cc_goals"])
        w = np.where(rng.random(n) < 0.15, 5.0, 1.0).astype(np.float32)
        _made[name] = (net, db, rows, torch.tensor(w, device=db.device), w, batch, n_batches)
    return _made[name]


def policy(net, batch_max, seed=3):
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    return DevicePolicy(*net, batch_max=batch_max, seed=seed)


def chain(pol, db, w, batch, n_batches, seed, lr=LR):
    """the existing entry points, one after the other: (losses [n_batches], idx [n_batches, batch])"""
    from iterative_learning_nmpc_amd.policy import weighted_sample
    idx = weighted_sample(w, n_batches * batch, seed).reshape(n_batches, batch)
    losses = [pol.train_step(*db.batch(idx[t].contiguous()), lr) for t in range(n_batches)]
    return torch.cat(losses), idx


def state(pol):
    return [t.cpu().numpy() for t in pol.get_parameters()]


def same_bits(a, b):
    return np.array_equal(np.asarray(a.cpu() if hasattr(a, "cpu") else a), np.asarray(b.cpu() if hasattr(b, "cpu") else b))


def assert_same_state(pol_a, pol_b, what):
    for name, a, b in zip(("theta", "running_mean", "running_var"), state(pol_a), state(pol_b)):
        assert np.array_equal(a, b), (what, name, int((a != b).sum()), float(np.abs(a - b).max()))


def assert_same_optimizer_state(pol_a, pol_b, what, steps):
    """Adam's moments and step count (nmpc_policy_get_opt_state), bit for bit; `steps`: the count both must have reached"""
    (ma, va, sa), (mb, vb, sb) = pol_a.get_optimizer_state(), pol_b.get_optimizer_state()
    assert sa == sb == steps, (what, sa, sb, steps)
    for name, a, b in (("m", ma, mb), ("v", va, vb)):
        assert same_bits(a, b), (what, name, int((a != b).sum()))
    assert bool((va > 0).any()) or steps == 0


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_epoch_equals_the_chain_of_entry_points_bit_for_bit(name):
    net, db, _, w, _, batch, n_batches = case(name)
    fused, ref = policy(net, batch), policy(net, batch)
    seed = 1234567891011
    losses, idx = fused.train_epoch(db, batch, n_batches, LR, seed, weights=w, return_idx=True)
    losses_ref, idx_ref = chain(ref, db, w, batch, n_batches, seed)
    assert idx.shape == (n_batches, batch) and idx.dtype == torch.int32 and same_bits(idx, idx_ref)
    assert same_bits(losses, losses_ref), (losses, losses_ref)
    assert_same_state(fused, ref, "one epoch")
    assert_same_optimizer_state(fused, ref, "one epoch", n_batches)
    # two more calls on the same handle: the optimiser's step count (the Adam bias corrections) carries over
    for nb, s in ((2, 77), (1, 2 ** 40 + 5)):
        losses, idx = fused.train_epoch(db, batch, nb, LR, s, weights=w, return_idx=True)
        losses_ref, idx_ref = chain(ref, db, w, batch, nb, s)
        assert same_bits(idx, idx_ref) and same_bits(losses, losses_ref)
    assert_same_state(fused, ref, "three epochs in a row")
    assert_same_optimizer_state(fused, ref, "three epochs in a row", n_batches + 3)
    assert bool(torch.isfinite(losses).all())
    # without idx_out, and with the database's own weight column as the default
    a, b = policy(net, batch), policy(net, batch)
    la = a.train_epoch(db, batch, 2, LR, 5)
    lb, _ = chain(b, db, db.weights[:len(db)], batch, 2, 5)
    assert same_bits(la, lb)
    assert_same_state(a, b, "default weights")
    assert_same_optimizer_state(a, b, "default weights", 2)
    assert a.train_epoch(db, batch, 0, LR, 5).shape == (0,)                    # no batches: nothing happens
    assert_same_state(a, b, "empty epoch")
    assert_same_optimizer_state(a, b, "empty epoch", 2)


# ---------------------------------------------------------------------------------------------- 2
def test_epoch_matches_the_numpy_oracles():
    """DatabaseOracle + oracle weighted_sample + PolicyOracle.train_step, two batches of case A; bounds: those of
    test_policy_forward_and_train_step_match_oracle (loss 1e-5 at step 0, 2e-3 at step 1, x max(1, loss); parameters with a
    strong gradient within 2e-5 after step 0, all within 2.01 lr)"""
    from oracle.database_oracle import DatabaseOracle
    from oracle.policy_oracle import weighted_sample as oracle_sample
    net, db, rows, w, w_np, batch, _ = case("A")
    seed = 424242
    do = DatabaseOracle(db.limit)
    do.append(*(rows[f].astype(np.float64) for f in ("states", "actions")), vc_goals=rows["vc_goals"].astype(np.float64),
              cc_goals=rows["cc_goals"].astype(np.float64))
    idx_o = oracle_sample(w_np, 2 * batch, seed).reshape(2, batch)
    one, o = policy_pair(*net, batch_max=batch)                   # stopped after step 0: the parameter bounds are step 0's
    two, _ = policy_pair(*net, batch_max=batch)
    l1, i1 = one.train_epoch(db, batch, 1, LR, seed, weights=w, return_idx=True)
    l2, i2 = two.train_epoch(db, batch, 2, LR, seed, weights=w, return_idx=True)
    assert np.array_equal(i2.cpu().numpy(), idx_o) and np.array_equal(i1.cpu().numpy(), idx_o[:1])
    assert same_bits(l1, l2[:1])
    for step in range(2):
        xo, yo = do.batch(idx_o[step])
        lo, _, go = o.train_step(xo.astype(np.float64), yo.astype(np.float64), LR)
        got = float(l2[step].item())
        print(f"step {step}: loss {got:.7f} oracle {lo:.7f} |diff| {abs(got - lo):.2e}")
        assert abs(got - lo) < (1e-5 if step == 0 else 2e-3) * max(1.0, lo)
        if step == 0:
            th, rm, rv = state(one)
            d = np.abs(th - o.theta)
            strong = np.abs(go) > 1e-2 * np.abs(go).max()
            print(f"step 0: parameters with a strong gradient {d[strong].max():.2e}, all {d.max():.2e}")
            assert d[strong].max() < 2e-5, d[strong].max()
            assert d.max() <= 2.01 * LR
            assert rel(rv, o.running_var) < 1e-5 and rel(rm, o.running_mean) < 1e-5


# ---------------------------------------------------------------------------------------------- 3
def test_zero_weight_rows_are_never_drawn_and_validate_the_epochs():
    from iterative_learning_nmpc_amd.learning import train_network
    net, db, _, w, _, batch, _ = case("A")
    n = len(db)
    held = np.r_[0, 100:198, n - 1]                         # a third of the rows: the first, the last, a run of neighbours
    assert len(held) == n // 3
    wz = w.clone(); wz[torch.as_tensor(held, device=w.device)] = 0.0
    pol = policy(net, batch)
    _, idx = pol.train_epoch(db, batch, 4, LR, 99, weights=wz, return_idx=True)
    drawn = np.unique(idx.cpu().numpy())
    assert not np.intersect1d(drawn, held).size and drawn.min() >= 0 and drawn.max() < n
    assert len(drawn) > 50                                   # 256 draws over 200 rows: not stuck on a few of them
    # train_network holds the same rows out by the same means; its validation loss after epoch e is the loss of a second run
    # that stops there, spelled out with the entry points
    weights_before = db.weights.clone()
    val_idx = torch.as_tensor(held, dtype=torch.int32, device=db.device)
    n_epoch, seed = 2, 17
    train_loss, val_loss = train_network(policy(net, batch), db, n_epoch, batch, lr=LR, seed=seed, val_idx=val_idx)
    n_batches = -(-(n - len(held)) // batch)
    assert train_loss.shape == (n_epoch, n_batches) and val_loss.shape == (n_epoch,)
    assert torch.equal(db.weights, weights_before)
    x_val, y_val = db.batch(val_idx)
    w_train = db.weights[:n].clone(); w_train[val_idx.long()] = 0.0
    again = policy(net, batch)
    for e in range(n_epoch):
        losses = again.train_epoch(db, batch, n_batches, LR, seed + e, weights=w_train)
        assert same_bits(losses, train_loss[e])
        assert same_bits(again.loss(x_val, y_val), val_loss[e:e + 1])
    assert bool(torch.isfinite(val_loss).all())
    # without validation rows: every row trains, the validation loss is NaN
    t2, v2 = train_network(policy(net, batch), db, 1, batch, lr=LR, seed=seed)
    assert t2.shape == (1, -(-n // batch)) and bool(torch.isnan(v2).all())


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [1, 64, 150])
def test_validation_loss_matches_the_oracle_and_touches_nothing(n):
    """batch_max = 64: one short chunk, one full chunk, three chunks with a short last one.  Bound: 1e-5 relative, the
    eval-forward bound of test_policy_forward_and_train_step_match_oracle."""
    pol, o = policy_pair(*NET_A, batch_max=64)
    twin, _ = policy_pair(*NET_A, batch_max=64)
    rng = np.random.default_rng(n)
    X, Y = rng.standard_normal((n, 47)), rng.standard_normal((n, 12))
    x, y = (torch.tensor(a, dtype=torch.float32, device=pol.device) for a in (X, Y))
    want = float(np.abs(o.forward(x.cpu().numpy().astype(np.float64), train=False) - y.cpu().numpy().astype(np.float64)).mean())
    before = state(pol)
    first, second = pol.loss(x, y), pol.loss(x, y)
    print(f"n = {n}: loss {first.item():.7f} oracle {want:.7f} relative error {abs(first.item() - want) / want:.2e}")
    assert first.shape == (1,) and abs(first.item() - want) < 1e-5 * want
    assert same_bits(first, second)
    for a, b in zip(before, state(pol)):
        assert np.array_equal(a, b)
    # no cache of the training pass was disturbed: the next step is the step of a policy that never evaluated
    xt, yt = (torch.tensor(rng.standard_normal((64, k)), dtype=torch.float32, device=pol.device) for k in (47, 12))
    for step in range(2):
        la, lb = pol.train_step(xt, yt, LR), twin.train_step(xt, yt, LR)
        assert same_bits(la, lb)
        pol.loss(x, y)
    assert_same_state(pol, twin, "training around loss calls")


# ---------------------------------------------------------------------------------------------- 5
def test_the_weight_column_rides_the_ring(tmp_path):
    from iterative_learning_nmpc_amd.database import FIELDS, DeviceDatabase
    rng = np.random.default_rng(0)
    db = DeviceDatabase(limit=10, n_state=5, n_action=2)
    assert db.weights.shape == (10,) and db.weights.dtype == torch.float32
    assert "weights" not in db.tables and "weights" not in db.widths and "weights" not in FIELDS
    for n in (7, 6):                                         # the second append wraps and moves the start
        s = rng.standard_normal((n, 5)).astype(np.float32)
        db.append(s, rng.standard_normal((n, 2)).astype(np.float32), vc_goals=np.zeros((n, 3), np.float32), weights=s[:, 0].copy())
    assert (db.start, db.length) == (3, 10)
    assert torch.equal(db.weights, db.tables["states"][:, 0])
    db.append(rng.standard_normal((2, 5)).astype(np.float32), np.zeros((2, 2), np.float32), vc_goals=np.zeros((2, 3), np.float32),
              weights=torch.tensor([2.0, 3.0], device=db.device))                  # device weights; slots 3 and 4
    assert db.weights[3:5].tolist() == [2.0, 3.0]
    with pytest.raises(ValueError, match="weights"):
        db.append(np.zeros((2, 5), np.float32), np.zeros((2, 2), np.float32), vc_goals=np.zeros((2, 3), np.float32), weights=np.ones(3))
    plain = DeviceDatabase(limit=10, n_state=5, n_action=2)
    plain.append(rng.standard_normal((4, 5)).astype(np.float32), np.zeros((4, 2), np.float32), vc_goals=np.zeros((4, 3), np.float32))
    assert plain.weights.tolist() == [1.0] * 4 + [0.0] * 6
    out = str(tmp_path / "db.npz")
    plain.save_as_npz(out)
    assert sorted(np.load(out).files) == sorted(FIELDS)
    loaded = DeviceDatabase(limit=10, n_state=5, n_action=2)
    loaded.load_from_npz(out)
    assert len(loaded) == 4 and loaded.weights[:4].tolist() == [1.0] * 4


# ---------------------------------------------------------------------------------------------- 6
# The rollout setup of tests/test_gpu_plan_labels.py (test_collect_rollouts_fills_the_database): B = 24 whole-body rollouts of
# 0.8 s, rollout 0 unpushed (the nominal), rollout 1 pushed down at 70 N, the posture predicates in the terminate mask so that
# some rollouts end early and are left out.
def _controller(B, dev):
    mpc = expert(dev, B, n_nodes=30)
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    return mpc


def _start(B, seed=2):
    rng = np.random.default_rng(seed)
    q0 = standing_start(B)[0]; q0[:, 6:] += rng.normal(0, 0.03, (B, 12))
    return rng, q0, np.zeros((B, 18))


def _terminate():
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    return TERMINATE_DEFAULT | _lib.NMPC_ROLLOUT_FLAG_HEIGHT | _lib.NMPC_ROLLOUT_FLAG_ROLL | _lib.NMPC_ROLLOUT_FLAG_PITCH


def _iteration(dev):
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    from iterative_learning_nmpc_amd.learning import learning_iteration
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    B, T = 24, 0.8
    rng, q0, v0 = _start(B)
    force = rng.uniform(-1, 1, (B, 3)); force /= np.linalg.norm(force, axis=1, keepdims=True); force *= rng.uniform(50, 70, (B, 1))
    force[0] = 0.0
    force[1] = [0.0, 0.0, -70.0]
    layer = BatchedTorqueLayer(**quadruped_tree(), device=dev)
    mpc = _controller(B, dev)
    db = DeviceDatabase(limit=32768, device=dev)
    pol = policy(NET_A, 64)
    out = learning_iteration(mpc, layer, db, pol, q0, v0, T, push=dict(start=0.2, duration=0.3, force=force), nominal=0,
                             ood_weight=5.0, terminate_mask=_terminate(), n_epoch=1, batch_size=64, lr=LR, seed=7, val_fraction=0.1)
    torch.cuda.synchronize()
    return mpc, db, pol, out


def test_one_joined_learning_iteration():
    dev = torch.device("cuda:0")
    mpc, db, pol, (err, weights, n_rows, train_loss, val_loss) = _iteration(dev)
    K = mpc.states.shape[1]
    valid = (mpc.failed & _terminate()) == 0
    n_valid = int(valid.sum())
    assert 0 < n_valid < 24 and n_rows == n_valid * K == len(db)
    assert torch.equal(db.weights[:n_rows], weights[valid].reshape(-1))
    n_val = int(0.1 * n_rows)
    assert n_val > 0 and bool((db.weights[n_rows - n_val:n_rows] > 0).all())      # the zeroing worked on a copy
    print("appended rows with the out-of-distribution weight:", int((weights[valid] == 5.0).sum()), "of", n_rows)
    assert train_loss.shape == (1, -(-(n_rows - n_val) // 64)) and val_loss.shape == (1,)
    assert bool(torch.isfinite(train_loss).all()) and bool(torch.isfinite(val_loss).all())
    assert all(np.isfinite(a).all() for a in state(pol))
    x_val, y_val = db.batch(torch.arange(n_rows - n_val, n_rows, dtype=torch.int32, device=dev))
    assert same_bits(pol.loss(x_val, y_val), val_loss)
    # a second identical run from fresh objects: the same bits
    mpc2, db2, pol2, out2 = _iteration(dev)
    assert out2[2] == n_rows and same_bits(out2[3], train_loss) and same_bits(out2[4], val_loss)
    assert torch.equal(db2.weights, db.weights)
    assert_same_state(pol, pol2, "two identical iterations")


# ---------------------------------------------------------------------------------------------- 7
def test_error_paths_leave_the_handle_usable():
    """each refusal is NMPC_E_ARG with a message in the handle's error slot, launches nothing and moves no counter: the next
    epoch on the handle is the chain's, bit for bit"""
    from iterative_learning_nmpc_amd._lib import NmpcError
    net, db, _, w, _, batch, _ = case("A")
    pol, ref = policy(net, batch), policy(net, batch)

    def refused(match, **over):
        args = dict(batch_size=batch, n_batches=2, lr=LR, seed=0, weights=w)
        args.update(over)
        with pytest.raises(NmpcError, match=r"\(-1\)") as e:
            pol.train_epoch(db, **args)
        msg = pol.lib.nmpc_policy_last_error(pol._h)
        assert msg and match in msg.decode() and match in str(e.value), msg

    def still_good(seed):
        losses, idx = pol.train_epoch(db, batch, 2, LR, seed, weights=w, return_idx=True)
        losses_ref, idx_ref = chain(ref, db, w, batch, 2, seed)
        assert same_bits(idx, idx_ref) and same_bits(losses, losses_ref)
        assert_same_state(pol, ref, f"after refusal {seed}")

    refused("batch_max", batch_size=batch + 1)
    still_good(1)
    db.set_goal_type("cc")                                   # 44 + 8 columns for a network of 47 inputs
    try:
        refused("n_in")
    finally:
        db.set_goal_type("vc")
    still_good(2)
    refused("BatchNorm", batch_size=1)
    still_good(3)
    refused("learning rate", lr=0.0)
    still_good(4)
    with pytest.raises(NmpcError, match="n >= 1"):
        pol.loss(torch.zeros(0, 47, device=pol.device), torch.zeros(0, 12, device=pol.device))
    still_good(5)
