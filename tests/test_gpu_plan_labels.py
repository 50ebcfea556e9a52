"""Action labels on the device: nmpc_plan_actions_batch against the fp64 oracle labels (tests/test_plan_labels.py:
references.plan_rows -> oracle/torque_oracle.py -> (tau + kd v_j) / kp + q_j, none of it code that runs on the device) and
against the chain of the existing torque kernels; labels recorded by the whole-body device rollouts against the plan they
were made from; termination, batch independence, error paths; rollouts -> database (collect.collect_rollouts).

The bar, in torque units per row (BAR): kp |A - A_ref| <= 1e-5 max|tau_ref| + 4 eps32 (kp |q_j| + kd |v_j|) -- what
tests/test_gpu_torque.py holds id_torques to, plus the fp32 representation of the two addends a label adds to the torque."""
import numpy as np
import pytest

from iterative_learning_nmpc_amd.workloads import quadruped_tree
from tests.plant_helpers import expert, standing_start
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import oracle_labels

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KP, KD = 20.0, 1.5
EPS32 = float(np.finfo(np.float32).eps)
STEPS = 40                                  # replanning_steps at 25 Hz replanning and a 1 ms simulation step


def make_layer(tree, dev="cuda:0"):
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    return BatchedTorqueLayer(**tree, device=dev)


def oracle_model(tree):
    from oracle import torque_oracle as to
    return to.TreeModel.from_arrays(tree)


def bar(tau_ref, q_ref, v_ref, kp=KP, kd=KD):
    return 1e-5 * np.abs(tau_ref).max(axis=-1, keepdims=True) + 4 * EPS32 * (kp * np.abs(q_ref[..., 6:]) + kd * np.abs(v_ref[..., 6:]))


def check_labels(A, m, X, U, zoh, dt_nodes, sim_dt, what, factor=1.0, kp=KP, kd=KD):
    """A (device, fp32) against the oracle labels of the fp32 plans X, U; prints the worst ratio to the bar before asserting"""
    ref, tau, q, v = oracle_labels(m, X.cpu().numpy().astype(np.float64), U.cpu().numpy().astype(np.float64), np.asarray(zoh),
                                   dt_nodes, sim_dt, kp, kd)
    err = kp * np.abs(A.cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / bar(tau, q, v, kp, kd)).max())
    print(f"{what}: worst kp |A - A_ref| / bar = {ratio:.3f} (max |tau_ref| {np.abs(tau).max():.1f})")
    assert np.isfinite(err).all() and ratio <= factor, (what, ratio)
    return ref, tau, q, v


def plans(B, kind, dev):
    """X [B, 31, 42], U [B, 30, 30] on the device: a real solve of the whole-body workload, or random plans of that magnitude"""
    from iterative_learning_nmpc_amd import wholebody as wbk
    from iterative_learning_nmpc_amd import workloads as wl
    if kind == "solve":
        from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
        w = wl.wholebody_trot(B=B, N=30, seed=3)
        s = BatchedNmpcSolver(w.model_id, w.N, B, dev)
        s.set_model_params(w.mp); s.set_cost_weights(w.W, w.W_e, w.meta["reg"], w.meta["reg_e"])
        t = {k: s.to_device(getattr(w, k)) for k in ("x0", "yref", "yref_e", "params", "X", "U")}
        X, U, st, _ = s.solve(t["x0"], t["yref"], t["yref_e"], t["params"], t["X"], t["U"])
        assert (st.cpu().numpy() != 1).all() and bool(torch.isfinite(X).all()) and bool(torch.isfinite(U).all())
        return X, U
    rng = np.random.default_rng(B)
    X = np.zeros((B, 31, 42)); U = np.zeros((B, 30, 30))
    X[:, :, :6] = rng.uniform(-0.3, 0.3, (B, 31, 6)); X[:, :, 2] += 0.3
    X[:, :, 6:18] = wbk.Q_HOME + rng.normal(0, 0.2, (B, 31, 12))
    X[:, :, 18:36] = rng.uniform(-1, 1, (B, 31, 18))
    U[:, :, :18] = rng.uniform(-5, 5, (B, 30, 18)); U[:, :, 18:] = rng.uniform(-40, 80, (B, 30, 12))
    return (torch.as_tensor(a, dtype=torch.float32, device=dev) for a in (X, U))


def controller_zoh(N, n=STEPS):
    """the hold table as the controller makes it (`LocomotionMPC.id_repeat`): int(j / 999 * (N - 1)) -- at N = 30 zero up to
    step 34 and one from step 35 on (35 / 999 * 29 = 1.016), at N = 25 zero over all 40 steps"""
    from iterative_learning_nmpc_amd.references import zero_order_hold_index
    return zero_order_hold_index(1000, N)[:n]


@pytest.mark.parametrize("B", [1, 257, 1000])
@pytest.mark.parametrize("perturb", [0.0, 0.3])
def test_plan_actions_match_oracle_labels_and_the_kernel_chain(dev, B, perturb):
    """the kernel against the oracle labels (bar) and against id_torques -> pd_target_action on the fp32 cast of plan_rows
    (twice the bar: each side is within it of the oracle), for solved and random plans, the controller's hold table and a
    random non-decreasing one"""
    from iterative_learning_nmpc_amd import references as refs
    tree = quadruped_tree(seed=4, perturb=perturb)
    m, L = oracle_model(tree), make_layer(tree, dev)
    dt, sim_dt = 1.0 / 30, 1.0e-3
    rng = np.random.default_rng(7 + B)
    for kind in ("solve", "random"):
        X, U = plans(B, kind, dev)
        for zname, zoh in (("controller", controller_zoh(30)), ("random", np.sort(rng.integers(0, 30, STEPS)).astype(np.int32))):
            A = L.plan_actions(X, U, zoh, dt, sim_dt, KP, KD)
            assert A.shape == (B, STEPS, 12)
            ref, tau, q, v = check_labels(A, m, X, U, zoh, dt, sim_dt, f"B={B} perturb={perturb} {kind} zoh={zname}")
            qr, vr, ar, fr = (torch.as_tensor(x.reshape((B * STEPS,) + x.shape[2:]), dtype=torch.float32, device=dev)
                              for x in refs.plan_rows(X.cpu().numpy().astype(np.float64), U.cpu().numpy().astype(np.float64), zoh, dt, sim_dt))
            chain = L.pd_target_action(L.id_torques(qr, vr, ar, fr), qr, vr, KP, KD).reshape(B, STEPS, 12)
            d = KP * np.abs((A - chain).cpu().numpy().astype(np.float64))
            ratio = float((d / bar(tau, q, v)).max())
            print(f"   against the kernel chain: worst ratio {ratio:.3f}")
            assert ratio <= 2.0
    # skip flags leave a rollout's rows alone; the actuator permutation moves torques, not joints
    if B == 257:
        skip = torch.zeros(B, dtype=torch.int32, device=dev); skip[5] = 4; skip[6] = 2
        out = torch.full((B, STEPS, 12), -7.0, dtype=torch.float32, device=dev)
        L.plan_actions(X, U, zoh, dt, sim_dt, KP, KD, skip=skip, skip_mask=4, out=out)
        assert bool((out[5] == -7.0).all()) and torch.equal(out[6], A[6]) and torch.equal(out[:5], A[:5]) and torch.equal(out[7:], A[7:])
        perm = [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]
        Ap = L.plan_actions(X, U, zoh, dt, sim_dt, KP, KD, actuator_to_joint=perm).cpu().numpy().astype(np.float64)
        want = (tau[..., perm] + KD * v[..., 6:]) / KP + q[..., 6:]
        assert (KP * np.abs(Ap - want) <= bar(tau, q, v)).all()
        # that list is its own inverse: a scatter through it is the same array.  A rotation is not, and its inverse lies far off
        turn = [(i + 5) % 12 for i in range(12)]
        back = [(i + 7) % 12 for i in range(12)]
        assert all(back[turn[i]] == i for i in range(12)) and sum(turn[turn[i]] != i for i in range(12)) >= 8
        At = L.plan_actions(X, U, zoh, dt, sim_dt, KP, KD, actuator_to_joint=turn).cpu().numpy().astype(np.float64)
        want = (tau[..., turn] + KD * v[..., 6:]) / KP + q[..., 6:]
        apart = float(np.median(np.abs(tau[..., back] - tau[..., turn]) / bar(tau, q, v)))
        print(f"   rotated actuators: worst ratio {float((KP * np.abs(At - want) / bar(tau, q, v)).max()):.3f}; the inverse a median of {apart:.1e} bars apart")
        assert apart > 1e3
        assert (KP * np.abs(At - want) <= bar(tau, q, v)).all()


def _controller(B, dev):
    mpc = expert(dev, B, n_nodes=30)
    mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
    return mpc


def _start(B, seed=2):
    from iterative_learning_nmpc_amd import wholebody as wbk
    rng = np.random.default_rng(seed)
    q0 = standing_start(B)[0]; q0[:, 6:] += rng.normal(0, 0.03, (B, 12))
    return rng, q0, np.zeros((B, 18))


def test_rollout_labels_match_the_plan_they_were_made_from(dev):
    """one replanning interval per call (T = 0.0395: the float clock runs exactly 40 steps and one replan), four calls in a
    row: after each, mpc._X_dev / _U_dev are that replan's plan and mpc.actions must be its oracle labels (the 15-SQP
    first solve and three warm-started replans); then one call over four replans: rows 0..40 are the single-interval call's
    bit for bit, the last 40 rows are the labels of the final plan, every row is finite"""
    tree = quadruped_tree()
    m, L = oracle_model(tree), make_layer(tree, dev)
    _, q0, v0 = _start(3)
    mpc = _controller(3, dev)
    assert mpc.replanning_steps == STEPS
    steps, nodes, _ = mpc.replan_clock(0.0395)
    assert steps == STEPS and len(nodes) == 1
    dt = mpc.config_opt.time_horizon / mpc.config_opt.n_nodes
    zoh = mpc.id_repeat[:STEPS]
    q, v, first = q0, v0, None
    for call in range(4):
        assert mpc.replan_clock(0.0395)[0] == STEPS and len(mpc.replan_clock(0.0395)[1]) == 1
        S = mpc.open_loop_device(q, v, 0.0395, torque_layer=L, kp=KP, kd=KD)
        assert S.shape == (3, STEPS, 44) and mpc.actions.shape == (3, STEPS, 12) and int((mpc.failed & 1).sum()) == 0
        _, _, qr, _ = check_labels(mpc.actions, m, mpc._X_dev, mpc._U_dev, zoh, dt, mpc.sim_dt, f"rollout labels, call {call}")
        # the state under a label is the state of its row: joints of S (slots 24..36) are the fp32 cast of the same fp64 sample
        assert np.array_equal(S[:, :, 24:36].cpu().numpy(), qr[..., 6:].astype(np.float32))
        if call == 0:
            first = mpc.actions.clone()
        q, v = mpc.q_final.cpu().numpy(), mpc.v_final.cpu().numpy()
    long = _controller(3, dev)
    steps, nodes, _ = long.replan_clock(0.1595)
    assert steps == 4 * STEPS and len(nodes) == 4
    long.open_loop_device(q0, v0, 0.1595, torque_layer=L, kp=KP, kd=KD)
    A = long.actions
    assert A.shape == (3, 4 * STEPS, 12) and bool(torch.isfinite(A).all())
    assert torch.equal(A[:, :STEPS], first)
    check_labels(A[:, -STEPS:], m, long._X_dev, long._U_dev, zoh, dt, long.sim_dt, "last interval of four replans")


# The pushed batch below ends no rollout under the default terminate mask (solver failure | trunk on the ground): its rollouts
# raise velocity-tracking, height and joint-limit flags only (16, 24, 80), on the parent commit as well, and rollout 1, pushed
# down at 70 N, leaves the height band but recovers above the collision height.  The reference's simulator ends a rollout on
# any of its unsafe-state predicates (check_unsafe_state_v2, Rollout_combined_controller.py:367-431), so the tests that need a
# terminated rollout run the batch with the posture predicates in the mask as well: height, roll, pitch.
def _terminate():
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    return TERMINATE_DEFAULT | _lib.NMPC_ROLLOUT_FLAG_HEIGHT | _lib.NMPC_ROLLOUT_FLAG_ROLL | _lib.NMPC_ROLLOUT_FLAG_PITCH


@pytest.fixture(scope="module")
def pushed(dev):
    """the pushed batch of test_wholebody_device_rollouts_batch_and_termination (B = 24, T = 0.8, rollout 1 pushed down at
    70 N), rows per simulation step, through collect_rollouts (rollout 0, unpushed, is the nominal)"""
    from iterative_learning_nmpc_amd.collect import collect_rollouts
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    B, T = 24, 0.8
    rng, q0, v0 = _start(B)
    force = rng.uniform(-1, 1, (B, 3)); force /= np.linalg.norm(force, axis=1, keepdims=True); force *= rng.uniform(50, 70, (B, 1))
    force[0] = 0.0
    force[1] = [0.0, 0.0, -70.0]
    push = dict(start=0.2, duration=0.3, force=force)
    L = make_layer(quadruped_tree(), dev)
    mpc = _controller(B, dev)
    db = DeviceDatabase(limit=32768, device=dev)
    err, weights, n_rows = collect_rollouts(mpc, L, db, q0, v0, T, push=push, nominal=0, ood_weight=5.0, terminate_mask=_terminate())
    torch.cuda.synchronize()
    return dict(B=B, T=T, q0=q0, v0=v0, push=push, force=force, L=L, mpc=mpc, db=db, err=err, weights=weights, n_rows=n_rows)


def test_labels_change_nothing_else(dev, pushed):
    """the same rollout without a label buffer: S, failed, X, U are the same bits"""
    p = pushed
    plain = _controller(p["B"], dev)
    S = plain.open_loop_device(p["q0"], p["v0"], p["T"], push=p["push"], terminate_mask=_terminate())
    assert not hasattr(plain, "actions")
    assert torch.equal(S, p["mpc"].states) and torch.equal(plain.failed, p["mpc"].failed)
    assert torch.equal(plain._X_dev, p["mpc"]._X_dev) and torch.equal(plain._U_dev, p["mpc"]._U_dev)


def test_terminated_rollouts_hold_their_last_label_and_batches_are_independent(dev, pushed):
    p = pushed
    S, A, f = p["mpc"].states.cpu().numpy(), p["mpc"].actions.cpu().numpy(), p["mpc"].failed.cpu().numpy()
    term = np.nonzero(f >> 8)[0]
    print("terminated rollouts", term, "at replans", (f[term] >> 8) - 1)
    assert len(term) >= 1 and len(term) < p["B"], f                  # not vacuous: some end early, some run through
    assert (f & 1 == 0).all() and np.isfinite(A).all()
    for b in term:
        i = (f[b] >> 8) * STEPS - 1
        assert i < A.shape[1] - 1
        assert (A[b, i:] == A[b, i]).all() and (S[b, i:] == S[b, i]).all()
    for b in np.nonzero((f >> 8) == 0)[0][:4]:                       # a rollout that ran on keeps changing
        assert not (A[b, -1] == A[b, -STEPS - 1]).all()
    n = 3
    small = _controller(n, dev)
    small.open_loop_device(p["q0"][:n], p["v0"][:n], p["T"], push=dict(p["push"], force=p["force"][:n]), torque_layer=p["L"],
                           terminate_mask=_terminate())
    assert np.array_equal(small.actions.cpu().numpy(), A[:n]) and np.array_equal(small.failed.cpu().numpy(), f[:n])


def test_collect_rollouts_fills_the_database(dev, pushed):
    from iterative_learning_nmpc_amd.solver import tracking_error
    p = pushed
    mpc, db = p["mpc"], p["db"]
    S, A = mpc.states, mpc.actions
    K = S.shape[1]
    valid = (mpc.failed & _terminate()) == 0
    n_valid = int(valid.sum())
    assert 0 < n_valid < p["B"] and p["n_rows"] == n_valid * K and len(db) == n_valid * K
    assert torch.equal(db.tables["states"][:len(db)], S[valid].reshape(-1, 44))
    assert torch.equal(db.tables["actions"][:len(db)], A[valid].reshape(-1, 12))
    goal = torch.tensor([0.2, 0.0, 0.0], dtype=torch.float32, device=dev)
    assert torch.equal(db.tables["vc_goals"][:len(db)], goal.expand(len(db), 3))
    err_ref, _ = tracking_error(S.contiguous(), S[0].contiguous(), 4.0)
    assert torch.equal(p["err"], err_ref)
    w = p["weights"]
    assert w.shape == p["err"].shape and bool((w[~valid] == 0).all())
    assert bool(((w[valid] == 1.0) | (w[valid] == 5.0)).all()) and bool((w[valid][p["err"][valid] > 4.0] == 5.0).all())


def test_label_error_paths_leave_the_handle_usable(dev):
    from iterative_learning_nmpc_amd._lib import NmpcError
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    L = make_layer(quadruped_tree(), dev)
    _, q0, v0 = _start(3)
    mpc = _controller(3, dev)
    with pytest.raises(NmpcError, match="record_sim_steps"):
        mpc.open_loop_device(q0, v0, 0.0395, record_sim_steps=False, torque_layer=L)
    n = 23                                                            # a chain of 23 revolute joints: not the whole-body tree
    eye = np.tile(np.eye(3).reshape(9), (n, 1))
    chain = BatchedTorqueLayer(list(range(-1, n - 1)), [0] * n, np.tile([0.0, 0.0, 1.0], (n, 1)), eye, np.tile([0.1, 0.0, 0.0], (n, 1)),
                               np.ones(n), np.zeros((n, 3)), np.tile([1.0, 0, 0, 1.0, 0, 1.0], (n, 1)), [n - 1], np.zeros((1, 3)), 12, device=dev)
    with pytest.raises(NmpcError, match="n_joints"):
        mpc.open_loop_device(q0, v0, 0.0395, torque_layer=chain)
    X, U = plans(3, "random", dev)
    with pytest.raises(NmpcError, match="n_steps"):
        L.plan_actions(X, U, np.zeros(0, np.int32), 1.0 / 30, 1.0e-3)
    with pytest.raises(NmpcError, match="n_joints"):
        chain.plan_actions(X, U, np.zeros(STEPS, np.int32), 1.0 / 30, 1.0e-3)
    # the refused calls launched nothing and left no label buffer behind: the same controller now does what a fresh one does
    S = mpc.open_loop_device(q0, v0, 0.0395, torque_layer=L)
    fresh = _controller(3, dev)
    Sf = fresh.open_loop_device(q0, v0, 0.0395, torque_layer=L)
    assert torch.equal(S, Sf) and torch.equal(mpc.actions, fresh.actions) and torch.equal(mpc.failed, fresh.failed)
    plain = _controller(3, dev)
    assert torch.equal(plain.open_loop_device(q0, v0, 0.0395), S)
