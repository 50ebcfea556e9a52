"""GPU checks of the whole-body expert in closed loop on the ground-contact plant (nmpc_wb_rollout_set_plant behind
`LocomotionMPC.open_loop_device(..., plant=GroundContact())`).

A plant-mode replan is labels -> track -> observe, each a public call of the torque layer, so the reference of every comparison
is the chain of those calls through the Python layer and the bar is equality of the bit patterns.  The controller is
LocomotionMPC(batch=3, force_reference="gravity_share") with the default 25 nodes and the trot, from a standing start at Q_HOME;
T = 0.0395 s makes the float clock of `replan_clock` run exactly one replan of 40 simulation steps (0.0795: two, ...).

Measured on the MI355X at B = 64 over 1 s (DESIGN.md 8h has the table), the standing expert stays inside every fall predicate on
this plant -- the base settles from 0.300 m to 0.242 m, inside the height band [0.18, 0.45] --, so the standing test asserts
survival under the reference's predicates, not only finite rows."""
import numpy as np
import pytest

from tests.plant_helpers import FIVE, N_SUB, ONE, SHIFT, SOLVER, STEPS, THREE, TWO
from tests.plant_helpers import chain_of_public_calls, default_plant as plant, expert as controller, plant_rollout as rollout  # noqa: F401
from tests.plant_helpers import quadruped_layer, standing_start as start  # noqa: F401
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import bits, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HEIGHT, COLLISION = 8, 32                                 # bits of `failed`
SENTINEL = -77.0


@pytest.fixture(scope="module")
def one(dev, quadruped_layer):
    """one replan from the standing start: shared by the tests that compare with it"""
    mpc = controller(dev)
    q0, v0 = start()
    assert mpc.replanning_steps == STEPS and mpc.replan_clock(ONE)[0] == STEPS and len(mpc.replan_clock(ONE)[1]) == 1
    out = rollout(mpc, quadruped_layer, q0, v0, ONE)
    torch.cuda.synchronize()
    return dict(out, mpc=mpc, q0=q0, v0=v0)


# ---- 1. one replan is the chain of public calls -------------------------------------------------------------------------------------
def test_one_replan_is_the_chain_of_public_calls(quadruped_layer, one):
    o = one
    S, A, q, v, failed = chain_of_public_calls(o["mpc"], quadruped_layer, o["X"], o["U"], o["q0"], o["v0"], o["status"])
    got = (o["S"], o["A"], o["q"], o["v"])
    print("one replan: largest |rollout - chain| of S, A, q, v:", [float((a - b).abs().max()) for a, b in zip(got, (S, A, q, v))],
          "failed", o["failed"].tolist(), "chain", failed.tolist(), "status", o["status"].tolist())
    assert o["S"].shape == (3, STEPS, 44) and o["A"].shape == (3, STEPS, 12)
    assert all(same(a, b) for a, b in zip(got, (S, A, q, v)))
    assert torch.equal(o["failed"], failed)
    assert bool(torch.isfinite(o["S"]).all()) and bool(torch.isfinite(o["A"]).all())
    # row 0 is the state the rollout started from, before any simulation step: z and the joints of the start state
    assert same(o["S"][:, 0, 19], torch.as_tensor(o["q0"][:, 2], dtype=torch.float32, device=quadruped_layer.device))
    assert same(o["S"][:, 0, 24:36], torch.as_tensor(o["q0"][:, 6:], dtype=torch.float32, device=quadruped_layer.device))
    # and it is not the plan-following rollout
    plain = controller(quadruped_layer.device)
    assert not same(plain.open_loop_device(o["q0"], o["v0"], ONE), o["S"])


# ---- 2. replans in one call and in several --------------------------------------------------------------------------------------------
def test_three_replans_in_one_call_start_as_one_replan_does(dev, quadruped_layer, one):
    """Three replans in one call against calls of one replan.  The harness has no bit-for-bit continuation across calls, with
    or without a plant: the host's float clock (`replan_clock`) restarts with every call, so three calls of one replan solve at
    the optimisation nodes [0, 0, 0] where one call of three solves at [0, 1, 2], and the recorded phase and the push window
    start at the call.  Measured on the MI355X: across the three calls ref_state and failed agree, S, A, q, v, X, U do not.
    What holds, and is asserted: replan 0 of the long call is the one-replan call bit for bit in S and A, and the state that
    replan leaves is the same -- row STEPS of the long call is the observation of the short call's final q, v."""
    from iterative_learning_nmpc_amd.config import COLLISION_HEIGHT
    q0, v0 = one["q0"], one["v0"]
    long = controller(dev)
    steps, nodes, _ = long.replan_clock(THREE)
    assert steps == 3 * STEPS and nodes == [0, 1, 2]
    lo = rollout(long, quadruped_layer, q0, v0, THREE)
    assert lo["S"].shape == (3, 3 * STEPS, 44) and lo["A"].shape == (3, 3 * STEPS, 12)
    assert same(lo["S"][:, :STEPS], one["S"]) and same(lo["A"][:, :STEPS], one["A"])
    row = quadruped_layer.observe_rows(one["q"][:, None, :], one["v"][:, None, :], STEPS * long.sim_dt, long.sim_dt, float(long.config_gait.nominal_period),
                             collision_height=COLLISION_HEIGHT)
    assert same(row[:, 0], lo["S"][:, STEPS])
    assert bool(torch.isfinite(lo["S"]).all()) and bool(torch.isfinite(lo["A"]).all()) and int((lo["failed"] >> SHIFT).max()) == 0
    assert not same(lo["S"][:, STEPS:2 * STEPS, 1:], lo["S"][:, :STEPS, 1:])           # the later replans move on
    # the reason the calls cannot be compared further: a second call of one replan starts its clock again
    assert one["mpc"].replan_clock(ONE)[1] == [0]


# ---- 3. termination -------------------------------------------------------------------------------------------------------------------
def test_a_robot_on_the_ground_terminates_and_freezes_and_the_others_do_not_notice(dev, quadruped_layer):
    q0, v0 = start()
    healthy = rollout(controller(dev), quadruped_layer, q0, v0, THREE)
    low = q0.copy(); low[1, 2] = 0.05
    got = rollout(controller(dev), quadruped_layer, low, v0, THREE)
    first = rollout(controller(dev), quadruped_layer, low, v0, ONE)
    f = got["failed"].cpu().numpy()
    print("robot 1 starts at 0.05 m: failed", f, "stamps", f >> SHIFT)
    assert f[1] & COLLISION and (f[1] >> SHIFT) == 1
    assert same(got["S"][1, :STEPS], first["S"][1]) and same(got["A"][1, :STEPS], first["A"][1])
    assert bool((bits(got["S"][1, STEPS:]) == bits(got["S"][1, STEPS - 1])).all())          # later rows are held
    assert bool((bits(got["A"][1, STEPS:]) == bits(got["A"][1, STEPS - 1])).all())
    assert same(got["q"][1], first["q"][1]) and same(got["v"][1], first["v"][1])             # the plant is frozen where that interval left it
    for b in (0, 2):
        assert all(same(got[k][b], healthy[k][b]) for k in ("S", "A", "q", "v", "X", "U")) and f[b] == healthy["failed"][b].item()


# ---- 4. the last interval is observed ---------------------------------------------------------------------------------------------------
def test_a_robot_that_falls_in_the_last_interval_is_seen(dev, quadruped_layer):
    """A robot thrown upwards from z = 0.43 m leaves the height band [0.18, 0.45] at a time that grows as the speed falls; the
    speed at which it does so between the last recorded row (the state before step 39) and the state after step 39 is found
    by bisection on the rollout itself, three speeds per try (a ballistic base crosses at 0.31 m/s with 0.70 m/s at the start:
    0.3 mm per step, a window of speeds 8e-3 m/s wide; six tries resolve 1.5e-4 m/s)."""
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    mask = TERMINATE_DEFAULT | HEIGHT
    q0, v0 = start()
    q0[:, 2] = 0.43
    lo, hi, found = 0.4, 1.0, None
    for attempt in range(6):
        speeds = lo + (hi - lo) * np.array([0.25, 0.5, 0.75])
        v = v0.copy(); v[:, 2] = speeds
        out = rollout(controller(dev), quadruped_layer, q0, v, ONE, terminate_mask=mask)
        z_rows, z_end, f = out["S"][:, :, 19].cpu().numpy(), out["q"][:, 2].cpu().numpy(), out["failed"].cpu().numpy()
        above = (z_rows > 0.45).sum(1) + (z_end > 0.45)
        print(f"try {attempt}: speeds {speeds}, states above the band {above}, final z {z_end}, failed {f}")
        hit = [b for b in range(3) if above[b] == 1 and z_end[b] > 0.45]
        if hit:
            found = (hit[0], z_rows, f)
            break
        if above[0] > 1: hi = speeds[0]
        elif above[1] > 1: lo, hi = speeds[0], speeds[1]
        elif above[2] > 1: lo, hi = speeds[1], speeds[2]
        else: lo = speeds[2]
    assert found is not None, "no speed found that leaves the band in the last step"
    b, z_rows, f = found
    assert (z_rows[b] >= 0.18).all() and (z_rows[b] <= 0.45).all() and not f[b] & SOLVER       # safe at every recorded row
    assert f[b] & HEIGHT and (f[b] >> SHIFT) == 1                                               # n_replans = 1


# ---- 5. detaching, refusals -----------------------------------------------------------------------------------------------------------
def test_detach_restores_the_plan_following_rollout(dev, quadruped_layer):
    q0, v0 = start()
    mpc = controller(dev)
    s = mpc.solver._device_solver()
    s.set_rollout_plant(quadruped_layer, plant(), N_SUB, mpc.Kp, mpc.Kd, s.to_device(mpc.id_repeat[:STEPS], torch.int32))
    s.set_rollout_plant(None)
    S = mpc.open_loop_device(q0, v0, TWO, torque_layer=quadruped_layer)
    fresh = controller(dev)
    Sf = fresh.open_loop_device(q0, v0, TWO, torque_layer=quadruped_layer)
    assert same(S, Sf) and same(mpc.actions, fresh.actions) and torch.equal(mpc.failed, fresh.failed)
    assert same(mpc.q_final, fresh.q_final) and same(mpc._X_dev, fresh._X_dev) and same(mpc._U_dev, fresh._U_dev)


def test_refusals_launch_nothing(dev, quadruped_layer, one):
    from iterative_learning_nmpc_amd._lib import NmpcError
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    q0, v0 = one["q0"], one["v0"]
    mpc = controller(dev)
    s = mpc.solver._device_solver()
    rows, io = [], s._rollout_io

    def sentinel_io(*a):                                          # the S of the call, pre-filled: a refused call leaves it as it is
        S, failed = io(*a)
        S.fill_(SENTINEL)
        rows.append(S)
        return S, failed
    s._rollout_io = sentinel_io

    def refused(match, **kw):
        n = len(rows)
        args = dict(torque_layer=quadruped_layer, plant=plant(), plant_substeps=N_SUB)
        args.update(kw)
        with pytest.raises(NmpcError, match=match):
            mpc.open_loop_device(q0, v0, ONE, **args)
        torch.cuda.synchronize()
        assert len(rows) == n + 1 and bool((rows[-1] == SENTINEL).all()), match
    refused("record_sim_steps", record_sim_steps=False)
    refused("n_sub must be at least 1", plant_substeps=0)
    n = 23                                                        # a chain of 23 revolute joints: not the whole-body tree
    eye = np.tile(np.eye(3).reshape(9), (n, 1))
    chain = BatchedTorqueLayer(list(range(-1, n - 1)), [0] * n, np.tile([0.0, 0.0, 1.0], (n, 1)), eye, np.tile([0.1, 0.0, 0.0], (n, 1)),
                               np.ones(n), np.zeros((n, 3)), np.tile([1.0, 0, 0, 1.0, 0, 1.0], (n, 1)), [n - 1], np.zeros((1, 3)), 12, device=dev)
    refused("n_joints", torque_layer=chain)
    refused("slip_velocity must be positive", plant=GroundContact(slip_velocity=0.0))
    refused("must be finite", plant=GroundContact(stiffness=float("inf")))
    attach = s.set_rollout_plant                                  # labels attached with other gains than the plant's
    s.set_rollout_plant = lambda L, *a: attach(L, a[0], a[1], a[2], a[3] + 0.25) if L is not None else attach(None)
    refused("gains")
    s.set_rollout_plant = attach
    # the refused calls left nothing behind: the same controller now does what a fresh one did
    s._rollout_io = io
    out = rollout(mpc, quadruped_layer, q0, v0, ONE)
    assert all(same(out[k], one[k]) for k in ("S", "A", "q", "v", "X", "U")) and torch.equal(out["failed"], one["failed"])


# ---- 6. collection, standing ----------------------------------------------------------------------------------------------------------
def test_collect_rollouts_on_the_plant_fills_the_database(dev, quadruped_layer):
    from iterative_learning_nmpc_amd.collect import collect_rollouts
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    q0, v0 = start()
    low = q0.copy(); low[1, 2] = 0.05                             # one rollout is invalid
    mpc = controller(dev)
    db = DeviceDatabase(limit=4096, device=dev)
    err, weights, n_rows = collect_rollouts(mpc, quadruped_layer, db, low, v0, TWO, plant=plant(), plant_substeps=N_SUB)
    S, A = mpc.states, mpc.actions
    K = S.shape[1]
    valid = (mpc.failed & TERMINATE_DEFAULT) == 0
    print("collect on the plant: valid", valid.tolist(), "rows", n_rows)
    assert K == 2 * STEPS and valid.tolist() == [True, False, True] and n_rows == 2 * K and len(db) == 2 * K
    assert torch.equal(db.tables["states"][:len(db)], S[valid].reshape(-1, 44))
    assert torch.equal(db.tables["actions"][:len(db)], A[valid].reshape(-1, 12))
    reference = rollout(controller(dev), quadruped_layer, low, v0, TWO)
    assert same(S, reference["S"]) and same(A, reference["A"])
    assert bool((weights[~valid] == 0).all()) and err.shape == (3, K)


def test_the_standing_expert_survives_on_the_plant(dev, quadruped_layer):
    """the standing case of the measured table at B = 3, T = 0.2 s (5 replans), under the predicates of that table: solver,
    collision, height band [0.18, 0.45] m, roll and pitch within 25 degrees.  The B = 64, 1 s run survives entirely."""
    from iterative_learning_nmpc_amd.config import TERMINATE_DEFAULT
    mask = TERMINATE_DEFAULT | HEIGHT | 2 | 4
    q0, v0 = start()
    mpc = controller(dev)
    assert len(mpc.replan_clock(FIVE)[1]) == 5
    out = rollout(mpc, quadruped_layer, q0, v0, FIVE, terminate_mask=mask)
    f = out["failed"].cpu().numpy()
    z = out["S"][:, :, 19]
    survived = (f >> SHIFT) == 0
    print(f"standing, B = 3, T = 0.2 s: failed {f}, stamps {f >> SHIFT}, base height {float(z.min()):.4f} .. {float(z.max()):.4f} m, "
          f"survived {survived.tolist()}")
    assert out["S"].shape == (3, 5 * STEPS, 44)
    assert bool(torch.isfinite(out["S"]).all()) and bool(torch.isfinite(out["A"]).all())
    assert bool(torch.isfinite(out["q"]).all()) and bool(torch.isfinite(out["v"]).all())
    assert survived.all() and not (f & mask).any()
