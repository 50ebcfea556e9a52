"""GPU checks of the plant-push switch of the whole-body rollouts (nmpc_wb_rollout_set_plant_push behind
`LocomotionMPC.open_loop_device(..., plant=..., push_as_force=True)`): with the switch on, every replan hands the rollout's push to
its track launch as a force, with the window moved to that replan's substeps, and the advance kernel pushes nothing.

The set-up is that of tests/test_gpu_wb_plant_rollout.py: LocomotionMPC(batch=3, force_reference="gravity_share"), a standing start
at Q_HOME, T = 0.0795 s = two replans of 40 simulation steps of 1 ms, two substeps each.  The push starts at 25 ms, inside replan
0, and ends at 55 ms, inside replan 1: in substeps of 0.5 ms the window is [50, 110), for replan 1 [-30, 30).

The reference of the comparison is the host-driven chain: per replan the rollout's own label rows through a pushed
`contact_track` (held to the pushed step in tests/test_gpu_push_track.py) and `observe_rows` on the states it went through.  The
rollout's workspaces Qw, Vw live in the solver for the call only, so their rows are compared through the rows of S made from
them (everything of a state but x, y); x, y are compared where the rollout hands a whole state out, its final q, v: of the two
replans, and of a rollout of the first replan alone, which is the state between the two."""
import numpy as np
import pytest

from tests.plant_helpers import N_SUB, ONE, STEPS, TWO
from tests.plant_helpers import default_plant as plant, expert as controller, plant_rollout, quadruped_layer, standing_start as start  # noqa: F401
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

START, DURATION = 0.025, 0.030
FIRST, COUNT = 50, 60                      # lround(START n_sub / sim_dt), lround(DURATION n_sub / sim_dt)


def the_push():
    force = np.random.default_rng(70).uniform(-80, 80, (3, 3)).astype(np.float32)
    return dict(start=START, duration=DURATION, force=force)


def rollout(mpc, L, T=TWO, **kw):
    """from the standing start, waited for, without the plans"""
    return plant_rollout(mpc, L, *start(), T, sync=True, plans=False, **kw)


def test_as_a_force_every_replan_is_the_pushed_track_of_its_label_rows(dev, quadruped_layer):
    from iterative_learning_nmpc_amd.config import COLLISION_HEIGHT
    mpc, L, push = controller(dev), quadruped_layer, the_push()
    assert mpc.replanning_steps == STEPS and len(mpc.replan_clock(TWO)[1]) == 2 and abs(mpc.sim_dt - 1e-3) < 1e-12
    assert FIRST == round(START * N_SUB / mpc.sim_dt) and COUNT == round(DURATION * N_SUB / mpc.sim_dt)
    out = rollout(mpc, L, push=push, push_as_force=True)
    assert out["S"].shape == (3, 2 * STEPS, 44) and int((out["failed"] >> 8).max()) == 0       # nobody terminated: no row is a held one
    assert L._push is None
    q0, v0 = start()
    q = torch.as_tensor(q0, dtype=torch.float32, device=L.device).contiguous()
    v = torch.as_tensor(v0, dtype=torch.float32, device=L.device).contiguous()
    F = torch.as_tensor(push["force"], device=L.device)
    period = float(mpc.config_gait.nominal_period)
    for r in range(2):
        rows = slice(r * STEPS, (r + 1) * STEPS)
        L.set_push(F, FIRST - r * STEPS * N_SUB, COUNT)
        try:
            q, v, Q, V = L.contact_track(q, v, out["A"][:, rows], mpc.sim_dt / N_SUB, N_SUB, kp=mpc.Kp, kd=mpc.Kd, ground=plant())
        finally:
            L.set_push(None)
        S = L.observe_rows(Q, V, r * STEPS * mpc.sim_dt, mpc.sim_dt, period, collision_height=COLLISION_HEIGHT)
        print(f"replan {r}: largest |rollout - chain| of its rows of S {float((S - out['S'][:, rows]).abs().max()):.3e}")
        assert same(S, out["S"][:, rows]), r
        if r == 0:      # the whole state between the replans, x and y included: the final q, v of a rollout of replan 0 alone
            first = rollout(controller(dev), L, T=ONE, push=push, push_as_force=True)
            assert same(first["S"], out["S"][:, rows]) and same(first["A"], out["A"][:, rows])
            assert same(q, first["q"]) and same(v, first["v"])
    print("final q, v:", float((q - out["q"]).abs().max()), float((v - out["v"]).abs().max()))
    assert same(q, out["q"]) and same(v, out["v"])
    # and the push is felt: not the un-pushed plant rollout, not the velocity jump
    plain = rollout(controller(dev), L)
    jump = rollout(controller(dev), L, push=push)
    assert same(plain["S"][:, :FIRST // N_SUB + 1], out["S"][:, :FIRST // N_SUB + 1])           # rows up to the first pushed step
    assert not same(plain["v"], out["v"]) and not same(jump["v"], out["v"])


def test_the_switch_off_is_the_rollout_it_was(dev, quadruped_layer):
    push = the_push()
    ref = rollout(controller(dev), quadruped_layer, T=ONE, push=dict(push, start=0.0))
    mpc = controller(dev)
    mpc.solver._device_solver().set_rollout_plant_push(False)
    got = rollout(mpc, quadruped_layer, T=ONE, push=dict(push, start=0.0))
    assert all(same(got[k], ref[k]) for k in ("S", "A", "q", "v")) and torch.equal(got["failed"], ref["failed"])
    # the velocity jump is there: the final v differs from the un-pushed rollout's
    assert not same(rollout(controller(dev), quadruped_layer, T=ONE)["v"], ref["v"])


def test_refusals(dev, quadruped_layer):
    from iterative_learning_nmpc_amd._lib import NmpcError
    push, L = the_push(), quadruped_layer
    q0, v0 = start()
    # the caller's own push on the plant's torque handle and the rollout's as a force: which one is meant
    L.set_push(torch.as_tensor(push["force"], device=L.device), 0, 4)
    try:
        with pytest.raises(NmpcError, match="push of the caller's"):
            controller(dev).open_loop_device(q0, v0, ONE, torque_layer=L, plant=plant(), plant_substeps=N_SUB, push=push, push_as_force=True)
    finally:
        L.set_push(None)
    # as a force, and no plant to push
    mpc = controller(dev)
    with pytest.raises(ValueError, match="needs the contact plant"):
        mpc.open_loop_device(q0, v0, ONE, push=push, push_as_force=True)
    s = mpc.solver._device_solver()
    s.set_rollout_plant_push(True)
    try:
        with pytest.raises(NmpcError, match="needs a plant"):
            mpc.open_loop_device(q0, v0, ONE, push=push)
    finally:
        s.set_rollout_plant_push(False)
