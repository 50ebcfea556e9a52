"""GPU checks of the push windows per rollout in the device rollouts (nmpc_wb_rollout_set_push_windows and
nmpc_rollout_set_push_windows behind `open_loop_device(push={"start": [B], "duration": [B], ...})`): rollout b of a call with
windows attached is held bit for bit to rollout b of the same call -- same B, same row -- whose scalar window is b's.

The whole-body set-up is that of tests/test_gpu_push_plant_rollout.py: LocomotionMPC(batch=4, force_reference="gravity_share"), a
standing start at Q_HOME, three replans of 40 simulation steps of 1 ms, on the plant two substeps each.  Rollout 0 is pushed in
replan 0, rollout 1 in replan 1, rollout 2 over replans 1 and 2, rollout 3 not at all."""
import numpy as np
import pytest

from tests.plant_helpers import N_SUB, STEPS, default_plant as plant, expert, held_row_by_row, quadruped_layer, standing_start  # noqa: F401
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import rows_equal, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, REPLANS = 4, 3
# the velocity jump acts per replanning interval of 40 ms: windows that open at a replan
JUMP = dict(start=np.array([0.0, 0.04, 0.04, 0.02]), duration=np.array([0.03, 0.03, 0.05, 0.0]))
# the force acts per substep of 0.5 ms: windows that open and close inside the intervals
FORCE = dict(start=np.array([0.0125, 0.045, 0.03, 0.02]), duration=np.array([0.02, 0.03, 0.06, 0.0]))


def controller(dev):
    return expert(dev, B)


def start():
    return standing_start(B)


def force():
    return np.random.default_rng(70).uniform(-80, 80, (B, 3)).astype(np.float32)


def rollout(dev, L, push, n_replans=REPLANS, mpc=None, resume=False, **kw):
    mpc = controller(dev) if mpc is None else mpc
    q0, v0 = (mpc.q_final, mpc.v_final) if resume else start()
    S = mpc.open_loop_device(q0, v0, None, n_replans=n_replans, resume=resume, torque_layer=L, push=push, **kw)
    torch.cuda.synchronize()
    return dict(S=S, actions=mpc.actions, q=mpc.q_final, v=mpc.v_final, failed=mpc.failed)


def held_rollout_by_rollout(dev, L, windows, keys, **kw):
    """the rollout under the windows per rollout against the rollout under the scalar window of each: the push is an argument of
    the call, so "attaching" sets the one the next call is made with"""
    use = {}
    attach = lambda: use.update(push=dict(windows, force=force()))      # noqa: E731
    attach_window_of = lambda b: use.update(push=dict(use["push"], start=float(windows["start"][b]), duration=float(windows["duration"][b])))      # noqa: E731
    plain = rollout(dev, L, None, **kw)
    got, moved = held_row_by_row(lambda: rollout(dev, L, use["push"], **kw), attach, attach_window_of, range(B), keys,
                                 lambda b, k: f"rollout {b} {k}: largest |windowed - uniform|", plain=plain, moved_by=("v",))
    assert got["S"].shape == (B, REPLANS * STEPS, 44)
    # the pushes are felt, and the rollout without one is its row of the un-pushed run
    assert moved == [True, True, True, False]
    assert rows_equal(got, plain, 3, keys)
    return got


def test_velocity_jumps_per_rollout_are_the_uniform_runs(dev, quadruped_layer):
    mpc = controller(dev)
    assert mpc.replanning_steps == STEPS and abs(mpc.sim_dt - 1e-3) < 1e-12
    held_rollout_by_rollout(dev, quadruped_layer, JUMP, ("S", "failed", "q", "v"))


@pytest.mark.parametrize("integrator", ["explicit", "implicit"])
def test_forces_on_the_plant_per_rollout_are_the_uniform_runs(dev, quadruped_layer, integrator):
    kw = dict(plant=plant(), plant_substeps=N_SUB, push_as_force=True, integrator=integrator)
    try:
        held_rollout_by_rollout(dev, quadruped_layer, FORCE, ("S", "failed", "q", "v", "actions"), **kw)
    finally:
        quadruped_layer.set_integrator("explicit")
    assert quadruped_layer._push is None and quadruped_layer._push_windows is None


def test_velocity_jumps_on_the_plant_per_rollout_are_the_uniform_runs(dev, quadruped_layer):
    held_rollout_by_rollout(dev, quadruped_layer, JUMP, ("S", "failed", "q", "v", "actions"), plant=plant(), plant_substeps=N_SUB)


def test_resumed_stretches_with_windows_are_the_rows_of_the_one_call(dev, quadruped_layer):
    kw = dict(plant=plant(), plant_substeps=N_SUB, push_as_force=True)
    push = dict(FORCE, force=force())
    one = rollout(dev, quadruped_layer, push, **kw)
    mpc = controller(dev)
    first = rollout(dev, quadruped_layer, push, n_replans=2, mpc=mpc, **kw)
    second = rollout(dev, quadruped_layer, push, n_replans=1, mpc=mpc, resume=True, **kw)
    for k in ("S", "actions"):
        assert same(torch.cat([first[k], second[k]], 1), one[k]), k
    assert same(second["q"], one["q"]) and same(second["v"], one["v"]) and torch.equal(second["failed"], one["failed"])
    # and the velocity jump on the same clock
    one = rollout(dev, quadruped_layer, dict(JUMP, force=force()))
    mpc = controller(dev)
    first = rollout(dev, quadruped_layer, dict(JUMP, force=force()), n_replans=2, mpc=mpc)
    second = rollout(dev, quadruped_layer, dict(JUMP, force=force()), n_replans=1, mpc=mpc, resume=True)
    assert same(torch.cat([first["S"], second["S"]], 1), one["S"]) and same(second["v"], one["v"])


def test_rollout_refusals(dev, quadruped_layer):
    from iterative_learning_nmpc_amd._lib import NmpcError
    mpc = controller(dev)
    s = mpc.solver._device_solver()
    q0, v0 = start()
    # windows attached and no push_force
    s.set_rollout_push_windows(JUMP["start"], JUMP["duration"])
    try:
        with pytest.raises(NmpcError, match="no push_force"):
            mpc.open_loop_device(q0, v0, None, n_replans=1)
    finally:
        s.set_rollout_push_windows(None)
    # fewer windows than rollouts
    s.set_rollout_push_windows(JUMP["start"][:3], JUMP["duration"][:3])
    try:
        with pytest.raises(NmpcError, match="B exceeds rows"):
            mpc.open_loop_device(q0, v0, None, n_replans=1, push=dict(start=0.0, duration=0.01, force=force()))
    finally:
        s.set_rollout_push_windows(None)
    with pytest.raises(ValueError, match="come together"):
        s.set_rollout_push_windows(JUMP["start"], None)
    with pytest.raises(ValueError, match="one per rollout"):
        mpc.open_loop_device(q0, v0, None, n_replans=1, push=dict(start=JUMP["start"][:3], duration=0.01, force=force()))
    # the centroidal entry point on a whole-body handle, and only one pointer
    assert s.lib.nmpc_rollout_set_push_windows(s._h, None, None, 0) == -1
    t = torch.zeros(4, device=s.device)
    assert s.lib.nmpc_wb_rollout_set_push_windows(s._h, t.data_ptr(), None, 4) == -1 and b"come together" in s.lib.nmpc_last_error(s._h)
    assert s.lib.nmpc_wb_rollout_set_push_windows(s._h, t.data_ptr(), t.data_ptr(), 0) == -1 and b"rows must be" in s.lib.nmpc_last_error(s._h)
    # nothing was left attached: the rollout runs
    mpc.open_loop_device(q0, v0, None, n_replans=1)


def test_centroidal_velocity_jumps_per_rollout_are_the_uniform_runs(dev):
    from iterative_learning_nmpc_amd.mpc import BatchedLocomotionMPC

    def run(push):
        mpc = BatchedLocomotionMPC(B, n_nodes=50, device=dev, footsteps=True)
        mpc.set_command(np.zeros(3), 0.0)
        x0 = np.zeros((B, 12)); x0[:, 2] = 0.3
        dtr = mpc.replanning_steps * mpc.sim_dt
        if push is not None:
            push = dict(push, start=np.asarray(push["start"]) * dtr, duration=np.asarray(push["duration"]) * dtr)
            if push["start"].ndim == 0:
                push.update(start=float(push["start"]), duration=float(push["duration"]))
        S, _ = mpc.open_loop_device(x0, REPLANS * dtr, push)
        torch.cuda.synchronize()
        assert S.shape[0] == B
        return dict(S=S, failed=mpc.failed, x=mpc.x_final)

    # in replanning intervals: replan 0, replan 1, replans 1 and 2, none
    starts, durations = np.array([0.0, 1.0, 1.0, 0.5]), np.array([0.6, 0.6, 1.6, 0.0])
    F = force().astype(np.float64) * 0.5
    got, plain = run(dict(start=starts, duration=durations, force=F)), run(None)
    keys, moved = ("S", "failed", "x"), []
    for b in range(B):
        ref = run(dict(start=starts[b], duration=durations[b], force=F))
        assert rows_equal(got, ref, b, keys), b
        moved.append(not rows_equal(ref, plain, b, ("x",)))
    assert moved == [True, True, True, False] and rows_equal(got, plain, 3, keys)


def test_collection_with_windows_appends_the_rows_and_weights_of_the_uniform_runs(dev, quadruped_layer):
    from iterative_learning_nmpc_amd.collect import collect_rollouts
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    T = (REPLANS * STEPS - 0.5) * 1.0e-3              # the float clock runs three whole intervals
    # Rollout 0 is the nominal one every error is measured against, so it has to be the same rollout under every window: its
    # force is zero, and the push is the velocity jump, where a zero force adds +0 to v and is no push.  (As a force it would
    # not do: a pushed substep under a zero force is not the un-pushed substep bit for bit)
    F = force(); F[0] = 0.0
    kw = dict(nominal=0, plant=plant(), plant_substeps=N_SUB)

    def collect(push, **more):
        mpc, db = controller(dev), DeviceDatabase(limit=1024, norm_input=False, device=dev)
        err, weights, n_rows = collect_rollouts(mpc, quadruped_layer, db, *start(), T, push=push, **kw, **more)
        torch.cuda.synchronize()
        return dict(err=err, weights=weights, n_rows=n_rows, failed=mpc.failed, db=db)

    got = collect(dict(JUMP, force=F))
    cut = collect(dict(JUMP, force=F), chunk_replans=2)
    assert got["err"].shape == (B, REPLANS * STEPS)
    assert same(cut["err"], got["err"]) and same(cut["weights"], got["weights"]) and cut["n_rows"] == got["n_rows"]
    rows = 0
    for b in range(B):
        ref = collect(dict(start=float(JUMP["start"][b]), duration=float(JUMP["duration"][b]), force=F))
        assert rows_equal(got, ref, b, ("err", "weights", "failed")), b
        assert float(ref["err"][b].max()) > 0.0 or b in (0, 3)        # the pushed rollouts leave the nominal one
        rows += STEPS * REPLANS if float(ref["weights"][b].max()) > 0 else 0      # an invalid rollout has weight 0 and appends nothing
    assert got["n_rows"] == len(got["db"]) == rows
