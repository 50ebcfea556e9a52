"""The host clock of `LocomotionMPC.open_loop_device` resumes: stretches of whole replanning intervals, run one after the other
from the stored float time, replan at the nodes of one run over all of them; what cannot be continued is refused before
anything touches a device.  No GPU: the controller is constructed and its clock is run, nothing is solved."""
import numpy as np
import pytest

from iterative_learning_nmpc_amd import wholebody as wb
from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC


@pytest.fixture(scope="module")
def controller():
    return LocomotionMPC(print_info=False, n_nodes=30)


def run_stretches(mpc, stretches):
    """what `open_loop_device` does with the clock over these stretches: the first a cold start, the others resumed"""
    mpc.reset(reset_solver=False)
    nodes = []
    for i, k in enumerate(stretches):
        steps, n, node_end, time_end = mpc.replan_clock_intervals(k, resume=i > 0)
        assert steps == k * mpc.replanning_steps and len(n) == k
        nodes += n
        mpc.sim_step += steps
        mpc.sim_time, mpc.clock_step = time_end, (mpc.clock_step if i else 0) + steps
        mpc.current_opt_node = node_end
    return nodes, mpc.current_opt_node, mpc.sim_time, mpc.sim_step


@pytest.mark.parametrize("stretches", [(2, 3, 1), (5, 5, 3)], ids=["6", "13_past_one_cycle"])
def test_resumed_stretches_replan_at_the_nodes_of_one_run(controller, stretches):
    mpc = controller
    total = sum(stretches)
    one = run_stretches(mpc, (total,))
    cut = run_stretches(mpc, stretches)
    assert cut[0] == one[0] and cut[1:] == one[1:]          # the nodes, the last node, the float time (the same double), the steps
    if total == 13:                                        # the case is what it claims: the rollout is longer than a gait cycle
        assert total * mpc.replanning_steps * mpc.sim_dt > mpc.config_gait.nominal_period
    # ... and they are `replan_clock`'s over the same steps: its loop runs while sim_time <= T, T half a step short of the end
    mpc.reset(reset_solver=False)
    steps, nodes, node_end = mpc.replan_clock((total * mpc.replanning_steps - 0.5) * mpc.sim_dt)
    assert (steps, nodes, node_end) == (one[3], one[0], one[1])


def test_a_restarted_clock_differs_from_a_resumed_one(controller):
    """the thing the feature is about: three cold calls of one replan start their float time at 0 each, and the node, which
    passes a node time only on that float time, falls behind"""
    mpc = controller
    mpc.reset(reset_solver=False)
    nodes = []
    for _ in range(3):
        steps, n, node_end, _ = mpc.replan_clock_intervals(1, resume=False)
        nodes += n
        mpc.sim_step += steps
        mpc.current_opt_node = node_end
    assert run_stretches(mpc, (1, 1, 1))[0] == run_stretches(mpc, (3,))[0] == [0, 1, 2]
    assert nodes == [0, 1, 1]


def test_resume_without_n_replans_is_refused(controller):
    mpc = controller
    mpc.reset(reset_solver=False)
    q0 = np.concatenate([[0.0, 0.0, 0.27, 0.0, 0.0, 0.0], wb.Q_HOME])
    with pytest.raises(ValueError, match="n_replans"):
        mpc.open_loop_device(q0, np.zeros(18), 0.1, resume=True)
    with pytest.raises(ValueError, match="one of them"):
        mpc.open_loop_device(q0, np.zeros(18))
    with pytest.raises(ValueError, match="one of them"):
        mpc.open_loop_device(q0, np.zeros(18), 0.1, n_replans=2)


def test_resume_after_a_call_that_ended_inside_an_interval_is_refused(controller):
    mpc = controller
    mpc.reset(reset_solver=False)
    # the books a `trajectory_time` call leaves: replan_clock(0.1) stops 20 steps into the third interval
    steps, nodes, node_end = mpc.replan_clock(0.1)
    assert steps % mpc.replanning_steps != 0
    mpc.sim_step += steps
    mpc.clock_step, mpc.current_opt_node = steps, node_end
    q0 = np.concatenate([[0.0, 0.0, 0.27, 0.0, 0.0, 0.0], wb.Q_HOME])
    with pytest.raises(ValueError, match="interval boundary"):
        mpc.open_loop_device(q0, np.zeros(18), n_replans=2, resume=True)
    with pytest.raises(ValueError, match="interval boundary"):
        mpc.replan_clock_intervals(2, resume=True)
    assert (mpc.sim_step, mpc.clock_step, mpc.current_opt_node) == (steps, steps, node_end)      # a refusal changes nothing


def test_reset_zeroes_the_stored_time(controller):
    mpc = controller
    run_stretches(mpc, (2,))
    assert mpc.sim_time > 0.0 and mpc.clock_step == 2 * mpc.replanning_steps
    mpc.reset(reset_solver=False)
    assert mpc.sim_time == 0.0 and mpc.clock_step == 0 and mpc.sim_step == 0


def test_replan_clock_is_what_it_was(controller):
    """existing callers: the float time starts at 0 whatever is stored, and nothing is stored by it"""
    mpc = controller
    run_stretches(mpc, (2,))
    before = (mpc.sim_time, mpc.clock_step, mpc.sim_step, mpc.current_opt_node)
    steps, nodes, node_end = mpc.replan_clock(0.1)
    assert steps % mpc.replanning_steps == 20 and len(nodes) == 3
    assert (mpc.sim_time, mpc.clock_step, mpc.sim_step, mpc.current_opt_node) == before
