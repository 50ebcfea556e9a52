"""`LocomotionMPC.label_clock`: the node and the simulation-step count of every row of a table of visited states, on the float
clock of `replan_clock`.  Host code only."""
import numpy as np
import pytest

pytest.importorskip("torch")


@pytest.fixture(scope="module")
def mpc():
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    return LocomotionMPC(print_info=False, device="cuda:0", n_nodes=30, force_reference="gravity_share")


def brute(mpc, steps):
    """the node the clock of `open_loop` shows at each of the simulation steps `steps`, one `if` per step as the loop has it"""
    sim_time, node, at = 0.0, mpc.current_opt_node, []
    for _ in range(max(steps) + 1):
        if sim_time >= (node + 1) * mpc.dt_nodes:
            node += 1
        at.append(node)
        sim_time = sim_time + mpc.sim_dt
    return [at[s] for s in steps]


def test_rows_at_the_replanning_interval_are_the_replans(mpc):
    """dt_row = replanning_steps sim_dt, t0 = 0: the nodes of `replan_clock` over the same span, and k replanning_steps steps;
    the span runs past one gait cycle, so the node passes nodes_per_cycle (it is not wrapped: the window wraps on the device)"""
    rs, npc = mpc.replanning_steps, mpc.contact_planner.nodes_per_cycle
    K = int(np.ceil((npc + 3) * mpc.dt_nodes / (rs * mpc.sim_dt))) + 1
    _, replans, _ = mpc.replan_clock(((K - 1) * rs + 0.5) * mpc.sim_dt)      # half a step of room: the clock accumulates floats
    nodes, ref_steps = mpc.label_clock(K, 0.0, rs * mpc.sim_dt)
    assert len(replans) >= K and nodes == replans[:K]
    assert ref_steps == [k * rs for k in range(K)]
    assert nodes[0] == 0 and nodes[-1] > npc and all(b >= a for a, b in zip(nodes, nodes[1:]))


def test_rows_off_the_simulation_grid_and_a_start_time(mpc):
    """a dt_row that is no multiple of sim_dt: row k sits at the nearest simulation step; t0 moves every row"""
    dt_row, K = 0.0137, 40
    nodes, ref_steps = mpc.label_clock(K, 0.0, dt_row)
    want = [int(round(k * dt_row / mpc.sim_dt)) for k in range(K)]
    assert ref_steps == want and len(set(np.diff(want))) > 1            # 13 or 14 steps apart
    assert nodes == brute(mpc, want)
    later, steps_later = mpc.label_clock(K, 0.25, dt_row)
    assert steps_later == [int(round((0.25 + k * dt_row) / mpc.sim_dt)) for k in range(K)] and later == brute(mpc, steps_later)
    assert later[0] == brute(mpc, [250])[0] > 0
    # a policy rollout's rows: n_sub dt = 20 x 0.5 ms
    nodes, ref_steps = mpc.label_clock(100, 0.0, 20 * 5e-4)
    assert ref_steps == [10 * k for k in range(100)] and nodes == brute(mpc, ref_steps)


def test_the_clock_starts_from_the_controllers_counters_and_leaves_them(mpc):
    before = (mpc.sim_step, mpc.current_opt_node, mpc.plan_step)
    mpc.current_opt_node = 7
    try:
        nodes, _ = mpc.label_clock(3, 0.0, mpc.replanning_steps * mpc.sim_dt)
        assert nodes[0] == 7 and nodes == brute(mpc, [0, mpc.replanning_steps, 2 * mpc.replanning_steps])
        assert mpc.current_opt_node == 7
    finally:
        mpc.current_opt_node = before[1]
    assert (mpc.sim_step, mpc.current_opt_node, mpc.plan_step) == before
    with pytest.raises(ValueError):
        mpc.label_clock(0, 0.0, 0.01)
    with pytest.raises(ValueError):
        mpc.label_clock(3, 0.0, 0.0)
