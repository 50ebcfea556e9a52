"""tests/rollout_step_reference.py before it judges a kernel: its restatement of `build_problem` for an arbitrary contact table
against `BatchedLocomotionMPC.build_problem` (golden-pinned planners) on the configured gaits, and its small tools.  No GPU."""
import numpy as np
import pytest

from tests import rollout_step_reference as R


def _case(gait_name, N, node, footsteps, height_offset, seed):
    rng = np.random.default_rng(seed)
    B = 6
    m = R.host_mpc(B, gait_name, N, height_offset, footsteps)
    x = rng.normal(0, 0.3, (B, 12)); x[:, 2] = 0.3 + rng.normal(0, 0.05, B); x[:, 3] = rng.uniform(-3, 3, B)
    x[0, 2] = height_offset - 0.01                                         # a base below the ground
    m.v_des, m.w_des = rng.normal(0, 0.3, (B, 3)), rng.normal(0, 0.3, (B, 3))
    m.base_ref_vel_tracking = rng.normal(0, 0.5, (B, 12))
    m.foot_pos = rng.normal(0, 0.3, (B, 4, 3))
    m.current_opt_node = node
    return m, x


@pytest.mark.parametrize("gait_name,N", [("trot", 50), ("trot", 20), ("slow_trot", 50)])
@pytest.mark.parametrize("footsteps", [False, True])
def test_restatement_equals_build_problem_on_the_configured_gaits(gait_name, N, footsteps):
    npc = R.host_mpc(1, gait_name, N).contact_planner.nodes_per_cycle
    for node in (0, 1, npc // 2, npc // 2 + 1, npc - 1, npc, 3 * npc + 5):
        m, x = _case(gait_name, N, node, footsteps, 0.05 if node % 2 else 0.0, node)
        want = m.build_problem(x)
        got = R.build_problem(m.contact_planner.gait_sequence, node, N, x, m.v_des, m.w_des, m.base_ref_vel_tracking, m.foot_pos,
                              weight=-m.mp[5] * m.mp[1], t_horizon=m.config_opt.time_horizon, nom_height=m.config_gait.nom_height,
                              height_offset=m.height_offset, footsteps=footsteps, period=m.config_gait.nominal_period,
                              stance_ratio=m.config_gait.stance_ratio, hip_offset=m.raibert.offset_hip_b[:, :2],
                              foot_size=m.raibert.foot_size)
        for name, g, w in zip(("yref", "yref_e", "params"), got, want):
            assert g.shape == w.shape and np.isfinite(w).all()
            assert np.array_equal(g[..., :4] if name == "params" else g[..., 12:], w[..., :4] if name == "params" else w[..., 12:]), (name, node)
            # the hip offset is rotated entry by entry here and by a matrix product there: a rounding or two of fp64 apart
            assert np.abs(g - w).max() <= 4 * np.finfo(float).eps * max(1.0, np.abs(w).max()), (name, node, np.abs(g - w).max())
        if footsteps:
            assert np.abs(want[2][:, :, 4:]).max() > 0.1                   # the window holds touch-downs: the planner was at work


def test_touch_downs_are_read_cyclically():
    gait = np.array([[0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1]], np.int8)
    c, make = R.contact_window(gait, 3, 6)                                 # columns 3 0 1 2 3 0
    assert np.array_equal(c[0], [0, 0, 1, 1, 0, 0]) and np.array_equal(make[0], [0, 0, 1, 0, 0, 0])
    assert not make[1].any() and not make[2].any()                         # always standing, never standing: no touch-down
    assert np.array_equal(c[3], [1, 1, 0, 0, 1, 1]) and np.array_equal(make[3], [1, 0, 0, 0, 1, 0])   # column 3 follows a swing column
    _, make0 = R.contact_window(gait, 0, 2)
    assert np.array_equal(make0[3], [0, 0])                                # column 0's predecessor is column 3, across the wrap: standing


def test_a_foot_standing_through_the_window_is_not_anchored():
    gait = np.array([[1, 1, 1, 1], [1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 1, 1]], np.int8)
    x = np.zeros((1, 12)); x[0, :3] = [1.0, 2.0, 0.3]
    foot = np.arange(12.0).reshape(1, 4, 3) + 1
    loc = R.foot_locations(gait, 0, 5, x, foot, np.zeros((1, 3)), np.zeros((1, 3)), dt_nodes=0.2, period=0.5, stance_ratio=[0.5] * 4,
                           hip_offset=np.zeros((4, 2)), height_offset=0.0, foot_size=0.01)[0]
    assert (loc[:, 0] == 0).all()                                          # stands throughout: argmin = 0, nothing is kept
    assert (loc[:2, 1] == foot[0, 1]).all() and (loc[2, 1] == 0).all() and np.array_equal(loc[3, 1], [1.0, 2.0, 0.01])
    assert (loc[:, 2] == 0).all()                                          # never stands
    assert (loc[0, 3] == 0).all() and np.array_equal(loc[1, 3], [1.0, 2.0, 0.01])


def test_ulps_counts_floats():
    one = np.float32(1.0)
    assert R.ulps([one, -one, 0.0], [np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), -0.0]).tolist() == [1, 1, 0]
    tiny = np.nextafter(np.float32(0), one)
    assert R.ulps([tiny], [-tiny])[0] == 2 and R.ulps([np.nan], [0.0])[0] > 1 << 30


def test_fp32_rows_follow_the_fp64_rows():
    rng = np.random.default_rng(0)
    m = R.host_mpc(3, "trot", 50, record_sim_steps=True)
    X = rng.normal(0, 0.3, (3, 51, 12)).astype(np.float32).astype(np.float64)
    params = np.zeros((3, 51, 16)); params[:, :, :4] = rng.integers(0, 2, (3, 51, 4)); params[:, :, 4:] = rng.normal(0, 0.3, (3, 51, 12))
    params = R.widen(params)
    m.foot_pos = R.widen(rng.normal(0, 0.3, (3, 4, 3)))
    want = m.sim_step_rows(X, params, 0)[:, :, 1:]
    got = R.sim_rows_fp32(X, params, m.foot_pos, True, dt_nodes=m.dt_nodes, sim_dt=m.sim_dt, steps=m.replanning_steps)
    assert got.dtype == np.float32 and np.abs(got - want).max() < 2e-5 * np.abs(want).max() and np.abs(got - want).max() > 0
