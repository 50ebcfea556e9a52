"""The references of tests/policy_rollout_reference.py, checked on the CPU against what they are built on: the row against the
closed-form kinematics of the whole-body model, the normalisation against the database oracle, the loop against the contact
step it is made of, the predicates against hand-made states."""
import numpy as np

from iterative_learning_nmpc_amd import wholebody
from oracle.database_oracle import DatabaseOracle
from oracle.policy_oracle import PolicyOracle
from tests import contact_reference as cr
from tests import fd_reference as fr
from tests import policy_rollout_reference as pr


def standing_like(B, seed):
    """random states around the standing pose: every base coordinate moved, joints within 0.3 rad of STAND"""
    rng = np.random.default_rng(seed)
    q = np.zeros((B, 18)); q[:, 2] = 0.3
    q[:, :6] += rng.uniform(-0.3, 0.3, (B, 6)); q[:, 6:] = fr.STAND + rng.uniform(-0.3, 0.3, (B, 12))
    return q, rng.uniform(-1, 1, (B, 18))


def standing_oracle(dtype=np.float64, n_goal=3):
    """all weights zero, last bias = STAND: the constant action"""
    o = PolicyOracle(44 + n_goal, 12, 2, 8, True, dtype)
    o.view()["b2"][:] = fr.STAND
    return o


def test_the_rows_feet_are_the_closed_form_feet_of_the_untilted_tree():
    """The untilted tree's offsets (0.19, 0.047, 0.095, 0.213, 0.213) are wholebody.GEOMETRY's: base_wrt_feet of the row equals
    the one built from wholebody.feet_position_w.  The tree is the authority for the policy rollout; the figure is printed."""
    m = fr.quadruped()
    q, v = standing_like(16, 0)
    worst = 0.0
    for b in range(16):
        r = pr.row(m, q[b], v[b], 0.25)
        closed = (q[b, :2] - wholebody.feet_position_w(q[b])[:, :2]).reshape(-1)
        worst = max(worst, np.abs(r[pr.GROUPS["base_wrt_feet"]] - closed).max())
    print(f"base_wrt_feet, tree against closed form: {worst:.2e}")
    assert worst < 1e-12


def test_the_row_has_the_layout_of_the_recorded_state():
    m = fr.quadruped(perturb=0.3)
    q, v = standing_like(1, 1)
    r = pr.row(m, q[0], v[0], pr.phase(0.8125, 0.5))
    assert r.shape == (44,) and r[0] == 0.625
    assert np.array_equal(r[1:4], v[0, :3]) and np.array_equal(r[7:19], v[0, 6:]) and r[19] == q[0, 2] and np.array_equal(r[24:36], q[0, 6:])
    assert abs(np.linalg.norm(r[20:24]) - 1) < 1e-12 and r[20] >= 0
    # at rest the rate slots are zeros; a pure roll rate is the body's x rate
    assert not np.any(pr.row(m, q[0], np.zeros(18), 0.0)[1:19])
    only_roll = np.zeros(18); only_roll[5] = 0.7
    assert np.allclose(pr.row(m, q[0], only_roll, 0.0)[4:7], [0.7, 0, 0], atol=1e-15)
    r32 = pr.row(m, q[0].astype(np.float32), v[0].astype(np.float32), 0.625, np.float32)
    assert r32.dtype == np.float32 and np.abs(r32 - r).max() < 1e-6


def test_the_normalisation_is_the_database_oracles_batch_assembly():
    m = fr.quadruped(perturb=0.3)
    B = 9
    q, v = standing_like(B, 2)
    rows = np.stack([pr.row(m, q[b].astype(np.float32), v[b].astype(np.float32), pr.phase(0.01 * b, 0.5), np.float32) for b in range(B)])
    goals = np.random.default_rng(3).uniform(-1, 1, (B, 3)).astype(np.float32)
    for norm in (True, False):
        db = DatabaseOracle(16, norm_input=norm)
        db.append(rows, np.zeros((B, 12)), vc_goals=goals)
        x = db.batch(np.arange(B))[0]
        stats = (db.states_mean, db.states_std) if norm else (None, None)
        mine = np.stack([pr.normalise(rows[b], goals[b], *stats, s_first=1, dtype=np.float32) for b in range(B)])
        assert mine.dtype == np.float32 and np.array_equal(mine, x)
    # the phase stays raw from column 1 on, and is normalised from column 0 on
    db = DatabaseOracle(16)
    db.append(rows, np.zeros((B, 12)), vc_goals=goals)
    first0 = pr.normalise(rows[1], goals[1], db.states_mean, db.states_std, s_first=0, dtype=np.float32)
    assert first0[0] == np.float32((np.float64(rows[1, 0]) - db.states_mean[0]) / db.states_std[0])
    assert pr.normalise(rows[1], goals[1], db.states_mean, db.states_std, dtype=np.float32)[0] == rows[1, 0]


def test_a_constant_action_reproduces_the_contact_step():
    """3 x 2 substeps under the standing policy are three contact steps of two substeps with q_des = STAND, exactly."""
    m, g = fr.quadruped(perturb=0.3), cr.Ground()
    q, v = standing_like(1, 4)
    q, v = q[0], v[0]
    q[2] += 0.001 - cr.feet(m, q)[0][:, 2].min()
    goal, tau = np.array([0.3, 0.0, 0.0]), np.random.default_rng(5).uniform(-2, 2, 12)
    for dtype, fd in ((np.float64, fr.fd_ref), (np.float32, fr.aba)):
        o = standing_oracle(dtype)
        S, A, q1, v1 = pr.rollout_ref(m, g, o, q, v, 3, 5e-4, 2, goal, tau_ff=tau, s_mean=np.zeros(44), s_std=np.ones(44), fd=fd, dtype=dtype)
        assert np.array_equal(A, np.tile(fr.STAND.astype(dtype), (3, 1)))
        qc, vc = np.array(q, dtype), np.array(v, dtype)
        for k in range(3):
            assert np.array_equal(S[k], pr.row(m, qc, vc, pr.phase(k * 2 * float(np.float32(5e-4)), 0.5), dtype))
            qc, vc = cr.contact_step_ref(m, g, qc, vc, 5e-4, 2, tau, fr.STAND, 20.0, 1.5, fd=fd, dtype=dtype)[:2]
        assert np.array_equal(q1, qc) and np.array_equal(v1, vc) and q1.dtype == np.dtype(dtype)
    assert S[2, 0] == 0.004


def test_the_predicates():
    m = fr.quadruped()
    up = np.zeros(18); up[2] = 0.3; up[6:] = fr.STAND
    z = np.zeros(18)

    def flags(**change):
        q = up.copy()
        for i, x in change.items():
            q[int(i[1:])] = x
        q = q.astype(np.float32)
        with np.errstate(invalid="ignore"):
            return pr.flags_ref(pr.row(m, q, z.astype(np.float32), 0.0, np.float32), q[6:], 0.08)

    assert flags() == 0
    assert flags(q5=0.5) == pr.FLAG_ROLL and flags(q5=-0.5) == pr.FLAG_ROLL and flags(q5=0.4) == 0
    assert flags(q4=-0.5) == pr.FLAG_PITCH and flags(q3=2.0) == 0
    assert flags(q2=0.5) == pr.FLAG_HEIGHT and flags(q2=0.15) == pr.FLAG_HEIGHT
    assert flags(q2=0.05) == pr.FLAG_HEIGHT | pr.FLAG_COLLISION
    assert flags(q8=-0.9) == pr.FLAG_JOINT_LIMIT and flags(q6=1.3) == pr.FLAG_JOINT_LIMIT and flags(q16=0.3) == pr.FLAG_JOINT_LIMIT
    assert flags(q2=np.nan) == pr.FLAG_SOLVER and flags(q2=np.inf) == pr.FLAG_SOLVER | pr.FLAG_HEIGHT
