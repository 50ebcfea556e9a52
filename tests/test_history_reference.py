"""The numpy restatement of the history on the policy input (tests/history_reference.py) against its closed form and against the
database oracle's assembly.  No GPU.

Every word of a wide row is a copy, so the chained pushes are compared with the closed form as bit patterns; the normalised columns
are the oracle's own fp64 expression on the same float32 words and are compared as bit patterns too."""
import numpy as np
import pytest

from oracle.database_oracle import DatabaseOracle
from tests import history_reference as hr

B, K, NS, NU = 3, 6, 44, 12
DEPTHS = [(1, 0), (3, 2), (2, 5), (16, 16)]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(11)
    O = rng.normal(0.0, 1.5, (B, K, NS)).astype(np.float32)
    O[:, :, 5] = -0.0                                     # a sign bit that a copy keeps and an arithmetic pass may lose
    A = rng.uniform(-1.0, 1.0, (B, K, NU)).astype(np.float32)
    S0 = rng.normal(0.0, 1.5, (B, NS)).astype(np.float32)
    posture = rng.uniform(-1.0, 1.0, (B, NU)).astype(np.float32)
    for x in (O, A, S0, posture):
        x.setflags(write=False)
    return O, A, S0, posture


@pytest.mark.parametrize("n_obs,n_act", DEPTHS)
def test_chained_pushes_are_the_closed_form(rows, n_obs, n_act):
    O, A, S0, posture = rows
    W, hist, act = hr.chained(O, A, S0, posture, n_obs, n_act)
    want = hr.closed_form(O, A, S0, posture, n_obs, n_act)
    assert W.shape == (B, K, hr.width(n_obs, n_act)) and np.array_equal(bits(W), bits(want))
    # the observed rows: slot 0 keeps the row that came in last, slot h holds the row of h - 1 steps before it after the ageing
    assert np.array_equal(bits(hist[:, 0]), bits(O[:, K - 1]))
    for h in range(1, n_obs):
        assert np.array_equal(bits(hist[:, h]), bits(O[:, K - h] if K - h >= 0 else S0)), h
    # the action slots alike: slot i is the target issued i + 1 steps before the next one
    for i in range(n_act):
        assert np.array_equal(bits(act[:, i]), bits(A[:, K - 1 - i] if K - 1 - i >= 0 else posture)), i
    # row 0 is the incoming row, then the fill
    assert np.array_equal(bits(W[:, 0, :NS]), bits(O[:, 0]))
    assert np.array_equal(bits(W[:, 0, NS:NS * n_obs]), bits(np.tile(S0, (1, n_obs - 1))))
    assert np.array_equal(bits(W[:, 0, NS * n_obs:]), bits(np.tile(posture, (1, n_act))))


def test_two_chains_of_three_steps_are_the_chain_of_six(rows):
    O, A, S0, posture = rows
    whole = hr.chained(O, A, S0, posture, 3, 2)[0]
    hist, act = hr.reset(S0, posture, 3, 2)
    got = []
    for k in range(K):
        hist[:, 0] = O[:, k]
        got.append(hr.push(hist, act)[0])
        hr.push_actions(act, A[:, k])
    assert np.array_equal(bits(np.stack(got, 1)), bits(whole))


def test_a_push_moves_nothing_but_the_older_observed_rows(rows):
    O, A, S0, posture = rows
    hist, act = hr.reset(S0, posture, 3, 2)
    hist[:, 0], hist[:, 1], hist[:, 2] = O[:, 0], O[:, 1], O[:, 2]
    act[:, 0], act[:, 1] = A[:, 0], A[:, 1]
    before = act.copy()
    W, X = hr.push(hist, act, goal=np.ones((B, 3), np.float32), s_mean=None, s_std=None)
    assert np.array_equal(bits(W), bits(np.concatenate([O[:, 0], O[:, 1], O[:, 2], A[:, 0], A[:, 1]], 1)))
    assert np.array_equal(bits(X[:, :-3]), bits(W)) and (X[:, -3:] == 1.0).all()
    assert np.array_equal(bits(hist), bits(np.stack([O[:, 0], O[:, 0], O[:, 1]], 1))) and np.array_equal(bits(act), bits(before))
    hr.push_actions(act, A[:, 2])
    assert np.array_equal(bits(act), bits(np.stack([A[:, 2], A[:, 0]], 1)))


@pytest.mark.parametrize("n_obs,n_act", DEPTHS)
def test_normalised_columns_are_the_database_oracles_assembly(rows, n_obs, n_act):
    O, A, S0, posture = rows
    W = hr.closed_form(O, A, S0, posture, n_obs, n_act).reshape(B * K, -1)
    rng = np.random.default_rng(5)
    db = DatabaseOracle(limit=64, norm_input=True, goal_type="vc")
    goals = rng.uniform(-0.5, 0.5, (B * K, 3)).astype(np.float32)
    db.append(W, np.zeros((B * K, NU), np.float32), vc_goals=goals)
    idx = rng.permutation(B * K)
    want = db.batch(idx)[0]
    got = np.concatenate([hr.normalise(W[idx], db.states_mean, db.states_std, 1), goals[idx]], axis=1)
    assert want.dtype == np.float32 and want.shape == (B * K, hr.width(n_obs, n_act) + 3)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[:, 0]), bits(W[idx, 0]))      # the phase column stays raw
    # and raw throughout without statistics
    assert np.array_equal(bits(hr.normalise(W, None, None, 1)), bits(W))
