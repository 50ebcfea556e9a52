"""The numpy restatement of the delay line (tests/delay_reference.py) has the properties the header states for the rule, and agrees
with a second model written another way: a queue per robot that takes one target per control step and hands out the one it took
d steps ago.  Random float32 rows, NaN-free, compared with exact equality: the rule only moves rows.  No GPU."""
import numpy as np
import pytest

from tests.delay_reference import delay_line

NU = 12


def draw(seed, B, n_steps, depth):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n_steps, NU)).astype(np.float32), rng.standard_normal((B, depth, NU)).astype(np.float32)


def queue_model(issued, history, delay):
    """one robot at a time, one control step at a time: `past` lists every target ever issued, oldest first"""
    depth = history.shape[1]
    applied, new = np.empty_like(issued), np.empty_like(history)
    for b in range(issued.shape[0]):
        d = min(max(int(delay[b]), 0), depth)
        past = [history[b, j] for j in range(depth - 1, -1, -1)]
        for k in range(issued.shape[1]):
            past.append(issued[b, k])
            applied[b, k] = past[-1 - d]
        for j in range(depth):
            new[b, j] = past[-1 - j]
    return applied, new


@pytest.mark.parametrize("n_steps", [1, 3, 4, 5, 7, 11])      # below, at and above depth = 4
def test_the_restatement_is_the_queue(n_steps):
    depth = 4
    delay = np.array([0, 1, 2, 3, 4, 9, -3, 64, 2])
    I, H = draw(n_steps, len(delay), n_steps, depth)
    P, Hn = delay_line(I, H, delay)
    Pq, Hq = queue_model(I, H, delay)
    assert np.array_equal(P, Pq) and np.array_equal(Hn, Hq)


@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 6), (3, 4), (4, 4), (7, 2), (5, 9)])
def test_feeding_n1_then_n2_rows_is_feeding_n1_plus_n2(n1, n2):
    depth = 4
    delay = np.array([0, 1, 2, 3, 4, 9, -3])
    I, H = draw(10 * n1 + n2, len(delay), n1 + n2, depth)
    P, Hn = delay_line(I, H, delay)
    P1, H1 = delay_line(I[:, :n1], H, delay)
    P2, H2 = delay_line(I[:, n1:], H1, delay)
    assert np.array_equal(np.concatenate([P1, P2], axis=1), P) and np.array_equal(H2, Hn)


@pytest.mark.parametrize("n_steps", [1, 4, 7])
def test_no_delay_is_the_identity_and_the_register_still_moves(n_steps):
    I, H = draw(n_steps, 3, n_steps, 4)
    P, Hn = delay_line(I, H, np.zeros(3, np.int64))
    assert np.array_equal(P, I)
    assert np.array_equal(Hn, delay_line(I, H, np.array([1, 2, 4]))[1])      # what the register holds does not depend on the delay


@pytest.mark.parametrize("n_steps", [1, 3, 4, 7])
def test_rows_come_from_where_the_rule_says(n_steps):
    depth = 4
    I, H = draw(n_steps, depth + 1, n_steps, depth)
    P, Hn = delay_line(I, H, np.arange(depth + 1))
    for d in range(depth + 1):
        for k in range(n_steps):
            want = I[d, k - d] if k >= d else H[d, d - 1 - k]
            assert np.array_equal(P[d, k], want)
        for j in range(depth):
            want = I[d, n_steps - 1 - j] if j < n_steps else H[d, j - n_steps]
            assert np.array_equal(Hn[d, j], want)


def test_the_delay_is_clamped_into_the_register():
    depth = 4
    I, H = draw(0, 4, 6, depth)
    P, Hn = delay_line(I, H, np.array([9, 64, -3, -1]))
    Pc, Hc = delay_line(I, H, np.array([depth, depth, 0, 0]))
    assert np.array_equal(P, Pc) and np.array_equal(Hn, Hc)
    assert np.array_equal(P[0, :depth], H[0, ::-1]) and np.array_equal(P[0, depth:], I[0, :6 - depth])
    assert np.array_equal(P[2], I[2])


def test_the_inputs_are_left_alone():
    I, H = draw(5, 2, 3, 4)
    I0, H0 = I.copy(), H.copy()
    delay_line(I, H, np.array([1, 3]))
    assert np.array_equal(I, I0) and np.array_equal(H, H0)
