"""The numpy restatement of the training-noise and observed-row rules (tests/input_noise_reference.py) is itself right: at the
fourth counter word 1 the variate keeps its bound and its moments and is another stream than the sensor rule's word 0, the
restated variate at word 0 is the sensor rule's, a column without sigma keeps its bits, an observed row is the perturbed raw input,
and `torque.training_sigma` is the hand computation.  No GPU."""
import numpy as np

from tests import input_noise_reference as ir
from tests import noise_reference as nr


def test_the_variate_at_word_one_keeps_its_bound_and_is_another_stream():
    a, b, j = np.meshgrid(np.arange(40), np.arange(25), np.arange(nr.N_SLOTS), indexing="ij")
    t0, t1 = ir.integer_variate4(a, b, j, 0, 3), ir.integer_variate4(a, b, j, ir.TRAINING_WORD, 3)
    assert np.array_equal(t0, nr.integer_variate(a, b, j, 3))             # word 0 is the sensor rule's text
    assert t1.dtype == np.int64 and int(np.abs(t1).max()) <= nr.T_MAX
    assert (t1 != t0).mean() > 0.99                                        # equal (a, b, j), another stream
    assert abs(float(np.corrcoef(t0.ravel(), t1.ravel())[0, 1])) < 0.02    # 44 000 pairs: a standard error of 0.0048
    g = ir.variate4(a, b, j, ir.TRAINING_WORD, 3)
    assert g.dtype == np.float32 and np.array_equal(g, t1.astype(np.float32) * nr.C) and float(np.abs(g).max()) <= 3.4641
    # counters are taken mod 2^32, and every one of them is read
    assert np.array_equal(ir.integer_variate4(a + 2 ** 32, b + 2 ** 32, j, 1 + 2 ** 32, 3), t1)
    for other in (ir.integer_variate4(a + 1, b, j, 1, 3), ir.integer_variate4(a, b + 1, j, 1, 3), ir.integer_variate4(a, b, j, 1, 4)):
        assert (other != t1).mean() > 0.99


def test_the_variate_at_word_one_has_zero_mean_and_unit_variance():
    """the bounds tests/test_noise_reference.py holds the sensor variate to: 200 000 draws, the standard error of the mean is
    0.0022 and that of the variance 0.0029, so both bars of 0.02 are some seven standard errors"""
    n = 200_000
    sample, col = np.divmod(np.arange(n), nr.N_SLOTS)
    t = ir.integer_variate4(sample, 3, col, ir.TRAINING_WORD, 11)
    g = ir.variate4(sample, 3, col, ir.TRAINING_WORD, 11).astype(np.float64)
    mean, var, top = float(g.mean()), float(g.var()), float(np.abs(g).max())
    print(f"  g at word 1 over {n} draws: mean {mean:+.5f}, var {var:.5f}, max |g| {top:.4f}, max |t| {int(np.abs(t).max())}")
    assert abs(mean) < 0.02 and abs(var - 1.0) < 0.02
    assert top <= 3.4641 and int(np.abs(t).max()) <= nr.T_MAX


def test_a_column_without_sigma_keeps_its_bits():
    rng = np.random.default_rng(0)
    B, n = 6, 10
    X = rng.normal(size=(B, 47)).astype(np.float32)
    X[:, 5] = -0.0
    sigma = np.full(n, 0.1, np.float32)
    sigma[[0, 5]] = 0.0
    std = rng.uniform(0.5, 2.0, 44)
    for s_std in (None, std):
        Y = ir.input_noise(X, sigma, 9, 4, 16, s_std)
        moved = Y.view(np.int32) != X.view(np.int32)
        want = np.zeros_like(moved)
        want[:, :n] = sigma != 0
        assert Y.dtype == np.float32 and np.array_equal(moved, want)
        assert np.signbit(Y[:, 5]).all()                   # -0.0 stays -0.0: the column is not written
    zeros = ir.input_noise(X, np.zeros(44, np.float32), 9, 4, 16, std)
    assert np.array_equal(zeros.view(np.int32), X.view(np.int32))
    # row i of a call at first_sample f is row 0 of a call at first_sample f + i, and the epoch is read
    whole = ir.input_noise(X, sigma, 9, 4, 16, std)
    for i in (0, 3, 5):
        assert np.array_equal(ir.input_noise(X[i:i + 1], sigma, 9, 4, 16 + i, std), whole[i:i + 1])
    assert not np.array_equal(ir.input_noise(X, sigma, 9, 5, 16, std), whole)
    # the same perturbation in the column's own unit, up to the two roundings to float32 (|X| < 8: half an ulp is 4.8e-7)
    raw = ir.input_noise(X, sigma, 9, 4, 16)
    d_raw, d_norm = (Y[:, 1:n].astype(np.float64) - X[:, 1:n] for Y in (raw, whole))
    assert np.abs(d_norm * std[1:n] - d_raw).max() < 1.5e-6 and np.abs(d_raw).max() > 0.05
    assert np.array_equal(raw[:, 0], whole[:, 0])          # column 0 is in front of s_first = 1: never divided


def test_an_observed_row_is_the_raw_input_the_sensor_rule_perturbs():
    rng = np.random.default_rng(1)
    B = 7
    S = rng.normal(size=(B, 44)).astype(np.float32)
    noise = np.zeros((B, 88), np.float32)
    noise[:, 7:19] = 0.1
    noise[1, 44 + 19] = 0.01
    noise[:, 44 + 3] = rng.uniform(-0.05, 0.05, B)
    X = np.concatenate([S, np.full((B, 3), 5.0, np.float32)], axis=1)
    for first_robot, step in ((0, 0), (2 ** 32 - 3, 70000)):
        O = ir.observed_rows(S, noise, 9, first_robot, step)
        assert O.dtype == np.float32 and np.array_equal(O, nr.observe_noise(X, noise, 9, first_robot, step)[:, :44])
        moved = O.view(np.int32) != S.view(np.int32)
        assert np.array_equal(moved.any(axis=0), ((noise[:, :44] != 0) | (noise[:, 44:] != 0)).any(axis=0))
    assert np.array_equal(ir.observed_rows(S, None, 9, 0, 0).view(np.int32), S.view(np.int32))
    assert np.array_equal(ir.observed_rows(S, np.zeros_like(noise), 9, 0, 0).view(np.int32), S.view(np.int32))


def test_training_sigma_is_the_hand_computation():
    from iterative_learning_nmpc_amd.torque import sample_noise, training_sigma
    table = np.zeros((2, 88), np.float32)
    table[0, 3], table[1, 3] = 3.0, 0.0                    # sigma 3 and 0, bias 4 and 0: sqrt((9 + 16 + 0 + 0) / 2)
    table[0, 44 + 3] = 4.0
    table[:, 7] = (1.0, 7.0)                               # sigma alone: sqrt((1 + 49) / 2) = 5
    table[:, 44 + 20] = (-0.5, 0.5)                        # bias alone, either sign: 0.5
    got = training_sigma(table)
    assert got.shape == (44,) and got.dtype == np.float32
    want = np.zeros(44, np.float32)
    want[3], want[7], want[20] = np.float32(np.sqrt(12.5)), 5.0, 0.5
    assert np.array_equal(got, want)
    drawn = sample_noise(33, 5)
    assert np.array_equal(training_sigma(drawn), ir.training_sigma(drawn)) and training_sigma(drawn)[0] == 0.0
    assert (training_sigma(drawn)[1:] > 0).all()
    for bad in (np.zeros((2, 87)), np.zeros(88), "loud"):
        try:
            training_sigma(bad)
        except ValueError as e:
            assert "noise: " in str(e)
        else:
            raise AssertionError(bad)
