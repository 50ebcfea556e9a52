"""The numpy restatement of the sensor-noise rule (tests/noise_reference.py) is itself right: its generator is the Philox of the
policy oracle where the two overlap, the variate has the moments and the bound the header states, distinct robots, steps and slots
draw distinct numbers, and a slot without noise keeps its bits.  No GPU."""
import numpy as np

from tests import noise_reference as nr


def test_the_generator_is_the_oracles_on_the_counters_it_has():
    from oracle.policy_oracle import philox4x32_10
    i = np.concatenate([np.arange(1000), [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]])
    for seed in (0, 7, 0x123456789ABCDEF0, 2 ** 64 - 1):
        a0, a1 = philox4x32_10(i, seed)
        b0, b1 = nr.philox4x32_10(i, 0, 0, 0, seed)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1), seed
    # the other three counter words are read: each of them moves the output
    base = nr.philox4x32_10(5, 0, 0, 0, 7)
    for c in ((5, 1, 0, 0), (5, 0, 1, 0), (5, 0, 0, 1)):
        assert nr.philox4x32_10(*c, 7) != base, c


def test_the_scale_is_the_float32_the_header_names():
    assert nr.C.dtype == np.float32 and float(nr.C).hex() == "0x1.bb67ae0000000p-16"
    assert float(np.float32(nr.T_MAX) * nr.C) <= 3.4641


def test_the_variate_has_zero_mean_unit_variance_and_a_bounded_tail():
    """200 000 draws of seed 11: the standard error of the mean is 1 / sqrt(n) = 0.0022, that of the variance sqrt((kurtosis - 1) /
    n) = 0.0029 (a sum of four uniforms has kurtosis 3 - 1.2 / 4 = 2.7), so both bars of 0.02 are some seven standard errors"""
    n = 200_000
    robot, slot = np.divmod(np.arange(n), nr.N_SLOTS)
    t = nr.integer_variate(robot, 3, slot, 11)
    g = nr.variate(robot, 3, slot, 11)
    assert g.dtype == np.float32 and t.dtype == np.int64
    mean, var, top = float(g.astype(np.float64).mean()), float(g.astype(np.float64).var()), float(np.abs(g).max())
    print(f"  g over {n} draws: mean {mean:+.5f}, var {var:.5f}, max |g| {top:.4f}, max |t| {int(np.abs(t).max())}")
    assert abs(mean) < 0.02 and abs(var - 1.0) < 0.02
    assert top <= 3.4641 and int(np.abs(t).max()) <= nr.T_MAX
    assert np.array_equal(g, t.astype(np.float32) * nr.C)


def test_robots_steps_slots_and_seeds_draw_distinct_numbers():
    r, s, j = np.meshgrid(np.arange(6), np.arange(5), np.arange(nr.N_SLOTS), indexing="ij")
    t = nr.integer_variate(r, s, j, 3)
    for axis in range(3):                                  # along a robot, a step, a slot: no two neighbours agree everywhere
        a, b = np.take(t, range(t.shape[axis] - 1), axis), np.take(t, range(1, t.shape[axis]), axis)
        assert (a != b).mean() > 0.99, axis
    assert len(np.unique(t)) > 0.98 * t.size              # hardly a collision among 1320 draws with a spread of 37 837
    assert (nr.integer_variate(r, s, j, 4) != t).mean() > 0.99
    # counters are taken mod 2^32
    assert np.array_equal(nr.integer_variate(r + 2 ** 32, s + 2 ** 32, j, 3), t)
    assert not np.array_equal(nr.integer_variate(r, s + 2 ** 16, j, 3), t)


def test_a_slot_without_noise_keeps_its_bits():
    rng = np.random.default_rng(0)
    B = 3
    X = rng.normal(size=(B, nr.N_SLOTS + 3)).astype(np.float32)
    X[:, 5] = -0.0
    noise = np.zeros((B, 2 * nr.N_SLOTS), np.float32)
    noise[:, 7:19] = 0.1                                   # sigma on the joint rates
    noise[1, nr.N_SLOTS + 19] = 0.01                       # a bias alone on robot 1's height
    std = rng.uniform(0.5, 2.0, nr.N_SLOTS)
    for s_std in (None, std):
        Y = nr.observe_noise(X, noise, 9, 0, 4, s_std)
        moved = Y.view(np.int32) != X.view(np.int32)
        want = np.zeros_like(moved)
        want[:, 7:19] = True
        want[1, 19] = True
        assert Y.dtype == np.float32 and np.array_equal(moved, want)
        assert np.signbit(Y[:, 5]).all()                   # -0.0 stays -0.0: the slot is not written, not "written with + 0"
    raw, norm = nr.observe_noise(X, noise, 9, 0, 4), nr.observe_noise(X, noise, 9, 0, 4, std)
    d_raw, d_norm = (Y[:, 7:19].astype(np.float64) - X[:, 7:19] for Y in (raw, norm))
    # the same perturbation in the column's own unit, up to the two roundings to float32: half an ulp of |X| < 8 is 4.8e-7, once as
    # it is and once times s_std <= 2
    assert np.abs(d_norm * std[7:19] - d_raw).max() < 1.5e-6 and np.abs(d_raw).max() > 0.05
    zeros = nr.observe_noise(X, np.zeros_like(noise), 9, 0, 4, std)
    assert np.array_equal(zeros.view(np.int32), X.view(np.int32))
