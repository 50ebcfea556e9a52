"""Host side of the push windows per rollout (`mpc.sample_push_windows`, `mpc.sample_pushes` with arrays, `mpc.push_windows`):
what is drawn, what is passed through and what is refused.  No GPU."""
import numpy as np
import pytest

from iterative_learning_nmpc_amd import mpc

PERIOD = 0.5


def test_sample_push_windows_is_deterministic_for_a_seed():
    a, b = mpc.sample_push_windows(64, (3, 1), PERIOD), mpc.sample_push_windows(64, (3, 1), PERIOD)
    assert sorted(a) == ["duration", "start"]
    assert np.array_equal(a["start"], b["start"]) and np.array_equal(a["duration"], b["duration"])
    c = mpc.sample_push_windows(64, (3, 2), PERIOD)
    assert not np.array_equal(a["start"], c["start"]) and not np.array_equal(a["duration"], c["duration"])


@pytest.mark.parametrize("n_points,duration", [(10, (0.2, 0.4)), (4, (0.05, 0.1)), (1, (0.3, 0.3))])
def test_starts_lie_on_the_grid_and_durations_in_range(n_points, duration):
    n = 512
    w = mpc.sample_push_windows(n, 11, PERIOD, n_points=n_points, duration=duration)
    assert w["start"].shape == (n,) and w["duration"].shape == (n,)
    assert w["start"].dtype == np.float64 and w["duration"].dtype == np.float64
    k = np.round(w["start"] / (PERIOD / n_points))
    assert np.array_equal(w["start"], k * (PERIOD / n_points)) and k.min() >= 0 and k.max() <= n_points - 1       # k period / n_points, inside one period
    assert np.all(w["start"] < PERIOD)
    assert set(np.round(k).astype(int)) == set(range(n_points))                              # 512 draws reach every point
    assert np.all(w["duration"] >= duration[0]) and np.all(w["duration"] <= duration[1])
    if duration[0] < duration[1]:
        assert len(np.unique(w["duration"])) > n // 2                                          # drawn per rollout, not once


def test_sample_push_windows_refuses_a_grid_without_points():
    with pytest.raises(ValueError):
        mpc.sample_push_windows(4, 0, PERIOD, n_points=0)
    with pytest.raises(ValueError):
        mpc.sample_push_windows(4, 0, 0.0)


def reference_sample_pushes(n, seed, start=0.0, duration=0.3, magnitude=(50.0, 70.0)):
    """`sample_pushes` as it was before it took arrays"""
    rng = np.random.default_rng(seed)
    force = rng.uniform(-1.0, 1.0, (n, 3))
    force /= np.linalg.norm(force, axis=1, keepdims=True) + 1e-6
    force *= rng.uniform(magnitude[0], magnitude[1], (n, 1))
    return dict(start=float(start), duration=float(duration), force=force)


@pytest.mark.parametrize("kw", [{}, dict(start=0.25, duration=0.1), dict(start=np.float32(0.5), duration=1, magnitude=(10.0, 20.0))])
def test_sample_pushes_with_scalars_is_what_it_was(kw):
    got, ref = mpc.sample_pushes(7, (1, 2), **kw), reference_sample_pushes(7, (1, 2), **kw)
    assert sorted(got) == sorted(ref)
    assert type(got["start"]) is float and type(got["duration"]) is float
    assert got["start"] == ref["start"] and got["duration"] == ref["duration"]
    assert np.array_equal(got["force"], ref["force"])
    assert mpc.push_windows(got, 7) is None and mpc.push_windows(None, 7) is None


def test_sample_pushes_passes_arrays_through():
    w = mpc.sample_push_windows(7, 5, PERIOD)
    got = mpc.sample_pushes(7, (1, 2), **w)
    assert np.array_equal(got["force"], reference_sample_pushes(7, (1, 2))["force"])          # the force draw does not move
    assert np.array_equal(got["start"], w["start"]) and np.array_equal(got["duration"], w["duration"])
    merged = dict(mpc.sample_pushes(7, (1, 2)), **w)
    start, duration = mpc.push_windows(merged, 7)
    assert np.array_equal(start, w["start"]) and np.array_equal(duration, w["duration"])
    # one array and one scalar: the scalar holds for every rollout
    start, duration = mpc.push_windows(dict(start=w["start"], duration=0.25, force=None), 7)
    assert np.array_equal(start, w["start"]) and np.array_equal(duration, np.full(7, 0.25))
    got = mpc.sample_pushes(7, 0, start=0.1, duration=list(w["duration"]))
    assert np.array_equal(got["start"], np.full(7, 0.1)) and np.array_equal(got["duration"], w["duration"])


def test_arrays_of_the_wrong_length_are_refused():
    w = mpc.sample_push_windows(6, 5, PERIOD)
    with pytest.raises(ValueError, match="start"):
        mpc.sample_pushes(7, 0, start=w["start"], duration=0.3)
    with pytest.raises(ValueError, match="duration"):
        mpc.sample_pushes(7, 0, start=0.0, duration=w["duration"])
    with pytest.raises(ValueError, match="start"):
        mpc.push_windows(dict(start=w["start"], duration=np.zeros(7), force=None), 7)
    with pytest.raises(ValueError, match="duration"):
        mpc.push_windows(dict(start=np.zeros(7), duration=np.zeros((7, 1)), force=None), 7)
