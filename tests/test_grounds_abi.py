"""A ground per robot exists in every layer and what the host decides about it is decided rightly: nmpc_contact_set_grounds
(include/nmpc_torque.h) is declared, exported by libnmpc_hip.so and bound with the header's argument list; host input of
`BatchedTorqueLayer.set_grounds` is validated by the rules a single ground is refused by; `torque.sample_grounds` is deterministic
in its rng, stays inside its ranges and leaves undrawn columns at the base.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

from tests.abi_header import declaration, lib  # noqa: F401

GOOD = [[0.0, 1e4, 3.0, 0.8, 0.05, 0.0], [0.01, 5e3, 1.0, 0.2, 0.02, 12.0]]


def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", "nmpc_contact_set_grounds")
    assert names == ["torque", "rows", "n_rows"]
    assert types == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert lib.nmpc_contact_set_grounds is not None
    assert _lib.SIGNATURES["nmpc_contact_set_grounds"] == (ctypes.c_int, types)


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_contact_set_grounds(None, None, 0) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)


def test_the_calls_that_honour_the_table_keep_their_signatures():
    assert len(declaration("nmpc_torque.h", "nmpc_contact_forces_batch")[0]) == 7
    assert len(declaration("nmpc_torque.h", "nmpc_contact_step_batch")[0]) == 17
    assert len(declaration("nmpc_torque.h", "nmpc_contact_track_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16


def unbuilt_layer():
    """a layer that never reached a device: `set_grounds` validates host input before it touches the library"""
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    return BatchedTorqueLayer.__new__(BatchedTorqueLayer)


@pytest.mark.parametrize("spoil,text", [(lambda r: r.__setitem__((1, 3), -0.1), "row 1: stiffness, damping and mu must not be negative"),
                                        (lambda r: r.__setitem__((0, 4), 0.0), "row 0: slip_velocity must be positive"),
                                        (lambda r: r.__setitem__((1, 0), np.nan), "row 1: the contact parameters must be finite"),
                                        (lambda r: r.__setitem__((0, 5), np.inf), "row 0: the contact parameters must be finite"),
                                        (lambda r: r.__setitem__((0, 1), -1.0), "row 0: stiffness, damping and mu must not be negative")])
def test_set_grounds_refuses_bad_host_rows(spoil, text):
    import torch
    from iterative_learning_nmpc_amd.torque import ground_table
    rows = np.array(GOOD, np.float32)
    assert np.array_equal(ground_table(rows), rows) and ground_table(rows).dtype == np.float32
    spoil(rows)
    for given in (rows, rows.tolist(), torch.as_tensor(rows)):
        with pytest.raises(ValueError, match=text):
            ground_table(given if not isinstance(given, torch.Tensor) else given.numpy())
        with pytest.raises(ValueError, match=text):
            unbuilt_layer().set_grounds(given)


@pytest.mark.parametrize("shape", [(6,), (2, 5), (2, 7), (0, 6), (2, 3, 6)])
def test_set_grounds_refuses_a_wrong_shape(shape):
    from iterative_learning_nmpc_amd.torque import ground_table
    with pytest.raises(ValueError, match="grounds: expected"):
        ground_table(np.ones(shape, np.float32))
    with pytest.raises(ValueError, match="grounds: expected"):
        unbuilt_layer().set_grounds(np.ones(shape, np.float32))
    with pytest.raises(ValueError, match="grounds"):
        ground_table([])
    with pytest.raises(ValueError, match="grounds"):
        ground_table("floor")


def test_a_sequence_of_grounds_becomes_its_rows():
    from iterative_learning_nmpc_amd.torque import GROUND_COLUMNS, GroundContact, ground_table
    assert GROUND_COLUMNS == ("ground_z", "stiffness", "damping", "mu", "slip_velocity", "tau_max")
    rows = ground_table([GroundContact(), GroundContact(ground_z=0.01, mu=0.3, tau_max=12.0)])
    assert np.array_equal(rows, np.array([[0.0, 1e4, 3.0, 0.8, 0.05, 0.0], [0.01, 1e4, 3.0, 0.3, 0.05, 12.0]], np.float32))
    with pytest.raises(ValueError, match="slip_velocity must be positive"):
        ground_table([GroundContact(), GroundContact(slip_velocity=-1.0)])


RANGES = dict(mu=(0.2, 1.2), stiffness=(5e3, 2e4), damping=(1.0, 5.0), ground_z=(-0.01, 0.01), tau_max=(5.0, 30.0))


def test_sample_grounds_is_deterministic_in_its_rng():
    from iterative_learning_nmpc_amd.torque import sample_grounds
    a = sample_grounds(257, np.random.default_rng(3), **RANGES)
    b = sample_grounds(257, np.random.default_rng(3), **RANGES)
    c = sample_grounds(257, np.random.default_rng(4), **RANGES)
    assert a.shape == (257, 6) and a.dtype == np.float32
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    rng = np.random.default_rng(3)                        # one generator, two tables: the second goes on where the first ended
    assert np.array_equal(sample_grounds(257, rng, **RANGES), a) and not np.array_equal(sample_grounds(257, rng, **RANGES), a)


def test_sample_grounds_stays_inside_its_ranges():
    from iterative_learning_nmpc_amd.torque import GROUND_COLUMNS, sample_grounds
    rows = sample_grounds(4096, np.random.default_rng(0), **RANGES).astype(np.float64)
    for name, (lo, hi) in RANGES.items():
        x = rows[:, GROUND_COLUMNS.index(name)]
        assert lo <= x.min() and x.max() <= hi, name
        assert x.min() < lo + 0.05 * (hi - lo) and x.max() > hi - 0.05 * (hi - lo), name      # and fills them
        assert len(np.unique(x)) > 4000, name                                                     # a draw per robot
    # a range of one point is that point
    assert np.all(sample_grounds(5, np.random.default_rng(0), mu=(0.5, 0.5))[:, 3] == np.float32(0.5))
    with pytest.raises(ValueError, match="lo <= hi"):
        sample_grounds(5, np.random.default_rng(0), mu=(1.0, 0.5))
    with pytest.raises(ValueError, match="must not be negative"):
        sample_grounds(64, np.random.default_rng(0), mu=(-1.0, -0.5))


def test_sample_grounds_leaves_undrawn_columns_at_the_base():
    from iterative_learning_nmpc_amd.torque import GroundContact, sample_grounds
    base = GroundContact(ground_z=0.02, stiffness=8e3, damping=2.0, mu=0.6, slip_velocity=0.03, tau_max=25.0)
    want = np.array([0.02, 8e3, 2.0, 0.6, 0.03, 25.0], np.float32)
    rows = sample_grounds(33, np.random.default_rng(1), base=base)
    assert np.array_equal(rows, np.tile(want, (33, 1)))
    rows = sample_grounds(33, np.random.default_rng(1), base=base, mu=(0.2, 1.2))
    assert np.array_equal(rows[:, [0, 1, 2, 4, 5]], np.tile(want[[0, 1, 2, 4, 5]], (33, 1))) and len(np.unique(rows[:, 3])) == 33
    assert np.array_equal(sample_grounds(2, np.random.default_rng(1))[0], np.array([0.0, 1e4, 3.0, 0.8, 0.05, 0.0], np.float32))      # tau_max None -> 0
    # a column that is not drawn takes nothing from the generator
    assert np.array_equal(sample_grounds(33, np.random.default_rng(1), mu=(0.2, 1.2))[:, 3], rows[:, 3])


def test_python_layers_take_the_table():
    from iterative_learning_nmpc_amd import learning, torque
    assert list(inspect.signature(torque.BatchedTorqueLayer.set_grounds).parameters) == ["self", "grounds"]
    assert inspect.signature(torque.BatchedTorqueLayer.set_grounds).parameters["grounds"].default is None
    sg = inspect.signature(torque.sample_grounds).parameters
    assert list(sg) == ["B", "rng", "base", "mu", "stiffness", "damping", "ground_z", "tau_max"]
    assert sg["base"].default == torque.GroundContact() and all(sg[k].default is None for k in list(sg)[3:])
    for f in (learning.evaluate_policy, learning.dagger_iteration):
        assert inspect.signature(f).parameters["grounds"].default is None
