"""A delay per robot exists in every layer and what the host decides about it is decided rightly: nmpc_contact_set_delays and
nmpc_delay_line_batch (include/nmpc_torque.h) are declared, exported by libnmpc_hip.so and bound with the header's argument lists,
NMPC_DELAY_MAX_DEPTH stands in the header and in the binding; host input of `BatchedTorqueLayer.set_delays` is validated;
`torque.sample_delays` is deterministic in its seed and stays inside its range.  No GPU."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from tests.abi_header import declaration, header, lib  # noqa: F401

P, I = ctypes.c_void_p, ctypes.c_int


def test_symbols_are_declared_exported_and_bound_as_the_header_declares_them(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", "nmpc_contact_set_delays")
    assert names == ["torque", "delay", "history", "depth", "work", "work_rows", "rows"]
    assert types == [P, P, P, I, P, I, I]
    assert lib.nmpc_contact_set_delays is not None
    assert _lib.SIGNATURES["nmpc_contact_set_delays"] == (I, types)
    names, types = declaration("nmpc_torque.h", "nmpc_delay_line_batch")
    assert names == ["torque", "B", "n_steps", "issued", "issued_rows", "applied", "applied_rows", "skip", "skip_mask", "stream"]
    assert types == [P, I, I, P, I, P, I, P, I, P]
    assert lib.nmpc_delay_line_batch is not None
    assert _lib.SIGNATURES["nmpc_delay_line_batch"] == (I, types)


def test_the_depth_limit_stands_in_the_header_and_in_the_binding():
    from iterative_learning_nmpc_amd import _lib, torque
    m = re.search(r"#define\s+NMPC_DELAY_MAX_DEPTH\s+(\d+)", header("nmpc_torque.h"))
    assert m and int(m.group(1)) == 64
    assert _lib.NMPC_DELAY_MAX_DEPTH == 64 and torque.DELAY_MAX_DEPTH == 64


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_contact_set_delays(None, None, None, 0, None, 0, 0) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    assert lib.nmpc_delay_line_batch(None, 1, 1, None, 1, None, 1, None, 0, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)


def test_the_calls_that_honour_the_table_keep_their_signatures():
    assert len(declaration("nmpc_torque.h", "nmpc_contact_step_batch")[0]) == 17
    assert len(declaration("nmpc_torque.h", "nmpc_contact_track_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16


def unbuilt_layer():
    """a layer that never reached a device: `set_delays` validates host input before it touches the library"""
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    return BatchedTorqueLayer.__new__(BatchedTorqueLayer)


@pytest.mark.parametrize("bad,text", [([0, 1, -1], "row 2: the delay must be in"), ([65, 0], "row 0: the delay must be in"),
                                      ([0.0, 1.0], "need integers"), ([0.5], "need integers"), ([True, False], "need integers"),
                                      ([[0, 1]], "expected"), (3, "expected"), ([], "need integers|expected"), ("late", "need integers")])
def test_delay_table_refuses_bad_host_input(bad, text):
    import torch
    from iterative_learning_nmpc_amd.torque import delay_table
    with pytest.raises(ValueError, match="delays: .*(" + text + ")"):
        delay_table(bad)
    with pytest.raises(ValueError, match="delays: .*(" + text + ")"):
        unbuilt_layer().set_delays(bad)
    if isinstance(bad, list) and bad and not isinstance(bad[0], list):
        with pytest.raises(ValueError, match="delays: "):
            unbuilt_layer().set_delays(torch.as_tensor(bad))


def test_delay_table_takes_what_is_valid():
    from iterative_learning_nmpc_amd.torque import delay_table
    for given in ([0, 3, 64], np.array([0, 3, 64], np.int64), np.array([0, 3, 64], np.uint8)):
        rows = delay_table(given)
        assert rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"] and np.array_equal(rows, [0, 3, 64])
    with pytest.raises(ValueError, match=r"delays: expected \[>= 4\]"):
        delay_table([0, 1, 2], 4)
    assert len(delay_table([0, 1, 2, 3, 4], 4)) == 5


def test_set_delays_refuses_a_depth_or_work_rows_out_of_range():
    for kw, text in ((dict(depth=0), "depth"), (dict(depth=65), "depth"), (dict(work_rows=0), "work_rows")):
        with pytest.raises(ValueError, match="delays: " + text):
            layer = unbuilt_layer()
            layer.device = "cpu"
            layer.set_delays([0, 1], **kw)


def test_sample_delays_is_deterministic_and_stays_inside_its_range():
    from iterative_learning_nmpc_amd.torque import sample_delays
    a, b, c = sample_delays(257, 3, steps=(1, 5)), sample_delays(257, 3, steps=(1, 5)), sample_delays(257, 4, steps=(1, 5))
    assert a.shape == (257,) and a.dtype == np.int32
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a[0] == 0 and set(a[1:].tolist()) == {1, 2, 3, 4, 5}      # row 0 is on time, the others fill the range, ends included
    assert set(sample_delays(64, 0).tolist()) == {0, 1, 2}
    assert np.array_equal(sample_delays(5, 0, steps=(2, 2)), [0, 2, 2, 2, 2])
    for steps, text in (((2, 1), "lo <= hi"), ((0.0, 2.0), "integers"), ((0, 65), "must be in"), ((-1, -1), "must be in"), (3, "range")):
        with pytest.raises(ValueError, match=text):
            sample_delays(8, 0, steps=steps)
    with pytest.raises(ValueError, match="at least 1"):
        sample_delays(0, 0)


def test_python_layers_take_the_table():
    from iterative_learning_nmpc_amd import learning, torque
    sd = inspect.signature(torque.BatchedTorqueLayer.set_delays).parameters
    assert list(sd) == ["self", "delays", "depth", "work_rows"]
    assert sd["delays"].default is None and sd["depth"].default is None and sd["work_rows"].default == 64
    assert list(inspect.signature(torque.BatchedTorqueLayer.reset_delay_history).parameters) == ["self", "q"]
    assert list(inspect.signature(torque.BatchedTorqueLayer.delay_line).parameters)[:2] == ["self", "issued"]
    ss = inspect.signature(torque.sample_delays).parameters
    assert list(ss) == ["n", "seed", "steps"] and ss["steps"].default == (0, 2)
    for f in (learning.evaluate_policy, learning.dagger_iteration):
        assert inspect.signature(f).parameters["delays"].default is None
