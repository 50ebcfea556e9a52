"""The forward-dynamics entry points of include/nmpc_torque.h exist in every layer: exported by libnmpc_hip.so, bound with
the header's argument lists, and behind methods of BatchedTorqueLayer.  No GPU: what is decided on the host is checked."""
import ctypes
import inspect

import pytest

from tests.abi_header import declaration, lib  # noqa: F401

NAMES = ("nmpc_fd_accel_batch", "nmpc_fd_step_batch")


def header_arguments(name):
    """The ctypes argument list the header's declaration of `name` asks for."""
    return declaration("nmpc_torque.h", name)[1]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_bound_as_the_header_declares_it(lib, name):
    from iterative_learning_nmpc_amd import _lib
    assert getattr(lib, name) is not None
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args == header_arguments(name)


def test_argument_lists():
    assert len(header_arguments("nmpc_fd_accel_batch")) == 8 and len(header_arguments("nmpc_fd_step_batch")) == 15


def test_layer_has_both_methods():
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    from iterative_learning_nmpc_amd.trajectory_io import KD, KP
    assert list(inspect.signature(BatchedTorqueLayer.forward_dynamics).parameters) == ["self", "q", "v", "tau", "f"]
    step = inspect.signature(BatchedTorqueLayer.step).parameters
    assert list(step) == ["self", "q", "v", "dt", "n_sub", "tau_ff", "q_des", "kp", "kd", "f"]
    assert (step["n_sub"].default, step["kp"].default, step["kd"].default) == (1, KP, KD)


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_fd_accel_batch(None, 1, None, None, None, None, None, None) == -1
    assert lib.nmpc_fd_step_batch(None, 1, 1, 1e-3, None, None, None, None, 0.0, 0.0, None, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
