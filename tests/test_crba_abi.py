"""The composite-inertia entry points of include/nmpc_torque.h exist in every layer: nmpc_mass_matrix_batch and
nmpc_centroidal_batch are declared, exported by libnmpc_hip.so, bound with the header's argument lists, and behind methods of
BatchedTorqueLayer.  No GPU: what is decided on the host is checked."""
import ctypes
import inspect

import pytest

from tests.abi_header import declaration, lib  # noqa: F401

ARGUMENTS = {"nmpc_mass_matrix_batch": ["handle", "B", "q", "M", "stream"],
             "nmpc_centroidal_batch": ["handle", "B", "q", "v", "com", "h", "Ag", "stream"]}


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib, name):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", name)
    assert names == ARGUMENTS[name]
    assert getattr(lib, name) is not None
    assert _lib.SIGNATURES[name] == (ctypes.c_int, types)


def test_layer_has_both_methods():
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    assert list(inspect.signature(BatchedTorqueLayer.mass_matrix).parameters) == ["self", "q"]
    c = inspect.signature(BatchedTorqueLayer.centroidal).parameters
    assert list(c) == ["self", "q", "v", "jacobian"]
    assert c["v"].default is None and c["jacobian"].default is False


def test_the_other_methods_keep_their_parameters():
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    assert list(inspect.signature(BatchedTorqueLayer.forward_dynamics).parameters) == ["self", "q", "v", "tau", "f"]
    assert list(inspect.signature(BatchedTorqueLayer.id_torques).parameters) == ["self", "q_plan", "v_plan", "a_plan", "f_plan"]


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_mass_matrix_batch(None, 1, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    assert lib.nmpc_centroidal_batch(None, 1, None, None, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
