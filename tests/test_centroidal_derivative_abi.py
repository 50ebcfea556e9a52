"""The momentum-derivative entry point of include/nmpc_torque.h exists in every layer: nmpc_centroidal_derivatives_batch is
declared, exported by libnmpc_hip.so, bound with the header's argument list, and behind a method of BatchedTorqueLayer.  No GPU:
what is decided on the host is checked."""
import ctypes
import inspect

from tests.abi_header import declaration, lib  # noqa: F401

NAME = "nmpc_centroidal_derivatives_batch"


def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", NAME)
    assert names == ["handle", "B", "q", "v", "dh_dq", "dcom_dq", "hdot_bias", "stream"]
    assert getattr(lib, NAME) is not None
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, types)


def test_layer_has_the_method_and_the_others_keep_their_parameters():
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    c = inspect.signature(BatchedTorqueLayer.centroidal_derivatives).parameters
    assert list(c) == ["self", "q", "v", "com_jacobian", "bias"]
    assert c["com_jacobian"].default is False and c["bias"].default is False
    assert list(inspect.signature(BatchedTorqueLayer.centroidal).parameters) == ["self", "q", "v", "jacobian"]
    assert list(inspect.signature(BatchedTorqueLayer.mass_matrix).parameters) == ["self", "q"]


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_centroidal_derivatives_batch(None, 1, None, None, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
