"""nmpc_debug_read_centroidal_rollout_problem exists in every layer: declared in include/nmpc.h, exported by libnmpc_hip.so, bound
in _lib.SIGNATURES with the header's argument list, and the Python solver has the method.  No GPU: what is decided on the host
is checked."""
import ctypes
import inspect

from tests.abi_header import declaration, lib  # noqa: F401

NAME = "nmpc_debug_read_centroidal_rollout_problem"


def test_symbol_is_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    assert getattr(lib, NAME) is not None
    names, types = declaration("nmpc.h", NAME)
    assert names == ["handle", "b", "yref_host", "yref_e_host", "params_host"]
    res, args = _lib.SIGNATURES[NAME]                            # host arrays: bound as float pointers, like nmpc_debug_read_workspace
    assert res is ctypes.c_int and len(args) == len(types) == 5 and args[:2] == types[:2] == [ctypes.c_void_p, ctypes.c_int]
    assert args[2:] == [ctypes.POINTER(ctypes.c_float)] * 3


def test_the_whole_body_read_back_is_as_it_was(lib):
    from iterative_learning_nmpc_amd import _lib
    names, _ = declaration("nmpc.h", "nmpc_debug_read_rollout_problem")
    assert names == ["handle", "b", "x0_host", "yref_host"] and len(_lib.SIGNATURES["nmpc_debug_read_rollout_problem"][1]) == 4


def test_a_null_handle_is_refused_on_the_host(lib):
    assert getattr(lib, NAME)(None, 0, None, None, None) == -1


def test_the_python_solver_has_the_method():
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    assert list(inspect.signature(BatchedNmpcSolver.debug_centroidal_rollout_problem).parameters) == ["self", "b"]
