"""nmpc_wb_set_momentum_model exists in every layer: declared in include/nmpc.h, exported by libnmpc_hip.so, bound in
_lib.SIGNATURES with the header's argument list, and the Python solver has the method.  No GPU: what is decided on the host is
checked."""
import ctypes
import inspect

from tests.abi_header import declaration, header, lib  # noqa: F401


def test_symbol_is_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    assert getattr(lib, "nmpc_wb_set_momentum_model") is not None
    names, types = declaration("nmpc.h", "nmpc_wb_set_momentum_model")
    res, args = _lib.SIGNATURES["nmpc_wb_set_momentum_model"]
    assert names == ["handle", "torque_handle", "model"]
    assert res is ctypes.c_int and args == types == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]


def test_the_debug_read_is_declared_and_bound(lib):
    from iterative_learning_nmpc_amd import _lib
    assert getattr(lib, "nmpc_debug_read_momentum") is not None
    names, types = declaration("nmpc.h", "nmpc_debug_read_momentum")
    assert names == ["handle", "b", "k", "mrec_host", "dcons_host"]
    res, args = _lib.SIGNATURES["nmpc_debug_read_momentum"]      # host arrays: bound as float pointers, like nmpc_debug_read_workspace
    assert res is ctypes.c_int and len(args) == len(types) == 5 and args[:3] == types[:3]


def test_the_header_names_both_models():
    text = header("nmpc.h")
    assert "#define NMPC_WB_MOMENTUM_DECLARED    0" in text and "#define NMPC_WB_MOMENTUM_ARTICULATED 1" in text


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_wb_set_momentum_model(None, None, 1) == -1
    assert lib.nmpc_debug_read_momentum(None, 0, 0, None, None) == -1


def test_the_python_solver_has_the_method():
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    p = inspect.signature(BatchedNmpcSolver.set_momentum_model).parameters
    assert list(p) == ["self", "model", "torque_layer"] and p["model"].default == "declared" and p["torque_layer"].default is None
    assert BatchedNmpcSolver.MOMENTUM_MODELS == {"declared": 0, "articulated": 1}


def test_the_facade_has_the_option():
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.quadruped_solver import QuadrupedAcadosSolver
    for cls in (QuadrupedAcadosSolver, LocomotionMPC):
        p = inspect.signature(cls.__init__).parameters
        assert p["momentum_model"].default == "declared" and p["torque_layer"].default is None
    mpc = LocomotionMPC(print_info=False)
    assert mpc.momentum_model == mpc.solver.momentum_model == "declared" and mpc.solver.dyn.torque_layer is None
    for bad in (dict(momentum_model="articulated"), dict(momentum_model="rigid")):
        try:
            LocomotionMPC(print_info=False, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
