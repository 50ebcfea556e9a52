"""nmpc_state_momentum_batch and nmpc_wb_set_state_momentum exist in every layer: declared in the headers, exported by
libnmpc_hip.so, bound in _lib.SIGNATURES with the header's argument list, and the Python objects have the methods, with
"declared" as the source they start with.  No GPU: what is decided on the host is checked."""
import ctypes
import inspect

import pytest

from tests.abi_header import declaration, header, lib  # noqa: F401

ENTRY_POINTS = {
    "nmpc_state_momentum_batch": ("nmpc_torque.h", ["handle", "B", "q", "v", "qv_stride", "h", "h_stride", "h2", "h2_stride", "skip",
                                                    "skip_mask", "stream"]),
    "nmpc_wb_set_state_momentum": ("nmpc.h", ["handle", "source"]),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_symbol_is_exported_and_bound_as_the_header_declares_it(lib, name):
    from iterative_learning_nmpc_amd import _lib
    header_file, arg_names = ENTRY_POINTS[name]
    assert getattr(lib, name) is not None
    names, types = declaration(header_file, name)
    res, args = _lib.SIGNATURES[name]
    assert names == arg_names
    assert res is ctypes.c_int and args == types


def test_the_header_names_both_sources():
    text = header("nmpc.h")
    assert "#define NMPC_WB_STATE_MOMENTUM_DECLARED 0" in text and "#define NMPC_WB_STATE_MOMENTUM_TREE     1" in text


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_wb_set_state_momentum(None, 1) == -1
    assert lib.nmpc_wb_set_state_momentum(None, 0) == -1
    assert lib.nmpc_state_momentum_batch(None, 1, None, None, 18, None, 6, None, 0, None, 0, None) == -1


def test_the_python_layers_have_the_methods():
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.quadruped_solver import QuadrupedAcadosSolver
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    p = inspect.signature(BatchedTorqueLayer.state_momentum).parameters
    assert list(p) == ["self", "q", "v", "out", "skip", "skip_mask"]
    assert p["out"].default is None and p["skip"].default is None and p["skip_mask"].default == 0
    assert BatchedNmpcSolver.STATE_MOMENTUM == {"declared": 0, "tree": 1}
    for cls in (BatchedNmpcSolver, QuadrupedAcadosSolver, LocomotionMPC):
        p = inspect.signature(cls.set_state_momentum).parameters
        assert list(p) == ["self", "source"] and p["source"].default == "declared"


def test_the_controller_starts_with_the_declared_source():
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    mpc = LocomotionMPC(print_info=False)
    assert mpc.state_momentum == mpc.solver.state_momentum == "declared"
    mpc.set_state_momentum("declared")                       # the default is always accepted, device solver or not
    with pytest.raises(ValueError):
        mpc.set_state_momentum("articulated")                # not a source
    with pytest.raises(RuntimeError, match="articulated"):
        mpc.set_state_momentum("tree")                       # needs the articulated momentum model
    assert mpc.state_momentum == "declared"
    mpc._declared_momentum_only("open_loop_device")          # a declared controller is never refused
