"""The clock of a continued whole-body rollout exists in every layer: nmpc_wb_rollout_set_clock (include/nmpc.h) is declared,
exported by libnmpc_hip.so and bound with the header's argument list, and the Python layers take the keywords.  No GPU: what
is decided on the host is checked."""
import ctypes
import inspect

from tests.abi_header import declaration, lib, struct_fields  # noqa: F401


def test_set_clock_is_declared_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc.h", "nmpc_wb_rollout_set_clock")
    assert names == ["handle", "replan0"]
    assert lib.nmpc_wb_rollout_set_clock is not None
    assert _lib.SIGNATURES["nmpc_wb_rollout_set_clock"] == (ctypes.c_int, types)


def test_the_rollout_cfg_and_the_rollout_call_are_what_they_were():
    """the clock is attached by a call: the pinned structure stays"""
    from iterative_learning_nmpc_amd import _lib
    assert _lib.NmpcWbRolloutCfg._fields_ == struct_fields("nmpc.h", "nmpc_wb_rollout_cfg")
    assert len(_lib.NmpcWbRolloutCfg._fields_) == 20


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_wb_rollout_set_clock(None, 0) == -1


def test_python_layers_take_the_clock():
    from iterative_learning_nmpc_amd import collect, learning
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    assert list(inspect.signature(BatchedNmpcSolver.set_rollout_clock).parameters) == ["self", "replan0"]
    p = inspect.signature(LocomotionMPC.open_loop_device).parameters
    assert list(p)[:4] == ["self", "q0", "v0", "trajectory_time"]
    assert p["n_replans"].default is None and p["resume"].default is False
    assert inspect.signature(BatchedNmpcSolver.wb_rollout).parameters["failed"].default is None
    for fn in (collect.collect_rollouts, learning.learning_iteration):
        assert inspect.signature(fn).parameters["chunk_replans"].default is None, fn.__name__
