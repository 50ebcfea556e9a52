"""The entry points of the push on the contact plant exist in every layer: nmpc_contact_set_push with nmpc_push_cfg
(include/nmpc_torque.h) and nmpc_wb_rollout_set_plant_push (include/nmpc.h) are declared, exported by libnmpc_hip.so and bound
with the headers' argument lists and fields; the Python layers take the push.  No GPU: what is decided on the host is checked."""
import ctypes
import inspect

import pytest

from tests import abi_header
from tests.abi_header import declaration, lib, struct_fields  # noqa: F401

ARGUMENTS = {"nmpc_contact_set_push": ("nmpc_torque.h", ["torque", "push"]),
             "nmpc_wb_rollout_set_plant_push": ("nmpc.h", ["handle", "as_force"])}


@pytest.fixture(autouse=True)
def push_cfg_pointer(monkeypatch):
    """the one argument type the shared header reader has not met: a pointer to a host structure, bound as a void pointer"""
    monkeypatch.setitem(abi_header.C_TYPES, "const nmpc_push_cfg *", ctypes.c_void_p)


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib, name):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration(ARGUMENTS[name][0], name)
    assert names == ARGUMENTS[name][1]
    assert getattr(lib, name) is not None
    assert _lib.SIGNATURES[name] == (ctypes.c_int, types)


def test_the_push_cfg_is_the_headers_struct():
    from iterative_learning_nmpc_amd import _lib
    fields = struct_fields("nmpc_torque.h", "nmpc_push_cfg")
    assert [n for n, _ in fields] == ["force", "force_rows", "joint", "first_substep", "n_substeps"]
    assert _lib.NmpcPushCfg._fields_ == fields
    assert ctypes.sizeof(_lib.NmpcPushCfg) == 24


def test_the_plant_calls_keep_their_signatures():
    """the push is attached by a call: the pinned argument lists are the ones they were"""
    assert len(declaration("nmpc_torque.h", "nmpc_contact_step_batch")[0]) == 17
    assert len(declaration("nmpc_torque.h", "nmpc_contact_track_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16


def test_python_layers_take_the_push():
    from iterative_learning_nmpc_amd import collect, learning
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    sp = inspect.signature(BatchedTorqueLayer.set_push).parameters
    assert list(sp) == ["self", "force", "start_substep", "n_substeps", "joint"]
    assert [sp[k].default for k in list(sp)[1:]] == [None, 0, 0, 5]
    for fn in (learning.evaluate_policy, learning.dagger_iteration):
        assert inspect.signature(fn).parameters["push"].default is None, fn.__name__
    for fn in (LocomotionMPC.open_loop_device, collect.collect_rollouts, learning.learning_iteration):
        assert inspect.signature(fn).parameters["push_as_force"].default is False, fn.__name__
    assert list(inspect.signature(BatchedNmpcSolver.set_rollout_plant_push).parameters) == ["self", "as_force"]
    assert "push" not in inspect.signature(BatchedTorqueLayer.policy_rollout).parameters


def test_a_null_handle_is_refused_on_the_host(lib):
    from iterative_learning_nmpc_amd import _lib
    cfg = _lib.NmpcPushCfg(None, 1, 5, 0, 1)
    assert lib.nmpc_contact_set_push(None, ctypes.byref(cfg)) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    assert lib.nmpc_contact_set_push(None, None) == -1
    assert lib.nmpc_wb_rollout_set_plant_push(None, 1) == -1
