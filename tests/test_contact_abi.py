"""The contact-plant entry points of include/nmpc_torque.h exist in every layer: exported by libnmpc_hip.so, bound with the
header's argument lists, and behind methods of BatchedTorqueLayer.  No GPU: what is decided on the host is checked."""
import ctypes
import dataclasses
import inspect

import pytest

from tests.abi_header import declaration, lib, struct_fields  # noqa: F401

NAMES = ("nmpc_foot_kinematics_batch", "nmpc_contact_forces_batch", "nmpc_contact_step_batch")


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
    assert [len(header_arguments(n)) for n in NAMES] == [7, 7, 17]


def test_the_cfg_structure_has_the_headers_fields():
    from iterative_learning_nmpc_amd import _lib
    fields = struct_fields("nmpc_torque.h", "nmpc_contact_cfg")
    names = [n for n, _ in fields]
    assert names == ["ground_z", "stiffness", "damping", "mu", "slip_velocity", "tau_max"]
    assert fields == [(n, ctypes.c_float) for n in names]
    assert [(n, t) for n, t in _lib.NmpcContactCfg._fields_] == fields


def test_layer_has_the_methods_and_the_defaults():
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, GroundContact
    from iterative_learning_nmpc_amd.trajectory_io import KD, KP
    assert list(inspect.signature(BatchedTorqueLayer.foot_kinematics).parameters) == ["self", "q", "v"]
    assert inspect.signature(BatchedTorqueLayer.foot_kinematics).parameters["v"].default is None
    assert list(inspect.signature(BatchedTorqueLayer.contact_forces).parameters) == ["self", "q", "v", "ground"]
    step = inspect.signature(BatchedTorqueLayer.contact_step).parameters
    assert list(step) == ["self", "q", "v", "dt", "n_sub", "tau_ff", "q_des", "kp", "kd", "ground"]
    assert (step["n_sub"].default, step["tau_ff"].default, step["q_des"].default, step["kp"].default, step["kd"].default) == (1, None, None, KP, KD)
    assert step["ground"].default == GroundContact()
    assert dataclasses.asdict(GroundContact()) == dict(ground_z=0.0, stiffness=1e4, damping=3.0, mu=0.8, slip_velocity=0.05, tau_max=None)
    cfg = GroundContact(tau_max=5.0, ground_z=-1.0).cfg()
    assert (cfg.ground_z, cfg.stiffness, cfg.tau_max) == (-1.0, 1e4, 5.0) and GroundContact().cfg().tau_max == 0.0


def test_the_references_defaults_are_the_layers():
    from iterative_learning_nmpc_amd.torque import GroundContact
    from tests.contact_reference import Ground
    assert dataclasses.asdict(Ground()) == dataclasses.asdict(GroundContact())


def test_a_null_handle_is_refused_on_the_host(lib):
    from iterative_learning_nmpc_amd import _lib
    cfg = _lib.NmpcContactCfg(0.0, 1e4, 3.0, 0.8, 0.05, 0.0)
    assert lib.nmpc_foot_kinematics_batch(None, 1, None, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    assert lib.nmpc_contact_forces_batch(None, 1, ctypes.byref(cfg), None, None, None, None) == -1
    assert lib.nmpc_contact_step_batch(None, 1, 1, 5e-4, ctypes.byref(cfg), None, None, None, None, 0.0, 0.0, None, None, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
