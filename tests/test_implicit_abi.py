"""The integrator of the contact plant exists in every layer: nmpc_contact_set_integrator and the two NMPC_INTEGRATOR_* constants
(include/nmpc_torque.h) are declared, exported by libnmpc_hip.so and bound as the header declares them; the Python layers take
the `integrator=` keyword (the three plant calls of the layer keep the parameter lists tests/test_contact_abi.py,
tests/test_contact_track_abi.py and tests/test_policy_rollout_abi.py pin: there the integrator is `set_integrator`'s) and refuse an unknown name before anything runs.  No GPU: what is decided on the host is checked."""
import ctypes
import inspect
import re

import pytest

from tests.abi_header import declaration, header, lib  # noqa: F401


def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", "nmpc_contact_set_integrator")
    assert names == ["torque", "mode"]
    assert lib.nmpc_contact_set_integrator is not None
    assert _lib.SIGNATURES["nmpc_contact_set_integrator"] == (ctypes.c_int, types)


def test_the_constants_are_the_headers():
    from iterative_learning_nmpc_amd import _lib, torque
    defines = dict(re.findall(r"#define\s+(NMPC_INTEGRATOR_\w+)\s+(\d+)", header("nmpc_torque.h")))
    assert defines == {"NMPC_INTEGRATOR_EXPLICIT": "0", "NMPC_INTEGRATOR_LINEARLY_IMPLICIT": "1"}
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value)
    assert torque.INTEGRATORS == {"explicit": 0, "implicit": 1}


def test_a_null_handle_is_refused_with_text(lib):
    assert lib.nmpc_contact_set_integrator(None, 1) == -1
    assert b"null" in lib.nmpc_torque_last_error(None)


def test_the_plant_calls_keep_their_signatures():
    """the integrator is set by a call: the pinned argument lists are the ones they were"""
    assert len(declaration("nmpc_torque.h", "nmpc_contact_step_batch")[0]) == 17
    assert len(declaration("nmpc_torque.h", "nmpc_contact_track_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16


def test_python_layers_take_the_integrator_and_refuse_unknown_names():
    from iterative_learning_nmpc_amd import collect, learning
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer, integrator_mode
    takers = (learning.evaluate_policy, learning.dagger_iteration, learning.learning_iteration, collect.collect_rollouts, LocomotionMPC.open_loop_device)
    for fn in takers:
        assert inspect.signature(fn).parameters["integrator"].default is None, fn.__qualname__
    assert list(inspect.signature(BatchedTorqueLayer.set_integrator).parameters) == ["self", "integrator"]
    assert integrator_mode("explicit") == 0 and integrator_mode("implicit") == 1
    for bad in ("rk4", "Implicit", "", 1, None):
        with pytest.raises(ValueError, match="integrator"):
            integrator_mode(bad)
    # every taker refuses the name before it touches a device: a layer that was never created is enough
    L = BatchedTorqueLayer.__new__(BatchedTorqueLayer)
    for call in (lambda: L.set_integrator("rk4"),
                 lambda: learning.evaluate_policy(L, None, None, None, None, None, 1.0, integrator="rk4"),
                 lambda: learning.dagger_iteration(None, L, None, None, None, None, None, 1.0, integrator="rk4"),
                 lambda: LocomotionMPC.open_loop_device(None, None, None, 1.0, plant=object(), integrator="rk4")):
        with pytest.raises(ValueError, match="integrator"):
            call()
    with pytest.raises(ValueError, match="give plant"):
        LocomotionMPC.open_loop_device(None, None, None, 1.0, integrator="implicit")
