"""The entry points of the push windows per rollout exist in every layer: nmpc_contact_set_push_windows (include/nmpc_torque.h),
nmpc_rollout_set_push_windows and nmpc_wb_rollout_set_push_windows (include/nmpc.h) are declared, exported by libnmpc_hip.so and
bound with the headers' argument lists; the structs the windows could have gone into are the ones they were.  No GPU: what is
decided on the host is checked."""
import ctypes
import inspect
import re

import pytest

from tests.abi_header import declaration, header, lib  # noqa: F401

ARGUMENTS = {"nmpc_contact_set_push_windows": ("nmpc_torque.h", ["torque", "first_substep", "n_substeps", "rows"]),
             "nmpc_rollout_set_push_windows": ("nmpc.h", ["handle", "start", "duration", "rows"]),
             "nmpc_wb_rollout_set_push_windows": ("nmpc.h", ["handle", "start", "duration", "rows"])}
# typedef -> (header, the binding's mirror, bytes, fields): as they were before there were windows per rollout
STRUCTS = {"nmpc_rollout_cfg": ("nmpc.h", "NmpcRolloutCfg", 152, 23), "nmpc_wb_rollout_cfg": ("nmpc.h", "NmpcWbRolloutCfg", 96, 20),
           "nmpc_push_cfg": ("nmpc_torque.h", "NmpcPushCfg", 24, 5), "nmpc_policy_rollout_cfg": ("nmpc_torque.h", "NmpcPolicyRolloutCfg", 56, 11)}


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_symbol_is_declared_exported_and_bound_as_the_header_declares_it(lib, name):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration(ARGUMENTS[name][0], name)
    assert names == ARGUMENTS[name][1]
    assert types == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert getattr(lib, name) is not None
    assert _lib.SIGNATURES[name] == (ctypes.c_int, types)


def header_field_names(header_file, typedef_name):
    """the field names of `typedef struct { ... } typedef_name;` in declaration order, array fields by their name"""
    body = re.search(r"typedef struct \{([^}]*)\} " + typedef_name + r";", header(header_file)).group(1)
    names = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.match(r"^(const )?(long long|int|float|double) (.+)$", decl)
        assert m, decl
        names += [re.match(r"^\*? ?(\w+)(\[\d+\])?$", n.strip()).group(1) for n in m.group(3).split(",")]
    return names


@pytest.mark.parametrize("typedef", sorted(STRUCTS))
def test_the_structs_are_unchanged_in_size_and_fields(typedef):
    from iterative_learning_nmpc_amd import _lib
    header_file, mirror, size, count = STRUCTS[typedef]
    cls = getattr(_lib, mirror)
    names = header_field_names(header_file, typedef)
    assert names == [n for n, _ in cls._fields_] and len(names) == count
    assert ctypes.sizeof(cls) == size
    assert not any("window" in n for n in names)


def test_the_window_fields_of_the_structs_are_the_scalars_they_were():
    from iterative_learning_nmpc_amd import _lib
    for cls in (_lib.NmpcRolloutCfg, _lib.NmpcWbRolloutCfg):
        f = dict(cls._fields_)
        assert f["push_start"] is ctypes.c_float and f["push_duration"] is ctypes.c_float
    f = dict(_lib.NmpcPushCfg._fields_)
    assert f["first_substep"] is ctypes.c_int and f["n_substeps"] is ctypes.c_int


def test_the_calls_that_take_a_push_keep_their_signatures():
    assert len(declaration("nmpc_torque.h", "nmpc_contact_step_batch")[0]) == 17
    assert len(declaration("nmpc_torque.h", "nmpc_contact_track_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16
    # (the rollout calls take argument types the shared reader does not bind: their arguments are counted)
    count = lambda name: len(re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header("nmpc.h")).group(1).split(","))      # noqa: E731
    assert count("nmpc_rollout_batch") == 17 and count("nmpc_wb_rollout_batch") == 19


def test_python_layers_take_the_windows():
    from iterative_learning_nmpc_amd import mpc
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    sp = inspect.signature(BatchedTorqueLayer.set_push).parameters
    assert list(sp) == ["self", "force", "start_substep", "n_substeps", "joint"]
    assert [sp[k].default for k in list(sp)[1:]] == [None, 0, 0, 5]
    assert list(inspect.signature(BatchedNmpcSolver.set_rollout_push_windows).parameters) == ["self", "start", "duration"]
    sw = inspect.signature(mpc.sample_push_windows).parameters
    assert list(sw) == ["n", "seed", "period", "n_points", "duration"]
    assert sw["n_points"].default == 10 and sw["duration"].default == (0.2, 0.4)
    assert list(inspect.signature(mpc.sample_pushes).parameters) == ["n", "seed", "start", "duration", "magnitude"]


def test_a_null_handle_is_refused_on_the_host(lib):
    assert lib.nmpc_contact_set_push_windows(None, None, None, 0) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    assert lib.nmpc_rollout_set_push_windows(None, None, None, 0) == -1
    assert lib.nmpc_wb_rollout_set_push_windows(None, None, None, 0) == -1
