"""The optimiser-state entry points of include/nmpc_policy.h (nmpc_policy_get_opt_state, nmpc_policy_set_opt_state), as far
as a machine without a GPU decides: they are exported and bound with the declared signatures, and a null handle comes back
as NMPC_E_ARG with a message in the policy family's error slot.  (A policy handle cannot be made without a device: the
checks behind the handle -- null moments, a negative step -- and the copies are exercised in tests/test_gpu_policy_grad.py.)"""
import ctypes

from tests.abi_header import declaration, lib  # noqa: F401

NEW = ("nmpc_policy_get_opt_state", "nmpc_policy_set_opt_state")


def test_new_symbols_are_exported_and_bound(lib):
    from iterative_learning_nmpc_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(raw, name) is not None
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_signatures_mirror_the_header():
    """argument by argument, read from the header: pointers to device memory and the stream are void pointers in the
    binding, `long long *step` is a pointer to a long long, `long long step` a long long"""
    from iterative_learning_nmpc_amd import _lib
    for name in NEW:
        want = declaration("nmpc_policy.h", name)[1]                 # an `int name(...)`, or it is not found
        assert ctypes.POINTER(ctypes.c_longlong) in want or ctypes.c_longlong in want
        assert _lib.SIGNATURES[name] == (ctypes.c_int, want), (name, want)


def test_a_null_handle_is_refused_with_a_message_in_the_family_slot(lib):
    one = ctypes.c_void_p(8)                     # a non-null placeholder, never dereferenced on these paths
    step = ctypes.c_longlong(-7)
    before = lib.nmpc_dataset_last_error()
    assert lib.nmpc_policy_loss(None, 4, one, one, one, None) == -1              # something else in the slot first
    assert b"opt_state" not in lib.nmpc_policy_last_error(None)
    assert lib.nmpc_policy_get_opt_state(None, one, one, ctypes.byref(step), None) == -1
    msg = lib.nmpc_policy_last_error(None)
    assert msg and b"get_opt_state" in msg and b"handle" in msg
    assert step.value == -7                                                      # nothing was written
    assert lib.nmpc_policy_get_opt_state(None, None, None, None, None) == -1
    assert lib.nmpc_policy_set_opt_state(None, one, one, 3, None) == -1
    msg = lib.nmpc_policy_last_error(None)
    assert msg and b"set_opt_state" in msg and b"handle" in msg
    # ... and with every other argument wrong as well: still NMPC_E_ARG, nothing is dereferenced
    assert lib.nmpc_policy_set_opt_state(None, None, None, -1, None) == -1
    # the other families' slots are theirs
    assert lib.nmpc_dataset_last_error() == before
