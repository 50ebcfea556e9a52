"""The epoch and validation-loss entry points of include/nmpc_policy.h, as far as a machine without a GPU decides:
they are exported and bound, and what their argument checks refuse on the host comes back as NMPC_E_ARG with a message
in the policy family's error slot.  (A policy handle cannot be made without a device, so the checks behind the handle --
widths, batch range, learning rate -- are exercised in tests/test_gpu_train_epoch.py.)"""
import ctypes

import pytest

from tests.abi_header import lib, struct_fields  # noqa: F401

NEW = ("nmpc_policy_train_epoch_scratch", "nmpc_policy_train_epoch", "nmpc_policy_loss")


def test_new_symbols_are_exported_and_bound(lib):
    from iterative_learning_nmpc_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(raw, name) is not None
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_batch_source_mirrors_the_header():
    """field order and types of nmpc_batch_source, read from the header"""
    from iterative_learning_nmpc_amd import _lib
    assert struct_fields("nmpc_policy.h", "nmpc_batch_source") == list(_lib.NmpcBatchSource._fields_)


def test_epoch_and_loss_reject_bad_arguments_on_the_host(lib):
    from iterative_learning_nmpc_amd import _lib
    one = ctypes.c_void_p(8)                     # a non-null placeholder, never dereferenced on these paths
    src = _lib.NmpcBatchSource(one, 44, None, None, 1, one, 3, None, None, one, 12, 100)
    before = lib.nmpc_policy_last_error(None)
    # a null handle, with everything else in order: refused, and said so in the family's slot
    assert lib.nmpc_policy_train_epoch(None, ctypes.byref(src), one, 64, 2, 0, 1e-3, one, one, None, None) == -1
    msg = lib.nmpc_policy_last_error(None)
    assert msg and b"handle" in msg and msg != before
    # ... and with every other argument wrong as well: still NMPC_E_ARG, nothing is dereferenced
    assert lib.nmpc_policy_train_epoch(None, None, None, 0, -1, 0, 0.0, None, None, None, None) == -1
    assert lib.nmpc_policy_train_epoch(None, ctypes.byref(src), one, 64, 0, 0, 1e-3, one, one, None, None) == -1
    assert lib.nmpc_policy_loss(None, 4, one, one, one, None) == -1
    assert lib.nmpc_policy_loss(None, 0, None, None, None, None) == -1
    assert b"handle" in lib.nmpc_policy_last_error(None)
    # the other families' slots are theirs
    assert not lib.nmpc_dataset_last_error() or b"handle" not in lib.nmpc_dataset_last_error()


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 100000, 10 ** 7, 2 ** 31 - 1])
def test_epoch_scratch_covers_the_prefix_sums_and_their_block_totals(lib, n):
    """n sums, a total per 2048-row block (ceil(n / 2048) of them) and the grand total"""
    got = lib.nmpc_policy_train_epoch_scratch(n)
    assert got >= n + n // 2048 + 2
    assert got >= n + -(-n // 2048) + 1
    assert got < n + n // 2048 + 64              # a size rule, not a guess on the safe side
    assert lib.nmpc_policy_train_epoch_scratch(0) == 0 and lib.nmpc_policy_train_epoch_scratch(-5) == 0
