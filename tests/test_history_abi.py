"""The history on the policy input exists in every layer: nmpc_history_push_batch, nmpc_history_push_actions_batch and
nmpc_policy_rollout_set_history (include/nmpc_torque.h) are declared, exported by libnmpc_hip.so and bound with the header's argument
lists; NMPC_HISTORY_MAX is one number in the header and in Python; the calls that honour the attachment keep their signatures; what
the Python layers decide on the host is decided rightly.  No GPU."""
import ctypes
import inspect
import re

import pytest

from tests.abi_header import declaration, header, lib  # noqa: F401

P, I = ctypes.c_void_p, ctypes.c_int


def test_symbols_are_declared_exported_and_bound_as_the_header_declares_them(lib):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration("nmpc_torque.h", "nmpc_history_push_batch")
    assert names == ["torque", "B", "hist", "n_obs", "act", "n_act", "goal", "n_goal", "s_mean", "s_std", "s_first", "W", "w_stride", "X", "stream"]
    assert types == [P, I, P, I, P, I, P, I, P, P, I, P, I, P, P]
    assert lib.nmpc_history_push_batch is not None
    assert _lib.SIGNATURES["nmpc_history_push_batch"] == (I, types)
    names, types = declaration("nmpc_torque.h", "nmpc_history_push_actions_batch")
    assert names == ["torque", "B", "act", "n_act", "A", "a_stride", "stream"]
    assert types == [P, I, P, I, P, I, P]
    assert lib.nmpc_history_push_actions_batch is not None
    assert _lib.SIGNATURES["nmpc_history_push_actions_batch"] == (I, types)
    names, types = declaration("nmpc_torque.h", "nmpc_policy_rollout_set_history")
    assert names == ["torque", "hist", "n_obs", "act", "n_act", "W", "w_rows", "rows"]
    assert types == [P, P, I, P, I, P, I, I]
    assert lib.nmpc_policy_rollout_set_history is not None
    assert _lib.SIGNATURES["nmpc_policy_rollout_set_history"] == (I, types)


def test_the_deepest_history_is_one_number():
    from iterative_learning_nmpc_amd import _lib, torque
    m = re.search(r"#define\s+NMPC_HISTORY_MAX\s+(\d+)", header("nmpc_torque.h"))
    assert m and int(m.group(1)) == _lib.NMPC_HISTORY_MAX == torque.HISTORY_MAX == 16
    assert torque.history_width(1, 0) == 44 and torque.history_width(3, 2) == 156 and torque.history_width(16, 16) == 896


def test_a_null_handle_is_refused_on_the_host(lib):
    for call in (lambda: lib.nmpc_policy_rollout_set_history(None, None, 0, None, 0, None, 0, 0),
                 lambda: lib.nmpc_history_push_batch(None, 1, None, 1, None, 0, None, 0, None, None, 0, None, 0, None, None),
                 lambda: lib.nmpc_history_push_actions_batch(None, 1, None, 1, None, 12, None)):
        assert call() == -1
        assert b"handle" in lib.nmpc_torque_last_error(None)


def test_the_calls_that_honour_the_history_keep_their_signatures():
    assert len(declaration("nmpc_torque.h", "nmpc_observe_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16
    assert len(declaration("nmpc_torque.h", "nmpc_observed_rows_batch")[0]) == 8
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_set_observed")[0]) == 3


def test_python_layers_take_the_history():
    from iterative_learning_nmpc_amd import learning, torque
    L = torque.BatchedTorqueLayer
    sh = inspect.signature(L.set_history).parameters
    assert list(sh) == ["self", "n_obs", "n_act", "batch"] and sh["n_obs"].default == 1 and sh["n_act"].default == 0
    hp = inspect.signature(L.history_push).parameters
    assert list(hp) == ["self", "goal", "s_mean", "s_std", "s_first", "W"] and hp["s_first"].default == 1 and hp["W"].default is None
    assert list(inspect.signature(L.history_push_actions).parameters) == ["self", "A"]
    assert list(inspect.signature(L.reset_history).parameters) == ["self", "S0", "q"]
    assert list(inspect.signature(L.set_rollout_wide).parameters) == ["self", "W"]
    assert list(inspect.signature(L.history_table).parameters)[:5] == ["self", "O", "A", "S0", "q0"]
    assert isinstance(L.history, property) and isinstance(L.action_history, property)
    for f in (learning.evaluate_policy, learning.dagger_iteration):
        assert inspect.signature(f).parameters["history"].default is None


@pytest.mark.parametrize("n_obs,n_act,text", [(0, 0, "n_obs must be in"), (17, 0, "n_obs must be in"), (1, -1, "n_act must be in"), (1, 17, "n_act must be in")])
def test_bad_depths_are_refused_on_the_host(n_obs, n_act, text):
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    L = BatchedTorqueLayer.__new__(BatchedTorqueLayer)      # a layer that never reached a device
    with pytest.raises(ValueError, match="history: " + text):
        L.set_history(n_obs, n_act, batch=2)
    with pytest.raises(ValueError, match="history: " + text):
        L._history_depths(n_obs, n_act)
    with pytest.raises(ValueError, match="history: batch is needed"):
        L.set_history(1, 0)
