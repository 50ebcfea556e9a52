"""Observed rows beside a rollout and input noise in training exist in every layer: nmpc_policy_rollout_set_observed and
nmpc_observed_rows_batch (include/nmpc_torque.h), nmpc_policy_set_input_noise, nmpc_policy_input_noise_epoch and
nmpc_policy_input_noise_batch (include/nmpc_policy.h) are declared, exported by libnmpc_hip.so and bound with the header's argument
lists; the calls that honour them keep their signatures; the Python layers take the options and validate host input.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests.abi_header import declaration, lib  # noqa: F401

P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong

PROTOTYPES = {
    ("nmpc_torque.h", "nmpc_policy_rollout_set_observed"): (["torque", "O", "o_rows"], [P, P, I]),
    ("nmpc_torque.h", "nmpc_observed_rows_batch"): (["torque", "B", "S", "s_stride", "O", "o_stride", "step", "stream"], [P, I, P, I, P, I, LL, P]),
    ("nmpc_policy.h", "nmpc_policy_set_input_noise"): (["policy", "sigma", "n", "seed", "epoch0"], [P, P, I, LL, LL]),
    ("nmpc_policy.h", "nmpc_policy_input_noise_epoch"): (["policy", "epoch"], [P, ctypes.POINTER(LL)]),
    ("nmpc_policy.h", "nmpc_policy_input_noise_batch"): (["policy", "B", "X", "x_stride", "s_std", "s_first", "epoch", "first_sample", "stream"],
                                                         [P, I, P, I, P, I, LL, LL, P]),
}


@pytest.mark.parametrize("header,name", list(PROTOTYPES))
def test_symbols_are_declared_exported_and_bound_as_the_header_declares_them(lib, header, name):
    from iterative_learning_nmpc_amd import _lib
    names, types = declaration(header, name)
    assert (names, types) == PROTOTYPES[header, name]
    assert getattr(lib, name) is not None
    assert _lib.SIGNATURES[name] == (I, types)


def test_a_null_handle_is_refused_on_the_host(lib):
    epoch = LL(5)
    for call in (lambda: lib.nmpc_policy_rollout_set_observed(None, None, 0), lambda: lib.nmpc_observed_rows_batch(None, 1, None, 44, None, 44, 0, None),
                 lambda: lib.nmpc_policy_set_input_noise(None, None, 0, 0, 0), lambda: lib.nmpc_policy_input_noise_epoch(None, ctypes.byref(epoch)),
                 lambda: lib.nmpc_policy_input_noise_batch(None, 1, None, 44, None, 1, 0, 0, None)):
        assert call() == -1
    assert epoch.value == 5


def test_the_calls_that_honour_them_keep_their_signatures():
    assert len(declaration("nmpc_torque.h", "nmpc_policy_rollout_batch")[0]) == 16
    assert len(declaration("nmpc_torque.h", "nmpc_observe_batch")[0]) == 19
    assert len(declaration("nmpc_torque.h", "nmpc_observe_noise_batch")[0]) == 8
    assert len(declaration("nmpc_policy.h", "nmpc_policy_train_step")[0]) == 8
    # (its struct argument is a declaration the shared parser does not read: the arguments are counted in the header's text)
    text = " ".join(open(os.path.join(os.path.dirname(__file__), "..", "include", "nmpc_policy.h")).read().split())
    args = re.search(r"\bint nmpc_policy_train_epoch\s*\(([^)]*)\)\s*;", text).group(1)
    assert len(args.split(",")) == 11 and args.startswith("void *handle, const nmpc_batch_source *src")


def test_python_layers_take_the_options():
    from iterative_learning_nmpc_amd import learning, policy, torque
    si = inspect.signature(policy.DevicePolicy.set_input_noise).parameters
    assert list(si) == ["self", "sigma", "seed", "epoch0"] and [si[k].default for k in ("sigma", "seed", "epoch0")] == [None, 0, 0]
    assert isinstance(policy.DevicePolicy.input_noise_epoch, property)
    no = inspect.signature(policy.DevicePolicy.input_noise).parameters
    assert list(no) == ["self", "X", "epoch", "first_sample", "s_std", "s_first"]
    assert [no[k].default for k in ("first_sample", "s_std", "s_first")] == [0, None, 1]
    assert list(inspect.signature(torque.BatchedTorqueLayer.set_rollout_observed).parameters) == ["self", "O"]
    ob = inspect.signature(torque.BatchedTorqueLayer.observed_rows).parameters
    assert list(ob) == ["self", "S", "step", "out"] and ob["out"].default is None
    assert list(inspect.signature(torque.training_sigma).parameters) == ["noise"]
    assert inspect.signature(learning.evaluate_policy).parameters["record_observed"].default is False
    tn = inspect.signature(learning.train_network).parameters
    assert tn["input_noise"].default is None and tn["input_noise_seed"].default == 0
    for f in (learning.learning_iteration, learning.dagger_iteration):
        p = inspect.signature(f).parameters
        assert p["train_noise"].default is None and p["train_noise_seed"].default == 0
    assert inspect.signature(learning.dagger_iteration).parameters["store"].default == "true"


def unbuilt_policy(n_in=47):
    """a policy that never reached a device: `set_input_noise` validates host input before it touches the library"""
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    p = DevicePolicy.__new__(DevicePolicy)
    p.dims, p._h, p._input_noise = (n_in, 12, 2, 32, False), None, None
    return p


@pytest.mark.parametrize("sigma,text", [(np.zeros(0), "expected"), (np.zeros(48), "expected"), (np.zeros((2, 44)), "expected"), (0.1, "expected"),
                                        ("loud", "need a float array"), (np.r_[np.zeros(5), np.nan], "must be finite"),
                                        (np.r_[np.zeros(5), np.inf], "must be finite"), (np.r_[0.1, -0.1], "must not be negative")])
def test_set_input_noise_refuses_bad_host_input(sigma, text):
    with pytest.raises(ValueError, match="input noise: sigma.*" + text):
        unbuilt_policy().set_input_noise(sigma)


def test_set_input_noise_refuses_an_epoch_out_of_range():
    for epoch0 in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="epoch0"):
            unbuilt_policy().set_input_noise(np.zeros(44), epoch0=epoch0)


def test_dagger_iteration_refuses_an_unknown_store_before_anything_runs():
    from iterative_learning_nmpc_amd import learning
    for store in ("seen", "", "True"):
        with pytest.raises(ValueError, match="store: expected 'true' or 'observed'"):
            learning.dagger_iteration(None, None, None, None, None, None, None, 0.1, store=store)
