"""ctypes binding of libnmpc_hip.so (include/nmpc.h).  No fallback: if the HIP library is missing
or does not load, importing callers get a loud ImportError -- there is no CPU path in the product."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# NMPC_HIP_LIB points diagnostics (tools/) at an alternative build of the same C-ABI
LIB_PATH = os.environ.get("NMPC_HIP_LIB") or os.path.join(_HERE, "libnmpc_hip.so")

# the C-ABI constants of include/nmpc.h (tests/test_abi.py checks them against the header)
NMPC_OK = 0
NMPC_STATUS_OK, NMPC_STATUS_NAN, NMPC_STATUS_MAXITER, NMPC_STATUS_MINSTEP, NMPC_STATUS_QP = 0, 1, 2, 3, 4
STATUS_NAMES = {NMPC_STATUS_OK: "ok", NMPC_STATUS_NAN: "nan", NMPC_STATUS_MAXITER: "max_iter",
                NMPC_STATUS_MINSTEP: "min_step", NMPC_STATUS_QP: "qp_failure"}
# bits of a rollout's failed[b]; above NMPC_ROLLOUT_TERM_SHIFT: 1 + the replan that terminated the rollout
NMPC_ROLLOUT_FLAG_SOLVER = 1
NMPC_ROLLOUT_FLAG_ROLL = 2
NMPC_ROLLOUT_FLAG_PITCH = 4
NMPC_ROLLOUT_FLAG_HEIGHT = 8
NMPC_ROLLOUT_FLAG_VEL_TRACKING = 16
NMPC_ROLLOUT_FLAG_COLLISION = 32
NMPC_ROLLOUT_FLAG_JOINT_LIMIT = 64      # whole-body rollouts only
NMPC_ROLLOUT_FLAG_MASK = 0xFF
NMPC_ROLLOUT_TERM_SHIFT = 8
# the integrators of the contact plant (include/nmpc_torque.h, nmpc_contact_set_integrator)
NMPC_INTEGRATOR_EXPLICIT = 0
NMPC_INTEGRATOR_LINEARLY_IMPLICIT = 1
# the deepest shift register of a delay line (include/nmpc_torque.h, nmpc_contact_set_delays)
NMPC_DELAY_MAX_DEPTH = 64
# the deepest observation or action history on the policy input (include/nmpc_torque.h, nmpc_policy_rollout_set_history)
NMPC_HISTORY_MAX = 16

# every symbol include/*.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "nmpc_model_dims": (c_int, [c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "nmpc_model_output_dims": (c_int, [c_int, POINTER(c_int), POINTER(c_int)]),
    "nmpc_create": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "nmpc_destroy": (None, [c_void_p]),
    "nmpc_last_error": (c_char_p, [c_void_p]),
    "nmpc_workspace_bytes": (c_size_t, [c_void_p]),
    "nmpc_set_model_params": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "nmpc_set_weights": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_float, c_float]),
    "nmpc_set_opts": (c_int, [c_void_p, c_int, c_int, c_float, c_float, c_int]),
    "nmpc_set_contact_patterns": (c_int, [c_void_p, c_int]),
    "nmpc_set_skip": (c_int, [c_void_p, c_void_p, c_int]),
    "nmpc_wb_rollout_set_actions": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p]),
    "nmpc_wb_rollout_set_plant": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_wb_rollout_set_plant_push": (c_int, [c_void_p, c_int]),
    "nmpc_wb_rollout_set_clock": (c_int, [c_void_p, c_int]),
    "nmpc_rollout_set_push_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "nmpc_wb_rollout_set_push_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "nmpc_wb_set_momentum_model": (c_int, [c_void_p, c_void_p, c_int]),
    "nmpc_wb_set_state_momentum": (c_int, [c_void_p, c_int]),
    "nmpc_set_ipm": (c_int, [c_void_p, c_float, c_float, c_float, c_float, c_float, c_float]),
    "nmpc_shift_warm_start": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "nmpc_solve_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_shift_solve_batch": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_riccati_batch": (c_int, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 12),
    "nmpc_tracking_error": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_float, c_float, c_void_p]),
    "nmpc_rollout_batch": (c_int, [c_void_p, c_int, c_void_p] + [c_void_p] * 14),
    "nmpc_wb_rollout_batch": (c_int, [c_void_p, c_int, c_void_p] + [c_void_p] * 16),
    "nmpc_wb_label_states_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_void_p] * 6 + [c_int] + [c_void_p] * 7
                                   + [c_int] + [c_void_p] * 4),
    # include/nmpc_policy.h
    "nmpc_policy_create": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "nmpc_policy_destroy": (None, [c_void_p]),
    "nmpc_policy_last_error": (ctypes.c_char_p, [c_void_p]),
    "nmpc_policy_param_count": (ctypes.c_size_t, [c_void_p]),
    "nmpc_policy_get_dims": (c_int, [c_void_p, c_void_p, POINTER(c_int)]),
    "nmpc_policy_set_params": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_get_params": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_get_opt_state": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(ctypes.c_longlong), c_void_p]),
    "nmpc_policy_set_opt_state": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p]),
    "nmpc_policy_forward": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_train_step": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "nmpc_weighted_sample": (c_int, [c_void_p, ctypes.c_longlong, c_int, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p]),
    "nmpc_gather_rows": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "nmpc_policy_train_epoch_scratch": (ctypes.c_size_t, [ctypes.c_longlong]),
    "nmpc_policy_train_epoch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_ulonglong, c_float, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_loss": (c_int, [c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_set_input_noise": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong]),
    "nmpc_policy_input_noise_epoch": (c_int, [c_void_p, POINTER(ctypes.c_longlong)]),
    "nmpc_policy_input_noise_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong, c_void_p]),
    # include/nmpc_dataset.h
    "nmpc_dataset_last_error": (ctypes.c_char_p, []),
    "nmpc_ring_append": (c_int, [c_void_p, c_int, ctypes.c_longlong, c_void_p, ctypes.c_longlong, ctypes.c_longlong, c_void_p]),
    "nmpc_column_stats_scratch": (ctypes.c_size_t, [c_int]),
    "nmpc_column_stats": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_assemble_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p, c_int, ctypes.c_longlong, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    # include/nmpc_torque.h
    "nmpc_torque_create": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "nmpc_torque_destroy": (None, [c_void_p]),
    "nmpc_torque_last_error": (ctypes.c_char_p, [c_void_p]),
    "nmpc_id_torques_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_fd_accel_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_fd_step_batch": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_mass_matrix_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "nmpc_centroidal_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_centroidal_derivatives_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_state_momentum_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                          c_void_p]),
    "nmpc_foot_kinematics_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_contact_forces_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_contact_step_batch": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                        c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_contact_set_push": (c_int, [c_void_p, c_void_p]),
    "nmpc_contact_set_push_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "nmpc_contact_set_grounds": (c_int, [c_void_p, c_void_p, c_int]),
    "nmpc_contact_set_payloads": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "nmpc_contact_set_actuators": (c_int, [c_void_p, c_void_p, c_int]),
    "nmpc_contact_set_delays": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int]),
    "nmpc_delay_line_batch": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "nmpc_contact_set_noise": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong]),
    "nmpc_contact_noise_step": (c_int, [c_void_p, POINTER(ctypes.c_longlong)]),
    "nmpc_observe_noise_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_void_p]),
    "nmpc_contact_set_integrator": (c_int, [c_void_p, c_int]),
    "nmpc_observe_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, ctypes.c_double, ctypes.c_double, c_void_p, c_int, c_void_p,
                                   c_void_p, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "nmpc_policy_rollout_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "nmpc_policy_rollout_set_states": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "nmpc_policy_rollout_set_observed": (c_int, [c_void_p, c_void_p, c_int]),
    "nmpc_observed_rows_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_void_p]),
    "nmpc_history_push_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                        c_void_p, c_int, c_void_p, c_void_p]),
    "nmpc_history_push_actions_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "nmpc_policy_rollout_set_history": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int]),
    "nmpc_contact_track_batch": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_float, c_float, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "nmpc_observe_rows_batch": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, c_float, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "nmpc_pd_torques_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                      c_void_p, c_void_p]),
    "nmpc_pd_target_action_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                            c_void_p, c_void_p]),
    "nmpc_plan_actions_batch": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_double,
                                        ctypes.c_double, c_float, c_float, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "nmpc_debug_read_tile": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_float)]),
    "nmpc_debug_set_buffer": (c_int, [c_void_p, c_void_p]),
    "nmpc_debug_read_workspace": (c_int, [c_void_p, c_int, c_size_t, c_size_t, POINTER(c_float)]),
    "nmpc_debug_wb_layout": (c_int, [c_int, POINTER(c_size_t)]),
    "nmpc_debug_read_momentum": (c_int, [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float)]),
    "nmpc_debug_read_rollout_problem": (c_int, [c_void_p, c_int, POINTER(c_float), POINTER(c_float)]),
    "nmpc_debug_read_centroidal_rollout_problem": (c_int, [c_void_p, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
}


class NmpcPolicyDims(ctypes.Structure):
    _fields_ = [("n_in", c_int), ("n_out", c_int), ("n_hidden", c_int), ("hidden", c_int),
                ("batch_norm", c_int), ("batch_max", c_int)]


class NmpcBatchSource(ctypes.Structure):
    _fields_ = [("states", c_void_p), ("n_state", c_int), ("s_mean", c_void_p), ("s_std", c_void_p), ("s_first", c_int),
                ("goals", c_void_p), ("n_goal", c_int), ("g_mean", c_void_p), ("g_std", c_void_p),
                ("actions", c_void_p), ("n_action", c_int), ("n_rows", ctypes.c_longlong)]


class NmpcTreeModel(ctypes.Structure):
    _fields_ = [("n_joints", c_int), ("n_actuated", c_int), ("n_feet", c_int),
                ("parent", POINTER(c_int)), ("type", POINTER(c_int)), ("axis", POINTER(c_float)),
                ("placement", POINTER(c_float)), ("mass", POINTER(c_float)), ("com", POINTER(c_float)),
                ("inertia", POINTER(c_float)), ("foot_joint", POINTER(c_int)), ("foot_offset", POINTER(c_float)),
                ("gravity", c_float * 3)]


class NmpcContactCfg(ctypes.Structure):
    _fields_ = [("ground_z", c_float), ("stiffness", c_float), ("damping", c_float), ("mu", c_float),
                ("slip_velocity", c_float), ("tau_max", c_float)]


class NmpcPushCfg(ctypes.Structure):
    _fields_ = [("force", c_void_p), ("force_rows", c_int), ("joint", c_int), ("first_substep", c_int), ("n_substeps", c_int)]


class NmpcPolicyRolloutCfg(ctypes.Structure):
    _fields_ = [("n_steps", c_int), ("n_sub", c_int), ("dt", c_float), ("kp", c_float), ("kd", c_float),
                ("t0", ctypes.c_double), ("period", ctypes.c_double), ("collision_height", c_float),
                ("term_mask", c_int), ("n_goal", c_int), ("s_first", c_int)]


class NmpcRolloutCfg(ctypes.Structure):
    _fields_ = [("n_replans", c_int), ("nodes_per_replan", c_int), ("replanning_steps", c_int),
                ("nodes_per_cycle", c_int), ("start_node", c_int), ("first_solve", c_int),
                ("max_sqp_first", c_int), ("nlp_tol_first", c_float), ("nlp_tol", c_float),
                ("sim_dt", ctypes.c_double), ("time_horizon", ctypes.c_double), ("nom_height", ctypes.c_double),
                ("height_offset", ctypes.c_double), ("push_start", c_float), ("push_duration", c_float),
                ("footsteps", c_int), ("record_sim_steps", c_int), ("hip_offset", c_float * 8),
                ("stance_ratio", c_float * 4), ("nominal_period", c_float), ("foot_size", c_float),
                ("terminate_mask", c_int), ("collision_height", c_float)]


class NmpcWbRolloutCfg(ctypes.Structure):
    _fields_ = [("n_replans", c_int), ("replanning_steps", c_int), ("nodes_per_cycle", c_int), ("first_solve", c_int),
                ("last_node", c_int), ("max_sqp_first", c_int), ("nlp_tol_first", c_float), ("nlp_tol", c_float),
                ("sim_dt", ctypes.c_double), ("time_horizon", ctypes.c_double), ("nom_height", ctypes.c_double),
                ("height_offset", ctypes.c_double), ("step_height", c_float), ("push_start", c_float), ("push_duration", c_float),
                ("record_sim_steps", c_int), ("force_reference_gravity", c_int), ("nominal_period", c_float),
                ("terminate_mask", c_int), ("collision_height", c_float)]


class NmpcWbLabelCfg(ctypes.Structure):
    _fields_ = [("n_rows", c_int), ("nodes_per_cycle", c_int), ("max_sqp", c_int), ("nlp_tol", c_float),
                ("sim_dt", ctypes.c_double), ("time_horizon", ctypes.c_double), ("nom_height", ctypes.c_double),
                ("height_offset", ctypes.c_double), ("step_height", c_float), ("force_reference_gravity", c_int),
                ("kp", c_float), ("kd", c_float), ("terminate_mask", c_int)]


class NmpcDims(ctypes.Structure):
    _fields_ = [("model_id", c_int), ("N", c_int), ("B_max", c_int), ("precision", c_int)]


_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP library once; raise ImportError with build instructions if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or iterative_learning_nmpc_amd/csrc/build.sh). "
            "This package has no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise ImportError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


class NmpcError(RuntimeError):
    pass


# the last-error call of each family of the C-ABI (the dataset calls keep one error per process and take no handle)
_LAST_ERROR = {"solve": "nmpc_last_error", "policy": "nmpc_policy_last_error", "torque": "nmpc_torque_last_error",
               "dataset": "nmpc_dataset_last_error"}


def check(rc: int, handle=None, what: str = "", family: str = "solve") -> None:
    """Raise NmpcError for a non-zero return code, with the library's text of the family's last error."""
    if rc != NMPC_OK:
        last_error = getattr(load(), _LAST_ERROR[family])
        msg = last_error() if family == "dataset" else last_error(handle)
        raise NmpcError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t: Optional[torch.Tensor]) -> Optional[c_void_p]:
    """a tensor's device address as a pointer argument (None: NULL)"""
    return None if t is None else c_void_p(t.data_ptr())


def stream(device) -> c_void_p:
    """the current stream of `device` as the stream argument"""
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)
