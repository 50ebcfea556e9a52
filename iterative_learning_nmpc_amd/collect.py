"""Rollouts -> database, on the device: the data-collection step of one learning iteration.

The reference rolls the expert out, records (state, goal, action) per simulation step (DAgger/utils/RolloutMPC.py:168-258),
drops the rollouts that ended early (RolloutMPC.py:424-437) and appends the rest to its database
(DAgger/utils/database.py:105-154); the out-of-distribution rule then weights what the training step samples
(Behavior_Cloning/utils/data_collection_force_perturbation.py:138-156).  Here the rollouts are one `open_loop_device`
with the action labels recorded beside the state rows, and the rows go from that call's buffers into the
`DeviceDatabase` tables without passing through the host."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .config import TERMINATE_DEFAULT
from .parallel import learning_update, ood_threshold
from .solver import tracking_error


def collect_rollouts(mpc, layer, db, q0, v0, T: float, push: Optional[dict] = None, nominal: int = 0, ood_weight: float = 5.0,
                     terminate_mask: int = TERMINATE_DEFAULT, kp: Optional[float] = None, kd: Optional[float] = None, plant=None,
                     plant_substeps: int = 2, push_as_force: bool = False, integrator: Optional[str] = None,
                     chunk_replans: Optional[int] = None):
    """One batch of whole-body expert rollouts of `T` seconds into `db`.

    mpc: a `LocomotionMPC` (batch B, command set); layer: the robot's `BatchedTorqueLayer`; db: a `DeviceDatabase` with
    44-slot states and 12-slot actions; rollout `nominal` is the unperturbed one the others are measured against.
    Rows of the valid rollouts -- those that no bit of `terminate_mask` ended -- are appended in rollout order with the goal
    the recorder stores (the commanded v_des, one copy per row).  Returns (err [B, K] tracking errors against the nominal
    rollout on the reference's own 44-slot row and its own threshold 4.0, weights [B, K] of
    `parallel.learning_update`: 0 on invalid rollouts, `ood_weight` where err > 4.0, else 1; rows appended).  The weights of
    the appended rows go into the database with them (`db.weights`).
    plant (a `torque.GroundContact`, None: the plant follows the plan): the expert runs in closed loop on the ground-contact
    plant with `plant_substeps` substeps per simulation step (`open_loop_device`): the rows are then states of the plant, each
    with the PD target the expert applied from it.  push: the dict of `mpc.sample_pushes`, whose "start" and "duration" may
    be arrays of B (a window per rollout, e.g. merged from `mpc.sample_push_windows`), with or without `chunk_replans`.  kp, kd: as `open_loop_device` (None: its defaults).  push_as_force (with
    plant): the push is a force on the plant's trunk instead of a velocity jump per replanning interval.  integrator (with
    plant): the plant's integrator, as `open_loop_device` takes it (None: as the layer is set).  A ground, a payload, an actuator or a delay per
    rollout takes no keyword: a table attached on `layer` (`set_grounds`, `set_payloads`, `set_actuators`, `set_delays`) is seen by the plant of this call.
    After the call `mpc.actions`, `mpc.failed` and the returned S of the rollout are as `open_loop_device` leaves them
    (`mpc.states` keeps S).
    chunk_replans (None: one call, as above): the rollout runs as stretches of `chunk_replans` replans, the last one shorter --
    the first a cold start, the others `open_loop_device(resume=True)` from the state the one before left --, and each
    stretch's rows, labels and weights are appended before the next one runs, so that S and the labels are never larger than
    one stretch (`mpc.states`, `mpc.actions`: the last one's).  The replans are those the one call makes for `T`, all of them
    whole intervals: where `T` ends inside an interval, the stretches run it to its end.  The rows of a stretch are those of the
    one call, bit for bit, and so are their errors and weights (the nominal rollout is in every stretch); the database
    holds them stretch by stretch, within a stretch in rollout order.  A stretch appends the rollouts that are valid at its
    end: a rollout that terminates contributes nothing from that stretch on -- no row at or beyond its stamp -- but keeps the
    stretches before it, which the one call, seeing the whole rollout invalid, leaves out.  err and weights are the
    stretches' side by side, [B, K]."""
    run = dict(push=push, record_sim_steps=True, terminate_mask=terminate_mask, torque_layer=layer, kp=kp, kd=kd, plant=plant,
               plant_substeps=plant_substeps, push_as_force=push_as_force, integrator=integrator)
    if chunk_replans is None:
        S = mpc.open_loop_device(q0, v0, T, **run).contiguous()
        mpc.states = S
        return _append_valid(mpc, db, S, nominal, ood_weight, terminate_mask)
    if int(chunk_replans) < 1:
        raise ValueError("chunk_replans must be at least 1")
    total = len(mpc.replan_clock(T)[1])
    q, v, done, parts = q0, v0, 0, []
    while done < total:
        k = min(int(chunk_replans), total - done)
        S = mpc.open_loop_device(q, v, None, n_replans=k, resume=done > 0, **run).contiguous()
        mpc.states = S
        parts.append(_append_valid(mpc, db, S, nominal, ood_weight, terminate_mask))
        q, v, done = mpc.q_final, mpc.v_final, done + k
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), sum(p[2] for p in parts)


def _append_valid(mpc, db, S, nominal: int, ood_weight: float, terminate_mask: int):
    """the rows S [B, K, 44] of the rollout (or stretch) `mpc` has just run, with `mpc.actions` and their weights, into `db`
    -> (err, weights, rows appended) of `collect_rollouts`"""
    A = mpc.actions
    B, K = S.shape[:2]
    threshold = ood_threshold(S.shape[2])                     # 4.0 on the 44-slot row: the reference's number, no mapping
    err, _ = tracking_error(S, S[nominal].contiguous(), threshold=threshold, ood_weight=ood_weight)
    valid = (mpc.failed & int(terminate_mask)) == 0
    _, weights = learning_update(err, threshold, ood_weight, valid)
    keep = torch.nonzero(valid).squeeze(1)                    # device index of the valid rollouts, in rollout order
    n_rows = int(keep.numel()) * K
    if n_rows:
        # the goal the recorder stores with every row (trajectory_io.TrajectoryRecorder.vc_goals): the rollout's commanded v_des
        goals = torch.as_tensor(np.broadcast_to(np.asarray(mpc.v_des, float), (B, 3)).copy(), dtype=torch.float32).to(S.device)
        db.append(S[keep].reshape(n_rows, S.shape[2]), A[keep].reshape(n_rows, A.shape[2]),
                  goals[keep].repeat_interleave(K, dim=0), weights=weights[keep].reshape(n_rows))
    return err, weights, n_rows
