"""Policy training from the device-resident database, and one whole learning iteration.

    BehavioralCloning.train_network     DAgger/utils/train_locosafedagger.py:66-138   -> train_network
    one DAgger iteration: roll the expert out, aggregate, train
        DAgger/utils/data_collection_locosafedagger.py:92-131                         -> learning_iteration

The pieces are `collect.collect_rollouts` (rollouts -> `DeviceDatabase`, with the out-of-distribution weight of every
row), `DevicePolicy.train_epoch` (an epoch of weighted batches in one library call) and `DevicePolicy.loss` (the
validation loss).  No table, batch, index or loss passes through the host, and nothing here waits for the device: what
comes back are device tensors.  `evaluate_policy` closes the loop on the declared contact plant: the trained policy drives
the robots, and what comes back is who stayed up and which states the learner visited.  `dagger_iteration` joins the two
halves: the learner's rollout, the expert's labels for the states it visited (`LocomotionMPC.label_states`), aggregate, train --
where `learning_iteration` aggregates the expert's own rollouts (behaviour cloning with pushes).

Declared choices:
  * Sampling is WITH replacement, as the reference's WeightedRandomSampler loader draws
    (Behavior_Cloning/examples/test_train_policy.py:128-134) -- also when every weight is 1, where the reference's plain
    loader would shuffle without replacement.  An epoch is ceil(n_train / batch_size) full batches.
  * The validation rows stay in the tables and get weight ZERO in a copy of the weight vector: the inverse-CDF lookup
    returns the first row whose prefix sum exceeds the target, which a row that adds nothing to the sum never is.  So
    the split needs no compaction of the tables, and the database's own weights are left as they are.
  * `learning_iteration` validates on the LAST floor(val_fraction * len(db)) physical rows of the database after the
    append (on a ring that has not wrapped: the newest rows)."""
from __future__ import annotations

from functools import partial
from typing import Optional

import torch

from ._lib import NMPC_ROLLOUT_TERM_SHIFT, NMPC_STATUS_NAN, NMPC_STATUS_QP
from .collect import collect_rollouts
from .mpc import push_windows
from .config import TERMINATE_DEFAULT
from .torque import N_STATE, NOMINAL_PERIOD, TABLES, GroundContact, history_width, integrator_mode
from .trajectory_io import KD, KP


def train_network(policy, db, n_epoch: int, batch_size: int, lr: float = 1e-3, seed: int = 0,
                  val_idx: Optional[torch.Tensor] = None, input_noise=None, input_noise_seed: int = 0):
    """`n_epoch` epochs of `policy` (a `DevicePolicy`) on `db` (a `DeviceDatabase`), rows drawn by `db.weights`.

    Epoch e is `policy.train_epoch` with seed `seed + e` over ceil(n_train / batch_size) batches, followed by the
    validation loss on the rows `val_idx` (distinct physical ring positions, int32 or int64, host or device), which are
    assembled once with `db.batch` and never trained on.  Returns (train_loss [n_epoch, n_batches], val_loss [n_epoch])
    on the device; without validation rows val_loss is NaN.
    input_noise: a vector sigma [n <= 44] in the units of the raw state columns (`torque.training_sigma` makes one of a table of
    sensor noise), attached for this call (`DevicePolicy.set_input_noise`) with the key `input_noise_seed` and epoch0 = 0, so
    that epoch e of the call perturbs its batches with the draws of epoch e; the validation loss stays on clean rows.  It is
    detached when the call ends, also by an exception.  None: the batches are trained on as they are assembled, unless the
    policy has a vector of the caller's attached, which then stays, is used and keeps counting its own epoch.  A policy that has
    one attached while `input_noise` is given is refused with ValueError, as `evaluate_policy` refuses its tables."""
    if input_noise is not None and policy._input_noise is not None:
        raise ValueError("input_noise: the policy has input noise attached already (set_input_noise)")
    n = len(db)
    weights = db.weights[:n].clone()
    n_val = 0
    if val_idx is not None:
        val_idx = torch.as_tensor(val_idx, device=db.device).to(torch.int32).contiguous()
        n_val = int(val_idx.numel())
    if n_val:
        weights[val_idx.long()] = 0.0
        x_val, y_val = db.batch(val_idx)
    n_train = n - n_val
    if n_train < 1:
        raise ValueError(f"no training rows: {n} rows in the database, {n_val} of them for validation")
    n_batches = -(-n_train // int(batch_size))
    train_loss = torch.empty(n_epoch, n_batches, dtype=torch.float32, device=db.device)
    val_loss = torch.full((n_epoch,), float("nan"), dtype=torch.float32, device=db.device)
    try:
        if input_noise is not None:
            policy.set_input_noise(input_noise, seed=input_noise_seed, epoch0=0)
        for e in range(n_epoch):
            train_loss[e] = policy.train_epoch(db, batch_size, n_batches, lr, seed + e, weights=weights)
            if n_val:
                val_loss[e:e + 1] = policy.loss(x_val, y_val)
    finally:
        if input_noise is not None:
            policy.set_input_noise(None)
    return train_loss, val_loss


def learning_iteration(mpc, layer, db, policy, q0, v0, T: float, push: Optional[dict] = None, nominal: int = 0,
                       ood_weight: float = 5.0, terminate_mask: int = TERMINATE_DEFAULT, kp: Optional[float] = None,
                       kd: Optional[float] = None, n_epoch: int = 1, batch_size: int = 256, lr: float = 1e-3, seed: int = 0,
                       val_fraction: float = 0.0, plant=None, plant_substeps: int = 2, push_as_force: bool = False,
                       integrator: Optional[str] = None, chunk_replans: Optional[int] = None, train_noise=None, train_noise_seed: int = 0):
    """One DAgger iteration, from rollouts to updated parameters: `collect.collect_rollouts` (its arguments up to `kd`, and
    `plant` / `plant_substeps` / `push_as_force` / `integrator`: the expert on the ground-contact plant, pushed by a force, under the named integrator;
    `chunk_replans`: the rollout in stretches of that many replans, each appended before the next runs) appends the valid rollouts and their weights to `db`, then
    `train_network` trains `policy` on all of `db`, validating on its last floor(val_fraction * len(db)) physical rows.  Returns (err, weights, n_rows, train_loss, val_loss): what
    the two parts return.  A table of grounds, of payloads, of actuators or of delays attached on `layer` (`set_grounds`,
    `set_payloads`, `set_actuators`, `set_delays`) is seen by the plant of the rollouts; there is no keyword for any of them.
    train_noise, train_noise_seed: `train_network`'s input_noise and its key -- the expert's rollouts have no sensor, so a cloned
    policy meets sensor noise only in the batches it is trained on."""
    if not 0.0 <= val_fraction < 1.0:
        raise ValueError("val_fraction must be in [0, 1)")
    err, weights, n_rows = collect_rollouts(mpc, layer, db, q0, v0, T, push=push, nominal=nominal, ood_weight=ood_weight,
                                            terminate_mask=terminate_mask, kp=kp, kd=kd, plant=plant, plant_substeps=plant_substeps,
                                            push_as_force=push_as_force, integrator=integrator, chunk_replans=chunk_replans)
    n = len(db)
    if n == 0:
        raise ValueError("the database is empty: no rollout of the batch was valid")
    n_val = int(val_fraction * n)
    val_idx = torch.arange(n - n_val, n, dtype=torch.int32, device=db.device) if n_val else None
    train_loss, val_loss = train_network(policy, db, n_epoch, batch_size, lr=lr, seed=seed, val_idx=val_idx, input_noise=train_noise,
                                         input_noise_seed=train_noise_seed)
    return err, weights, n_rows, train_loss, val_loss


def evaluate_policy(layer, policy, db, q0, v0, goal, T: float, dt: float = 5e-4, n_sub: int = 20, tau_ff=None, kp: float = KP,
                    kd: float = KD, ground=None, t0: float = 0.0, period: Optional[float] = None,
                    terminate_mask: int = TERMINATE_DEFAULT, collision_height: float = 0.08, record_states: bool = False,
                    push: Optional[dict] = None, integrator: Optional[str] = None, grounds=None, payloads=None, actuators=None,
                    delays=None, noise=None, noise_seed: int = 0, record_observed: bool = False, history=None):
    """`policy` (a `DevicePolicy`) in the loop on the ground-contact plant of `layer` (a `BatchedTorqueLayer`) for T seconds
    from q0, v0 [B, 18]: round(T / (n_sub dt)) control steps of `layer.policy_rollout`, the policy input normalised as `db`
    (a `DeviceDatabase`, or None: raw) normalises its batches (DAgger/utils/RolloutPolicy.py, PolicyController, on the
    declared plant).  Returns a dict of device tensors, nothing here waits for the device:
        failed          int32 [B]: the flag bits every robot raised, above them the stamp of its termination
        survived        bool [B]: no stamp, failed >> 8 == 0
        steps_survived  int32 [B]: control steps before the observation that terminated the robot (all of them if none did)
        S, A            [B, n_steps, 44], [B, n_steps, 12]: the states visited and the actions taken -- the rows of a
                        terminated robot from its stamp on are those of a fallen robot; cut there
        q, v            [B, 18]: the state after the last control step
        Q, V            with record_states=True, [B, n_steps, 18]: the plant state before every control step, row k the state
                        row k of S was made of (`BatchedTorqueLayer.set_rollout_states`, attached for this call) -- what
                        `LocomotionMPC.label_states` starts the expert's solves from.
        O               with record_observed=True, [B, n_steps, 44]: row k the raw state row as the sensors showed it in control
                        step k -- row k of S under the draw of the noise that the policy's input of that step carried
                        (`BatchedTorqueLayer.set_rollout_observed`, attached for this call); without noise it is S.
    push: the dict of `mpc.sample_pushes` -- {"start": s, "duration": s, "force": [B, 3] N} -- as a force on the trunk
    (`BatchedTorqueLayer.set_push`, attached for this call): the substeps round(start / dt) <= s < round(start / dt) +
    round(duration / dt) of the rollout are pushed.  None, or a duration that rounds to no substep: the rollout is the bits it
    is without.  "start" and "duration" may be arrays of B: a window per robot, each converted with the same round(t / dt)
    (`set_push` with arrays), robot b being the bits it is under the scalar window of its own.  A layer that has a push of the caller's attached already is refused with ValueError: the call would replace
    it and leave nothing attached.
    integrator: "explicit" or "implicit" sets the layer's integrator first (`BatchedTorqueLayer.set_integrator`; it stays
    set), None leaves it as it is.  With "implicit", dt = 2e-3 and n_sub = 5 run the same 10 ms control step in a quarter of
    the substeps.
    grounds: a table of grounds, one row per robot (`BatchedTorqueLayer.set_grounds` takes it and validates it; `sample_grounds`
    draws one), attached for this call: robot b stands on the ground of row b and has its torque limit, and `ground` is
    ignored.  None: every robot is on `ground`.  A layer that has a table of the caller's attached already is refused with
    ValueError, as for a push.
    payloads: a table of payloads, one row (m_p, r) per robot (`BatchedTorqueLayer.set_payloads` takes it and validates it;
    `sample_payloads` draws one), attached to the trunk for this call: robot b carries row b on the plant.  None: nobody carries
    anything.  A layer that has a table of the caller's attached already is refused with ValueError in the same way.
    actuators: a table of actuators, one row (kp, kd, damping, armature) per robot (`BatchedTorqueLayer.set_actuators` takes it and
    validates it; `sample_actuators` draws one), attached for this call in the same way: the plant answers the policy's PD targets
    with the gains of row b, and `kp`, `kd` are not read for the law.  None: every robot has the nominal drive of `kp`, `kd`.
    delays: a table of delays, one integer per robot (`BatchedTorqueLayer.set_delays` takes it and validates it; `sample_delays`
    draws one), attached for this call in the same way, in control steps of n_sub dt: the plant answers in control step k the
    target the policy issued in step k - d_b, and A holds the issued targets.  None: nobody is late, unless the layer has a
    table of the caller's attached, which then stays and is used.  Either way the shift register starts the rollout holding
    the posture of q0 (`BatchedTorqueLayer.reset_delay_history`).
    noise: a table of sensor noise, one row (sigma[44], bias[44]) per robot in the units of the raw state row
    (`BatchedTorqueLayer.set_noise` takes it and validates it; `torque.noise_table` builds one, `sample_noise` draws one), attached
    for this call in the same way with the key `noise_seed`, first_robot = 0 and the noise step 0: the policy acts on what the
    sensors of robot b show, while S, failed, Q, V and the plant are those of the true state.  None: the policy reads the true
    state, unless the layer has a table of the caller's attached, which then stays, is used and keeps counting its own noise
    step.  A layer that has one attached while `noise` is given is refused with ValueError as for the other tables.
    history: (n_obs, n_act), observation and action history on the policy input (`BatchedTorqueLayer.set_history`), attached for
    this call: `policy` has 44 n_obs + 12 n_act + n_goal inputs and `db` (or None: raw) the state width 44 n_obs + 12 n_act; the
    registers start holding the true row of (q0, v0, t0) and the posture of q0 (`reset_history`), and the dict has
        W               [B, n_steps, n_wide]: row k the raw wide row the policy was shown in control step k
                        (`BatchedTorqueLayer.set_rollout_wide`), what a database of that width stores.
    None: the policy is memoryless, unless the layer has a history of the caller's attached, which then stays, is used and keeps
    its registers as they are.  A layer that has one attached while `history` is given is refused with ValueError as for the tables."""
    if integrator is not None:
        integrator_mode(integrator)                       # an unknown name is refused before anything is attached
    if history is not None:
        n_obs, n_act = (int(x) for x in history)
        n_wide = history_width(*layer._history_depths(n_obs, n_act))      # bad depths are refused before anything is attached
    n_steps = int(round(float(T) / (int(n_sub) * float(dt))))
    if n_steps < 1:
        raise ValueError(f"T = {T} s is shorter than one control step of {n_sub} x {dt} s")

    def set_push(push):
        if push is None:
            return layer.set_push(None)
        force = torch.as_tensor(push["force"], dtype=torch.float32, device=layer.device).reshape(-1, 3)
        windows = push_windows(push, force.shape[0])
        if windows is None:
            layer.set_push(force, start_substep=int(round(float(push["start"]) / float(dt))),
                           n_substeps=int(round(float(push["duration"]) / float(dt))))
        else:                                             # a window per robot, each converted as the scalar one is
            first, count = ([int(round(float(t) / float(dt))) for t in w] for w in windows)
            layer.set_push(force, start_substep=first, n_substeps=count)

    # what this call attaches to the layer and takes off again: (name, value, what the layer has attached, setter, in words)
    given = dict(grounds=grounds, payloads=payloads, actuators=actuators, delays=delays, noise=noise)      # the keywords are explicit: one entry per name of TABLES
    keywords = dict(noise=dict(seed=noise_seed))
    parts = [("push", push, layer._push, set_push, "a push")]
    parts += [(name, given[name], getattr(layer, "_" + name), partial(getattr(layer, "set_" + name), **keywords.get(name, {})), "a table of " + name)
              for name in TABLES]
    parts = [part for part in parts if part[1] is not None]
    for name, _, attached, _, what in parts:
        if attached is not None:
            raise ValueError(f"{name}: the layer has {what} attached already (set_{name})")
    if record_observed and layer._observed is not None:
        raise ValueError("record_observed: the layer has observed rows attached already (set_rollout_observed)")
    if history is not None and layer._history is not None:
        raise ValueError("history: the layer has a history attached already (set_history)")
    states = {}
    if record_states:
        B = torch.as_tensor(q0).reshape(-1, layer.n).shape[0]
        states = {k: torch.empty(B, n_steps, layer.n, dtype=torch.float32, device=layer.device) for k in ("Q", "V")}
        layer.set_rollout_states(states["Q"], states["V"])
    if record_observed:
        B = torch.as_tensor(q0).reshape(-1, layer.n).shape[0]
        states["O"] = torch.empty(B, n_steps, N_STATE, dtype=torch.float32, device=layer.device)
        layer.set_rollout_observed(states["O"])
    try:
        if integrator is not None:
            layer.set_integrator(integrator)
        for _, value, _, setter, _ in sorted(parts, key=lambda part: part[0] == "push"):      # the tables, then the push
            setter(value)
        if layer._delays is not None:
            layer.reset_delay_history(q0)
        if history is not None:
            q_start, v_start = layer._in(q0, (layer.n,), "q0"), layer._in(v0, (layer.n,), "v0")
            B = layer._batch(q_start, v_start)
            layer.set_history(n_obs, n_act, batch=B)
            states["W"] = torch.empty(B, n_steps, n_wide, dtype=torch.float32, device=layer.device)
            layer.set_rollout_wide(states["W"])
            # the true row of the start state: the flags-free observation of one row, which draws no noise and moves no noise step
            S0 = layer.observe_rows(q_start[:, None, :], v_start[:, None, :], t0, int(n_sub) * float(dt), NOMINAL_PERIOD if period is None else period,
                                    collision_height=collision_height)
            layer.reset_history(S0[:, 0], q_start)
        q, v, S, A, failed = layer.policy_rollout(policy, q0, v0, n_steps, dt, n_sub, goal, tau_ff=tau_ff, kp=kp, kd=kd,
                                                  ground=GroundContact() if ground is None else ground, t0=t0,
                                                  period=NOMINAL_PERIOD if period is None else period, db=db,
                                                  terminate_mask=terminate_mask, collision_height=collision_height)
    finally:
        for _, _, _, setter, _ in parts:
            setter(None)
        if record_states:
            layer.set_rollout_states(None)
        if record_observed:
            layer.set_rollout_observed(None)
        if history is not None:
            layer.set_history(None)
    stamp = failed >> NMPC_ROLLOUT_TERM_SHIFT
    return dict(failed=failed, survived=stamp == 0, steps_survived=torch.where(stamp == 0, torch.full_like(stamp, n_steps), stamp - 1),
                S=S, A=A, q=q, v=v, **states)


def dagger_iteration(mpc, layer, db, policy, q0, v0, goal, T: float, dt: float = 5e-4, n_sub: int = 20, kp: Optional[float] = None,
                     kd: Optional[float] = None, ground=None, terminate_mask: int = TERMINATE_DEFAULT, collision_height: float = 0.08,
                     n_epoch: int = 1, batch_size: int = 256, lr: float = 1e-3, seed: int = 0, val_fraction: float = 0.0,
                     push: Optional[dict] = None, integrator: Optional[str] = None, grounds=None, payloads=None, actuators=None,
                     delays=None, noise=None, noise_seed: int = 0, store: str = "true", train_noise=None, train_noise_seed: int = 0,
                     history=None):
    """One DAgger iteration proper: the LEARNER drives, the expert says what it would have done where the learner went.
        1. `evaluate_policy(record_states=True)`: `policy` drives the ground-contact plant of `layer` for T seconds from q0, v0
           [B, 18] under `goal` [B, 3] (the velocity command the controller `mpc` -- a `LocomotionMPC` of batch B -- has been
           given with `set_command`), pushed by `push` (the dict of `mpc.sample_pushes`, as `evaluate_policy` takes it:
           a force on the trunk; None: no push) -- the perturbation the learner is to survive;
        2. `mpc.label_states` on the visited Q, V with dt_row = n_sub dt and the rollout's `failed`: the expert's first solve
           from every state up to each robot's termination and the PD target it would apply from it;
        3. the rows (S[b, k], A*[b, k], goal[b]) with k < steps_survived[b] whose solve neither ended in NaN nor in a QP failure
           are appended to `db` with weight 1 -- chosen by a mask and `nonzero` on the device, in (b, k) order;
        4. `train_network` on all of `db`, validating on its last floor(val_fraction * len(db)) physical rows, as
           `learning_iteration` does.
    kp, kd: the gains of the policy's PD law and of the labels alike (None: the controller's Kp, Kd), so that an action and
    its label mean the same torque.  integrator: the plant's integrator, as `evaluate_policy` takes it.  grounds: a ground per
    robot for the learner's rollout, as `evaluate_policy` takes it (attached for that call; the labels are the expert's solves and
    stand on no plant).  payloads: a payload per robot for the learner's rollout, in the same way: the plant carries it, the
    labels are the nominal expert's -- the expert's model does not describe the load, which is the point.  actuators: an actuator per
    robot for the learner's rollout, in the same way: the plant has the drives of the table, the labels are formed with the nominal
    `kp`, `kd` -- `label_states` on the visited states, with or without the table.  delays: a delay per robot for the
    learner's rollout, in the same way: the plant is late, the expert's labels are those of the visited states and know no delay.
    noise, noise_seed: sensor noise per robot for the learner's rollout, in the same way: the learner drives on what its sensors
    show; the expert's labels always come from the true states Q, V.  store: which rows go into the database beside those labels --
    "true" (the default): the true rows S[b, k]; "observed": O[b, k], the rows the learner's sensors showed
    (`evaluate_policy(record_observed=True)`, returned as O), with the same choice of rows, so that a policy deployed on noisy
    inputs is trained on (what it saw, what the expert would do from the true state); any other string is a ValueError before
    anything runs.  train_noise, train_noise_seed: `train_network`'s input_noise and its key, noise on the batches in training.
    history: (n_obs, n_act), as `evaluate_policy` takes it: the learner is shown the wide row of every step, and W[b, k], the raw wide
    row, is appended in place of S[b, k] with the same choice of rows -- `store` is not read, the wide row is what the sensors
    showed -- so that `db.batch` of an appended row is bit for bit the input the learner acted on, under the statistics the rollout
    used.  A `db` whose state width is not 44 n_obs + 12 n_act is refused with ValueError before anything runs.
    Returns `evaluate_policy`'s dict with A_star [B, K, 12], status int32 [B, K], n_rows, train_loss and val_loss added."""
    if store not in ("true", "observed"):
        raise ValueError(f"store: expected 'true' or 'observed', got {store!r}")
    if history is not None:
        n_wide = history_width(*layer._history_depths(*history))
        if db.widths["states"] != n_wide:
            raise ValueError(f"history: the database stores states of width {db.widths['states']}, the wide row has {n_wide}")
    if not 0.0 <= val_fraction < 1.0:
        raise ValueError("val_fraction must be in [0, 1)")
    if integrator is not None:
        integrator_mode(integrator)
    kp, kd = float(mpc.Kp if kp is None else kp), float(mpc.Kd if kd is None else kd)
    out = evaluate_policy(layer, policy, db, q0, v0, goal, T, dt=dt, n_sub=n_sub, kp=kp, kd=kd, ground=ground,
                          terminate_mask=terminate_mask, collision_height=collision_height, record_states=True, push=push,
                          integrator=integrator, grounds=grounds, payloads=payloads, actuators=actuators, delays=delays,
                          noise=noise, noise_seed=noise_seed, record_observed=store == "observed" and history is None, history=history)
    A_star, status = mpc.label_states(out["Q"], out["V"], layer, dt_row=int(n_sub) * float(dt), failed=out["failed"], kp=kp, kd=kd)
    S = out["S"]
    B, K = S.shape[:2]
    alive = torch.arange(K, device=S.device)[None, :] < out["steps_survived"][:, None]
    keep = torch.nonzero((alive & (status != NMPC_STATUS_NAN) & (status != NMPC_STATUS_QP)).reshape(-1)).squeeze(1)      # device index, (b, k) order
    n_rows = int(keep.numel())
    if n_rows:
        goals = torch.as_tensor(goal, dtype=torch.float32, device=S.device).reshape(B, -1)
        # what the learner saw (its wide row, or its one observed row), or the true rows; the labels are those of the true states
        rows = out["W"] if history is not None else out["O"] if store == "observed" else S
        db.append(rows.reshape(B * K, -1)[keep], A_star.reshape(B * K, -1)[keep], goals.repeat_interleave(K, dim=0)[keep])
    n = len(db)
    if n == 0:
        raise ValueError("the database is empty: no visited state of the batch got a label")
    n_val = int(val_fraction * n)
    val_idx = torch.arange(n - n_val, n, dtype=torch.int32, device=db.device) if n_val else None
    train_loss, val_loss = train_network(policy, db, n_epoch, batch_size, lr=lr, seed=seed, val_idx=val_idx, input_noise=train_noise,
                                         input_noise_seed=train_noise_seed)
    return dict(out, A_star=A_star, status=status, n_rows=n_rows, train_loss=train_loss, val_loss=val_loss)
