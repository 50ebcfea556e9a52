"""`LocomotionMPC` over the whole-body solver facade: the reference's controller calls, unchanged.

Restates the part of mpc_controller/mpc.py that drives the solver, with the reference's
names, on top of `quadruped_solver.QuadrupedAcadosSolver` (the C-ABI facade):
    __init__ bookkeeping             mpc.py:25-119   (gait / opt / cost configs, planner, replanning_steps)
    reset                            mpc.py:121-169
    set_command                      mpc.py:197-202
    increment_base_ref_position      mpc.py:204-208
    compute_base_ref_vel_tracking    mpc.py:210-272  (references.base_ref_vel_tracking, golden-pinned)
    optimize                         mpc.py:317-369  (contacts, peaks, [Raibert locations], base refs, init, solve)
    set_convergence_on_first_iter    mpc.py:464-473
    interpolate_trajectory_with_derivatives / id_repeat   mpc.py:142,371-414  (references.hermite_upsample)
    open_loop                        mpc.py:416-462  (simulator-free receding horizon: plant = interpolated plan)
Batch = 1 keeps the reference's array shapes; `batch > 1` adds a leading axis to q, v and every returned array
(all rollouts share the gait clock).  MuJoCo, the keyboard goal, plotting and the asynchronous executor are outside
the path (C8, C10, C11).
"""
from __future__ import annotations

import contextlib
from collections import defaultdict
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

from . import wholebody as wb
from .config import COLLISION_HEIGHT, N_SQP_FIRST, TERMINATE_DEFAULT, get_quadruped_config
from .contact_planner import ContactPlanner, RaiberContactPlanner
from .profiling import print_timings, time_fn
from .quadruped_solver import QuadrupedAcadosSolver
from .trajectory_io import KD, KP
from .references import base_ref_cnt_restricted, base_ref_vel_tracking, hermite_upsample, increment_base_ref_position
from .workloads import FEET


class LocomotionMPC:
    def __init__(self, path_urdf: str = "", feet_frame_names=FEET, robot_name: str = "go2", gait_name: str = "trot",
                 joint_ref: Optional[np.ndarray] = None, interactive_goal: bool = False, sim_dt: float = 1.0e-3,
                 height_offset: float = 0., contact_planner: str = "", print_info: bool = True,
                 compute_timings: bool = True, solve_async: bool = False, batch: int = 1, device="cuda:0",
                 n_nodes: Optional[int] = None, force_reference: str = "zero", momentum_model: str = "declared",
                 torque_layer=None):
        """momentum_model, torque_layer: as `QuadrupedAcadosSolver` -- "articulated" solves with the centroidal momentum of the
        tree of `torque_layer` and takes x0's `h` from it; `optimize` and `open_loop` work in that mode, `open_loop_device` and
        `label_states` (whose kernels build x0 from the declared map) raise until `set_state_momentum("tree")`."""
        self.batch = int(batch)
        self.config_gait, self.config_opt, self.config_cost = get_quadruped_config(gait_name, robot_name)
        if n_nodes is not None:                      # BASELINE configs[2] asks for N = 30; the reference runs 25
            self.config_opt.n_nodes = int(n_nodes)
        self.print_info = print_info
        self.height_offset = height_offset
        self.solver = QuadrupedAcadosSolver(path_urdf, list(feet_frame_names), self.config_opt, self.config_cost,
                                            height_offset, print_info, compute_timings, batch=batch, device=device,
                                            force_reference=force_reference, momentum_model=momentum_model,
                                            torque_layer=torque_layer)
        self.momentum_model = self.solver.momentum_model
        self.nq, self.nv, self.nu, self.n_foot = 18, 18, wb.N_JOINTS, 4
        self.joint_ref = np.asarray(joint_ref, float) if joint_ref is not None else wb.Q_HOME.copy()   # mpc.py:73-81
        self._contact_planner_str = contact_planner
        if contact_planner.lower() == "raibert":                                            # mpc.py:75-92
            q0 = np.zeros(18)
            q0[6:] = self.joint_ref
            self.solver.dyn.update_pin(q0, np.zeros(18))
            offset_hip_b = np.array(self.solver.dyn.get_feet_position_w())
            offset_hip_b[:, -1] = 0.
            self.contact_planner = RaiberContactPlanner(list(feet_frame_names), self.solver.dt_nodes, self.config_gait,
                                                        offset_hip_b, y_offset=0.02, x_offset=0.04, foot_size=0.0085,
                                                        cache_cnt=False)
            self.restrict_cnt = True
        else:
            self.contact_planner = ContactPlanner(list(feet_frame_names), self.solver.dt_nodes, self.config_gait)
            self.restrict_cnt = False
        self.solver.set_contact_restriction(self.restrict_cnt)
        self.Kp, self.Kd = self.config_opt.Kp, self.config_opt.Kd
        self.sim_dt = sim_dt
        self.dt_nodes = self.solver.dt_nodes
        self.replanning_freq = self.config_opt.replanning_freq
        self.replanning_steps = int(1 / (self.replanning_freq * sim_dt))                    # mpc.py:113
        self.compute_timings = compute_timings
        self.reset(reset_solver=False)

    def reset(self, reset_solver: bool = True) -> None:                                     # mpc.py:121-169
        if reset_solver:
            self.solver.reset()
        self.first_solve, self.diverged = True, False
        self.sim_step = self.plan_step = self.current_opt_node = self.delay = 0
        self.sim_time, self.clock_step = 0.0, 0       # the float clock `open_loop_device` stopped at, and the steps it has summed
        sh = (self.batch, 3) if self.batch > 1 else (3,)
        self.v_des, self.w_des = np.zeros(sh), np.zeros(sh)
        self.base_ref_vel_tracking = np.zeros((self.batch, 12) if self.batch > 1 else 12)
        self.n_interp_plan = round(self.config_opt.time_horizon / self.sim_dt)
        self.id_repeat = np.int32(np.linspace(0, 1, self.n_interp_plan) * (self.config_opt.n_nodes - 1))   # mpc.py:142
        self.timings = defaultdict(list)

    def set_command(self, v_des=np.zeros((3,)), w_yaw: float = 0.) -> None:                 # mpc.py:197-202
        self.v_des = np.broadcast_to(np.asarray(v_des, float), self.v_des.shape).copy()
        self.w_des[..., 2] = w_yaw

    def increment_base_ref_position(self):                                                  # mpc.py:204-208
        increment_base_ref_position(self.base_ref_vel_tracking, self.v_des, self.w_des, self.sim_dt)

    def compute_base_ref_vel_tracking(self, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:   # mpc.py:210-272
        return base_ref_vel_tracking(q, self.v_des, self.w_des, self.base_ref_vel_tracking, self.config_opt.time_horizon,
                                     self.config_gait.nom_height, self.height_offset)

    def compute_base_ref_cnt_restricted(self, q, contact_locations):                        # mpc.py:274-315
        return base_ref_cnt_restricted(contact_locations, self.config_gait.nom_height, self.height_offset)

    def _replan(self) -> bool:                                                              # mpc.py:171-175
        return self.sim_step % self.replanning_steps == 0

    def set_convergence_on_first_iter(self):                                                # mpc.py:464-473
        """iteration policy of the solve about to run: the first one gets N_SQP_FIRST SQP iterations at a tenth of the
        configured tolerances; the configured policy is restored during the first replanning interval after it"""
        cfg = self.solver.config_opt
        if self.first_solve:
            policy = (N_SQP_FIRST, cfg.nlp_tol / 10., cfg.qp_tol / 10.)
        elif self.sim_step <= self.replanning_steps:
            policy = (cfg.max_iter, cfg.nlp_tol, cfg.qp_tol)
        else:
            return
        for setter, value in zip((self.solver.set_max_iter, self.solver.set_nlp_tol, self.solver.set_qp_tol), policy):
            setter(value)

    def solver_inputs(self, q: np.ndarray, v: np.ndarray):
        """what `optimize` hands to `solver.init` (mpc.py:325-366), without solving"""
        N = self.config_opt.n_nodes
        self.solver.dyn.update_pin(q, v)
        cnt_sequence = self.contact_planner.get_contacts(self.current_opt_node, N + 1)
        swing_peak = self.contact_planner.get_peaks(self.current_opt_node, N + 1) if self.config_opt.opt_peak else None
        cnt_locations = None
        if self.restrict_cnt:
            assert self.batch == 1, "contact-location plans are per rollout: use batch = 1"
            if self._contact_planner_str.lower() == "raibert":
                com_xyz = np.asarray(q[:3], float)          # declared model: centre of mass at the base origin
                self.contact_planner.set_state(q[:3], v[:3], q[3:6][::-1], com_xyz, self.v_des, self.w_des[-1])
            cnt_locations = self.contact_planner.get_locations(self.current_opt_node, N + 1)
            base_ref, base_ref_e = self.compute_base_ref_cnt_restricted(q, cnt_locations)
        else:
            base_ref, base_ref_e = self.compute_base_ref_vel_tracking(q)
        if self.batch > 1:
            cnt_sequence = np.broadcast_to(cnt_sequence, (self.batch,) + cnt_sequence.shape)
            swing_peak = None if swing_peak is None else np.broadcast_to(swing_peak, (self.batch,) + swing_peak.shape)
        joint_ref = self.joint_ref if self.batch == 1 else np.broadcast_to(self.joint_ref, (self.batch, 12))
        return (self.current_opt_node, q, v, base_ref, base_ref_e, joint_ref, self.config_gait.step_height,
                cnt_sequence, cnt_locations, swing_peak)

    @time_fn("optimize")
    def optimize(self, q: np.ndarray, v: np.ndarray):                                       # mpc.py:317-369
        self.solver.init(*self.solver_inputs(q, v))
        return self.solver.solve()

    def interpolate_trajectory_with_derivatives(self, time_traj, positions, velocities, accelerations):   # mpc.py:388-414
        return hermite_upsample(time_traj, positions, velocities, accelerations, self.n_interp_plan)

    def open_loop(self, q0: np.ndarray, v0: np.ndarray, trajectory_time: float):
        """Simulator-free rollout (mpc.py:416-462): replan every `replanning_steps`, interpolate the plan to the
        simulation rate, follow it as if it were the plant.  q0, v0 in the solver's Euler layout.
        Returns q_traj[K(,B),18], one row per simulation step."""
        q, v = np.array(q0, float), np.array(v0, float)
        sim_time, q_rows, v_rows, a_rows, f_rows, time_traj = 0.0, [], [], [], [], None
        while sim_time <= trajectory_time:
            if sim_time >= (self.current_opt_node + 1) * self.dt_nodes:
                self.current_opt_node += 1
            if self._replan():
                self.set_convergence_on_first_iter()
                q_sol, v_sol, a_sol, f_sol, dt_sol = self.optimize(q, v)
                self.first_solve = False
                time_traj = np.concatenate(([0.], np.cumsum(dt_sol[0] if self.batch > 1 else dt_sol)))
                # interpolate_state_trajectory (mpc.py:371-386): sample 0 is the current state and is dropped
                if self.batch == 1:
                    qp, vp = self.interpolate_trajectory_with_derivatives(time_traj, q_sol, v_sol, a_sol)
                    self.q_plan, self.v_plan = qp[1:], vp[1:]
                else:
                    pl = [self.interpolate_trajectory_with_derivatives(time_traj, q_sol[b], v_sol[b], a_sol[b]) for b in range(self.batch)]
                    self.q_plan, self.v_plan = np.stack([p[0][1:] for p in pl], 1), np.stack([p[1][1:] for p in pl], 1)
                self.a_plan, self.f_plan = np.take(a_sol, self.id_repeat, axis=-2), np.take(f_sol, self.id_repeat, axis=-3)
                self.plan_step = 0
            q, v = self.q_plan[self.plan_step].copy(), self.v_plan[self.plan_step].copy()
            q_rows.append(q)
            v_rows.append(v)
            a_rows.append(self.a_plan[..., self.plan_step, :].copy())         # a_plan[plan_step], f_plan[plan_step] (mpc.py:583)
            f_rows.append(self.f_plan[..., self.plan_step, :, :].copy())
            self._step()
            sim_time = sim_time + self.sim_dt
        self.v_traj = np.stack(v_rows)                       # the velocities that go with the returned rows
        self.a_traj, self.f_traj = np.stack(a_rows), np.stack(f_rows)   # ... and the held accelerations and forces
        return np.stack(q_rows)

    def replan_clock(self, trajectory_time: float):
        """The float clock of `open_loop` without its solves: (number of simulation steps it runs, optimisation node of each
        of its replans) from the controller's current counters -- what `open_loop_device` hands to the device, so that both
        replan at the same nodes (the reference advances the node when the accumulated float time passes a node time,
        mpc.py:171-186, 427-431)."""
        steps, nodes, node, _ = self._run_clock(0.0, lambda sim_time, steps: sim_time <= trajectory_time)
        return steps, nodes, node

    def _run_clock(self, sim_time: float, go_on):
        """the one text of the float clock: from float time `sim_time` and the controller's counters while go_on(sim_time, steps
        run) holds -> (steps run, node of each replan, node at the end, float time at the end)"""
        sim_step, node, nodes, steps = self.sim_step, self.current_opt_node, [], 0
        while go_on(sim_time, steps):
            if sim_time >= (node + 1) * self.dt_nodes:
                node += 1
            if sim_step % self.replanning_steps == 0:
                nodes.append(node)
            sim_step += 1
            steps += 1
            sim_time = sim_time + self.sim_dt
        return steps, nodes, node, sim_time

    def replan_clock_intervals(self, n_replans: int, resume: bool = False):
        """`replan_clock` for exactly `n_replans` whole replanning intervals -> (steps = n_replans * replanning_steps, the node of
        each replan, the node at the end, the float time at the end).  resume=False: the float time starts at 0, as
        `replan_clock`'s.  resume=True: it goes on from `self.sim_time`, where the previous `open_loop_device` stopped, summing
        sim_time = sim_time + sim_dt in the order of one long run -- the doubles, and with them the nodes, of stretches run one
        after the other are those of one run over all of them.  Nothing of the controller is changed: `open_loop_device` stores
        what this returns.  The counters must stand on an interval boundary (ValueError)."""
        n_replans = int(n_replans)
        if n_replans < 1:
            raise ValueError("n_replans must be at least 1")
        if self.sim_step % self.replanning_steps or (resume and self.clock_step % self.replanning_steps):
            raise ValueError("whole replanning intervals start on an interval boundary: the previous call ended "
                             f"{self.sim_step % self.replanning_steps} steps into an interval")
        total = n_replans * self.replanning_steps
        return self._run_clock(self.sim_time if resume else 0.0, lambda sim_time, steps: steps < total)

    def state_rows(self, q_traj: np.ndarray, v_traj: np.ndarray, t0_step: int = 0) -> np.ndarray:
        """states of this controller (Euler layout, [K, 18] each; K, B, 18 for a batch) as the reference's recorded rows
        [phase, v_mj(18), q_mj[2:](17), base_wrt_feet(8)] (DAgger/utils/RolloutMPC.py:221): row j is the state after
        simulation step t0_step + j"""
        from .trajectory_io import convert_to_mujoco
        q_traj, v_traj = np.asarray(q_traj, float), np.asarray(v_traj, float)
        if q_traj.ndim == 3:
            return np.stack([self.state_rows(q_traj[:, b], v_traj[:, b], t0_step) for b in range(q_traj.shape[1])])
        period = self.config_gait.nominal_period
        rows = np.zeros((len(q_traj), 44))
        for j, (q, v) in enumerate(zip(q_traj, v_traj)):
            q_mj, v_mj = convert_to_mujoco(q, v)
            tw = (t0_step + j + 1) * self.sim_dt
            bwf = (q[None, :2] - wb.feet_position_w(q)[:, :2]).reshape(8)
            rows[j] = np.concatenate([[np.round(np.fmod(tw, period) / period, 4)], v_mj, q_mj[2:], bwf])
        return rows

    def open_loop_device(self, q0: np.ndarray, v0: np.ndarray, trajectory_time: Optional[float] = None, push: Optional[dict] = None,
                         record_sim_steps: bool = True, terminate_mask: int = TERMINATE_DEFAULT,
                         collision_height: float = COLLISION_HEIGHT, torque_layer=None, kp: Optional[float] = None,
                         kd: Optional[float] = None, plant=None, plant_substeps: int = 2, push_as_force: bool = False,
                         integrator: Optional[str] = None, n_replans: Optional[int] = None, resume: bool = False):
        """`open_loop` with the whole rollout on the device (nmpc_wb_rollout_batch): per replan the problem is assembled from
        the plant state by a kernel, solved with the warm-start shift folded in, and the up-sampled plan is followed for
        `replanning_steps` simulation steps -- one host call, no round trip per replan, the whole batch at once.
        Returns S [B, K, 44] (device): the recorded rows of `state_rows` -- one per simulation step, K as `open_loop`
        runs, or one per replan (the state it starts from) with record_sim_steps=False.  push = {"start", "duration",
        "force": [B, 3]}: velocity impulse F dt / m on the base per replanning interval; "start" and "duration" may be arrays of
        B, a window per rollout (`BatchedNmpcSolver.set_rollout_push_windows`, attached for this call: rollout b is the bits
        it is under the scalar window of its own, in every mode below and across resumed calls).  The controller's counters,
        reference and solution views advance as in `open_loop`; `self.failed` holds the NMPC_ROLLOUT_FLAG_* bits,
        `self.q_final` / `self.v_final` the plant state.
        torque_layer (a `BatchedTorqueLayer` of the robot; needs rows per simulation step): the expert's action labels are
        recorded beside the rows -- `self.actions` [B, K, 12] (device), row j = (tau + kd v_j) / kp + q_j of the state in S's
        row j, tau the inverse-dynamics torque of the plan that row was taken from (`references.plan_rows`); kp, kd default to
        the recorder's KP, KD.
        plant (a `torque.GroundContact`; needs torque_layer and rows per simulation step): the expert runs in closed loop on
        the declared ground-contact plant instead of following its plan (nmpc_wb_rollout_set_plant) -- between replans the
        robot is driven by tau_id + Kp (q_plan - q) + Kd (v_plan - v) (mpc.py:583-599) through `plant_substeps` substeps of
        sim_dt / plant_substeps per simulation step, and every replan starts from the state the plant is in.  kp, kd then
        default to the controller's Kp, Kd.  Row j of S is the plant state BEFORE simulation step j and `self.actions` row j
        the PD target applied from it (RolloutMPC.py:168-258); a robot that falls in the last interval is flagged too.
        A ground per rollout takes no keyword here: attach the table on torque_layer (`BatchedTorqueLayer.set_grounds`) before
        the call -- rollout b then stands on row b, the values of `plant` are ignored, and `collect_rollouts` and
        `learning_iteration`, which run this call, see the same table.  A payload per rollout likewise
        (`BatchedTorqueLayer.set_payloads`): the plant of rollout b carries row b, the plans and the labels are those of the
        nominal model.  An actuator per rollout likewise (`BatchedTorqueLayer.set_actuators`): the plant of rollout b answers the
        labels with the gains, the joint damping and the rotor inertia of row b, the labels are formed with the nominal kp, kd.
        A delay per rollout likewise (`BatchedTorqueLayer.set_delays`, in simulation steps; its work_rows must hold the
        `replanning_steps` of one interval, ValueError otherwise): the plant of rollout b answers in simulation step j the label
        of step j - d_b, `self.actions` holds the labels as issued.  A call that starts a rollout fills the shift register with
        the posture of q0 (`reset_delay_history`); resume=True leaves it as the previous call left it, so that the stretches are
        the one call.
        push_as_force (needs plant): the push is a force on the trunk of the plant over the substeps its window covers
        (nmpc_wb_rollout_set_plant_push), where the feet and the torque limit answer it, instead of the velocity jump per
        replanning interval.
        integrator (needs plant): "explicit" or "implicit" sets the integrator of torque_layer's plant first
        (`BatchedTorqueLayer.set_integrator`; it stays set), None leaves it as it is.
        n_replans=K (instead of trajectory_time, which is then None): exactly K whole replanning intervals, K * replanning_steps
        simulation steps -- S, `self.actions`, the plant state and the counters end on an interval boundary, where a later call
        can go on.  resume=True (needs n_replans, and a previous call that ended on a boundary; ValueError otherwise): the call
        CONTINUES the rollout of the previous call instead of starting one -- q0, v0 are the `q_final`, `v_final` it left, the
        float clock goes on from `self.sim_time` (`replan_clock_intervals`), and the device counts its replans from the replan the
        rollout has reached (`BatchedNmpcSolver.set_rollout_clock`, set for this call): the recorded phase, the push window --
        `push` times are those of the whole rollout, counted from its first call -- and the stamps in `self.failed` are the long
        rollout's, and the stretches' rows, one after the other, are bit for bit the rows of one call over all of them.  The
        flags the previous call left in `self.failed` are carried on (a copy: the tensor the previous call returned stays as it
        is): a rollout that entered the call terminated stays frozen, its rows of the call are its frozen state -- cut at its
        stamp.  Between two stretches the host may `set_command`, look at `self.failed`, save or stop."""
        import torch
        from .mpc import push_windows
        # 1. what the arguments alone decide, and the clock: a refused call has touched neither the device nor the solver's options
        if (trajectory_time is None) == (n_replans is None):
            raise ValueError("open_loop_device: give trajectory_time or n_replans, one of them")
        if resume and n_replans is None:
            raise ValueError("resume: a continued call runs whole replanning intervals, give n_replans")
        if integrator is not None:
            from .torque import integrator_mode
            integrator_mode(integrator)                   # an unknown name is refused before anything runs
            if plant is None:
                raise ValueError("integrator: the integrator is the contact plant's, give plant")
        clock = self._device_clock(trajectory_time, n_replans, resume)
        n_replans, replan0 = len(clock.nodes), clock.clock_step0 // self.replanning_steps
        self._declared_momentum_only("open_loop_device")
        if plant is not None and torque_layer is None:
            raise ValueError("plant: the contact plant lives in the torque layer, give torque_layer")
        if push_as_force and plant is None:
            raise ValueError("push_as_force: a push as a force needs the contact plant, give plant")
        delays = getattr(torque_layer, "_delays", None) if plant is not None else None
        if delays is not None and delays.work_rows < self.replanning_steps:
            raise ValueError(f"delays: a replanning interval has {self.replanning_steps} simulation steps, the attached table has work_rows = "
                             f"{delays.work_rows} (set_delays(..., work_rows=))")
        kp = (self.Kp if plant is not None else KP) if kp is None else kp
        kd = (self.Kd if plant is not None else KD) if kd is None else kd
        windows = push_windows(push, self.batch)      # a window per rollout: attached for this call, the cfg's own window unused
        if windows is not None:
            push = dict(push, start=0.0, duration=0.0)
        # 2. the device inputs
        fs, cfg_o = self.solver, self.config_opt
        s = fs._device_solver()
        s.set_max_iter(cfg_o.max_iter); s.set_nlp_tol(cfg_o.nlp_tol); s.set_max_qp_iter(cfg_o.max_qp_iter)
        fs._opts.update(max_iter=cfg_o.max_iter, nlp_tol=cfg_o.nlp_tol, qp_tol=cfg_o.qp_tol)
        failed_in = self.failed.clone() if replan0 else None        # a continued rollout keeps its flags and stamps
        q, v, v_des, w_des, ref_state, status = self._device_inputs(s, q0, v0)
        if delays is not None and not resume:
            torque_layer.reset_delay_history(q)           # the posture held before the expert spoke
        actions = None
        if torque_layer is not None:
            rows = n_replans * (self.replanning_steps if record_sim_steps else 1)
            A = torch.zeros(self.batch, rows, 12, dtype=torch.float32, device=s.device)
            actions = (torque_layer, s.to_device(self.id_repeat[:self.replanning_steps], torch.int32), A, kp, kd)
        # 3. the attachments, 4. the call
        with self._rollout_attachments(s, actions, integrator, None if plant is None else (torque_layer, plant, plant_substeps, kp, kd),
                                       push_as_force, replan0, windows):
            S, failed = s.wb_rollout(
                *self._gait_tensors(s), clock.nodes, q, v, v_des, w_des, ref_state, s.to_device(self.joint_ref),
                self._by_rollout(s, push["force"]) if push else None,
                self._X_dev, self._U_dev, status, failed=failed_in, n_replans=n_replans, replanning_steps=self.replanning_steps,
                first_solve=int(self.first_solve), last_node=int(fs.last_node), max_sqp_first=N_SQP_FIRST,
                nlp_tol_first=cfg_o.nlp_tol / 10.0, nlp_tol=cfg_o.nlp_tol, push_start=float(push["start"]) if push else 0.0,
                push_duration=float(push["duration"]) if push else 0.0, record_sim_steps=int(record_sim_steps),
                nominal_period=float(self.config_gait.nominal_period), terminate_mask=int(terminate_mask),
                collision_height=float(collision_height), **self._problem_cfg())
        # 5. the books
        self._commit_rollout(clock, q, v, ref_state, status, failed, None if actions is None else actions[2])
        return S[:, :clock.steps] if record_sim_steps else S

    def _device_clock(self, trajectory_time, n_replans, resume):
        """the clock of one `open_loop_device` call, from the controller's counters: over `trajectory_time` as `replan_clock` runs
        it, or over `n_replans` whole intervals (`replan_clock_intervals`, which refuses what cannot be continued) -> steps, nodes,
        node_end, time_end as `_run_clock` names them, and clock_step0: the steps the rollout it continues has run (0: it starts one)"""
        if n_replans is None:
            steps, nodes, node_end, time_end = self._run_clock(0.0, lambda sim_time, steps: sim_time <= trajectory_time)
        else:
            steps, nodes, node_end, time_end = self.replan_clock_intervals(n_replans, resume)
        return SimpleNamespace(steps=steps, nodes=nodes, node_end=node_end, time_end=time_end, clock_step0=self.clock_step if resume else 0)

    def _by_rollout(self, s, a, dtype=None):
        """a host array with one row per rollout on the device of `s` (float32 unless told otherwise)"""
        return s.to_device(np.asarray(a, np.float64).reshape(self.batch, -1), *(() if dtype is None else (dtype,)))

    def _device_inputs(self, s, q0, v0):
        """the tensors of one `open_loop_device` call -> (q, v [B, 18] float32: copies, the plant state the call moves; v_des, w_des,
        ref_state float64; status int32 [B]); `_X_dev`, `_U_dev` are zeroed for a first solve"""
        import torch
        B, N, dev = self.batch, self.config_opt.n_nodes, s.device
        # (the q_final, v_final of the call that is continued may be handed over as they are: device tensors, copied)
        q, v = (a.to(dev, torch.float32).reshape(B, -1).clone() if isinstance(a, torch.Tensor) else self._by_rollout(s, a) for a in (q0, v0))
        v_des, w_des, ref_state = (self._by_rollout(s, a, torch.float64) for a in (self.v_des, self.w_des, self.base_ref_vel_tracking))
        if getattr(self, "_X_dev", None) is None or self.first_solve:
            self._X_dev = torch.zeros(B, N + 1, 42, dtype=torch.float32, device=dev)
            self._U_dev = torch.zeros(B, N, 30, dtype=torch.float32, device=dev)
        return q, v, v_des, w_des, ref_state, torch.zeros(B, dtype=torch.int32, device=dev)

    @staticmethod
    @contextlib.contextmanager
    def _rollout_attachments(s, actions, integrator, plant, push_as_force, replan0, windows):
        """What one `open_loop_device` call attaches to the device solver `s` for the duration of its rollout: actions and plant
        (the arguments of `set_rollout_actions` / `set_rollout_plant`, None: not attached; integrator: set on the plant's layer
        first, where it stays), the push as a force, the clock and the windows per rollout (`rollout_push_windows`) -- in this
        order, and detached in the reverse one whatever happens, an attach call that raises included: the handle ends with
        nothing of the call attached."""
        with contextlib.ExitStack() as detach:
            if actions is not None:
                detach.callback(s.set_rollout_actions, None)
                s.set_rollout_actions(*actions)
            if plant is not None:
                if integrator is not None:
                    plant[0].set_integrator(integrator)
                detach.callback(s.set_rollout_plant, None)
                s.set_rollout_plant(*plant)
            if push_as_force:
                detach.callback(s.set_rollout_plant_push, False)
                s.set_rollout_plant_push(True)
            detach.callback(s.set_rollout_clock, 0)
            s.set_rollout_clock(replan0)
            detach.enter_context(s.rollout_push_windows(windows))
            yield

    def _commit_rollout(self, clock, q, v, ref_state, status, failed, A) -> None:
        """the bookkeeping of a rollout that ran, as `open_loop` leaves it"""
        fs = self.solver
        self.first_solve = False
        self.sim_step += clock.steps
        self.sim_time, self.clock_step = clock.time_end, clock.clock_step0 + clock.steps
        self.current_opt_node = clock.node_end
        fs.last_node = clock.nodes[-1]
        ref = ref_state.cpu().numpy()
        # (open_loop integrates the reference once per simulation step it runs; the device does it per full replanning interval)
        self.base_ref_vel_tracking = ref if self.batch > 1 else ref[0]
        self.failed, self.status_dev = failed, status
        self.q_final, self.v_final = q, v
        if A is not None:
            self.actions = A[:, :clock.steps]
        fs.parse_sol(self._X_dev.cpu().numpy().astype(np.float64), self._U_dev.cpu().numpy().astype(np.float64))

    def _problem_cfg(self) -> dict:
        """the cfg fields of the problem that `open_loop_device` and `label_states` hand over alike"""
        return dict(nodes_per_cycle=self.contact_planner.nodes_per_cycle, sim_dt=self.sim_dt, time_horizon=self.config_opt.time_horizon,
                    nom_height=self.config_gait.nom_height, height_offset=self.height_offset,
                    step_height=float(self.config_gait.step_height),
                    force_reference_gravity=int(self.solver.force_reference == "gravity_share"))

    def _gait_tensors(self, s):
        """(gait_sequence, peak_swing) of the contact planner as int8 on the device of `s`"""
        import torch
        return tuple(s.to_device(t, torch.int8) for t in (self.contact_planner.gait_sequence, self.contact_planner.peak_swing))

    def label_clock(self, n_rows: int, t0: float, dt_row: float):
        """The float clock of `replan_clock` for rows that are not replans: row k of a table of visited states was reached at
        time t0 + k dt_row, that is at simulation step round((t0 + k dt_row) / sim_dt) of a rollout that starts from the
        controller's current counters.  -> (nodes [n_rows]: the optimisation node the clock shows at that step, ref_steps
        [n_rows]: the simulation steps run by then, over which the base reference has been integrated).  Host code only."""
        if n_rows < 1 or t0 < 0.0 or not dt_row > 0.0:
            raise ValueError("label_clock: need n_rows >= 1, t0 >= 0 and dt_row > 0")
        ref_steps = [int(round((t0 + k * dt_row) / self.sim_dt)) for k in range(n_rows)]
        sim_time, node, node_at = 0.0, self.current_opt_node, []
        for _ in range(ref_steps[-1] + 1):
            if sim_time >= (node + 1) * self.dt_nodes:
                node += 1
            node_at.append(node)
            sim_time = sim_time + self.sim_dt
        return [node_at[s] for s in ref_steps], ref_steps

    def label_states(self, Q, V, torque_layer, t0: float = 0.0, dt_row: Optional[float] = None, failed=None,
                     kp: Optional[float] = None, kd: Optional[float] = None):
        """DAgger relabelling (nmpc_wb_label_states_batch): what this expert would have done in states somebody else reached.
        Q, V [B, K, 18] (device, B = the controller's batch): row k of robot b is a plant state at time t0 + k dt_row of a rollout
        under the controller's command, dt_row defaulting to the replanning interval (`BatchedTorqueLayer.set_rollout_states`
        records them beside a policy rollout; there dt_row = n_sub dt).  Every state gets the expert's FIRST solve -- cold start,
        N_SQP_FIRST iterations at a tenth of the tolerance -- at the node and with the base reference `label_clock` gives its
        row, and the label is the PD target of simulation step 0 of that plan: the target applied from the state, the pairing of
        plant mode (`open_loop_device(plant=...)`), whose gains kp, kd default to the controller's Kp, Kd as well.  failed
        (int32 [B], a policy rollout's): the states from a robot's termination on are left out, their rows stay zero.
        -> (A [B, K, 12], status int32 [B, K]) on the device.  Not a replan of the controller: its counters, reference, views
        and `_X_dev` / `_U_dev` are as they were."""
        import torch
        self._declared_momentum_only("label_states")
        s = self.solver._device_solver()
        if not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[0] != self.batch:
            raise ValueError(f"Q: need a float32 tensor [{self.batch}, K, 18] on the GPU")
        nodes, ref_steps = self.label_clock(Q.shape[1], t0, self.replanning_steps * self.sim_dt if dt_row is None else dt_row)
        by_robot = lambda a: self._by_rollout(s, a, torch.float64)   # noqa: E731
        A, status, _, _ = s.label_states(
            torque_layer, *self._gait_tensors(s), s.to_device(nodes, torch.int32), s.to_device(ref_steps, torch.int32), Q, V,
            by_robot(self.v_des), by_robot(self.w_des), by_robot(self.base_ref_vel_tracking), s.to_device(self.joint_ref),
            s.to_device(self.id_repeat[:1], torch.int32), failed=failed, max_sqp=N_SQP_FIRST, nlp_tol=self.config_opt.nlp_tol / 10.0,
            kp=float(self.Kp if kp is None else kp), kd=float(self.Kd if kd is None else kd), terminate_mask=int(TERMINATE_DEFAULT),
            **self._problem_cfg())
        return A, status

    def set_state_momentum(self, source: str = "declared") -> None:
        """Where `open_loop_device` and `label_states` take the momentum slots of a measured state from
        (`BatchedNmpcSolver.set_state_momentum`).  "declared" (the default): the declared map, so both raise on an articulated
        controller.  "tree" (momentum_model="articulated" only): the momentum of the tree, computed on the device behind every
        prepare kernel -- what `optimize` puts into x0 on the host; the weight share of force_reference="gravity_share" and a
        push's velocity jump then take the mass of the tree."""
        self.solver.set_state_momentum(source)

    @property
    def state_momentum(self) -> str:
        return self.solver.state_momentum

    def _declared_momentum_only(self, who: str) -> None:
        if self.momentum_model != "declared" and self.state_momentum == "declared":
            raise RuntimeError(f"{who}: the device builds the momentum of x0 from the declared map; with momentum_model="
                               f"\"{self.momentum_model}\" use optimize / open_loop")

    def _step(self) -> None:                                                                # mpc.py:183-186
        self.increment_base_ref_position()
        self.sim_step += 1
        self.plan_step += 1

    def print_timings(self):
        print_timings(self.timings)
        self.solver.print_timings()
