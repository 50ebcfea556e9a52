"""Batched MPC controller: the host-side mirror of `LocomotionMPC` for B rollouts at once.

Restates the control flow of mpc_controller/mpc.py on top of the batched HIP solver:
    set_command                      mpc.py:197-202
    compute_base_ref_vel_tracking    mpc.py:210-272   (vectorised over the batch, same quantisation)
    optimize                         mpc.py:317-369   (contact flags -> references -> init -> solve)
    set_convergence_on_first_iter    mpc.py:464-473   (15 SQP iterations on the first solve)
    open_loop                        mpc.py:416-462   (simulator-free receding horizon: plant = plan)
    _replan / _step bookkeeping      mpc.py:171-186
    RaiberContactPlanner.get_locations + stance anchoring   contact_planner.py:265-322, solver.py:194-210 (footsteps=True)
    interpolate_state_trajectory     mpc.py:371-414   (record_sim_steps=True: one recorded row per simulation step)
The plant is the declared centroidal model; the whole-body controller is `mpc_wholebody.py`;
MuJoCo is outside this path.  All rollouts of a batch share the
gait clock (they are replanned at the same nodes), which is how the reference generates its perturbed
rollouts from one nominal rollout (data_collection_*_perturbed.py:176-247).
"""
from __future__ import annotations

from collections import defaultdict
from typing import Optional, Tuple

import numpy as np
import torch

from .config import COLLISION_HEIGHT, N_SQP_FIRST, TERMINATE_DEFAULT, get_quadruped_config
from .contact_planner import ContactPlanner, RaiberContactPlanner
from .profiling import print_timings, time_fn
from .references import _euler_rate_matrix, _hermite, base_ref_vel_tracking, increment_base_ref_position
from .solver import BatchedNmpcSolver
# bits of `failed` (include/nmpc.h NMPC_ROLLOUT_FLAG_*); above them 1 + the replan that terminated the rollout
from .solver import (NMPC_ROLLOUT_FLAG_COLLISION as FLAG_COLLISION, NMPC_ROLLOUT_FLAG_HEIGHT as FLAG_HEIGHT,
                     NMPC_ROLLOUT_FLAG_MASK as FLAG_MASK, NMPC_ROLLOUT_FLAG_PITCH as FLAG_PITCH, NMPC_ROLLOUT_FLAG_ROLL as FLAG_ROLL,
                     NMPC_ROLLOUT_FLAG_SOLVER as FLAG_SOLVER, NMPC_ROLLOUT_FLAG_VEL_TRACKING as FLAG_VEL_TRACKING,
                     NMPC_ROLLOUT_TERM_SHIFT as TERM_SHIFT)
from .workloads import FEET, HIP_OFFSETS, MODEL_CENTROIDAL, model_params


def sample_pushes(n: int, seed, start=0.0, duration=0.3, magnitude=(50.0, 70.0)) -> dict:
    """n base pushes as the reference's data collection draws them (bc_experimental.yaml:32-35,
    data_collection_force_perturbation.py:213-248): direction uniform in the cube, normalised, magnitude uniform in
    `magnitude` newtons.  seed: anything numpy's SeedSequence takes (e.g. (rank, iteration, attempt)).
    start, duration: seconds, or arrays of n (a window per rollout, e.g. `sample_push_windows`'s), passed through."""
    rng = np.random.default_rng(seed)
    force = rng.uniform(-1.0, 1.0, (n, 3))
    force /= np.linalg.norm(force, axis=1, keepdims=True) + 1e-6
    force *= rng.uniform(magnitude[0], magnitude[1], (n, 1))
    if np.ndim(start) == 0 and np.ndim(duration) == 0:
        return dict(start=float(start), duration=float(duration), force=force)
    start, duration = push_windows(dict(start=start, duration=duration), n)
    return dict(start=start, duration=duration, force=force)


def sample_push_windows(n: int, seed, period: float, n_points: int = 10, duration=(0.2, 0.4)) -> dict:
    """A push window per rollout as the reference's data collection draws them
    (data_collection_pretrain_omini_vc_policy_1direction_perturbed.py:191-247): the start at one of `n_points` equally spaced
    replanning points of the gait cycle, k period / n_points with k uniform in 0 .. n_points - 1, and a duration uniform in
    `duration` seconds.  -> {"start": [n], "duration": [n]} (float64), which merges into a push dict:
    dict(sample_pushes(n, seed), **sample_push_windows(n, seed, period))."""
    if n_points < 1 or not period > 0.0:
        raise ValueError("sample_push_windows: need n_points >= 1 and period > 0")
    rng = np.random.default_rng(seed)
    point = rng.integers(0, n_points, n)
    return dict(start=point * (float(period) / n_points), duration=rng.uniform(duration[0], duration[1], n))


def push_windows(push: Optional[dict], n: int):
    """The windows of a push dict whose "start" or "duration" is an array: (start [n], duration [n]) float64, a scalar among the
    two holding for every rollout; None for a dict with scalar windows (or no dict), which takes the uniform path.  An array
    of another length than n is refused with ValueError."""
    if push is None or (np.ndim(push["start"]) == 0 and np.ndim(push["duration"]) == 0):
        return None
    out = []
    for key in ("start", "duration"):
        a = push[key]
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(n, float(a))
        if a.shape != (n,):
            raise ValueError(f"push[{key!r}]: need a scalar or {n} entries (one per rollout), got shape {a.shape}")
        out.append(a)
    return out[0], out[1]


def state_row_flags(rows: np.ndarray, v_des: np.ndarray, collision_height: float = COLLISION_HEIGHT) -> np.ndarray:
    """NMPC_ROLLOUT_FLAG_* bits of recorded 19-slot state rows [B, R, 19] (check_unsafe_state_v2,
    Rollout_combined_controller.py:367-431, + the collision height), OR-ed over the R rows: what the device's advance
    kernel raises, in fp32 like it."""
    r = np.asarray(rows, np.float32)
    lim = np.float32(25.0) * np.float32(0.017453292519943295)
    vd = np.asarray(v_des, np.float64).astype(np.float32)
    f = np.zeros(r.shape[:2], np.int32)
    f |= np.where(np.abs(r[:, :, 10]) > lim, FLAG_ROLL, 0)
    f |= np.where(np.abs(r[:, :, 9]) > lim, FLAG_PITCH, 0)
    f |= np.where((r[:, :, 7] < np.float32(0.18)) | (r[:, :, 7] > np.float32(0.45)), FLAG_HEIGHT, 0)
    f |= np.where((np.abs(r[:, :, 1] - vd[:, None, 0]) > np.float32(0.10)) | (np.abs(r[:, :, 2] - vd[:, None, 1]) > np.float32(0.10)),
                  FLAG_VEL_TRACKING, 0)
    f |= np.where(r[:, :, 7] < np.float32(collision_height), FLAG_COLLISION, 0)
    f |= np.where(~(np.abs(r[:, :, 7]) <= np.float32(1e30)), FLAG_SOLVER, 0)
    return np.bitwise_or.reduce(f, axis=1)


class BatchedLocomotionMPC:
    """B centroidal rollouts driven by one batched NMPC solve per replanning step."""

    def __init__(self, batch: int, gait_name: str = "trot", robot_name: str = "go2", n_nodes: int = 50,
                 device="cuda:0", sim_dt: float = 1.0e-3, height_offset: float = 0.0,
                 compute_timings: bool = True, mass: float = 15.0, inertia=(0.11, 0.27, 0.33),
                 footsteps: bool = False, record_sim_steps: bool = False, terminate_mask: int = TERMINATE_DEFAULT,
                 collision_height: float = COLLISION_HEIGHT):
        """footsteps: stance feet anchored, touch-downs at Raibert targets (False: the feet stay under the initial hips
        for the whole rollout -- the stance-frozen rollouts of round 1).  record_sim_steps: one state row per
        simulation step (the plan up-sampled as mpc.py:371-414) instead of one per replan.
        device None: the host side alone -- the configuration, the planners and the host helpers (`build_problem`,
        `plan_foot_locations`, `sim_step_rows`, `record_state`, ...), no solver and no tensors: nothing that solves or rolls."""
        self.batch = int(batch)
        self.footsteps, self.record_sim_steps = bool(footsteps), bool(record_sim_steps)
        # early termination (include/nmpc.h, nmpc_rollout_cfg.terminate_mask): a rollout that raises one of these flags is
        # frozen; `invalid_mask` is what open_loop_device_valid discards and redoes (the same bits by default)
        self.terminate_mask, self.collision_height = int(terminate_mask) & FLAG_MASK, float(collision_height)
        self.invalid_mask = self.terminate_mask
        self.config_gait, self.config_opt, self.config_cost = get_quadruped_config(gait_name, robot_name)
        self.n_nodes = int(n_nodes)
        self.height_offset = height_offset
        self.sim_dt = sim_dt
        self.dt_nodes = self.config_opt.time_horizon / self.n_nodes
        self.replanning_freq = self.config_opt.replanning_freq
        self.replanning_steps = int(1 / (self.replanning_freq * sim_dt))                # mpc.py:113
        self.nodes_per_replan = max(1, int(round(self.replanning_steps * sim_dt / self.dt_nodes)))
        self.contact_planner = ContactPlanner(FEET, self.dt_nodes, self.config_gait)
        # footstep targets: the reference's Raibert planner with its offsets (mpc.py:80-91), stateless (cache_cnt=False)
        offs = HIP_OFFSETS.copy(); offs[:, 2] = 0.0
        self.raibert = RaiberContactPlanner(FEET, self.dt_nodes, self.config_gait, offs, y_offset=0.02, x_offset=0.04,
                                            foot_size=0.0085, height_offset=height_offset, cache_cnt=False)
        self.compute_timings = compute_timings
        self.timings = defaultdict(list)

        self.mp = model_params(dt=self.dt_nodes, mass=mass, Ixx=inertia[0], Iyy=inertia[1], Izz=inertia[2])
        self.solver = self.device = None
        if device is None:
            self.reset()
            return
        self.solver = BatchedNmpcSolver(MODEL_CENTROIDAL, self.n_nodes, self.batch, device, compute_timings)
        self.solver.set_contact_patterns(gait_sequence=self.contact_planner.gait_sequence)   # kernel by gait
        self.device = self.solver.device
        self.solver.set_model_params(self.mp)
        W = np.concatenate([self.config_cost.W_base, self.config_cost.W_cnt_f_reg.ravel()])
        self.solver.set_cost_weights(W, self.config_cost.W_e_base, self.config_cost.reg_eps,
                                     self.config_cost.reg_eps_e)
        self.solver.set_max_qp_iter(self.config_opt.max_qp_iter)
        self.reset()

    # -- state ------------------------------------------------------------------------------------
    def _reset_host(self) -> None:
        B = self.batch
        self.first_solve = True
        self.sim_step = 0
        self.current_opt_node = 0
        self.v_des = np.zeros((B, 3))
        self.w_des = np.zeros((B, 3))
        self.base_ref_vel_tracking = np.zeros((B, 12))
        self.foot_pos = None
        self.timings = defaultdict(list)

    def reset(self) -> None:
        B, N = self.batch, self.n_nodes
        self._reset_host()
        if self.solver is None:
            return
        self.X = torch.zeros(B, N + 1, 12, dtype=torch.float32, device=self.device)
        self.U = torch.zeros(B, N, 12, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.stats = torch.zeros(B, 4, dtype=torch.float32, device=self.device)
        self.solver.last_node = 0

    def set_command(self, v_des=np.zeros(3), w_yaw=0.0) -> None:
        self.v_des = np.broadcast_to(np.asarray(v_des, dtype=np.float64), (self.batch, 3)).copy()
        self.w_des[:, 2] = w_yaw

    def set_convergence_on_first_iter(self) -> None:
        if self.first_solve:
            self.solver.set_max_iter(N_SQP_FIRST)
            self.solver.set_nlp_tol(self.config_opt.nlp_tol / 10.0)
        elif self.sim_step <= self.replanning_steps:
            self.solver.set_max_iter(self.config_opt.max_iter)
            self.solver.set_nlp_tol(self.config_opt.nlp_tol)

    def _replan(self) -> bool:
        return self.sim_step % self.replanning_steps == 0

    def compute_base_ref_vel_tracking(self, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        return base_ref_vel_tracking(q, self.v_des, self.w_des, self.base_ref_vel_tracking, self.config_opt.time_horizon,
                                     self.config_gait.nom_height, self.height_offset)

    def increment_base_ref_position(self, n_steps: int = 1, rows=None) -> None:
        """mpc.py:204-208, once per simulation step, over the batch (rows: mask of the rollouts that advance)."""
        rows = slice(None) if rows is None else rows
        s = self.base_ref_vel_tracking[rows]
        for _ in range(n_steps):
            increment_base_ref_position(s, self.v_des[rows], self.w_des[rows], self.sim_dt)
        self.base_ref_vel_tracking[rows] = s

    # -- one replanning step --------------------------------------------------------------------
    def build_problem(self, x: np.ndarray):
        """Per-stage references and parameters for the current node (host side, as mpc.py:332-366)."""
        B, N = self.batch, self.n_nodes
        contacts = self.contact_planner.get_contacts(self.current_opt_node, N + 1).astype(np.float64)  # [4,N+1]
        base_ref, base_ref_e = self.compute_base_ref_vel_tracking(x)
        if self.foot_pos is None:   # feet under the hips at the first call (setup_initial_feet_pos, solver.py:194)
            self.foot_pos = x[:, None, :3] * [1, 1, 0] + HIP_OFFSETS[None]
        params = np.zeros((B, N + 1, 16))
        params[:, :, :4] = contacts.T[None]
        if self.footsteps:
            params[:, :, 4:] = self.plan_foot_locations(x, contacts).reshape(B, N + 1, 12)
        else:
            params[:, :, 4:] = self.foot_pos.reshape(B, 1, 12)
        n_stance = np.maximum(contacts[:, :N].sum(0), 1.0)
        yref = np.zeros((B, N, 24))
        yref[:, :, :12] = base_ref[:, None, :]
        yref[:, :, 14::3] = (contacts[:, :N].T * (-self.mp[5] * self.mp[1] / n_stance)[:, None])[None]
        return yref, base_ref_e, params

    def plan_foot_locations(self, x: np.ndarray, contacts: np.ndarray) -> np.ndarray:
        """[B, N+1, 4, 3]: Raibert targets from every touch-down of the window on (contact_planner.py:265-322), then a foot
        in contact at node 0 keeps its current position up to its next swing node (solver.py:194-210, argmin and all)."""
        B, N = self.batch, self.n_nodes
        out = np.zeros((B, N + 1, 4, 3))
        for b in range(B):
            self.raibert.set_state(x[b, :3], x[b, 6:9], x[b, [5, 4, 3]], x[b, :3], self.v_des[b], self.w_des[b, 2])
            locs = self.raibert.get_locations(self.current_opt_node, N + 1)            # [4, N+1, 3]
            for f in range(4):
                if contacts[f, 0]:
                    locs[f, :int(np.argmin(contacts[f]))] = self.foot_pos[b, f]
            out[b] = np.moveaxis(locs, 0, 1)
        return out

    def touch_down(self, params: np.ndarray, rows=None) -> None:
        """feet that stand at the node the plant has reached are where the plan put them (rows: mask of the rollouts
        that advance -- a terminated one is frozen)"""
        npr = self.nodes_per_replan
        for f in range(4):
            on = params[:, npr, f] > 0.5
            if rows is not None:
                on &= rows
            self.foot_pos[on, f] = params[on, npr, 4 + 3 * f:7 + 3 * f]

    def sim_step_rows(self, X: np.ndarray, params: np.ndarray, replan_index: int) -> np.ndarray:
        """[B, replanning_steps, 19]: the plan up-sampled to the simulation rate as `interpolate_state_trajectory` does
        (mpc.py:371-414): positions on cubic Hermite segments through (q_k, qdot_k), velocities through (v_k, a_{k-1})
        with the reference's one-node shift of the accelerations (mpc.py:409-410); sample j at t = (j + 1) sim_dt."""
        B, N, dtn = self.batch, self.n_nodes, self.dt_nodes
        t_nodes = np.arange(N + 1) * dtn
        t_q = (np.arange(self.replanning_steps) + 1) * self.sim_dt
        seg = np.minimum(np.floor(t_q / dtn + 1e-9).astype(int), N - 1)
        period = self.config_gait.nominal_period
        t_w = (replan_index * self.replanning_steps + np.arange(self.replanning_steps) + 1) * self.sim_dt
        phase = np.round(np.fmod(t_w, period) / period, 4)
        rows = np.zeros((B, self.replanning_steps, 19))
        for b in range(B):
            Xb = X[b]
            thd = np.stack([_euler_rate_matrix(Xb[k, 3:6]) @ Xb[k, [11, 10, 9]] for k in range(N + 1)])
            pos = _hermite(t_nodes, Xb[:, :6], np.concatenate([Xb[:, 6:9], thd], axis=1), t_q)
            acc = (Xb[1:, 6:12] - Xb[:-1, 6:12]) / dtn
            vel = _hermite(t_nodes, Xb[:, 6:12], np.concatenate([acc[:1], acc]), t_q)
            stands = params[b, seg, :4] > 0.5                                             # [steps, 4]
            feet = np.where(stands[:, :, None] & self.footsteps, params[b, seg, 4:].reshape(-1, 4, 3), self.foot_pos[b][None])
            bwf = (pos[:, None, :2] - feet[:, :, :2]).reshape(-1, 8)
            rows[b] = np.concatenate([phase[:, None], vel, pos[:, 2:6], bwf], axis=1)
        return rows

    @time_fn("optimize")
    def optimize(self, x: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
        """One batched replanning solve from the states x[B,12]; returns device X[B,N+1,12], U[B,N,12]."""
        s = self.solver
        yref, yref_e, params = self.build_problem(x)
        self._params = params
        if self.first_solve:
            self.X[:] = s.to_device(np.repeat(x[:, None, :], self.n_nodes + 1, axis=1))
            self.U[:] = s.to_device(yref[:, :, 12:])
        # warm start (solver.py:304-322): the shift is folded into the solve
        shift = 0 if (self.first_solve or not self.config_opt.warm_start_sol) else self.current_opt_node - s.last_node
        s.last_node = self.current_opt_node
        s.solve(s.to_device(x), s.to_device(yref), s.to_device(yref_e), s.to_device(params),
                self.X, self.U, self.status, self.stats, shift=shift)
        return self.X, self.U

    # -- simulator-free rollout -------------------------------------------------------------------
    def open_loop(self, x0: np.ndarray, trajectory_time: float, push: Optional[dict] = None):
        """Receding-horizon rollout where the plant follows the plan (mpc.py:416-462).

        Returns (S[B,K,19] float32 device, t[K]): one recorded state per replanning step, in the
        slot order of the reference's recorded state (DAgger/utils/RolloutMPC.py:221):
            [phase, v(6) = rdot, body rates, q[2:] = z, yaw, pitch, roll, base_wrt_feet(8)].
        push = {"start": s, "duration": s, "force": [B,3] N}: a base push applied to the plant as the
        velocity impulse F dt / m per replanning interval (the reference pushes the MuJoCo base,
        data_collection_force_perturbation.py:213-248).
        `self.failed` [B] int32 (device): NMPC_ROLLOUT_FLAG_* bits of the recorded states, and above them 1 + the replan
        that terminated the rollout (`terminate_mask`: frozen from then on, its solves skipped, rows repeated) -- the
        same bookkeeping as `open_loop_device`.
        """
        x = np.array(x0, dtype=np.float64)
        n_replans = int(np.floor(trajectory_time / (self.replanning_steps * self.sim_dt) + 1e-9))
        dt_replan = self.replanning_steps * self.sim_dt
        rec, times = [], []
        flags = np.zeros(self.batch, np.int32)
        skip = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.solver.set_skip(skip, self.terminate_mask)
        try:
            for i in range(n_replans):
                t_now = i * dt_replan
                dead = (flags & self.terminate_mask) != 0
                skip.copy_(torch.as_tensor(flags))
                self.set_convergence_on_first_iter()
                X, _ = self.optimize(x)
                self.first_solve = False
                st = self.status.cpu().numpy()
                flags[~dead & ((st == 1) | (st == 4))] |= FLAG_SOLVER
                if self.record_sim_steps:
                    rows = self.sim_step_rows(X.double().cpu().numpy(), self._params, i)
                    times.extend(t_now + (np.arange(self.replanning_steps) + 1) * self.sim_dt)
                else:
                    rows = self.record_state(x, t_now)[:, None, :]
                    times.append(t_now)
                if dead.any():
                    rows[dead] = rec[-1][dead, -1:, :]
                rec.append(rows)
                flags[~dead] |= state_row_flags(rows[~dead], self.v_des[~dead], self.collision_height)
                newly = ~dead & ((flags & self.terminate_mask) != 0)
                flags[newly] |= (i + 1) << TERM_SHIFT
                go = ~dead & ~newly                                                 # these advance: plant = plan
                x_new = X[:, self.nodes_per_replan, :].double().cpu().numpy()
                # (half a simulation step of slack on both ends of the window, as nmpc_rollout_batch: float-safe)
                if push is not None and push["start"] - 0.5 * self.sim_dt <= t_now < push["start"] + push["duration"] - 0.5 * self.sim_dt:
                    x_new[:, 6:9] += np.asarray(push["force"]) * dt_replan / self.mp[1]
                x[go] = x_new[go]
                if self.footsteps:
                    self.touch_down(self._params, go)
                self.sim_step += self.replanning_steps
                self.current_opt_node += self.nodes_per_replan
                self.increment_base_ref_position(self.replanning_steps, go)
        finally:
            self.solver.set_skip(None, 0)
        self._x_last = x
        self.failed = torch.as_tensor(flags).to(self.device)
        S = torch.as_tensor(np.concatenate(rec, axis=1), dtype=torch.float32).to(self.device).contiguous()
        return S, np.asarray(times)

    def _device_rollout(self, n_replans, start_node, first_solve, push, x, v_des, w_des, ref_state, foot, X, U, status):
        """One nmpc_rollout_batch call on explicit device tensors (x, ref_state, foot, X, U are updated in place).
        Returns (S, failed)."""
        s, period = self.solver, self.config_gait.nominal_period
        times = np.arange(n_replans) * self.replanning_steps * self.sim_dt
        if getattr(self, "_gait_dev", None) is None:
            self._gait_dev = s.to_device(self.contact_planner.gait_sequence, torch.int8)
        windows = push_windows(push, x.shape[0])
        if windows is not None:             # a window per rollout: attached for this call, the cfg's own window unused
            push = dict(push, start=0.0, duration=0.0)
        with s.rollout_push_windows(windows):
            return s.rollout(
                self._gait_dev, x, v_des, w_des, ref_state, foot, s.to_device(np.asarray(push["force"])) if push else None,
                np.round((times % period) / period, 4), X, U, status,
                n_replans=n_replans, nodes_per_replan=self.nodes_per_replan, replanning_steps=self.replanning_steps,
                nodes_per_cycle=self.contact_planner.nodes_per_cycle, start_node=start_node, first_solve=int(first_solve),
                max_sqp_first=N_SQP_FIRST, nlp_tol_first=self.config_opt.nlp_tol / 10.0, nlp_tol=self.config_opt.nlp_tol,
                sim_dt=self.sim_dt, time_horizon=self.config_opt.time_horizon, nom_height=self.config_gait.nom_height,
                height_offset=self.height_offset, push_start=float(push["start"]) if push else 0.0,
                push_duration=float(push["duration"]) if push else 0.0, footsteps=int(self.footsteps),
                record_sim_steps=int(self.record_sim_steps), hip_offset=self.raibert.offset_hip_b[:, :2].ravel().tolist(),
                stance_ratio=np.asarray(self.config_gait.stance_ratio, float).tolist(), nominal_period=float(period),
                foot_size=float(self.raibert.foot_size), terminate_mask=int(self.terminate_mask),
                collision_height=float(self.collision_height))

    def open_loop_device(self, x0: np.ndarray, trajectory_time: float, push: Optional[dict] = None):
        """`open_loop` with the whole rollout on the device: one C call launches every replanning
        step (references, shift, solve, plant update) on the stream -- no host round trip per replan.
        Same return value as `open_loop`; the controller state (X, U, node, reference) advances alike."""
        s, B = self.solver, self.batch
        dt_replan = self.replanning_steps * self.sim_dt
        n_replans = int(np.floor(trajectory_time / dt_replan + 1e-9))
        if self.foot_pos is None:
            self.foot_pos = np.asarray(x0)[:, None, :3] * [1, 1, 0] + HIP_OFFSETS[None]
        x = s.to_device(x0)
        v_des, w_des, ref_state = (s.to_device(a, torch.float64) for a in (self.v_des, self.w_des, self.base_ref_vel_tracking))
        foot = s.to_device(self.foot_pos.reshape(B, 12))
        S, failed = self._device_rollout(n_replans, self.current_opt_node, self.first_solve, push, x, v_des, w_des, ref_state,
                                         foot, self.X, self.U, self.status)
        # advance the host-side bookkeeping as open_loop does
        self.first_solve = False
        self.sim_step += n_replans * self.replanning_steps
        self.current_opt_node += n_replans * self.nodes_per_replan
        s.last_node = self.current_opt_node - self.nodes_per_replan
        self.base_ref_vel_tracking = ref_state.cpu().numpy()
        self.x_final, self.failed = x, failed          # failed: NMPC_ROLLOUT_FLAG_* bits (include/nmpc.h)
        if self.footsteps:
            self.foot_pos = foot.cpu().numpy().astype(np.float64).reshape(B, 4, 3)
        times = np.arange(n_replans) * dt_replan
        if self.record_sim_steps:
            times = (times[:, None] + (np.arange(self.replanning_steps) + 1) * self.sim_dt).ravel()
        return S, times

    def open_loop_device_valid(self, x0: np.ndarray, trajectory_time: float, push_sampler, nominal=(0,), max_attempts: int = 8,
                               fill_batch: int = 0):
        """Pushed rollouts with the reference's discard-and-redo: a rollout that terminates early is thrown away and rolled
        again from the same initial state with a NEW push, until it runs to the end
        (data_collection_pretrain_omini_vc_policy_1direction_perturbed.py:217-247, `while True: ... if not
        early_termination: break`; RolloutMPC.py:424-437).  Here the whole batch rolls on the device, the rollouts whose
        flags meet `invalid_mask` are gathered into a compacted batch, given new pushes and rolled again -- at most
        `max_attempts` times in all (the reference loops without a cap); what is still invalid then keeps its flags and
        gets no sampling weight in the learning update (parallel.learning_update).

        push_sampler(n, attempt) -> {"start", "duration", "force": [n, 3]} ("start" and "duration" scalars, or arrays of n: a
        window per rollout, and then per candidate of a redo pass); the rollouts listed in `nominal` are never
        pushed (and never redone).  `fill_batch` > 0: a redo pass over n rollouts rolls max(1, min(fill_batch, batch) // n) candidates
        of each, every one with its own new push, and keeps the FIRST that runs to the end -- the same distribution as the
        reference's one-after-the-other redo (independent pushes, first success kept), but the late passes over a
        handful of rollouts, which take fifty replans each however small they are, collapse into one.
        Call on a freshly reset controller.  Returns (S, t, info) with S, t as
        `open_loop_device` and info = {"attempt_sizes": rollouts run per attempt, "first_attempt": flag counts of the first
        pass}; `self.failed`, `self.x_final`, `self.X`, `self.U`, `self.foot_pos` hold the kept rollouts."""
        assert self.first_solve and self.current_opt_node == 0, "open_loop_device_valid starts from a reset controller"
        s, B, dev = self.solver, self.batch, self.device
        nominal = np.asarray(nominal, dtype=np.int64)
        x0 = np.asarray(x0, dtype=np.float64)
        ref0 = self.base_ref_vel_tracking.copy()
        foot0 = (self.foot_pos if self.foot_pos is not None else x0[:, None, :3] * [1, 1, 0] + HIP_OFFSETS[None]).copy()
        push = push_sampler(B, 0)
        force = np.array(push["force"], dtype=np.float64)
        force[nominal] = 0.0
        S, times = self.open_loop_device(x0, trajectory_time, dict(push, force=force))
        n_replans = int(np.floor(trajectory_time / (self.replanning_steps * self.sim_dt) + 1e-9))
        f0 = self.failed
        count = lambda bit: int((f0 & bit).ne(0).sum().item())
        info = {"attempt_sizes": [B],
                "first_attempt": {"invalid": count(self.invalid_mask), "solver": count(FLAG_SOLVER), "collision": count(FLAG_COLLISION),
                                  "roll": count(FLAG_ROLL), "pitch": count(FLAG_PITCH), "height": count(FLAG_HEIGHT),
                                  "velocity_tracking": count(FLAG_VEL_TRACKING)}}
        keep = torch.ones(B, dtype=torch.bool, device=dev)
        keep[torch.as_tensor(nominal, device=dev)] = False
        for attempt in range(1, max_attempts):
            idx = torch.nonzero((self.failed & self.invalid_mask).ne(0) & keep).flatten()
            n = int(idx.numel())                                   # (the one host round trip of an attempt)
            if n == 0:
                break
            cand = max(1, min(fill_batch, B) // n)                       # candidates per rollout of this pass (the solver holds B problems)
            m = n * cand
            idx_h = np.repeat(idx.cpu().numpy(), cand)                    # candidate j rolls rollout idx[j // cand]
            push_n = push_sampler(m, attempt)
            x = s.to_device(x0[idx_h])
            v_des, w_des, ref_state = (s.to_device(a[idx_h], torch.float64) for a in (self.v_des, self.w_des, ref0))
            foot = s.to_device(foot0[idx_h].reshape(m, 12))
            Xn = torch.zeros(m, self.n_nodes + 1, 12, dtype=torch.float32, device=dev)
            Un = torch.zeros(m, self.n_nodes, 12, dtype=torch.float32, device=dev)
            stn = torch.zeros(m, dtype=torch.int32, device=dev)
            Sn, failed_n = self._device_rollout(n_replans, 0, True, push_n, x, v_des, w_des, ref_state, foot, Xn, Un, stn)
            # the candidate kept for a rollout: its first valid one, or its first one if none is
            bad = (failed_n & self.invalid_mask).ne(0).view(n, cand)
            first_ok = torch.argmax((~bad).to(torch.int8), dim=1)         # (argmax of an all-zero row is 0)
            pick = torch.arange(n, device=dev) * cand + first_ok
            S[idx] = Sn[pick]
            self.failed[idx] = failed_n[pick]
            self.x_final[idx] = x[pick]
            self.X[idx] = Xn[pick]; self.U[idx] = Un[pick]; self.status[idx] = stn[pick]
            pick_h, rows_h = pick.cpu().numpy(), idx_h[::cand]
            self.base_ref_vel_tracking[rows_h] = ref_state.cpu().numpy()[pick_h]
            if self.footsteps:
                self.foot_pos[rows_h] = foot.cpu().numpy().astype(np.float64).reshape(m, 4, 3)[pick_h]
            info["attempt_sizes"].append(m)
        return S, times, info

    def record_state(self, x: np.ndarray, t: float) -> np.ndarray:
        period = self.config_gait.nominal_period
        phase = np.round((t % period) / period, 4)
        base_wrt_feet = (x[:, None, :2] - self.foot_pos[:, :, :2]).reshape(self.batch, 8)
        return np.concatenate([np.full((self.batch, 1), phase), x[:, 6:9], x[:, 9:12], x[:, 2:6],
                               base_wrt_feet], axis=1)

    def print_timings(self) -> None:
        print_timings(self.timings)
