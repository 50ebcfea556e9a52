"""Batched NMPC solver on MI355X: Python host mirror of the reference's solver surface.

`BatchedNmpcSolver` is the batched drop-in for the solve path of
`QuadrupedAcadosSolver` (mpc_controller/utils/solver.py:15-429): the reference's
    set_max_iter / set_nlp_tol / set_qp_tol      solver.py:75-79, mpc.py:464-473
    update_cost / set_cost_weights                solver.py:100-141
    warm_start_solver(i_node)                     solver.py:290-342
    init(...) + solve()                           solver.py:355-429
keep their names and meaning; arrays gain a leading batch axis and live on the GPU as torch
tensors (containers only -- all arithmetic is in libnmpc_hip.so).  Per-problem failures are
reported in `status` (acados numbering) instead of exceptions (mpc.py:562-569).
"""
from __future__ import annotations

import contextlib
import ctypes
from collections import defaultdict
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream
# the bits of the `failed` tensors that the rollouts return (include/nmpc.h), for the controllers
from ._lib import (NMPC_ROLLOUT_FLAG_COLLISION, NMPC_ROLLOUT_FLAG_HEIGHT, NMPC_ROLLOUT_FLAG_MASK,  # noqa: F401
                   NMPC_ROLLOUT_FLAG_PITCH, NMPC_ROLLOUT_FLAG_ROLL, NMPC_ROLLOUT_FLAG_SOLVER,
                   NMPC_ROLLOUT_FLAG_VEL_TRACKING, NMPC_ROLLOUT_TERM_SHIFT)
from .profiling import time_fn
from .trajectory_io import KD, KP
from .workloads import MODEL_DIMS, MP_NAMES


class BatchedNmpcSolver:
    """B independent NMPC problems of one model, solved together (one problem per wavefront)."""

    def __init__(self, model_id: int, n_nodes: int, batch_max: int, device="cuda:0",
                 compute_timings: bool = False, precision: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedNmpcSolver needs a HIP device; there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.model_id, self.n_nodes, self.batch_max = int(model_id), int(n_nodes), int(batch_max)
        d = MODEL_DIMS[self.model_id]
        self.nx, self.nu, self.np, self.ng = d["nx"], d["nu"], d["np"], d["ng"]
        self.ny, self.ny_e = d["ny"], d["ny_e"]      # cost residuals of a stage / of the terminal node
        self.compute_timings = compute_timings
        self.timings = defaultdict(list)
        self.last_node = 0
        # precision 0: fp32 throughout; 1: bf16 barrier product (mixed precision), see include/nmpc.h
        self.precision = int(precision)
        dims = _lib.NmpcDims(self.model_id, self.n_nodes, self.batch_max, self.precision)
        self._h = ctypes.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.nmpc_create(ctypes.byref(dims), dev_index, ctypes.byref(self._h)), None, "nmpc_create")
        self.momentum_model, self._momentum_layer = "declared", None      # set_momentum_model
        self.state_momentum = "declared"                                  # set_state_momentum
        self._opts = dict(max_iter=1, max_qp_iter=6, nlp_tol=0.0, qp_tol=1e-2, line_search=0)
        self._push_opts()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.nmpc_destroy(h)
            self._h = None

    # -- configuration (names as in solver.py:75-79,100-141) ------------------------------------
    def _push_opts(self):
        o = self._opts
        _lib.check(self.lib.nmpc_set_opts(self._h, o["max_iter"], o["max_qp_iter"], o["nlp_tol"],
                                          o["qp_tol"], o["line_search"]), self._h, "nmpc_set_opts")

    def set_max_iter(self, n: int):
        self._opts["max_iter"] = int(n); self._push_opts()

    def set_max_qp_iter(self, n: int):
        self._opts["max_qp_iter"] = int(n); self._push_opts()

    def set_nlp_tol(self, tol: float):
        self._opts["nlp_tol"] = float(tol); self._push_opts()

    def set_qp_tol(self, tol: float):
        self._opts["qp_tol"] = float(tol); self._push_opts()

    def set_line_search(self, on: bool):
        self._opts["line_search"] = int(bool(on)); self._push_opts()

    # contact patterns of a trot: diagonal pairs (feet 0+3, 1+2), four-foot stance, flight -- as 4-bit stance flags
    COMMON_CONTACT_PATTERNS = frozenset({0b1001, 0b0110, 0b1111, 0b0000})

    def set_contact_patterns(self, all_patterns: bool = None, gait_sequence=None):
        """Choose the kernel by the gait: `gait_sequence[4, nodes]` (0/1 stance flags, contact_planner.py)
        whose patterns all belong to a trot keeps the default kernel; any other pattern selects the
        kernel with a static stage body for every contact pattern (see include/nmpc.h)."""
        if all_patterns is None:
            g = np.asarray(gait_sequence).astype(np.int64)
            pats = set((g[0] | (g[1] << 1) | (g[2] << 2) | (g[3] << 3)).tolist())
            all_patterns = not pats <= self.COMMON_CONTACT_PATTERNS
        _lib.check(self.lib.nmpc_set_contact_patterns(self._h, int(bool(all_patterns))), self._h, "nmpc_set_contact_patterns")
        return bool(all_patterns)

    def set_skip(self, flags: Optional[torch.Tensor], mask: int = 0):
        """Leave problems out of the following solves: flags int32 [batch_max] on the device (kept alive by the caller
        and by this object), a problem with flags[b] & mask != 0 is skipped -- X, U, status untouched, no time spent
        (terminated rollouts).  None detaches.  The flags are read when the kernels run."""
        if flags is not None:
            self._chk(flags, (self.batch_max,), "flags", torch.int32)
        self._skip_flags = flags
        _lib.check(self.lib.nmpc_set_skip(self._h, ptr(flags), int(mask)), self._h, "nmpc_set_skip")

    def set_rollout_actions(self, layer, zoh: Optional[torch.Tensor] = None, A: Optional[torch.Tensor] = None,
                            kp: float = KP, kd: float = KD):
        """nmpc_wb_rollout_set_actions: while A [B, rows, 12] (rows as the S of the rollout) is attached, `wb_rollout` records
        the expert's action beside every state row -- per replan one `BatchedTorqueLayer.plan_actions` on that replan's plan.
        layer: the `BatchedTorqueLayer` of the robot; zoh int32 [replanning_steps] on the device: the held node of each step.
        `set_rollout_actions(None)` detaches.  This object keeps the three alive while they are attached."""
        if layer is None:
            self._labels = None
            _lib.check(self.lib.nmpc_wb_rollout_set_actions(self._h, None, None, 0.0, 0.0, None), self._h, "nmpc_wb_rollout_set_actions")
            return
        if not isinstance(A, torch.Tensor) or A.dim() != 3:
            raise ValueError("A: need a float32 tensor [B, rows, 12] on the GPU")
        self._chk(A, (A.shape[0], A.shape[1], 12), "A")
        self._chk_zoh(zoh)
        self._labels = (layer, zoh, A)
        _lib.check(self.lib.nmpc_wb_rollout_set_actions(self._h, layer._h, ptr(zoh), float(kp), float(kd), ptr(A)),
                   self._h, "nmpc_wb_rollout_set_actions")

    def set_rollout_plant(self, layer, ground=None, n_sub: int = 2, kp: float = KP, kd: float = KD,
                          zoh: Optional[torch.Tensor] = None):
        """nmpc_wb_rollout_set_plant: while a plant is attached, `wb_rollout` runs the expert in closed loop on the ground-contact
        plant of `layer` (a `BatchedTorqueLayer` of the robot) instead of following its plan: per replan the labels of the plan
        (`plan_actions`), `contact_track` over the interval with those rows as PD targets (n_sub substeps of sim_dt / n_sub per
        simulation step), `observe_rows` into S.  Row j of S is then the plant state before simulation step j, row j of the
        actions of `set_rollout_actions` (same kp, kd) the PD target applied from it.  ground: a `torque.GroundContact`; zoh
        int32 [replanning_steps] on the device, the held node of each step (not needed while `set_rollout_actions` is attached,
        whose zoh is used).  `set_rollout_plant(None)` detaches.  The workspaces of the call ([batch_max, replanning_steps, 12 /
        18 / 18]) are allocated here and kept alive, with layer and zoh, while the plant is attached."""
        if layer is None:
            self._plant = None
            _lib.check(self.lib.nmpc_wb_rollout_set_plant(self._h, None, None, 0, 0.0, 0.0, None, None, None, None), self._h,
                       "nmpc_wb_rollout_set_plant")
            return
        if zoh is not None:
            self._chk_zoh(zoh)
        labels = getattr(self, "_labels", None)
        steps = zoh.shape[0] if zoh is not None else (labels[1].shape[0] if labels is not None else 0)
        if steps < 1:
            raise ValueError("zoh: the plant needs the held node of each step, here or from set_rollout_actions")
        Aw = torch.zeros(self.batch_max, steps, 12, dtype=torch.float32, device=self.device)
        Qw, Vw = (torch.zeros(self.batch_max, steps, 18, dtype=torch.float32, device=self.device) for _ in range(2))
        cfg = ground.cfg() if ground is not None else None
        self._plant = (layer, zoh, Aw, Qw, Vw)
        _lib.check(self.lib.nmpc_wb_rollout_set_plant(self._h, layer._h, ctypes.byref(cfg) if cfg is not None else None, int(n_sub), float(kp),
                                                      float(kd), ptr(zoh), ptr(Aw), ptr(Qw), ptr(Vw)), self._h, "nmpc_wb_rollout_set_plant")

    def set_rollout_plant_push(self, as_force: bool = False):
        """nmpc_wb_rollout_set_plant_push: how a `wb_rollout` with a plant attached applies its push_force.  False (the
        default): the velocity jump F dt_replan / m per replanning interval of the plan-following rollouts.  True: a force on
        the trunk of the plant (`BatchedTorqueLayer.set_push`'s push, handed to every replan's track launch by the rollout
        itself) over the substeps of sim_dt / n_sub the window covers; a rollout without a plant is then refused, as is one
        whose torque layer has a push of the caller's attached."""
        _lib.check(self.lib.nmpc_wb_rollout_set_plant_push(self._h, int(bool(as_force))), self._h, "nmpc_wb_rollout_set_plant_push")

    def set_rollout_clock(self, replan0: int = 0):
        """nmpc_wb_rollout_set_clock: while replan0 > 0 is set, replan i of every following `wb_rollout` is replan replan0 + i of
        a longer rollout -- the recorded phase, the push window (push_start counts from the long rollout's step 0) and the
        stamp replan0 + i + 1 in `failed` are that rollout's, the rows written are this call's own.  0 (the default): a rollout
        starts at its call.  A negative value and a handle of another model are refused and leave the previous value in force."""
        _lib.check(self.lib.nmpc_wb_rollout_set_clock(self._h, int(replan0)), self._h, "nmpc_wb_rollout_set_clock")

    def set_rollout_push_windows(self, start=None, duration=None):
        """nmpc_rollout_set_push_windows / nmpc_wb_rollout_set_push_windows (by the model of this solver): while start, duration
        (B entries each, seconds from step 0 of the rollout; arrays or tensors) are attached, rollout b of every following
        `rollout` / `wb_rollout` is pushed with its push_force over its own window instead of the cfg's push_start /
        push_duration, duration[b] <= 0 meaning no push for it -- as a velocity jump or, with a plant and
        `set_rollout_plant_push(True)`, as a force.  Rollout b is the bits it is under the cfg window of its own.
        `set_rollout_push_windows(None)` detaches.  This object keeps the two tensors alive while they are attached; a rollout
        of more rollouts than they have entries, or one without a push_force, is refused."""
        call, name = ((self.lib.nmpc_wb_rollout_set_push_windows, "nmpc_wb_rollout_set_push_windows") if self.model_id == 2
                      else (self.lib.nmpc_rollout_set_push_windows, "nmpc_rollout_set_push_windows"))
        if start is None and duration is None:
            self._push_windows = None
            _lib.check(call(self._h, None, None, 0), self._h, name)
            return
        if start is None or duration is None:
            raise ValueError("start and duration come together or not at all")
        start, duration = (torch.as_tensor(np.asarray(x.detach().cpu()) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64),
                                           dtype=torch.float32).to(self.device).contiguous() for x in (start, duration))
        if start.dim() != 1 or start.shape != duration.shape or start.shape[0] < 1:
            raise ValueError(f"start, duration: need one entry per rollout each, got {tuple(start.shape)} and {tuple(duration.shape)}")
        self._push_windows = (start, duration)
        _lib.check(call(self._h, ptr(start), ptr(duration), start.shape[0]), self._h, name)

    @contextlib.contextmanager
    def rollout_push_windows(self, windows):
        """`set_rollout_push_windows(*windows)` for the duration of a block: attached at its entry, detached behind it whatever
        happens in it.  windows None (`mpc.push_windows` of a push with a scalar window): nothing is attached and nothing detached."""
        if windows is None:
            yield
            return
        try:
            self.set_rollout_push_windows(*windows)
            yield
        finally:
            self.set_rollout_push_windows(None)

    MOMENTUM_MODELS = {"declared": 0, "articulated": 1}      # NMPC_WB_MOMENTUM_* of include/nmpc.h

    def set_momentum_model(self, model: str = "declared", torque_layer=None):
        """nmpc_wb_set_momentum_model: the momentum map of the whole-body model.  "declared" (the default): one rigid body of
        the model parameters' mass and inertia at the base origin.  "articulated": com(q) and A_g(q) of the tree of
        `torque_layer` (a `BatchedTorqueLayer` of 18 joints in the coordinates of the model) in the consistency rows and the
        momentum rows of the dynamics; the layer is borrowed and kept alive by this object while the mode is on.  `solve` works
        in both modes; `wb_rollout` and `label_states` build x0's momentum from the declared map and are refused in the
        articulated mode until `set_state_momentum("tree")` gives x0 the momentum of the tree."""
        if model not in self.MOMENTUM_MODELS:
            raise ValueError(f"momentum model: one of {sorted(self.MOMENTUM_MODELS)}, got {model!r}")
        if model == "articulated" and torque_layer is None:
            raise ValueError("the articulated momentum model needs torque_layer")
        layer = torque_layer if model == "articulated" else None
        self.state_momentum = "declared"      # the library puts the switch back with every call, one it then refuses included
        _lib.check(self.lib.nmpc_wb_set_momentum_model(self._h, layer._h if layer is not None else None, self.MOMENTUM_MODELS[model]),
                   self._h, "nmpc_wb_set_momentum_model")
        self._momentum_layer = layer
        self.momentum_model = model

    STATE_MOMENTUM = {"declared": 0, "tree": 1}      # NMPC_WB_STATE_MOMENTUM_* of include/nmpc.h

    def set_state_momentum(self, source: str = "declared"):
        """nmpc_wb_set_state_momentum: where `wb_rollout` and `label_states` take the momentum slots of a measured state from.
        "declared" (the default): the declared map, so both are refused while the momentum model is "articulated".  "tree"
        (articulated mode only): h = A_g(q) v of the momentum model's tree, one `BatchedTorqueLayer.state_momentum` launch behind
        the prepare kernel of every replan or chunk; the robot's mass in the force reference's weight share and in a push's
        velocity jump is then the mass of the tree.  `set_momentum_model` puts the source back to "declared"."""
        if source not in self.STATE_MOMENTUM:
            raise ValueError(f"state momentum: one of {sorted(self.STATE_MOMENTUM)}, got {source!r}")
        _lib.check(self.lib.nmpc_wb_set_state_momentum(self._h, self.STATE_MOMENTUM[source]), self._h, "nmpc_wb_set_state_momentum")
        self.state_momentum = source

    def set_ipm(self, mu0=10.0, sigma=0.2, s_min=1.0, gamma=0.995, tau_min=0.1, merit_rho=1e3):
        _lib.check(self.lib.nmpc_set_ipm(self._h, mu0, sigma, s_min, gamma, tau_min, merit_rho),
                   self._h, "nmpc_set_ipm")

    def set_model_params(self, mp):
        mp = np.ascontiguousarray(mp, dtype=np.float32)
        assert mp.shape == (len(MP_NAMES),)
        _lib.check(self.lib.nmpc_set_model_params(
            self._h, mp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(mp)), self._h, "nmpc_set_model_params")

    def set_cost_weights(self, W, W_e, reg_eps: float = 1e-6, reg_eps_e: float = 1e-5):
        W = np.ascontiguousarray(W, dtype=np.float32)
        W_e = np.ascontiguousarray(W_e, dtype=np.float32)
        assert W.shape == (self.ny,) and W_e.shape == (self.ny_e,)
        fp = ctypes.POINTER(ctypes.c_float)
        _lib.check(self.lib.nmpc_set_weights(self._h, W.ctypes.data_as(fp), W_e.ctypes.data_as(fp),
                                             reg_eps, reg_eps_e), self._h, "nmpc_set_weights")

    update_cost = set_cost_weights

    # -- tensors --------------------------------------------------------------------------------
    def _chk(self, t: torch.Tensor, shape, name: str, dtype=torch.float32) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor on {self.device}")
        if t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: need contiguous {dtype} {tuple(shape)} on the GPU, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        return t

    def _chk_zoh(self, zoh, shape=None) -> None:
        """a hold table: int32 of `shape` on the device (None: one entry per simulation step of a replan, any number of them),
        every entry a node of the horizon"""
        if shape is None:
            if not isinstance(zoh, torch.Tensor) or zoh.dim() != 1:
                raise ValueError("zoh: need an int32 tensor [replanning_steps] on the GPU")
            shape = (zoh.shape[0],)
        self._chk(zoh, shape, "zoh", torch.int32)
        if not bool(((zoh >= 0) & (zoh < self.n_nodes)).all()):
            raise ValueError(f"zoh: node indices must lie in [0, {self.n_nodes})")

    def to_device(self, a, dtype=torch.float32) -> torch.Tensor:
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device).contiguous()

    # -- solve path -----------------------------------------------------------------------------
    @time_fn("warm_start_solver")
    def warm_start_solver(self, X: torch.Tensor, U: torch.Tensor, shift: int) -> None:
        """Shift the previous solution left by `shift` nodes in place (solver.py:304-322)."""
        B = X.shape[0]
        self._chk(X, (B, self.n_nodes + 1, self.nx), "X")
        self._chk(U, (B, self.n_nodes, self.nu), "U")
        _lib.check(self.lib.nmpc_shift_warm_start(self._h, B, int(shift), ptr(X), ptr(U),
                                                  stream(self.device)), self._h, "nmpc_shift_warm_start")

    @time_fn("solve")
    def solve(self, x0, yref, yref_e, params, X, U, status=None, stats=None, shift: int = 0
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Solve B problems in place on (X, U).  Returns (X, U, status[B] int32, stats[B,4]).

        shift > 0 folds `warm_start_solver(X, U, shift)` into the solve (same result, no extra
        launch: the first SQP iteration reads X, U through the shift's index map)."""
        B, N = x0.shape[0], self.n_nodes
        self._chk(x0, (B, self.nx), "x0")
        per_stage = yref.dim() == 3
        self._chk(yref, (B, N, self.ny) if per_stage else (B, self.ny), "yref")
        self._chk(yref_e, (B, self.ny_e), "yref_e")
        if self.np > 0:
            self._chk(params, (B, N + 1, self.np), "params")
        self._chk(X, (B, N + 1, self.nx), "X")
        self._chk(U, (B, N, self.nu), "U")
        if status is None:
            status = torch.empty(B, dtype=torch.int32, device=self.device)
        if stats is None:
            stats = torch.empty(B, 4, dtype=torch.float32, device=self.device)
        self._chk(status, (B,), "status", torch.int32)
        self._chk(stats, (B, 4), "stats")
        _lib.check(self.lib.nmpc_shift_solve_batch(
            self._h, B, int(shift), ptr(x0), ptr(yref), int(per_stage), ptr(yref_e),
            ptr(params) if self.np > 0 else None, ptr(X), ptr(U), ptr(status), ptr(stats),
            stream(self.device)), self._h, "nmpc_shift_solve_batch")
        return X, U, status, stats

    def riccati(self, Q, R, q, r, A, Bm, d, dx0):
        """LQ core on explicit dense stage data (test / building-block entry)."""
        Bsz, N, nx = A.shape[0], A.shape[1], A.shape[2]
        nu = Bm.shape[3]
        assert N == self.n_nodes
        dX = torch.empty(Bsz, N + 1, nx, dtype=torch.float32, device=self.device)
        dU = torch.empty(Bsz, N, nu, dtype=torch.float32, device=self.device)
        status = torch.empty(Bsz, dtype=torch.int32, device=self.device)
        for t in (Q, R, q, r, A, Bm, d, dx0):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device.type == "cuda"
        _lib.check(self.lib.nmpc_riccati_batch(
            self._h, Bsz, nx, nu, ptr(Q), ptr(R), ptr(q), ptr(r), ptr(A), ptr(Bm), ptr(d),
            ptr(dx0), ptr(dX), ptr(dU), ptr(status), stream(self.device)), self._h, "nmpc_riccati_batch")
        return dX, dU, status

    # -- device-resident rollouts (include/nmpc.h) ----------------------------------------------
    def rollout(self, gait, x, v_des, w_des, ref_state, foot_pos, push_force, phase, X, U, status, **cfg):
        """nmpc_rollout_batch: B = x.shape[0] centroidal rollouts from one call.  cfg: every field of nmpc_rollout_cfg by
        name; phase: host [n_replans].  x, ref_state, foot_pos, X, U and status are updated in place.
        Returns (S [B, rows, 19], failed [B] int32: NMPC_ROLLOUT_FLAG_* bits)."""
        c = _cfg(_lib.NmpcRolloutCfg, cfg)
        B = x.shape[0]
        self._chk(gait, (4, c.nodes_per_cycle), "gait", torch.int8)
        self._chk(x, (B, self.nx), "x")
        self._chk(foot_pos, (B, 12), "foot_pos")
        S, failed = self._rollout_io(c, B, v_des, w_des, ref_state, push_force, X, U, status, 19)
        phase = np.ascontiguousarray(phase, dtype=np.float32)
        assert phase.shape == (c.n_replans,)
        _lib.check(self.lib.nmpc_rollout_batch(
            self._h, B, ctypes.byref(c), ptr(gait), ptr(x), ptr(v_des), ptr(w_des), ptr(ref_state), ptr(foot_pos),
            ptr(push_force), phase.ctypes.data_as(ctypes.c_void_p), ptr(X), ptr(U), ptr(S), ptr(status), ptr(failed),
            stream(self.device)), self._h, "nmpc_rollout_batch")
        return S, failed

    def wb_rollout(self, gait, peaks, nodes, q, v, v_des, w_des, ref_state, joint_ref, push_force, X, U, status, failed=None, **cfg):
        """nmpc_wb_rollout_batch: B = q.shape[0] whole-body rollouts from one call.  cfg: every field of
        nmpc_wb_rollout_cfg by name; nodes: host, the optimisation node of each replan.  q, v, ref_state, X, U and status
        are updated in place.  Returns (S [B, rows, 44], failed [B] int32: NMPC_ROLLOUT_FLAG_* bits).  failed (int32 [B] on the
        device, None: zeros): the flags the rollouts enter the call with, updated in place and returned -- those a previous
        call left, where this one continues its rollouts (`set_rollout_clock`): a rollout that carries a stamp stays frozen."""
        c = _cfg(_lib.NmpcWbRolloutCfg, cfg)
        B = q.shape[0]
        for t, name in ((gait, "gait"), (peaks, "peaks")):
            self._chk(t, (4, c.nodes_per_cycle), name, torch.int8)
        self._chk(q, (B, 18), "q")
        self._chk(v, (B, 18), "v")
        self._chk(joint_ref, (12,), "joint_ref")
        S, fresh = self._rollout_io(c, B, v_des, w_des, ref_state, push_force, X, U, status, 44)
        if failed is None:
            failed = fresh
        else:
            self._chk(failed, (B,), "failed", torch.int32)
        assert len(nodes) == c.n_replans
        if getattr(self, "_labels", None) is not None:           # the attached label buffer must be this rollout's size
            _, zoh, A = self._labels
            self._chk(A, (B, S.shape[1], 12), "A (set_rollout_actions)")
            if c.record_sim_steps:
                self._chk(zoh, (c.replanning_steps,), "zoh (set_rollout_actions)", torch.int32)
        if getattr(self, "_plant", None) is not None and c.record_sim_steps:      # the plant's workspaces hold one replanning interval
            self._chk(self._plant[2], (self.batch_max, c.replanning_steps, 12), "workspace (set_rollout_plant: zoh has another length)")
        nodes = (ctypes.c_int * c.n_replans)(*nodes)
        _lib.check(self.lib.nmpc_wb_rollout_batch(
            self._h, B, ctypes.byref(c), ptr(gait), ptr(peaks), ctypes.cast(nodes, ctypes.c_void_p), ptr(q), ptr(v),
            ptr(v_des), ptr(w_des), ptr(ref_state), ptr(joint_ref), ptr(push_force), ptr(X), ptr(U), ptr(S), ptr(status),
            ptr(failed), stream(self.device)), self._h, "nmpc_wb_rollout_batch")
        return S, failed

    def label_states(self, layer, gait, peaks, node, ref_steps, Q, V, v_des, w_des, ref_state, joint_ref, zoh, failed=None,
                     A=None, status=None, X=None, U=None, **cfg):
        """nmpc_wb_label_states_batch: the expert's first solve from every visited state Q, V [B, K, 18] (a policy rollout's, with
        `BatchedTorqueLayer.set_rollout_states`; slices of longer tables are taken with their stride) and the PD target it would
        apply from it.  cfg: every field of nmpc_wb_label_cfg by name but n_rows (= K); node, ref_steps: int32 [K] on the
        device, the optimisation node of row k and the simulation steps the base reference has been integrated over by then;
        v_des, w_des, ref_state: float64 [B, 3 / 3 / 12], read only; zoh int32 [1]: the held node of simulation step 0; failed
        int32 [B] or None: the rollout's flags, states from a robot's termination on are left out (their A and status keep what
        the given tensors hold, zeros in new ones).  B K problems are solved in chunks of batch_max; X, U (the workspace of one
        chunk, [min(B K, batch_max), N + 1, 42] and [.., N, 30]) hold the plans of the last chunk afterwards.
        -> (A [B, K, 12], status int32 [B, K], X, U)."""
        if not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[1] < 1:
            raise ValueError("Q: need a float32 tensor [B, K, 18] on the GPU with K >= 1")
        B, K, N = Q.shape[0], Q.shape[1], self.n_nodes
        Q, qv_rows = layer._rows(Q, 18, "Q", B)
        V, v_rows = layer._rows(V, 18, "V", B)
        if V.shape[1] != K or v_rows != qv_rows:
            raise ValueError("Q, V: need the same rows and one layout")
        c = _cfg(_lib.NmpcWbLabelCfg, dict(cfg, n_rows=K))
        for t, name in ((gait, "gait"), (peaks, "peaks")):
            self._chk(t, (4, c.nodes_per_cycle), name, torch.int8)
        self._chk(node, (K,), "node", torch.int32)
        self._chk(ref_steps, (K,), "ref_steps", torch.int32)
        if not bool((node >= 0).all()) or not bool((ref_steps >= 0).all()):
            raise ValueError("node, ref_steps: must not be negative")
        self._chk(v_des, (B, 3), "v_des", torch.float64)
        self._chk(w_des, (B, 3), "w_des", torch.float64)
        self._chk(ref_state, (B, 12), "ref_state", torch.float64)
        self._chk(joint_ref, (12,), "joint_ref")
        self._chk_zoh(zoh, (1,))
        if failed is not None:
            self._chk(failed, (B,), "failed", torch.int32)
        chunk = min(B * K, self.batch_max)
        A = torch.zeros(B, K, 12, dtype=torch.float32, device=self.device) if A is None else A
        A, a_rows = layer._rows(A, 12, "A", B)
        if A.shape[1] != K:
            raise ValueError(f"A: need {K} rows")
        status = torch.zeros(B, K, dtype=torch.int32, device=self.device) if status is None else status
        X = torch.zeros(chunk, N + 1, self.nx, dtype=torch.float32, device=self.device) if X is None else X
        U = torch.zeros(chunk, N, self.nu, dtype=torch.float32, device=self.device) if U is None else U
        self._chk(status, (B, K), "status", torch.int32)
        self._chk(X, (chunk, N + 1, self.nx), "X")
        self._chk(U, (chunk, N, self.nu), "U")
        _lib.check(self.lib.nmpc_wb_label_states_batch(
            self._h, layer._h, B, ctypes.byref(c), ptr(gait), ptr(peaks), ptr(node), ptr(ref_steps), ptr(Q), ptr(V), qv_rows,
            ptr(v_des), ptr(w_des), ptr(ref_state), ptr(joint_ref), ptr(failed), ptr(zoh), ptr(A), a_rows, ptr(status), ptr(X), ptr(U),
            stream(self.device)), self._h, "nmpc_wb_label_states_batch")
        return A, status, X, U

    def _rollout_io(self, c, B, v_des, w_des, ref_state, push_force, X, U, status, row_width):
        """checks of the arguments both rollout calls share; the outputs S and failed"""
        N = self.n_nodes
        self._chk(v_des, (B, 3), "v_des", torch.float64)
        self._chk(w_des, (B, 3), "w_des", torch.float64)
        self._chk(ref_state, (B, 12), "ref_state", torch.float64)
        if push_force is not None:
            self._chk(push_force, (B, 3), "push_force")
        self._chk(X, (B, N + 1, self.nx), "X")
        self._chk(U, (B, N, self.nu), "U")
        self._chk(status, (B,), "status", torch.int32)
        rows = c.n_replans * (c.replanning_steps if c.record_sim_steps else 1)
        S = torch.empty(B, rows, row_width, dtype=torch.float32, device=self.device)
        return S, torch.zeros(B, dtype=torch.int32, device=self.device)

    def debug_tile(self, b: int, k: int, which: int) -> np.ndarray:
        """16x16 stage tile (row, col) of problem b: 0 A~, 1 B~, 2 K~, 3 Acl~ (test hook)."""
        out = np.zeros(256, dtype=np.float32)
        _lib.check(self.lib.nmpc_debug_read_tile(self._h, b, k, which,
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
                   self._h, "nmpc_debug_read_tile")
        return out.reshape(16, 16).copy()   # logical (row, col), zero padded

    def debug_workspace(self, b: int, offset: int, count: int) -> np.ndarray:
        """raw floats of problem b's workspace (test hook of the whole-body kernels)"""
        out = np.zeros(count, dtype=np.float32)
        _lib.check(self.lib.nmpc_debug_read_workspace(self._h, b, offset, count,
                                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
                   self._h, "nmpc_debug_read_workspace")
        return out

    def debug_wb_layout(self) -> dict:
        out = (ctypes.c_size_t * 8)()
        _lib.check(self.lib.nmpc_debug_wb_layout(self.n_nodes, out), self._h, "nmpc_debug_wb_layout")
        return dict(zip(("rec", "js", "qt", "kt", "arr", "stride", "NS", "REC"), (int(v) for v in out)))

    def debug_momentum(self, b: int, k: int):
        """(momentum record [228], dense consistency record [216]) of node k of problem b (test hook of the articulated mode)"""
        fp = ctypes.POINTER(ctypes.c_float)
        mrec, dcons = np.zeros(228, dtype=np.float32), np.zeros(216, dtype=np.float32)
        _lib.check(self.lib.nmpc_debug_read_momentum(self._h, b, k, mrec.ctypes.data_as(fp), dcons.ctypes.data_as(fp)),
                   self._h, "nmpc_debug_read_momentum")
        return mrec, dcons

    def debug_rollout_problem(self, b: int):
        """(x0 [42], yref [N, 90]) of problem b as the last replan of `wb_rollout` / the last chunk of `label_states` prepared
        it (test hook)"""
        fp = ctypes.POINTER(ctypes.c_float)
        x0, yref = np.zeros(self.nx, dtype=np.float32), np.zeros((self.n_nodes, self.ny), dtype=np.float32)
        _lib.check(self.lib.nmpc_debug_read_rollout_problem(self._h, b, x0.ctypes.data_as(fp), yref.ctypes.data_as(fp)),
                   self._h, "nmpc_debug_read_rollout_problem")
        return x0, yref

    def debug_centroidal_rollout_problem(self, b: int):
        """(yref [N, 24], yref_e [12], params [N + 1, 16]) of problem b as the prepare kernel of the last replan of `rollout`
        left them (test hook)"""
        fp = ctypes.POINTER(ctypes.c_float)
        N = self.n_nodes
        yref, yref_e, params = (np.zeros(s, dtype=np.float32) for s in ((N, 24), (12,), (N + 1, 16)))
        _lib.check(self.lib.nmpc_debug_read_centroidal_rollout_problem(self._h, b, yref.ctypes.data_as(fp), yref_e.ctypes.data_as(fp),
                                                                      params.ctypes.data_as(fp)),
                   self._h, "nmpc_debug_read_centroidal_rollout_problem")
        return yref, yref_e, params

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.nmpc_workspace_bytes(self._h))


def _cfg(struct, fields: dict):
    """a rollout configuration struct from ALL of its fields by name (array fields from sequences)"""
    names = [f for f, _ in struct._fields_]
    if set(fields) != set(names):
        raise TypeError(f"{struct.__name__}: missing {sorted(set(names) - set(fields))}, "
                        f"unknown {sorted(set(fields) - set(names))}")
    return struct(**{f: t(*fields[f]) if issubclass(t, ctypes.Array) else fields[f] for f, t in struct._fields_})


def tracking_error(S: torch.Tensor, S_nom: torch.Tensor, threshold: float = 4.0,
                   ood_weight: float = 5.0, with_weights: bool = True):
    """err[b,t] = ||S[b,t,1:] - S_nom[t,1:]||_2 and the OOD sampling weights
    (data_collection_force_perturbation.py:138-156; test_train_policy.py:127-134)."""
    lib = _lib.load()
    B, T, ns = S.shape
    assert S_nom.shape == (T, ns)
    for t in (S, S_nom):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.device.type == "cuda"
    err = torch.empty(B, T, dtype=torch.float32, device=S.device)
    w = torch.empty(B, T, dtype=torch.float32, device=S.device) if with_weights else None
    _lib.check(lib.nmpc_tracking_error(None, B, T, ns, ptr(S), ptr(S_nom), ptr(err), ptr(w),
                                       threshold, ood_weight, stream(S.device)), None, "nmpc_tracking_error")
    return (err, w) if with_weights else err
