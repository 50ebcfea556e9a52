"""Torque layer -- host mirror of `QuadrupedDynamics.id_torques` (mpc_controller/utils/dynamics.py:136-163),
`LocomotionMPC._compute_pd_torques` (mpc_controller/mpc.py:592-599) and the recorded action
(DAgger/utils/RolloutMPC.py:228-250) over the C-ABI of include/nmpc_torque.h, with a leading batch axis.

The robot is given as arrays (the reference reads a URDF through pinocchio; neither is in the image): a tree
of 1-DoF joints whose first six are the virtual base joints of the reference's state
[px, py, pz, yaw, pitch, roll, joints]."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream
from .config import TERMINATE_DEFAULT, GaitConfigFactory
from .trajectory_io import KD, KP, N_STATE

NOMINAL_PERIOD = GaitConfigFactory.get("trot").nominal_period      # the recorded phase of a row runs over the gait's nominal period
INTEGRATORS = {"explicit": _lib.NMPC_INTEGRATOR_EXPLICIT, "implicit": _lib.NMPC_INTEGRATOR_LINEARLY_IMPLICIT}


def integrator_mode(name) -> int:
    """the NMPC_INTEGRATOR_* constant of an integrator's name; ValueError for any other"""
    if not isinstance(name, str) or name not in INTEGRATORS:
        raise ValueError(f"integrator: expected one of {sorted(INTEGRATORS)}, got {name!r}")
    return INTEGRATORS[name]


@dataclass(frozen=True)
class GroundContact:
    """The declared ground-contact law of include/nmpc_torque.h: the plane z = ground_z, Hunt-Crossley normal force
    f_z = stiffness delta max(0, 1 - damping pd_z), regularised Coulomb friction of coefficient mu that is linear below
    slip_velocity, and the torque limit of the step (None: no limit).  The defaults let the 15 kg quadruped stand at
    dt = 0.5 ms; the explicit step needs mu f_z dt / (slip_velocity m_foot) < 2 and stiffness delta damping dt / m_foot < 2.
    The linearly implicit integrator (`BatchedTorqueLayer.set_integrator("implicit")`) holds them up to dt = 2 ms."""
    ground_z: float = 0.0
    stiffness: float = 1e4
    damping: float = 3.0
    mu: float = 0.8
    slip_velocity: float = 0.05
    tau_max: Optional[float] = None

    def cfg(self) -> _lib.NmpcContactCfg:
        return _lib.NmpcContactCfg(float(self.ground_z), float(self.stiffness), float(self.damping), float(self.mu),
                                   float(self.slip_velocity), 0.0 if self.tau_max is None else float(self.tau_max))


TABLES = ("grounds", "payloads", "actuators", "delays", "noise")      # per name: layer._<name> is what is attached or None, layer.set_<name>(None) detaches


def _draw(rng, n: int, name: str, r) -> np.ndarray:
    """n uniform draws of rng from the range r = (lo, hi) of column `name`, rounded to float32 and held to the float32 values
    inside [lo, hi]: one rng.uniform(lo, hi, n)"""
    lo, hi = (float(x) for x in r)
    if not lo <= hi:
        raise ValueError(f"{name}: need a range (lo, hi) with lo <= hi, got {r!r}")
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if lo32 < lo:
        lo32 = np.nextafter(lo32, np.float32(np.inf))
    if hi32 > hi:
        hi32 = np.nextafter(hi32, np.float32(-np.inf))
    if lo32 > hi32:
        raise ValueError(f"{name}: the range {r!r} holds no float32 value")
    return np.clip(rng.uniform(lo, hi, n).astype(np.float32), lo32, hi32)


def _float_table(name: str, table, width: int, B: int, rules, need=None, expected=None, one_for_all: bool = False) -> np.ndarray:
    """`table` as contiguous float32 rows [>= B, width] (one_for_all: a single row [width] stands for B of them), or the ValueError
    of the table `name`: `need` where it is no float array, `expected` where its shape is wrong, and the first of `rules`
    -- (message, rows -> mask of the rows that break it) -- that a row breaks, with the first such row"""
    try:
        rows = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name}: need {need or f'a float array [B, {width}]'}") from e
    if one_for_all and rows.shape == (width,):
        rows = np.broadcast_to(rows, (B, width))
    if rows.ndim != 2 or rows.shape[1] != width or rows.shape[0] < B:
        raise ValueError(f"{name}: expected {expected or f'[>= {B}, {width}]'}, got {tuple(rows.shape)}")
    for why, broken in rules:
        bad = broken(rows)
        if bad.any():
            raise ValueError(f"{name}: row {int(np.argmax(bad))}: {why}")
    return rows


GROUND_COLUMNS = ("ground_z", "stiffness", "damping", "mu", "slip_velocity", "tau_max")      # a row of a table of grounds: nmpc_contact_cfg's fields


def ground_table(grounds) -> np.ndarray:
    """Host input of `BatchedTorqueLayer.set_grounds` as a validated float32 [B, 6] array in the order of GROUND_COLUMNS: a
    sequence of `GroundContact` (tau_max None -> 0, no limit) or an array [B, 6].  The rules are those a single ground is
    refused by (contact_cfg_refusal of the library): every value finite, stiffness, damping and mu not negative,
    slip_velocity positive; a violation, a wrong shape or an empty table is a ValueError naming the first offending row."""
    if isinstance(grounds, (list, tuple)) and grounds and all(isinstance(g, GroundContact) for g in grounds):
        grounds = [[g.ground_z, g.stiffness, g.damping, g.mu, g.slip_velocity, 0.0 if g.tau_max is None else g.tau_max] for g in grounds]
    w = len(GROUND_COLUMNS)
    rules = (("the contact parameters must be finite", lambda r: ~np.isfinite(r).all(axis=1)),
             ("stiffness, damping and mu must not be negative", lambda r: (r[:, 1:4] < 0.0).any(axis=1)),
             ("slip_velocity must be positive", lambda r: ~(r[:, 4] > 0.0)))
    return _float_table("grounds", grounds, w, 1, rules, need=f"a sequence of GroundContact or a float array [B, {w}]",
                        expected=f"[B, {w}] with B >= 1")


def sample_grounds(B: int, rng, base: GroundContact = GroundContact(), mu=None, stiffness=None, damping=None, ground_z=None,
                   tau_max=None) -> np.ndarray:
    """A table of grounds for `BatchedTorqueLayer.set_grounds`: float32 [B, 6] in the order of GROUND_COLUMNS.  Each keyword is a
    range (lo, hi) drawn uniformly per robot from rng (a numpy Generator), or None to keep base's value in that column;
    slip_velocity is always base's.  Deterministic in rng: the columns are drawn in the order of GROUND_COLUMNS, B values each,
    and a column that is not drawn takes nothing from rng."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be at least 1")
    rows = np.repeat(ground_table([base]), B, axis=0)
    ranges = dict(ground_z=ground_z, stiffness=stiffness, damping=damping, mu=mu, tau_max=tau_max)
    for col, name in enumerate(GROUND_COLUMNS):
        if ranges.get(name) is not None:
            rows[:, col] = _draw(rng, B, name, ranges[name])
    return ground_table(rows)


PAYLOAD_COLUMNS = ("mass", "r_x", "r_y", "r_z")            # a row of a table of payloads: a point mass m_p at r in the frame of one body


def payload_table(payloads, B: int = 1) -> np.ndarray:
    """Host input of `BatchedTorqueLayer.set_payloads` as a validated float32 array [>= B, 4] in the order of PAYLOAD_COLUMNS:
    every value finite and the mass not negative; a violation, a wrong shape or fewer than B rows is a ValueError naming the
    first offending row."""
    rules = (("the payload must be finite", lambda r: ~np.isfinite(r).all(axis=1)), ("the mass must not be negative", lambda r: ~(r[:, 0] >= 0.0)))
    return _float_table("payloads", payloads, len(PAYLOAD_COLUMNS), max(int(B), 1), rules)


def sample_payloads(n: int, seed: int, mass=(0.0, 5.0), offset=((-0.1, 0.1), (-0.05, 0.05), (0.0, 0.1))) -> np.ndarray:
    """A table of payloads for `BatchedTorqueLayer.set_payloads`: float32 [n, 4], the mass drawn uniformly from `mass` (lo, hi) in
    kg and the position from the box `offset` ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)) in metres of the body frame.
    Deterministic in `seed`: the four columns are drawn in the order of PAYLOAD_COLUMNS, n values each."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    ranges = [tuple(float(x) for x in mass)] + [tuple(float(x) for x in side) for side in offset]
    if len(ranges) != 4 or any(len(r) != 2 for r in ranges):
        raise ValueError("need mass = (lo, hi) and offset = ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi))")
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 4), np.float32)
    for col, (name, r) in enumerate(zip(PAYLOAD_COLUMNS, ranges)):
        rows[:, col] = _draw(rng, n, name, r)
    return payload_table(rows, n)


ACTUATOR_COLUMNS = ("kp", "kd", "damping", "armature")     # a row of a table of actuators: the gains, the joint damping, the rotor inertia


def actuator_table(actuators, B: int = 1) -> np.ndarray:
    """Host input of `BatchedTorqueLayer.set_actuators` as a validated float32 array [>= B, 4] in the order of ACTUATOR_COLUMNS:
    every value finite, kp positive, and kd, damping and armature not negative; a violation, a wrong shape or fewer than B rows
    is a ValueError naming the first offending row."""
    rules = (("the actuator must be finite", lambda r: ~np.isfinite(r).all(axis=1)), ("kp must be positive", lambda r: ~(r[:, 0] > 0.0)),
             ("kd must not be negative", lambda r: ~(r[:, 1] >= 0.0)), ("damping must not be negative", lambda r: ~(r[:, 2] >= 0.0)),
             ("armature must not be negative", lambda r: ~(r[:, 3] >= 0.0)))
    return _float_table("actuators", actuators, len(ACTUATOR_COLUMNS), max(int(B), 1), rules)


def sample_actuators(n: int, seed: int, kp=(0.5 * KP, 1.5 * KP), kd=(0.5 * KD, 1.5 * KD), damping=(0.0, 0.2), armature=(0.0, 0.02)) -> np.ndarray:
    """A table of actuators for `BatchedTorqueLayer.set_actuators`: float32 [n, 4], each column drawn uniformly from its range
    (lo, hi) -- kp in N m/rad and kd in N m s/rad, by default within half of the nominal KP, KD on either side, the passive
    damping in N m s/rad, the rotor inertia in kg m^2.  Row 0 is the nominal actuator (KP, KD, 0, 0) whatever the ranges.
    Deterministic in `seed`: the four columns are drawn in the order of ACTUATOR_COLUMNS, n values each."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    ranges = [tuple(float(x) for x in r) for r in (kp, kd, damping, armature)]
    if any(len(r) != 2 for r in ranges):
        raise ValueError("need kp, kd, damping and armature as ranges (lo, hi)")
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 4), np.float32)
    for col, (name, r) in enumerate(zip(ACTUATOR_COLUMNS, ranges)):
        rows[:, col] = _draw(rng, n, name, r)
    rows[0] = (KP, KD, 0.0, 0.0)
    return actuator_table(rows, n)


DELAY_MAX_DEPTH = _lib.NMPC_DELAY_MAX_DEPTH                # the deepest shift register of a delay line, and so the largest delay


def delay_table(delays, B: int = 1) -> np.ndarray:
    """Host input of `BatchedTorqueLayer.set_delays` as a validated int32 array [>= B]: the control steps every robot lags by,
    integers with 0 <= d <= DELAY_MAX_DEPTH; a violation, a wrong shape or fewer than B entries is a ValueError naming the first
    offending row."""
    try:
        rows = np.asarray(delays)
    except (TypeError, ValueError) as e:
        raise ValueError("delays: need an integer array [B]") from e
    if rows.dtype.kind not in "iu":
        raise ValueError(f"delays: need integers (control steps), got {rows.dtype}")
    B = max(int(B), 1)
    if rows.ndim != 1 or rows.shape[0] < B:
        raise ValueError(f"delays: expected [>= {B}], got {tuple(rows.shape)}")
    bad = (rows < 0) | (rows > DELAY_MAX_DEPTH)
    if bad.any():
        raise ValueError(f"delays: row {int(np.argmax(bad))}: the delay must be in [0, {DELAY_MAX_DEPTH}] control steps")
    return np.ascontiguousarray(rows.astype(np.int32))


def sample_delays(n: int, seed: int, steps=(0, 2)) -> np.ndarray:
    """A table of delays for `BatchedTorqueLayer.set_delays`: int32 [n], each drawn uniformly from the integers lo .. hi of
    `steps` (both ends included), in control steps of the call that runs on it.  Row 0 has no delay whatever the range.
    Deterministic in `seed`."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    try:
        lo, hi = steps
    except (TypeError, ValueError) as e:
        raise ValueError("need steps as a range (lo, hi)") from e
    if any(not isinstance(x, (int, np.integer)) for x in (lo, hi)):
        raise ValueError(f"steps: need integers, got {steps!r}")
    if not lo <= hi:
        raise ValueError(f"steps: need a range (lo, hi) with lo <= hi, got {steps!r}")
    if lo < 0 or hi > DELAY_MAX_DEPTH:
        raise ValueError(f"steps: a delay must be in [0, {DELAY_MAX_DEPTH}] control steps, got {steps!r}")
    rows =np.random.default_rng(seed).integers(int(lo), int(hi) + 1, n)
    rows[0] = 0
    return delay_table(rows, n)


# the slots of the 44-slot state row by what measures them; slot 0, the phase, is the controller's own clock and has no sensor
NOISE_GROUPS = {"v_lin": slice(1, 4), "body_rates": slice(4, 7), "joint_rates": slice(7, 19), "z": slice(19, 20),
                "quaternion": slice(20, 24), "joints": slice(24, 36), "base_wrt_feet": slice(36, 44)}
# the default ceilings of `sample_noise` [decl]: declared values in the units of the raw row (m/s, rad/s, rad/s, m, 1, rad, m), the
# order of magnitude of a legged robot's estimator, IMU and encoders -- not the reference's, which runs its policies on the true state
NOISE_SIGMA_MAX = {"v_lin": 0.1, "body_rates": 0.05, "joint_rates": 0.5, "z": 0.01, "quaternion": 0.01, "joints": 0.01, "base_wrt_feet": 0.01}
NOISE_BIAS_MAX = {"v_lin": 0.05, "body_rates": 0.01, "joint_rates": 0.0, "z": 0.01, "quaternion": 0.005, "joints": 0.01, "base_wrt_feet": 0.005}


def noise_table(sigma, bias=None, B: int = 1) -> np.ndarray:
    """Host input of `BatchedTorqueLayer.set_noise` as a validated float32 array [>= B, 88]: row b is sigma[44], then bias[44], of
    robot b in the units of the raw 44-slot state row.  sigma, bias: [44], the same for all B robots, or [>= B, 44]; bias None:
    zeros.  sigma must be finite and not negative, bias finite; a violation, a wrong shape or fewer than B rows is a ValueError
    naming the first offending row."""
    B = max(int(B), 1)
    sigma, bias = (_float_table(f"noise: {name}", x, N_STATE, B, (), need=f"a float array [{N_STATE}] or [B, {N_STATE}]",
                                expected=f"[{N_STATE}] or [>= {B}, {N_STATE}]", one_for_all=True)
                   for name, x in (("sigma", sigma), ("bias", np.zeros(N_STATE, np.float32) if bias is None else bias)))
    n = min(sigma.shape[0], bias.shape[0])                # one may have been broadcast to B, the other given longer
    return _noise_rows(np.concatenate([sigma[:n], bias[:n]], axis=1))


def _noise_rows(table) -> np.ndarray:
    """a host table [B, 88] as `set_noise` is given it, through the rules of `noise_table`"""
    rules = (("sigma must be finite", lambda r: ~np.isfinite(r[:, :N_STATE]).all(axis=1)),
             ("sigma must not be negative", lambda r: ~(r[:, :N_STATE] >= 0.0).all(axis=1)),
             ("bias must be finite", lambda r: ~np.isfinite(r[:, N_STATE:]).all(axis=1)))
    return _float_table("noise", table, 2 * N_STATE, 1, rules)


def sample_noise(n: int, seed: int, sigma=None, bias=None) -> np.ndarray:
    """A table of sensor noise for `BatchedTorqueLayer.set_noise`: float32 [n, 88].  Per robot and group of NOISE_GROUPS one
    standard deviation, drawn uniformly from [0, ceiling of the group] and given to every slot of the group, and per robot and
    slot a bias drawn uniformly from [-ceiling, +ceiling] of its group.  sigma, bias: dicts of ceilings by group name that
    replace the defaults NOISE_SIGMA_MAX, NOISE_BIAS_MAX [decl] group by group (None: the defaults).  The phase, slot 0, is
    always exact, and row 0 is all zero whatever the ceilings: the robot with ideal sensors.  Deterministic in `seed`: the
    groups are drawn in the order of NOISE_GROUPS, sigma then bias."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    tops = []
    for name, given, default in (("sigma", sigma, NOISE_SIGMA_MAX), ("bias", bias, NOISE_BIAS_MAX)):
        given = {} if given is None else dict(given)
        unknown = sorted(set(given) - set(NOISE_GROUPS))
        if unknown:
            raise ValueError(f"{name}: unknown groups {unknown}, expected some of {list(NOISE_GROUPS)}")
        top = {g: float(given.get(g, default[g])) for g in NOISE_GROUPS}
        for g, hi in top.items():
            if not (np.isfinite(hi) and hi >= 0.0):
                raise ValueError(f"{name}: the ceiling of {g} must be finite and not negative, got {hi!r}")
        tops.append(top)
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 2 * N_STATE), np.float32)
    for g, slots in NOISE_GROUPS.items():
        width = slots.stop - slots.start
        for half, hi, draw in ((0, tops[0][g], rng.uniform(0.0, tops[0][g], (n, 1))), (1, tops[1][g], rng.uniform(-tops[1][g], tops[1][g], (n, width)))):
            hi32 = np.float32(hi)                         # the largest float32 inside the ceiling: a rounded draw is held to it
            if hi32 > hi:
                hi32 = np.nextafter(hi32, np.float32(-np.inf))
            rows[:, half * N_STATE + slots.start:half * N_STATE + slots.stop] = np.clip(draw.astype(np.float32), 0.0 if half == 0 else -hi32, hi32)
    rows[0] = 0.0
    return _noise_rows(rows)


def training_sigma(noise) -> np.ndarray:
    """The input noise a memoryless learner is trained with under a table of sensor noise: float32 [44] for
    `DevicePolicy.set_input_noise` / `learning.train_network(input_noise=...)` from a table [B, 88] as `set_noise` takes it
    (`noise_table`, `sample_noise`).  Per slot the root mean square over the robots of sqrt(sigma^2 + bias^2) [decl]: a policy
    without memory cannot tell a robot's constant bias from noise, so over the population the bias enters as variance -- the one
    declared way a per-robot bias enters the training noise; a persistent bias per episode is not drawn in training."""
    rows = _noise_rows(noise).astype(np.float64)
    sigma, bias = rows[:, :N_STATE], rows[:, N_STATE:]
    return np.sqrt((sigma ** 2 + bias ** 2).mean(axis=0)).astype(np.float32)


HISTORY_MAX = _lib.NMPC_HISTORY_MAX                        # the deepest history of observed rows, and of issued targets, on the policy input


def history_width(n_obs: int, n_act: int, nu: int = 12) -> int:
    """n_wide = 44 n_obs + 12 n_act: the width of the row a policy with a history is shown (`BatchedTorqueLayer.set_history`), and
    the state width of the database that stores such rows"""
    return N_STATE * int(n_obs) + int(nu) * int(n_act)


class BatchedTorqueLayer:
    def __init__(self, parent: Sequence[int], joint_type: Sequence[int], axis, placement_R, placement_p, mass, com, inertia,
                 foot_joint: Sequence[int], foot_offset, n_actuated: int, gravity=(0.0, 0.0, -9.81), device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedTorqueLayer needs a HIP device: there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device(device)
        n, nf = len(parent), len(foot_joint)
        f32 = lambda x, shape: np.ascontiguousarray(np.asarray(x, np.float32).reshape(shape))   # noqa: E731
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))                            # noqa: E731
        placement = np.concatenate([f32(placement_R, (n, 9)), f32(placement_p, (n, 3))], axis=1)
        arrays = dict(parent=i32(parent), type=i32(joint_type), axis=f32(axis, (n, 3)), placement=np.ascontiguousarray(placement),
                      mass=f32(mass, (n,)), com=f32(com, (n, 3)), inertia=f32(inertia, (n, 6)),
                      foot_joint=i32(foot_joint), foot_offset=f32(foot_offset, (nf, 3)))
        m = _lib.NmpcTreeModel()
        m.n_joints, m.n_actuated, m.n_feet = n, int(n_actuated), nf
        for k, a in arrays.items():
            setattr(m, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int if a.dtype == np.int32 else ctypes.c_float)))
        m.gravity = (ctypes.c_float * 3)(*[float(g) for g in gravity])
        self._h = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.nmpc_torque_create(ctypes.byref(m), idx, ctypes.byref(self._h)), None, "nmpc_torque_create", "torque")
        self.n, self.nu, self.n_feet = n, int(n_actuated), nf
        self.tree_mass = 0.0            # the total mass as the library sums it (float32, in joint order): the m_tree of the articulated model
        for m_i in arrays["mass"]:
            self.tree_mass = float(np.float32(np.float32(self.tree_mass) + m_i))
        self._states = None             # set_rollout_states: the attached (Q, V)
        self._push = None               # set_push: the attached force
        self._push_windows = None       # set_push with arrays: the attached (first substeps, counts)
        self._grounds = None            # set_grounds: the attached table
        self._payloads = None           # set_payloads: the attached table
        self._actuators = None          # set_actuators: the attached table
        self._delays = None             # set_delays: the attached table with its register and scratch
        self._noise = None              # set_noise: the attached table
        self._observed = None           # set_rollout_observed: the attached rows O
        self._history = None            # set_history: the attached registers, their depths and the wide rows W of set_rollout_wide

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.nmpc_torque_destroy(h)

    def _in(self, t, width, name):
        t = torch.as_tensor(t, dtype=torch.float32, device=self.device).contiguous()
        if t.dim() < 2 or tuple(t.shape[1:]) != tuple(width):
            raise ValueError(f"{name}: expected [B, {', '.join(map(str, width))}], got {tuple(t.shape)}")
        return t

    def _opt(self, t, width, name):
        return None if t is None else self._in(t, width, name)

    @staticmethod
    def _batch(*tensors):
        """the B that all given tensors share"""
        B = tensors[0].shape[0]
        if any(x is not None and x.shape[0] != B for x in tensors):
            raise ValueError("batch sizes differ")
        return B

    def _perm(self, actuator_to_joint):
        if actuator_to_joint is None:
            return None
        perm = torch.as_tensor(list(actuator_to_joint), dtype=torch.int32, device=self.device)
        if perm.numel() != self.nu or sorted(perm.tolist()) != list(range(self.nu)):
            raise ValueError("actuator_to_joint must be a permutation of range(nu)")
        return perm

    def _flags(self, x, like, name):
        """x, an int32 vector with one entry per row of `like` and on its device, or None"""
        B = like.shape[0]
        if x is not None and (x.dtype != torch.int32 or tuple(x.shape) != (B,) or not x.is_contiguous() or x.device != like.device):
            raise ValueError(f"{name}: need contiguous int32 ({B},) on {self.device}")
        return x

    def id_torques(self, q_plan, v_plan, a_plan, f_plan=None) -> torch.Tensor:
        """dynamics.py:136-163 per robot: q, v, a [B, n]; f [B, n_feet, 3] world-frame contact forces -> [B, nu]."""
        q = self._in(q_plan, (self.n,), "q_plan"); v = self._in(v_plan, (self.n,), "v_plan"); a = self._in(a_plan, (self.n,), "a_plan")
        f = self._opt(f_plan, (self.n_feet, 3), "f_plan")
        B = self._batch(q, v, a, f)
        tau = torch.empty(B, self.nu, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_id_torques_batch(self._h, B, ptr(q), ptr(v), ptr(a), ptr(f), ptr(tau), stream(self.device)),
                   self._h, "nmpc_id_torques_batch", "torque")
        return tau

    def forward_dynamics(self, q, v, tau=None, f=None) -> torch.Tensor:
        """nmpc_fd_accel_batch, the inverse of `id_torques`: q, v [B, n]; tau [B, nu] on the last nu joints (None = zero);
        f [B, n_feet, 3] world-frame contact forces (None = none) -> the accelerations [B, n]."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        tau = self._opt(tau, (self.nu,), "tau"); f = self._opt(f, (self.n_feet, 3), "f")
        B = self._batch(q, v, tau, f)
        a = torch.empty(B, self.n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_fd_accel_batch(self._h, B, ptr(q), ptr(v), ptr(tau), ptr(f), ptr(a), stream(self.device)),
                   self._h, "nmpc_fd_accel_batch", "torque")
        return a

    def step(self, q, v, dt: float, n_sub: int = 1, tau_ff=None, q_des=None, kp: float = KP, kd: float = KD, f=None):
        """nmpc_fd_step_batch: n_sub semi-implicit Euler substeps of length dt under constant f with
        tau = tau_ff + kp (q_des - q_j) - kd v_j re-evaluated every substep (q_des [B, nu]: a recorded action in joint
        order; None: tau = tau_ff; tau_ff None = zero) -> (q, v, a of the last substep), new tensors [B, n]."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        tau_ff = self._opt(tau_ff, (self.nu,), "tau_ff"); q_des = self._opt(q_des, (self.nu,), "q_des")
        f = self._opt(f, (self.n_feet, 3), "f")
        B = self._batch(q, v, tau_ff, q_des, f)
        q_out, v_out, a_out = (torch.empty(B, self.n, dtype=torch.float32, device=self.device) for _ in range(3))
        _lib.check(self.lib.nmpc_fd_step_batch(self._h, B, int(n_sub), float(dt), ptr(q), ptr(v), ptr(tau_ff), ptr(q_des), float(kp),
                                               float(kd), ptr(f), ptr(q_out), ptr(v_out), ptr(a_out), stream(self.device)),
                   self._h, "nmpc_fd_step_batch", "torque")
        return q_out, v_out, a_out

    def mass_matrix(self, q) -> torch.Tensor:
        """nmpc_mass_matrix_batch: q [B, n] -> the joint-space mass matrix M(q) [B, n, n] of the tree, symmetric bit for bit, with
        exact zeros between joints that are not on one path to the root."""
        q = self._in(q, (self.n,), "q")
        B = self._batch(q)
        M = torch.empty(B, self.n, self.n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_mass_matrix_batch(self._h, B, ptr(q), ptr(M), stream(self.device)), self._h, "nmpc_mass_matrix_batch", "torque")
        return M

    def centroidal(self, q, v=None, jacobian: bool = False):
        """nmpc_centroidal_batch: q [B, n], v [B, n] or None -> (com [B, 3], the world position of the tree's centre of mass;
        h [B, 6] = [linear; angular about com] in world axes, the centroidal momentum of the articulated tree, None without v)
        and, with jacobian=True, a third entry Ag [B, 6, n], the centroidal momentum map: h = Ag v."""
        q = self._in(q, (self.n,), "q")
        v = self._opt(v, (self.n,), "v")
        B = self._batch(q, v)
        com = torch.empty(B, 3, dtype=torch.float32, device=self.device)
        h = None if v is None else torch.empty(B, 6, dtype=torch.float32, device=self.device)
        Ag = torch.empty(B, 6, self.n, dtype=torch.float32, device=self.device) if jacobian else None
        _lib.check(self.lib.nmpc_centroidal_batch(self._h, B, ptr(q), ptr(v), ptr(com), ptr(h), ptr(Ag), stream(self.device)),
                   self._h, "nmpc_centroidal_batch", "torque")
        return (com, h, Ag) if jacobian else (com, h)

    def state_momentum(self, q, v, out=None, skip=None, skip_mask: int = 0):
        """nmpc_state_momentum_batch: q, v [B, n] plant states -> h [B, 6] = [linear; angular about com] in world axes, `centroidal`'s
        h from the outward pass alone (to fp32 rounding, not bit for bit), which is what the device rollouts put into x0
        (`BatchedNmpcSolver.set_state_momentum`).  q, v may be views whose rows are a common stride >= n apart; out: a float32
        view [B, 6] to write into (row stride >= 6, last axis dense), otherwise a new tensor; skip int32 [B]: a row with
        skip[b] & skip_mask != 0 is neither read nor written."""
        def strided(t, width, like):
            """t as it is if it is a float32 view [B, width] on `like`'s device with a dense last axis and rows >= width apart"""
            return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width and t.stride(1) == 1
                    and (t.shape[0] < 2 or t.stride(0) >= width) and (like is None or t.device == like.device))
        if not (strided(q, self.n, None) and strided(v, self.n, q) and q.stride(0) == v.stride(0) and q.device.type == self.device.type):
            q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")      # anything else: dense rows
        B = self._batch(q, v)
        if out is None:
            out = torch.empty(B, 6, dtype=torch.float32, device=q.device)
        if not strided(out, 6, q) or out.shape[0] != B:
            raise ValueError(f"out: need a float32 view [{B}, 6] on {q.device} with a dense last axis and rows at least 6 apart")
        self._flags(skip, q, "skip")
        stride = lambda t, width: max(t.stride(0), width)      # noqa: E731  (the stride of a single row is arbitrary)
        _lib.check(self.lib.nmpc_state_momentum_batch(self._h, B, ptr(q), ptr(v), stride(q, self.n), ptr(out), stride(out, 6), None, 0,
                                                      ptr(skip), int(skip_mask), stream(self.device)),
                   self._h, "nmpc_state_momentum_batch", "torque")
        return out

    def centroidal_derivatives(self, q, v, com_jacobian: bool = False, bias: bool = False):
        """nmpc_centroidal_derivatives_batch: q, v [B, n] -> dh_dq [B, 6, n], the derivative of `centroidal`'s h = Ag(q) v with
        respect to q at fixed v (rows in the slot order of h); with com_jacobian=True also dcom_dq [B, 3, n]; with bias=True also
        hdot_bias [B, 6] = dh_dq v, the part of h_dot that is not Ag a.  A tensor alone, or a tuple in that order."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        B = self._batch(q, v)
        new = lambda *shape: torch.empty(B, *shape, dtype=torch.float32, device=self.device)      # noqa: E731
        dh, dcom, hdot = new(6, self.n), (new(3, self.n) if com_jacobian else None), (new(6) if bias else None)
        _lib.check(self.lib.nmpc_centroidal_derivatives_batch(self._h, B, ptr(q), ptr(v), ptr(dh), ptr(dcom), ptr(hdot), stream(self.device)),
                   self._h, "nmpc_centroidal_derivatives_batch", "torque")
        out = tuple(x for x in (dh, dcom, hdot) if x is not None)
        return out[0] if len(out) == 1 else out

    def foot_kinematics(self, q, v=None):
        """nmpc_foot_kinematics_batch: q, v [B, n] (v None = at rest) -> world position and velocity of every foot point,
        (pos, vel), each [B, n_feet, 3]."""
        q = self._in(q, (self.n,), "q")
        v = self._opt(v, (self.n,), "v")
        B = self._batch(q, v)
        pos, vel = (torch.empty(B, self.n_feet, 3, dtype=torch.float32, device=self.device) for _ in range(2))
        _lib.check(self.lib.nmpc_foot_kinematics_batch(self._h, B, ptr(q), ptr(v), ptr(pos), ptr(vel), stream(self.device)),
                   self._h, "nmpc_foot_kinematics_batch", "torque")
        return pos, vel

    def contact_forces(self, q, v, ground: GroundContact) -> torch.Tensor:
        """nmpc_contact_forces_batch: the ground-contact law on the foot kinematics of q, v [B, n] (v None = at rest) ->
        f [B, n_feet, 3], the world-frame forces `forward_dynamics` would have to be handed."""
        q = self._in(q, (self.n,), "q")
        v = self._opt(v, (self.n,), "v")
        B = self._batch(q, v)
        f = torch.empty(B, self.n_feet, 3, dtype=torch.float32, device=self.device)
        cfg = ground.cfg()
        _lib.check(self.lib.nmpc_contact_forces_batch(self._h, B, ctypes.byref(cfg), ptr(q), ptr(v), ptr(f), stream(self.device)),
                   self._h, "nmpc_contact_forces_batch", "torque")
        return f

    def contact_step(self, q, v, dt: float, n_sub: int = 1, tau_ff=None, q_des=None, kp: float = KP, kd: float = KD,
                     ground: GroundContact = GroundContact()):
        """nmpc_contact_step_batch: `step` on the ground -- the contact forces of `ground` re-evaluated from (q, v) in every
        substep, the PD torque clamped to ground.tau_max -> (q, v, a, f, tau): the new state [B, n], and the acceleration
        [B, n], foot forces [B, n_feet, 3] and clamped torques [B, nu] of the last substep.  The substeps are those of the
        layer's integrator (`set_integrator`)."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        tau_ff = self._opt(tau_ff, (self.nu,), "tau_ff"); q_des = self._opt(q_des, (self.nu,), "q_des")
        B = self._batch(q, v, tau_ff, q_des)
        q_out, v_out, a_out = (torch.empty(B, self.n, dtype=torch.float32, device=self.device) for _ in range(3))
        f_out = torch.empty(B, self.n_feet, 3, dtype=torch.float32, device=self.device)
        tau_out = torch.empty(B, self.nu, dtype=torch.float32, device=self.device)
        cfg = ground.cfg()
        _lib.check(self.lib.nmpc_contact_step_batch(self._h, B, int(n_sub), float(dt), ctypes.byref(cfg), ptr(q), ptr(v), ptr(tau_ff),
                                                    ptr(q_des), float(kp), float(kd), ptr(q_out), ptr(v_out), ptr(a_out), ptr(f_out),
                                                    ptr(tau_out), stream(self.device)), self._h, "nmpc_contact_step_batch", "torque")
        return q_out, v_out, a_out, f_out, tau_out

    def _stats(self, s_mean, s_std, width: int = N_STATE):
        """the column statistics of the state rows as float64 device vectors [width], or (None, None)"""
        if (s_mean is None) != (s_std is None):
            raise ValueError("s_mean and s_std come together or not at all")
        if s_mean is None:
            return None, None
        out = [torch.as_tensor(x, dtype=torch.float64, device=self.device).contiguous() for x in (s_mean, s_std)]
        if any(tuple(x.shape) != (width,) for x in out):
            raise ValueError(f"s_mean, s_std: expected [{width}]")
        return out

    def _goal(self, goal, B):
        goal = torch.as_tensor(goal, dtype=torch.float32, device=self.device).contiguous()
        if goal.dim() != 2 or goal.shape[0] != B:
            raise ValueError(f"goal: expected [{B}, n_goal], got {tuple(goal.shape)}")
        return goal

    def observe(self, q, v, t: float, period: float, goal, s_mean=None, s_std=None, s_first: int = 1,
                collision_height: float = 0.08, failed: Optional[torch.Tensor] = None, step_index: int = 0, term_mask: int = 0):
        """nmpc_observe_batch: the plant state q, v [B, 18] (Euler layout) at time t as the reference's 44-slot state row
        (phase over `period`, base_wrt_feet from the tree's own feet) and the policy input [row, goal] with columns
        [s_first, 44) normalised by s_mean, s_std (float64 [44]; None: raw), as `DeviceDatabase.batch` assembles it.  failed:
        int32 [B] on the device, updated in place with the flags the state raises and, where a bit of term_mask is set and
        no stamp is present, the stamp step_index + 1 (None: nothing is written).  With a table of noise attached (`set_noise`) X
        is what the sensors of robot b show -- `observe_noise` at `noise_step`, which then moves on by one; S_row and failed are
        those of the true state.  -> (S_row [B, 44], X [B, 44 + n_goal])."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        B = self._batch(q, v)
        goal = self._goal(goal, B)
        s_mean, s_std = self._stats(s_mean, s_std)
        failed = self._flags(failed, q, "failed")
        S = torch.empty(B, N_STATE, dtype=torch.float32, device=self.device)
        X = torch.empty(B, N_STATE + goal.shape[1], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_observe_batch(self._h, B, ptr(q), ptr(v), float(t), float(period), ptr(goal), goal.shape[1], ptr(s_mean),
                                               ptr(s_std), int(s_first), float(collision_height), ptr(S), N_STATE, ptr(X), ptr(failed),
                                               int(step_index), int(term_mask), stream(self.device)),
                   self._h, "nmpc_observe_batch", "torque")
        return S, X

    def policy_rollout(self, policy, q, v, n_steps: int, dt: float, n_sub: int, goal, tau_ff=None, kp: float = KP, kd: float = KD,
                       ground: GroundContact = GroundContact(), t0: float = 0.0, period: float = NOMINAL_PERIOD, db=None,
                       s_mean=None, s_std=None, terminate_mask: int = TERMINATE_DEFAULT, collision_height: float = 0.08,
                       record: bool = True):
        """nmpc_policy_rollout_batch: n_steps control steps of `observe` -> `policy.forward` -> `contact_step` (n_sub substeps
        of dt, q_des = the action) in one library call, and a last flags-only observation; bit for bit that chain of calls
        with observation k at t0 + (k n_sub) float32(dt) and step index k.  policy: a `DevicePolicy` of 44 + n_goal inputs
        and 12 outputs with batch_max >= B; goal [B, n_goal]; tau_ff [B, 12] a constant feed-forward torque.  The policy
        input is normalised with the statistics of db (a `DeviceDatabase` whose norm_input is set: its states_mean /
        states_std from column 1 on, what its `batch_source()` hands the trainer for velocity goals; the goal is always fed
        raw, so a database that normalises its goals -- goal_type 'cc' with norm_input -- and an empty one are refused) or
        with s_mean, s_std given directly (from column 1 on).  One rollout per layer at a time: the dense actions of a step
        live in a buffer of the layer's handle, which grows (and then synchronises the device) for a larger batch.  Nothing is frozen: a robot whose flags hit terminate_mask is stamped in failed
        (failed >> 8 = 1 + the control step whose observation saw it) and keeps being stepped.
        The contact steps are those of the layer's integrator (`set_integrator`).  With a table of noise attached (`set_noise`)
        the policy acts on the perturbed input of each of its n_steps observations and `noise_step` moves on by n_steps; S holds
        the true rows, and the rows the sensors showed go to the tensor of `set_rollout_observed` if one is attached.
        With a history attached (`set_history`) the policy has n_wide + n_goal inputs and is shown the wide row of every step,
        normalised with the statistics of a db whose state width is n_wide (or s_mean, s_std [n_wide]); the raw wide rows go to the
        tensor of `set_rollout_wide` if one is attached, and both registers move on by n_steps.
        -> (q, v, S [B, n_steps, 44], A [B, n_steps, 12], failed int32 [B]); S and A are None with record=False."""
        q = self._in(q, (self.n,), "q").clone(); v = self._in(v, (self.n,), "v").clone()
        tau_ff = self._opt(tau_ff, (self.nu,), "tau_ff")
        B = self._batch(q, v, tau_ff)
        goal = self._goal(goal, B)
        if db is not None:
            if s_mean is not None or s_std is not None:
                raise ValueError("give db or s_mean / s_std, not both")
            if db.norm_input:
                if db.goal_type != "vc":
                    raise ValueError("a database that normalises its goals (goal_type 'cc' with norm_input) is not supported: the goal is fed raw")
                if db.states_mean is None:
                    raise ValueError("the database is empty: it has no statistics to normalise with")
                s_mean, s_std = db.states_mean, db.states_std
        hs = self._history
        n_in = N_STATE if hs is None else hs.n_wide      # the width of the row the policy is shown, and of its statistics
        s_mean, s_std = self._stats(s_mean, s_std, n_in)
        n_steps, n_goal = int(n_steps), goal.shape[1]
        if hs is not None and hs.W is not None and (hs.W.shape[0] != B or hs.W.shape[1] < n_steps):
            raise ValueError(f"W (set_rollout_wide): need [{B}, >= {n_steps}, {hs.n_wide}], got {tuple(hs.W.shape)}")
        states = self._states
        if states is not None and (states[0].shape[0] != B or states[0].shape[1] < n_steps):      # the attached tables must be this rollout's size
            raise ValueError(f"Q, V (set_rollout_states): need [{B}, >= {n_steps}, {self.n}], got {tuple(states[0].shape)}")
        seen = self._observed
        if seen is not None and (seen.shape[0] != B or seen.shape[1] < n_steps):
            raise ValueError(f"O (set_rollout_observed): need [{B}, >= {n_steps}, {N_STATE}], got {tuple(seen.shape)}")
        rows = max(n_steps, 0)
        S = torch.empty(B, rows, N_STATE, dtype=torch.float32, device=self.device) if record else None
        A = torch.empty(B, rows, self.nu, dtype=torch.float32, device=self.device) if record else None
        X = torch.empty(B, n_in + n_goal, dtype=torch.float32, device=self.device)
        failed = torch.zeros(B, dtype=torch.int32, device=self.device)
        cfg = _lib.NmpcPolicyRolloutCfg(n_steps, int(n_sub), float(dt), float(kp), float(kd), float(t0), float(period),
                                        float(collision_height), int(terminate_mask), n_goal, 1)
        g = ground.cfg()
        _lib.check(self.lib.nmpc_policy_rollout_batch(self._h, getattr(policy, "_h", None), B, ctypes.byref(cfg), ctypes.byref(g), ptr(q),
                                                      ptr(v), ptr(tau_ff), ptr(goal), ptr(s_mean), ptr(s_std), ptr(S), ptr(A), ptr(X),
                                                      ptr(failed), stream(self.device)),
                   self._h, "nmpc_policy_rollout_batch", "torque")
        return q, v, S, A, failed

    def set_integrator(self, integrator: str):
        """nmpc_contact_set_integrator: how `contact_step`, `contact_track`, `policy_rollout` and the expert on the plant take
        their substeps from now on.  "explicit" (the default): semi-implicit Euler on the explicit contact forces, stable at
        dt = 0.5 ms on the default ground.  "implicit": the linearly implicit step of include/nmpc_torque.h, which takes ground
        stiffness and damping, the friction regulariser and the PD law at the end of the substep and holds at dt = 1 - 2 ms
        (not at 4 ms, and with little gain at slip_velocity = 0.01).  `step`, `forward_dynamics` and `contact_forces` are not
        affected.  An unknown name is a ValueError; the mode that was set stays.  The three plant calls keep the parameter
        lists they had: the integrator is the layer's state, set here or through the `integrator=` keyword of
        `learning.evaluate_policy`, `learning.dagger_iteration` and `open_loop_device(..., plant=...)`."""
        mode = integrator_mode(integrator)
        _lib.check(self.lib.nmpc_contact_set_integrator(self._h, mode), self._h, "nmpc_contact_set_integrator", "torque")

    def set_rollout_states(self, Q: Optional[torch.Tensor] = None, V: Optional[torch.Tensor] = None):
        """nmpc_policy_rollout_set_states: while Q, V [B, rows, 18] (rows >= n_steps; slices [:, :k] of longer tables are taken
        with their stride) are attached, every `policy_rollout` of this layer writes the plant state before control step k into
        row k of both -- the states its rows of S were made of, which `LocomotionMPC.label_states` starts the expert's solves
        from.  Every other output of the rollout is the same bits.  `set_rollout_states(None)` detaches.  The layer keeps the two
        alive while they are attached; a rollout of another batch size than theirs is refused."""
        if Q is None and V is None:
            self._states = None
            _lib.check(self.lib.nmpc_policy_rollout_set_states(self._h, None, None, 0), self._h, "nmpc_policy_rollout_set_states", "torque")
            return
        if Q is None or V is None:
            raise ValueError("Q and V come together or not at all")
        if not isinstance(Q, torch.Tensor) or Q.dim() != 3:
            raise ValueError("Q: need a float32 [B, rows, 18] tensor")
        Q, qv_rows = self._rows(Q, self.n, "Q", Q.shape[0])
        V, v_rows = self._rows(V, self.n, "V", Q.shape[0])
        if V.shape[1] != Q.shape[1] or v_rows != qv_rows:
            raise ValueError("Q, V: need the same rows and one layout")
        self._states = (Q, V)
        _lib.check(self.lib.nmpc_policy_rollout_set_states(self._h, ptr(Q), ptr(V), qv_rows), self._h, "nmpc_policy_rollout_set_states", "torque")

    def set_rollout_observed(self, O: Optional[torch.Tensor] = None):
        """nmpc_policy_rollout_set_observed: while O [B, rows, 44] (rows >= n_steps; a slice [:, :k] of a longer table is taken
        with its stride) is attached, every `policy_rollout` of this layer writes into row k the raw 44-slot state row as the
        sensors of robot b showed it in control step k -- `observed_rows` of row k of S at the noise step that step's policy
        input was drawn at, by one more launch per control step; with no table of noise attached that is S itself.  Every other
        output of the rollout, and `noise_step`, is the same bits.  `set_rollout_observed(None)` detaches.  The layer keeps O alive
        while it is attached; a rollout of another batch size than O's is refused."""
        if O is None:
            self._observed = None
            _lib.check(self.lib.nmpc_policy_rollout_set_observed(self._h, None, 0), self._h, "nmpc_policy_rollout_set_observed", "torque")
            return
        if not isinstance(O, torch.Tensor) or O.dim() != 3:
            raise ValueError(f"O: need a float32 [B, rows, {N_STATE}] tensor")
        O, o_rows = self._rows(O, N_STATE, "O", O.shape[0])
        self._observed = O
        _lib.check(self.lib.nmpc_policy_rollout_set_observed(self._h, ptr(O), o_rows), self._h, "nmpc_policy_rollout_set_observed", "torque")

    def observed_rows(self, S: torch.Tensor, step: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nmpc_observed_rows_batch: the raw state rows S, float32 [B, >= 44] on the layer's device with dense rows, as the sensors
        of the attached table of noise (`set_noise`) show them at noise step `step`: slot j of robot b is float32(S + bias + sigma
        g) with the draw `observe` puts on the policy input at that step, and the bits of S where sigma and bias are zero or no
        table is attached.  The layer's own noise step is neither read nor moved.  out: float32 [B, >= 44] with dense rows to
        write the first 44 columns of (None: a new [B, 44] tensor; S itself: in place).  -> out."""
        def dense(t, name):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < N_STATE or t.device != self.device \
                    or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
                raise ValueError(f"{name}: need a float32 [B, >= {N_STATE}] tensor with dense rows on {self.device}")
            return t.stride(0) if t.shape[0] > 1 else t.shape[1]
        s_stride = dense(S, "S")
        if out is None:
            out = torch.empty(S.shape[0], N_STATE, dtype=torch.float32, device=self.device)
        o_stride = dense(out, "out")
        if out.shape[0] != S.shape[0]:
            raise ValueError("out: need as many rows as S")
        step = int(step)
        if not 0 <= step < 2 ** 63:
            raise ValueError("observed: step must be in [0, 2^63)")
        _lib.check(self.lib.nmpc_observed_rows_batch(self._h, S.shape[0], ptr(S), s_stride, ptr(out), o_stride, step, stream(self.device)),
                   self._h, "nmpc_observed_rows_batch", "torque")
        return out

    @staticmethod
    def _history_depths(n_obs, n_act):
        n_obs, n_act = int(n_obs), int(n_act)
        if not 1 <= n_obs <= HISTORY_MAX:
            raise ValueError(f"history: n_obs must be in [1, {HISTORY_MAX}], got {n_obs}")
        if not 0 <= n_act <= HISTORY_MAX:
            raise ValueError(f"history: n_act must be in [0, {HISTORY_MAX}], got {n_act}")
        return n_obs, n_act

    def _history_registers(self, n_obs, n_act, batch):
        """zeroed registers hist [batch, n_obs, 44] and act [batch, n_act, 12] (None with n_act = 0) with their depths and n_wide"""
        n_obs, n_act = self._history_depths(n_obs, n_act)
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"history: batch must be at least 1, got {batch}")
        hist = torch.zeros(batch, n_obs, N_STATE, dtype=torch.float32, device=self.device)
        act = torch.zeros(batch, n_act, self.nu, dtype=torch.float32, device=self.device) if n_act else None
        return SimpleNamespace(hist=hist, act=act, n_obs=n_obs, n_act=n_act, n_wide=history_width(n_obs, n_act), W=None, w_rows=0)

    def _attach_history(self, hs):
        """nmpc_policy_rollout_set_history with what `hs` holds, checked; then `_history` is hs"""
        _lib.check(self.lib.nmpc_policy_rollout_set_history(self._h, ptr(hs.hist), hs.n_obs, ptr(hs.act), hs.n_act, ptr(hs.W), hs.w_rows,
                                                            hs.hist.shape[0]), self._h, "nmpc_policy_rollout_set_history", "torque")
        self._history = hs

    def set_history(self, n_obs: Optional[int] = 1, n_act: int = 0, batch: Optional[int] = None):
        """nmpc_policy_rollout_set_history: observation and action history on the policy input.  While attached, a policy of
        `policy_rollout` has n_wide + n_goal inputs, n_wide = 44 n_obs + 12 n_act (`history_width`), and is shown in control step k
        the wide row [O_k | O_{k-1} | ... | O_{k-n_obs+1} | A_{k-1} | ... | A_{k-n_act}] -- O_j the raw 44-slot row as the sensors of
        the robot showed it in step j (`observed_rows`; S_j without a table of noise), A_j the PD target issued in step j --,
        normalised as `DeviceDatabase.batch` normalises a stored row of width n_wide, by two or three more launches per control
        step.  The layer allocates and keeps the two shift registers for `batch` robots (zeros; `reset_history` fills them,
        `history` and `action_history` are the tensors themselves); they move with every control step, so two rollouts of K steps
        are the rollout of 2 K.  Every other output of a rollout is the bits it is without a history when the policy is fed the
        same input.  Rollouts of more robots than `batch` are refused.  `set_history(None)` detaches and drops the registers and
        the wide rows of `set_rollout_wide`; detached, every call makes the launches and gives the bits it gives without."""
        if n_obs is None:
            self._history = None
            _lib.check(self.lib.nmpc_policy_rollout_set_history(self._h, None, 0, None, 0, None, 0, 0), self._h,
                       "nmpc_policy_rollout_set_history", "torque")
            return
        if batch is None:
            raise ValueError("history: batch is needed, the robots the registers are allocated for")
        self._attach_history(self._history_registers(n_obs, n_act, batch))

    def _attached_history(self):
        if self._history is None:
            raise ValueError("history: nothing is attached (set_history)")
        return self._history

    @property
    def history(self) -> Optional[torch.Tensor]:
        """the attached register of observed rows [batch, n_obs, 44] itself (slot 0: the incoming slot; write into it to set it), or None"""
        return None if self._history is None else self._history.hist

    @property
    def action_history(self) -> Optional[torch.Tensor]:
        """the attached register of issued targets [batch, n_act, 12] itself, or None (nothing attached, or n_act = 0)"""
        return None if self._history is None else self._history.act

    def _reset_history(self, hs, S0, q):
        S0 = self._in(S0, (N_STATE,), "S0"); q = self._in(q, (self.n,), "q")
        B = self._batch(S0, q)
        if B > hs.hist.shape[0]:
            raise ValueError(f"history: S0 has {B} rows, the registers {hs.hist.shape[0]}")
        hs.hist[:B] = S0[:, None, :]
        if hs.act is not None:
            hs.act[:B] = q[:, None, self.n - self.nu:]

    def reset_history(self, S0, q):
        """every slot of robot b's register of observed rows <- S0[b] [44], every slot of its action register <- q[b, n - nu:]: the
        row and the posture held before the controller spoke.  S0 [B, 44], q [B, n], B at most the registers' batch; robots beyond
        B keep theirs."""
        self._reset_history(self._attached_history(), S0, q)

    def _history_push(self, hs, goal, s_mean, s_std, s_first, W, want_x=True):
        goal = torch.as_tensor(goal, dtype=torch.float32, device=self.device).contiguous()
        if goal.dim() != 2:
            raise ValueError(f"goal: expected [B, n_goal], got {tuple(goal.shape)}")
        B, n_goal = goal.shape
        if B > hs.hist.shape[0]:
            raise ValueError(f"history: goal has {B} rows, the registers {hs.hist.shape[0]}")
        s_mean, s_std = self._stats(s_mean, s_std, hs.n_wide)
        w_stride = 0
        if W is not None:
            if not isinstance(W, torch.Tensor) or W.dtype != torch.float32 or W.dim() != 2 or W.shape != (B, W.shape[1]) or W.shape[1] < hs.n_wide \
                    or W.device != self.device or W.stride(1) != 1 or (B > 1 and W.stride(0) < W.shape[1]):
                raise ValueError(f"W: need a float32 [{B}, >= {hs.n_wide}] tensor with dense rows on {self.device}")
            w_stride = W.stride(0) if B > 1 else W.shape[1]
        X = torch.empty(B, hs.n_wide + n_goal, dtype=torch.float32, device=self.device) if want_x else None
        _lib.check(self.lib.nmpc_history_push_batch(self._h, B, ptr(hs.hist), hs.n_obs, ptr(hs.act), hs.n_act, ptr(goal), n_goal, ptr(s_mean),
                                                    ptr(s_std), int(s_first), ptr(W), w_stride, ptr(X), stream(self.device)),
                   self._h, "nmpc_history_push_batch", "torque")
        return X

    def history_push(self, goal, s_mean=None, s_std=None, s_first: int = 1, W: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nmpc_history_push_batch on the attached registers: the wide row of the first B robots (B the rows of goal [B, n_goal])
        -> the policy input X [B, n_wide + n_goal], columns [s_first, n_wide) normalised by s_mean, s_std (float64 [n_wide]; None:
        raw), the goal behind it raw; then the observed rows age by one slot, slot 0 keeping its content.  W: a float32
        [B, >= n_wide] tensor with dense rows that takes the raw wide row in its first n_wide columns, or None.  What control step k
        of `policy_rollout` does behind its observation while a history is attached."""
        return self._history_push(self._attached_history(), goal, s_mean, s_std, s_first, W)

    def _history_push_actions(self, hs, A):
        if hs.act is None:
            raise ValueError("history: n_act is 0, there is no action register")
        if not isinstance(A, torch.Tensor) or A.dtype != torch.float32 or A.dim() != 2 or A.shape[1] != self.nu or A.device != self.device \
                or A.stride(1) != 1 or (A.shape[0] > 1 and A.stride(0) < self.nu):
            raise ValueError(f"A: need a float32 [B, {self.nu}] tensor with dense rows on {self.device}")
        B = A.shape[0]
        if B > hs.act.shape[0]:
            raise ValueError(f"history: A has {B} rows, the registers {hs.act.shape[0]}")
        _lib.check(self.lib.nmpc_history_push_actions_batch(self._h, B, ptr(hs.act), hs.n_act, ptr(A), A.stride(0) if B > 1 else self.nu,
                                                            stream(self.device)), self._h, "nmpc_history_push_actions_batch", "torque")

    def history_push_actions(self, A: torch.Tensor):
        """nmpc_history_push_actions_batch on the attached action register: every slot of the first B robots moves up by one and
        slot 0 takes A [B, 12] (dense rows; a row A[:, k] of a table is taken with its stride), the target just issued.  What
        `policy_rollout` does behind its contact step while a history with n_act > 0 is attached."""
        self._history_push_actions(self._attached_history(), A)

    def set_rollout_wide(self, W: Optional[torch.Tensor] = None):
        """the raw wide rows beside a policy rollout: while W [B, rows, n_wide] (rows >= n_steps; a slice [:, :k] of a longer table
        is taken with its stride) is attached to the attached history, control step k of every `policy_rollout` writes robot b's
        raw wide row into W[b, k] -- the row a database of state width n_wide stores, of which `DeviceDatabase.batch` makes the
        bits the policy was shown.  `set_rollout_wide(None)` takes W off and leaves the history; the layer keeps W alive while it
        is attached; a rollout of another batch size than W's is refused."""
        hs = self._attached_history()
        w_rows = 0
        if W is not None:
            if not isinstance(W, torch.Tensor) or W.dim() != 3:
                raise ValueError(f"W: need a float32 [B, rows, {hs.n_wide}] tensor")
            W, w_rows = self._rows(W, hs.n_wide, "W", W.shape[0])
        self._attach_history(SimpleNamespace(**{**vars(hs), "W": W, "w_rows": w_rows}))

    def history_table(self, O: torch.Tensor, A: torch.Tensor, S0, q0, n_obs: Optional[int] = None, n_act: Optional[int] = None) -> torch.Tensor:
        """the wide rows of recorded rollouts: O [B, K, 44] (the rows the sensors showed, or the state rows) and A [B, K, 12] (the
        issued targets) -> W [B, K, n_wide], row k being [O_k | ... | O_{k-n_obs+1} | A_{k-1} | ... | A_{k-n_act}] with S0[b] [44]
        and q0[b, n - nu:] where the rollout had not begun -- K chained `history_push` / `history_push_actions` from
        `reset_history(S0, q0)` on scratch registers of the call's own, so W is what a `policy_rollout` from those registers
        leaves in `set_rollout_wide`.  For an expert's rollouts that are to train a history policy.  n_obs, n_act: the depths (None:
        those of the attached history); the attachment and its registers are not touched."""
        if n_obs is None or n_act is None:
            hs = self._attached_history()
            n_obs, n_act = hs.n_obs if n_obs is None else n_obs, hs.n_act if n_act is None else n_act
        if not isinstance(O, torch.Tensor) or O.dim() != 3:
            raise ValueError(f"O: need a float32 [B, K, {N_STATE}] tensor")
        B, K = O.shape[:2]
        O, _ = self._rows(O, N_STATE, "O", B)
        A, _ = self._rows(A, self.nu, "A", B)
        if A.shape[1] != K:
            raise ValueError(f"A: need {K} rows, got {A.shape[1]}")
        reg = self._history_registers(n_obs, n_act, max(B, 1))
        self._reset_history(reg, S0, q0)
        W = torch.empty(B, K, reg.n_wide, dtype=torch.float32, device=self.device)
        goal = torch.empty(B, 0, dtype=torch.float32, device=self.device)
        for k in range(K if B else 0):
            reg.hist[:, 0] = O[:, k]
            self._history_push(reg, goal, None, None, 0, W[:, k], want_x=False)
            if reg.act is not None:
                self._history_push_actions(reg, A[:, k])
        return W

    def set_push(self, force: Optional[torch.Tensor] = None, start_substep=0, n_substeps=0, joint: int = 5):
        """nmpc_contact_set_push: while force [B, 3] (N, world frame, no moment) is attached, robot b of every `contact_step`,
        `contact_track` and `policy_rollout` of this layer is pushed with force[b] at the origin of the body frame of `joint`
        (5: the trunk) in the substeps start_substep <= s < start_substep + n_substeps, s counted from 0 at the start of each
        call (s = k n_sub + i for substep i of control step k).  start_substep may be negative: the window is cut to the call,
        so a chain of calls with the window moved along is the long call.  Calls with more robots than force has rows are
        refused.  `set_push(None)` detaches; detached, or with a window that misses the call, every call is the bits it is
        without.  The layer keeps the tensor alive while it is attached.
        start_substep and n_substeps may also be integer arrays or tensors of B entries (one of them may stay a scalar, which
        then holds for every robot): a window per robot (nmpc_contact_set_push_windows), robot b pushed in
        start_substep[b] <= s < start_substep[b] + n_substeps[b], n_substeps[b] <= 0 meaning no push for it.  Robot b is then
        the bits it is under the scalar window of its own; the layer keeps the two tensors alive, and `set_push(None)`
        detaches them with the force.  With scalars the calls made are the ones made before there were arrays."""
        if force is None:
            self._push = None
            _lib.check(self.lib.nmpc_contact_set_push(self._h, None), self._h, "nmpc_contact_set_push", "torque")
            self._set_push_windows(None, None)
            return
        force = self._in(force, (3,), "force")
        per_robot = [not isinstance(x, (int, np.integer)) and np.ndim(x) > 0 for x in (start_substep, n_substeps)]
        first = count = None
        if any(per_robot):
            first, count = (self._window(x, force.shape[0], name) for x, name in ((start_substep, "start_substep"), (n_substeps, "n_substeps")))
            start_substep = n_substeps = 0
        cfg = _lib.NmpcPushCfg(force.data_ptr(), force.shape[0], int(joint), int(start_substep), int(n_substeps))
        _lib.check(self.lib.nmpc_contact_set_push(self._h, ctypes.byref(cfg)), self._h, "nmpc_contact_set_push", "torque")
        self._push = force
        self._set_push_windows(first, count)

    def _window(self, x, B, name):
        """x, B window entries (or one for all) as a contiguous int32 [B] tensor on the device"""
        if isinstance(x, torch.Tensor):
            if x.is_floating_point() or x.dtype == torch.bool:
                raise ValueError(f"{name}: need integers")
            t = x.to(device=self.device, dtype=torch.int32)
        else:
            a = np.asarray(x)
            if a.dtype.kind not in "iu":
                raise ValueError(f"{name}: need integers")
            t = torch.as_tensor(a.astype(np.int32), device=self.device)
        if t.dim() == 0:
            t = t.expand(B)
        if tuple(t.shape) != (B,):
            raise ValueError(f"{name}: need {B} entries (one per row of force), got {tuple(t.shape)}")
        return t.contiguous()

    def _set_push_windows(self, first, count):
        """attach the windows per robot, or detach them -- a call only where something is or was attached"""
        if first is None and self._push_windows is None:
            return
        self._push_windows = None if first is None else (first, count)
        _lib.check(self.lib.nmpc_contact_set_push_windows(self._h, ptr(first), ptr(count), 0 if first is None else first.shape[0]),
                   self._h, "nmpc_contact_set_push_windows", "torque")

    def set_grounds(self, grounds=None):
        """nmpc_contact_set_grounds: a ground and a torque limit of its own per robot.  grounds: a sequence of `GroundContact`, or
        a float array or tensor [B, 6] in the order of GROUND_COLUMNS (ground_z, stiffness, damping, mu, slip_velocity, tau_max;
        tau_max <= 0: no limit; `sample_grounds` draws one).  While the table is attached `contact_forces`, `contact_step`,
        `contact_track`, `policy_rollout` and the expert on the plant (`open_loop_device(..., plant=...)`, and with it
        `collect_rollouts` and `learning_iteration`, which take no keyword for it: attach the table on the layer they are
        given) read robot b's law from row b, and their `ground=` / `plant=` argument is ignored (it is still validated).
        Robot b is then the bits it is in the same call under the uniform ground of its row; every call is one launch under
        either integrator.  Calls with more robots than the table has rows are refused.
        Host input is validated by the rules a single ground is refused by (`ground_table`: ValueError) and uploaded; a tensor
        already on the layer's device is taken as given -- the device validates nothing, a NaN or a negative stiffness there is
        the caller's -- and in either case the layer keeps the table alive while it is attached.  `set_grounds(None)`
        detaches; detached, every call makes the launches and gives the bits it gives without."""
        if grounds is None:
            return self._detach("grounds", None, 0)
        rows = self._table(grounds, "grounds", (len(GROUND_COLUMNS),), ground_table)
        self._attach("grounds", rows, ptr(rows), rows.shape[0])

    def _table(self, table, name, shape, validate, dtype=torch.float32):
        """the rows of a table per robot on the device: a device tensor is checked to be `dtype` [B, *shape] and taken as given,
        host input goes through `validate` and is uploaded"""
        if isinstance(table, torch.Tensor) and table.is_cuda:
            if table.dtype != dtype or tuple(table.shape[1:]) != shape or table.dim() != 1 + len(shape) or table.shape[0] < 1 \
                    or table.device != self.device:
                raise ValueError(f"{name}: a device table must be {str(dtype).split('.')[-1]} [{', '.join(map(str, ('B',) + shape))}] "
                                 f"with B >= 1 on {self.device}")
            return table.contiguous()
        host = validate(table.numpy() if isinstance(table, torch.Tensor) else table)
        return torch.tensor(host, device=self.device)      # a copy: the caller's array may be read-only

    def _attach(self, name, kept, *args):
        """nmpc_contact_set_<name>(*args), checked; then `_<name>` is `kept`, which the layer keeps alive while it is attached"""
        fn = "nmpc_contact_set_" + name
        _lib.check(getattr(self.lib, fn)(self._h, *args), self._h, fn, "torque")
        setattr(self, "_" + name, kept)

    def _detach(self, name, *null):
        """`_<name>` is None, also where the call then fails; then nmpc_contact_set_<name> with its null arguments, checked"""
        setattr(self, "_" + name, None)
        fn = "nmpc_contact_set_" + name
        _lib.check(getattr(self.lib, fn)(self._h, *null), self._h, fn, "torque")

    def set_payloads(self, payloads=None, joint: Optional[int] = None):
        """nmpc_contact_set_payloads: a point-mass payload of its own per robot.  payloads: a float array or tensor [B, 4] in the
        order of PAYLOAD_COLUMNS (m_p >= 0 in kg, then its position r in the frame of body `joint`; `sample_payloads` draws one);
        joint None: the trunk, the last virtual base joint n - nu - 1.  While the table is attached robot b carries row b in
        `contact_step`, `contact_track`, `policy_rollout` and the expert on the plant (`open_loop_device(..., plant=...)`, and with
        it `collect_rollouts` and `learning_iteration`, which take no keyword for it: attach the table on the layer they are
        given), under either integrator, with or without a push or a table of grounds; every such call is one launch.  It is
        the plant alone that carries the load: `id_torques`, `forward_dynamics`, `step`, `mass_matrix`, `centroidal`,
        `state_momentum`, `contact_forces`, `plan_actions` and the expert's labels describe the nominal tree, with or without a
        table.  Calls with more robots than the table has rows are refused.
        Host input is validated (`payload_table`: ValueError) and uploaded; a tensor already on the layer's device is taken as
        given -- the device validates nothing -- and in either case the layer keeps the table alive while it is attached.
        `set_payloads(None)` detaches; detached, every call makes the launches and gives the bits it gives without."""
        if payloads is None:
            return self._detach("payloads", None, 0, 0)
        rows = self._table(payloads, "payloads", (len(PAYLOAD_COLUMNS),), payload_table)
        self._attach("payloads", rows, ptr(rows), rows.shape[0], self.n - self.nu - 1 if joint is None else int(joint))

    def set_actuators(self, actuators=None):
        """nmpc_contact_set_actuators: an actuator of its own per robot.  actuators: a float array or tensor [B, 4] in the order of
        ACTUATOR_COLUMNS (kp > 0 and kd >= 0, the gains of the PD law; damping >= 0, a passive joint damping in N m s/rad that
        acts after the torque limit; armature >= 0, the reflected rotor inertia in kg m^2 on the diagonal of the joint-space
        inertia; `sample_actuators` draws one); row b applies to every actuated joint of robot b.  While the table is attached
        `contact_step`, `contact_track`, `policy_rollout` and the expert on the plant (`open_loop_device(..., plant=...)`, and with
        it `collect_rollouts` and `learning_iteration`, which take no keyword for it: attach the table on the layer they are
        given) drive robot b by row b, under either integrator, with or without a push, a table of grounds or a table of
        payloads; every such call is one launch, and its `kp=`, `kd=` are validated as ever and not read for the law.  It is the
        plant alone that has these drives: `id_torques`, `forward_dynamics`, `step`, `mass_matrix`, `centroidal`,
        `contact_forces`, `pd_torques`, `pd_target_action`, `plan_actions` and the expert's labels keep the nominal model and the
        nominal gains, so a label meets gains it was not formed with -- which is the point.  Calls with more robots than the
        table has rows are refused.
        Host input is validated (`actuator_table`: ValueError) and uploaded; a tensor already on the layer's device is taken as
        given -- the device validates nothing -- and in either case the layer keeps the table alive while it is attached.
        `set_actuators(None)` detaches; detached, every call makes the launches and gives the bits it gives without."""
        if actuators is None:
            return self._detach("actuators", None, 0)
        rows = self._table(actuators, "actuators", (len(ACTUATOR_COLUMNS),), actuator_table)
        self._attach("actuators", rows, ptr(rows), rows.shape[0])

    def set_delays(self, delays=None, depth: Optional[int] = None, work_rows: int = 64):
        """nmpc_contact_set_delays: an actuation delay of its own per robot.  delays: an integer array or tensor [B], the control
        steps robot b's drive lags by (0 <= d <= DELAY_MAX_DEPTH; `sample_delays` draws one).  While the table is attached the
        PD target `contact_step`, `contact_track`, `policy_rollout` and the expert on the plant (`open_loop_device(..., plant=...)`,
        and with it `collect_rollouts` and `learning_iteration`, which take no keyword for it: attach the table on the layer they
        are given) apply to robot b in control step k is the one issued in control step k - d_b, and before that what the shift
        register `delay_history` [B, depth, nu] holds (slot j: the target issued j + 1 control steps before the next one;
        `reset_delay_history` fills it with a posture).  The unit is the control step of the call: n_sub dt of `contact_track` and
        `policy_rollout`, one simulation step of the expert on the plant.  Every call advances the register, so a chain of calls
        is the long call.  A of `policy_rollout` and the expert's recorded actions are the issued targets; `plan_actions`, the
        labels, `pd_torques` and `step` do not know about the delay -- it is the plant alone that is late.  A delayed call is bit
        for bit the un-delayed call on the rows `delay_line` gives, under either integrator, push, windows and the other tables.
        depth: the slots of the register (None: max(1, delays.max())); a delay beyond it is clamped to it on the device.
        work_rows: the most control steps one `contact_track` (one replanning interval of the expert) may have; the layer
        allocates and keeps the register (zeros) and the scratch [B, work_rows, nu] the applied rows go to.  Calls with more
        robots than the table has rows are refused.
        Host input is validated (`delay_table`: ValueError) and uploaded; an int32 tensor already on the layer's device is taken
        as given -- the device clamps it into [0, depth] and validates nothing else.  `set_delays(None)` detaches and drops the
        register; detached, every call makes the launches and gives the bits it gives without."""
        if delays is None:
            return self._detach("delays", None, None, 0, None, 0, 0)
        rows = self._table(delays, "delays", (), delay_table, dtype=torch.int32)
        if depth is None:
            depth = min(max(1, int(rows.max())), DELAY_MAX_DEPTH)
        depth, work_rows = int(depth), int(work_rows)
        if not 1 <= depth <= DELAY_MAX_DEPTH:
            raise ValueError(f"delays: depth must be in [1, {DELAY_MAX_DEPTH}], got {depth}")
        if work_rows < 1:
            raise ValueError(f"delays: work_rows must be at least 1, got {work_rows}")
        history = torch.zeros(rows.shape[0], depth, self.nu, dtype=torch.float32, device=self.device)
        work = torch.empty(rows.shape[0], work_rows, self.nu, dtype=torch.float32, device=self.device)
        self._attach("delays", SimpleNamespace(rows=rows, history=history, work=work, depth=depth, work_rows=work_rows),
                     ptr(rows), ptr(history), depth, ptr(work), work_rows, rows.shape[0])

    @property
    def delay_history(self) -> Optional[torch.Tensor]:
        """the attached shift register [B, depth, nu] itself (write into it to set it), or None"""
        return None if self._delays is None else self._delays.history

    def reset_delay_history(self, q):
        """every slot of robot b's register <- q[b, n - nu:]: the posture held before the controller spoke.  q [B, n], B at most the
        rows of the attached table; robots beyond B keep their register."""
        if self._delays is None:
            raise ValueError("delays: no table is attached (set_delays)")
        q = self._in(q, (self.n,), "q")
        history = self._delays.history
        if q.shape[0] > history.shape[0]:
            raise ValueError(f"delays: q has {q.shape[0]} rows, the table {history.shape[0]}")
        history[:q.shape[0]] = q[:, None, self.n - self.nu:]

    def delay_line(self, issued, out: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None, skip_mask: int = 0) -> torch.Tensor:
        """nmpc_delay_line_batch: issued [B, n_steps, nu] (a slice [:, :n_steps] of a longer table is taken with its stride)
        through the attached delays and register -> the applied rows [B, n_steps, nu], row k of robot b being the row issued d_b
        control steps earlier or, before that, what the register held; the register moves on by n_steps.  What `contact_track`
        does in front of its chain while the table is attached.  out: the tensor the rows go to (None: a new one); skip int32
        [B]: robots with skip[b] & skip_mask != 0 are left out, their rows of out and their register untouched."""
        if not isinstance(issued, torch.Tensor) or issued.dim() != 3:
            raise ValueError(f"issued: need a float32 [B, n_steps, {self.nu}] tensor on {self.device}")
        B = issued.shape[0]
        issued, issued_rows = self._rows(issued, self.nu, "issued", B)
        n_steps = issued.shape[1]
        if out is None:
            out = torch.empty(B, n_steps, self.nu, dtype=torch.float32, device=self.device)
        out, out_rows = self._rows(out, self.nu, "out", B)
        if out.shape[1] != n_steps:
            raise ValueError(f"out: need {n_steps} rows, got {out.shape[1]}")
        self._flags(skip, issued, "skip")
        _lib.check(self.lib.nmpc_delay_line_batch(self._h, B, n_steps, ptr(issued), issued_rows, ptr(out), out_rows, ptr(skip), int(skip_mask),
                                                  stream(self.device)), self._h, "nmpc_delay_line_batch", "torque")
        return out

    def set_noise(self, noise=None, seed: int = 0, first_robot: int = 0, step0: int = 0):
        """nmpc_contact_set_noise: sensor noise and bias of its own per robot on what the policy is shown.  noise: a float array or
        tensor [B, 88], row b being sigma[44] then bias[44] of robot b in the units of the raw 44-slot state row (`noise_table`
        builds one, `sample_noise` draws one).  While the table is attached every `observe`, and so every control step of
        `policy_rollout`, `learning.evaluate_policy` and `learning.dagger_iteration`, adds bias + sigma g to the row's slots of the
        policy input X by one more launch behind the observation's own -- g a zero-mean, unit-variance, bounded (|g| < 3.4641)
        variate that is a pure function of (seed, first_robot + b, noise step, slot), divided by the column's s_std where X is
        normalised -- and advances the layer's noise step (`noise_step`) by one; a slot whose sigma and bias are zero is not
        written.  The state rows S, the fall flags, the plant, the rows Q, V of `set_rollout_states`, the delay register and the
        expert's labels stay on the true state: only what the policy is shown moves.  seed: 64 bits; first_robot: robot b draws
        as robot first_robot + b of the population, so that shards of a population draw distinct streams and robot b of a batch
        is the batch of one with first_robot = b; step0: the noise step of the next observation.  Because the step moves on, two
        rollouts of K control steps are the rollout of 2 K.  Calls with more robots than the table has rows are refused.
        Host input is validated (`noise_table`: ValueError) and uploaded; a float32 tensor already on the layer's device is taken
        as given -- the device validates nothing -- and in either case the layer keeps the table alive while it is attached.
        `set_noise(None)` detaches; detached, every call makes the launches and gives the bits it gives without."""
        if noise is None:
            return self._detach("noise", None, 0, 0, 0, 0)
        rows = self._table(noise, "noise", (2 * N_STATE,), _noise_rows)
        first_robot, step0 = int(first_robot), int(step0)
        if not (0 <= first_robot < 2 ** 63 and 0 <= step0 < 2 ** 63):
            raise ValueError("noise: first_robot and step0 must be in [0, 2^63)")
        key = int(seed) & (2 ** 64 - 1)                   # the 64 bits of the key, as the signed argument that carries them
        self._attach("noise", rows, ptr(rows), rows.shape[0], key - 2 ** 64 if key >= 2 ** 63 else key, first_robot, step0)

    @property
    def noise_step(self) -> Optional[int]:
        """nmpc_contact_noise_step: the noise step the next observation with a policy input draws at, or None with nothing attached"""
        if self._noise is None:
            return None
        step = ctypes.c_longlong()
        _lib.check(self.lib.nmpc_contact_noise_step(self._h, ctypes.byref(step)), self._h, "nmpc_contact_noise_step", "torque")
        return step.value

    def observe_noise(self, X, step: int, s_std=None, s_first: int = 1) -> torch.Tensor:
        """nmpc_observe_noise_batch: the attached noise on the first 44 columns of X, a contiguous float32 [B, >= 44] tensor on
        the layer's device, IN PLACE, at noise step `step`; the layer's own noise step is neither read nor moved.  s_std: float64
        [44], the statistics X was normalised with from column s_first on (None: X is raw).  What `observe` does behind its own
        launch while the table is attached -- for the chain of the public calls, and to perturb a training batch.  -> X."""
        if not isinstance(X, torch.Tensor) or X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] < N_STATE or not X.is_contiguous() \
                or X.device != self.device:
            raise ValueError(f"X: need a contiguous float32 [B, >= {N_STATE}] tensor on {self.device}")
        if s_std is not None:
            s_std = torch.as_tensor(s_std, dtype=torch.float64, device=self.device).contiguous()
            if tuple(s_std.shape) != (N_STATE,):
                raise ValueError(f"s_std: expected [{N_STATE}]")
        step = int(step)
        if not 0 <= step < 2 ** 63:
            raise ValueError("noise: step must be in [0, 2^63)")
        _lib.check(self.lib.nmpc_observe_noise_batch(self._h, X.shape[0], ptr(X), X.shape[1], ptr(s_std), int(s_first), step, stream(self.device)),
                   self._h, "nmpc_observe_noise_batch", "torque")
        return X

    def _state_io(self, t, name):
        """t, a contiguous float32 [B, n] tensor on the device that a call updates in place"""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != self.n or not t.is_contiguous() \
                or t.device != self.device:
            raise ValueError(f"{name}: need a contiguous float32 [B, {self.n}] tensor on {self.device} (it is updated in place)")
        return t

    def _rows(self, t, width, name, B):
        """t [B, rows, width] float32 on the device whose rows of a robot are contiguous; -> (t, rows per robot in memory)"""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != B or t.shape[2] != width \
                or t.device != self.device:
            raise ValueError(f"{name}: need a float32 [{B}, rows, {width}] tensor on {self.device}")
        if B == 0 or t.shape[1] == 0:
            return t, t.shape[1]
        table = t.stride(0) >= t.shape[1] * width and t.stride(0) % width == 0      # robot b's rows start at b * stride(0)
        if t.stride(2) != 1 or t.stride(1) != width or not (table or B == 1):
            raise ValueError(f"{name}: rows must be dense and a robot's rows contiguous (a slice [:, :k] of a contiguous table is fine)")
        return t, (t.stride(0) // width if table else t.shape[1])

    def contact_track(self, q, v, A, dt: float, n_sub: int = 1, tau_ff=None, kp: float = KP, kd: float = KD,
                      ground: GroundContact = GroundContact(), Q: Optional[torch.Tensor] = None, V: Optional[torch.Tensor] = None,
                      record: bool = True, skip: Optional[torch.Tensor] = None, skip_mask: int = 0):
        """nmpc_contact_track_batch: A.shape[1] control steps of `contact_step` in one launch, step k with q_des = A[:, k]
        (n_sub substeps of dt each) -- with A the rows of `plan_actions`, the whole-body expert's PD law driving the plant over
        a replanning interval.  q, v [B, n]: contiguous float32 device tensors, updated IN PLACE.  A [B, n_steps, 12] (a slice
        [:, :n_steps] of a longer table is taken with its stride).  Q, V [B, n_steps, 18]: the state before every control step
        (row 0 is the start state), written into the given tensors (again slices are fine) or into new ones with record=True;
        None with record=False.  skip int32 [B]: robots with skip[b] & skip_mask != 0 are left out, their q, v and rows
        untouched.  Bit for bit the chain of `contact_step` calls, under either integrator (`set_integrator`).  With a table of
        delays attached (`set_delays`) A holds the issued targets and at most its work_rows control steps fit one call.
        -> (q, v, Q, V)."""
        q = self._state_io(q, "q"); v = self._state_io(v, "v")
        tau_ff = self._opt(tau_ff, (self.nu,), "tau_ff")
        B = self._batch(q, v, tau_ff)
        A, a_rows = self._rows(A, self.nu, "A", B)
        n_steps = A.shape[1]
        if self._delays is not None and n_steps > self._delays.work_rows:
            raise ValueError(f"delays: a track of {n_steps} control steps needs work_rows >= {n_steps}, the attached table has "
                             f"{self._delays.work_rows} (set_delays(..., work_rows=))")
        if (Q is None) != (V is None):
            raise ValueError("Q and V come together or not at all")
        if Q is None and record:
            Q, V = (torch.empty(B, n_steps, self.n, dtype=torch.float32, device=self.device) for _ in range(2))
        qv_rows = 0
        if Q is not None:
            Q, qv_rows = self._rows(Q, self.n, "Q", B)
            V, v_rows = self._rows(V, self.n, "V", B)
            if Q.shape[1] != n_steps or V.shape[1] != n_steps or v_rows != qv_rows:
                raise ValueError("Q, V: need n_steps rows each and one layout")
        self._flags(skip, q, "skip")
        cfg = ground.cfg()
        _lib.check(self.lib.nmpc_contact_track_batch(self._h, B, n_steps, int(n_sub), float(dt), ctypes.byref(cfg), ptr(q), ptr(v), ptr(tau_ff),
                                                     ptr(A), a_rows, float(kp), float(kd), ptr(Q), ptr(V), qv_rows, ptr(skip), int(skip_mask),
                                                     stream(self.device)), self._h, "nmpc_contact_track_batch", "torque")
        return q, v, Q, V

    def observe_rows(self, Q, V, t0: float, dt_row: float, period: float = NOMINAL_PERIOD, collision_height: float = 0.08,
                     S: Optional[torch.Tensor] = None, failed: Optional[torch.Tensor] = None, step_index: int = 0, term_mask: int = 0,
                     skip: Optional[torch.Tensor] = None, skip_mask: int = 0) -> torch.Tensor:
        """nmpc_observe_rows_batch: `observe` for every row of a table of plant states in one launch.  Q, V [B, n_rows, 18] (as
        `contact_track` writes them; slices of longer tables are taken with their stride); row k is observed at
        t0 + k dt_row.  -> S [B, n_rows, 44] (written into `S` if given, which may be a slice of the rows of a longer table).
        failed int32 [B]: updated in place with the flags of all rows and then, under `observe`'s rule, the stamp
        step_index + 1.  Robots with skip[b] & skip_mask != 0 are untouched.  Bit for bit the n_rows `observe` calls."""
        if not isinstance(Q, torch.Tensor) or Q.dim() != 3:
            raise ValueError("Q: need a float32 [B, n_rows, 18] tensor")
        B = Q.shape[0]
        Q, qv_rows = self._rows(Q, self.n, "Q", B)
        V, v_rows = self._rows(V, self.n, "V", B)
        n_rows = Q.shape[1]
        if V.shape[1] != n_rows or v_rows != qv_rows:
            raise ValueError("Q, V: need the same rows and one layout")
        if S is None:
            S = torch.empty(B, n_rows, N_STATE, dtype=torch.float32, device=self.device)
        S, s_rows = self._rows(S, N_STATE, "S", B)
        if S.shape[1] != n_rows:
            raise ValueError(f"S: need {n_rows} rows")
        self._flags(failed, Q, "failed"); self._flags(skip, Q, "skip")
        _lib.check(self.lib.nmpc_observe_rows_batch(self._h, B, n_rows, ptr(Q), ptr(V), qv_rows, float(t0), float(dt_row), float(period),
                                                    float(collision_height), ptr(S), s_rows, ptr(failed), int(step_index), int(term_mask),
                                                    ptr(skip), int(skip_mask), stream(self.device)),
                   self._h, "nmpc_observe_rows_batch", "torque")
        return S

    def compute_pd_torques(self, q, v, torques_ff, q_plan, v_plan, Kp: float, Kd: float) -> torch.Tensor:
        """mpc.py:592-599: torques_ff + Kp (q_plan[-nu:] - q[-nu:]) + Kd (v_plan[-nu:] - v[-nu:])."""
        q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        qp = self._in(q_plan, (self.n,), "q_plan"); vp = self._in(v_plan, (self.n,), "v_plan")
        ff = self._opt(torques_ff, (self.nu,), "torques_ff")
        tau = torch.empty(q.shape[0], self.nu, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_pd_torques_batch(self._h, q.shape[0], ptr(ff), ptr(q), ptr(v), ptr(qp), ptr(vp), float(Kp),
                                                  float(Kd), ptr(tau), stream(self.device)), self._h, "nmpc_pd_torques_batch", "torque")
        return tau

    def pd_target_action(self, tau, q, v, kp: float = 20.0, kd: float = 1.5, actuator_to_joint: Optional[Sequence[int]] = None):
        """RolloutMPC.py:228-250: action = (tau[perm] + kd v_j) / kp + q_j (kp = 20, kd = 1.5 in the reference)."""
        tau = self._in(tau, (self.nu,), "tau"); q = self._in(q, (self.n,), "q"); v = self._in(v, (self.n,), "v")
        perm = self._perm(actuator_to_joint)
        out = torch.empty_like(tau)
        _lib.check(self.lib.nmpc_pd_target_action_batch(self._h, tau.shape[0], ptr(tau), ptr(perm), ptr(q), ptr(v), float(kp),
                                                        float(kd), ptr(out), stream(self.device)),
                   self._h, "nmpc_pd_target_action_batch", "torque")
        return out

    def plan_actions(self, X, U, zoh, dt_nodes: float, sim_dt: float, kp: float = KP, kd: float = KD,
                     actuator_to_joint: Optional[Sequence[int]] = None, skip: Optional[torch.Tensor] = None, skip_mask: int = 0,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nmpc_plan_actions_batch: the recorded action of every step of the interval that follows a replan.  X [B, N+1, 42],
        U [B, N, 30]: whole-body plans with node spacing dt_nodes; zoh [n_steps]: the node whose a, f each step holds
        (`LocomotionMPC.id_repeat[:n_steps]`).  Row j is (id_torques(q, v, a, f) + kd v_j) / kp + q_j with q, v the plan at
        (j + 1) sim_dt and a, f = U[zoh[j]] -- `references.plan_rows` says which numbers those are.  -> [B, n_steps, 12]
        (written into `out` if given; rollouts with skip[b] & skip_mask != 0 are left as they are)."""
        X = torch.as_tensor(X, dtype=torch.float32, device=self.device).contiguous()
        if X.dim() != 3 or X.shape[1] < 2 or X.shape[2] != 42:
            raise ValueError(f"X: expected [B, N + 1, 42], got {tuple(X.shape)}")
        B, N = X.shape[0], X.shape[1] - 1
        U = self._in(U, (N, 30), "U")
        self._batch(X, U)
        zoh = torch.as_tensor(zoh, dtype=torch.int32, device=self.device).contiguous()
        n_steps = zoh.numel()
        if zoh.dim() != 1 or (n_steps and not bool(((zoh >= 0) & (zoh < N)).all())):
            raise ValueError(f"zoh: expected node indices [n_steps] in [0, {N})")
        perm = self._perm(actuator_to_joint)
        self._flags(skip, X, "skip")
        if out is None:
            out = torch.empty(B, n_steps, 12, dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, n_steps, 12) or not out.is_contiguous() or out.device != X.device:
            raise ValueError(f"out: need contiguous float32 ({B}, {n_steps}, 12) on {self.device}")
        _lib.check(self.lib.nmpc_plan_actions_batch(self._h, B, n_steps, N, ptr(X), ptr(U), ptr(zoh), float(dt_nodes), float(sim_dt),
                                                    float(kp), float(kd), ptr(perm), ptr(skip), int(skip_mask), ptr(out), n_steps,
                                                    stream(self.device)), self._h, "nmpc_plan_actions_batch", "torque")
        return out
