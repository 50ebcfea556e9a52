"""Host-side reference generation and post-processing of the MPC solve.

Restates (numerically identical, golden vectors in tests/golden/):
  rpy_to_matrix                         pin.rpy.rpyToMatrix as used at mpc_controller/mpc.py:205,227,238
  local_angular_to_euler_derivative     mpc_controller/utils/transform.py:72-78
  euler_derivative_to_local_angular     mpc_controller/utils/transform.py:80-86
  base_ref_vel_tracking                 LocomotionMPC.compute_base_ref_vel_tracking, mpc.py:210-272
  increment_base_ref_position           mpc.py:204-208
  hermite_upsample                      interpolate_trajectory_with_derivatives, mpc.py:388-414
  zero_order_hold_index                 id_repeat, mpc.py:142
  plan_rows                             what the plant and mpc.py:583 read of a plan at each simulation step [decl: device clock]
  base_ref_cnt_restricted               LocomotionMPC.compute_base_ref_cnt_restricted, mpc.py:274-315
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def rpy_to_matrix(rpy) -> np.ndarray:
    """R = Rz(yaw) Ry(pitch) Rx(roll) for rpy = (roll, pitch, yaw)."""
    r, p, y = (float(a) for a in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([
        [cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
        [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
        [-sp, cp * sr, cp * cr]])


def _euler_rate_matrix(ypr) -> np.ndarray:
    sx, cx = np.sin(ypr[2]), np.cos(ypr[2])
    sy, cy = np.sin(ypr[1]), np.cos(ypr[1])
    return np.array([[0.0, sx / cy, cx / cy], [0.0, cx, -sx], [1.0, sx * sy / cy, cx * sy / cy]])


def local_angular_to_euler_derivative(ypr_euler, w_local) -> np.ndarray:
    """(yaw,pitch,roll) rates from the body angular velocity (wx,wy,wz)."""
    return _euler_rate_matrix(ypr_euler) @ np.asarray(w_local)


def euler_derivative_to_local_angular(ypr_euler, v_euler) -> np.ndarray:
    """Body angular velocity (wx,wy,wz) from (yaw,pitch,roll) rates."""
    sx, cx = np.sin(ypr_euler[2]), np.cos(ypr_euler[2])
    sy, cy = np.sin(ypr_euler[1]), np.cos(ypr_euler[1])
    M = np.array([[-sy, 0.0, 1.0], [cy * sx, cx, 0.0], [cx * cy, -sx, 0.0]])
    return M @ np.asarray(v_euler)


def _rotate_rpy(rpy, v) -> np.ndarray:
    """rpy_to_matrix(rpy[b]) @ v[b] for rows rpy, v [B, 3], each component summed left to right
    R[i,0] v0 + R[i,1] v1 + R[i,2] v2 -- the order of the device's restatement (csrc/nmpc_rollout_common.hpp)."""
    r, p, y = rpy[:, 0], rpy[:, 1], rpy[:, 2]
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([cy * cp * v0 + (cy * sp * sr - sy * cr) * v1 + (cy * sp * cr + sy * sr) * v2,
                     sy * cp * v0 + (sy * sp * sr + cy * cr) * v1 + (sy * sp * cr - cy * sr) * v2,
                     -sp * v0 + cp * sr * v1 + cp * cr * v2], axis=1)


def base_ref_vel_tracking(q, v_des, w_des, base_ref_state, t_horizon: float, nom_height: float,
                          height_offset: float = 0.0, interactive: bool = False
                          ) -> Tuple[np.ndarray, np.ndarray]:
    """Running and terminal 12-dim base references for velocity tracking, of one row or of a batch of rows
    (every argument with a leading batch axis; a row is the same as a batch of one).

    q              current configuration, q[:3] position, q[3] yaw
    v_des, w_des   commanded base-frame linear velocity and (.., .., yaw-rate)
    base_ref_state the controller's integrated reference `base_ref_vel_tracking` (12,) or [B, 12]
    Keeps the reference's quantisation (np.round to 2 / 1 decimals, builtin round for yaw)
    and its crossed-bounds np.clip, which make the result what it is.
    """
    one = np.ndim(q) == 1
    q, v_des, w_des, state = (np.atleast_2d(np.asarray(a, float)) for a in (q, v_des, w_des, base_ref_state))
    ref = np.zeros((q.shape[0], 12))
    ref[:, :2] = np.round(q[:, :2], 2)
    ref[:, 2] = nom_height + height_offset
    ref[:, 3] = [round(float(y), 1) for y in q[:, 3]]
    v_glob = np.round(_rotate_rpy(state[:, 5:2:-1], v_des), 1)
    ref[:, 6:9] = v_glob
    ref[:, 9:12] = w_des[:, ::-1]

    ref_e = ref.copy()
    ref_e[:, 6:9] = _rotate_rpy(w_des * t_horizon, ref[:, 6:9])
    if interactive:
        pos_ref, yaw_ref = np.round(q[:, :3], 2), q[:, 3]
    else:
        pos_ref, yaw_ref = state[:, :3], state[:, 3]
    reach = v_glob[:, :2] * t_horizon
    ref_e[:, :2] = np.clip(pos_ref[:, :2] + reach, -ref[:, :2] + 1.2 * reach, ref[:, :2] + 1.2 * reach)
    yaw_reach = w_des[:, 2] * t_horizon
    ref_e[:, 3] = np.clip(yaw_ref + yaw_reach, -yaw_ref + 1.5 * yaw_reach, yaw_ref + 1.5 * yaw_reach)
    ref[:, :2] += 0.75 * (ref_e[:, :2] - ref[:, :2])
    ref[:, 3] += 0.75 * (ref_e[:, 3] - ref[:, 3])
    ref_e[:, 8] = 0.0
    ref_e[:, 4:6] = 0.0
    ref[:, 4:6] = 0.0
    ref_e[:, 10:12] = 0.0
    return (ref[0], ref_e[0]) if one else (ref, ref_e)


def increment_base_ref_position(base_ref_state, v_des, w_des, sim_dt: float) -> None:
    """Integrate the commanded velocity into the stored reference, in place (mpc.py:204-208): one row
    base_ref_state (12,) or a batch [B, 12] with v_des, w_des [B, 3]."""
    state = base_ref_state if base_ref_state.ndim == 2 else base_ref_state[None]
    v_des, w_des = (np.atleast_2d(np.asarray(a, float)) for a in (v_des, w_des))
    v_glob = np.round(_rotate_rpy(state[:, 5:2:-1], v_des), 1)
    state[:, :2] += v_glob[:, :2] * sim_dt
    state[:, 3] += w_des[:, 2] * sim_dt


def _hermite(t_knots, y, dy, t_query):
    """Piecewise cubic Hermite evaluation; y, dy are [K, d]; returns [len(t_query), d]."""
    t_knots = np.asarray(t_knots, float)
    seg = np.clip(np.searchsorted(t_knots, t_query, side="right") - 1, 0, len(t_knots) - 2)
    h = (t_knots[seg + 1] - t_knots[seg])[:, None]
    s = ((t_query - t_knots[seg]) / h[:, 0])[:, None]
    y0, y1, m0, m1 = y[seg], y[seg + 1], dy[seg], dy[seg + 1]
    h00 = (1 + 2 * s) * (1 - s) ** 2
    h10 = s * (1 - s) ** 2
    h01 = s * s * (3 - 2 * s)
    h11 = s * s * (s - 1)
    return h00 * y0 + h10 * h * m0 + h01 * y1 + h11 * h * m1


def hermite_upsample(time_traj, positions, velocities, accelerations, n_interp: int):
    """Cubic-Hermite upsampling of (q, v) and (v, a) to n_interp+1 uniformly spaced samples.

    positions, velocities: [K, d]; accelerations: [K-1, d] (first row is repeated in front,
    mpc.py:409-410).  Returns (pos[n_interp+1, d], vel[n_interp+1, d]).
    """
    time_traj = np.asarray(time_traj, float)
    t_query = np.linspace(time_traj[0], time_traj[-1], n_interp + 1)
    acc = np.concatenate((accelerations[:1], accelerations))
    return (_hermite(time_traj, np.asarray(positions), np.asarray(velocities), t_query),
            _hermite(time_traj, np.asarray(velocities), acc, t_query))


def zero_order_hold_index(n_interp: int, n_nodes: int) -> np.ndarray:
    """Node index held at each interpolated sample (mpc.py:142)."""
    return np.int32(np.linspace(0, 1, n_interp) * (n_nodes - 1))


def plan_rows(X, U, zoh, dt_nodes: float, sim_dt: float):
    """Row j of a whole-body plan, j = 0 .. len(zoh) - 1: the declared meaning of "the plan at simulation step j of the interval
    after a replan", in fp64.  X [.., N+1, 42] = [q(18), v(18), h(6)] and U [.., N, 30] = [a(18), f(4x3)] per node, nodes
    dt_nodes apart.  Returns (q [.., n, 18], v [.., n, 18], a [.., n, 18], f [.., n, 4, 3]):
      q, v   the plan at t = (j + 1) sim_dt on the cubic Hermite segments of `hermite_upsample` (mpc.py:388-414; velocities
             through (v_k, a_max(k-1,0))), the segment chosen as the device rollouts choose it (k = floor(t / dt_nodes + 1e-9));
      a, f   of node zoh[j]: the zero-order hold a_sol[id_repeat], f_sol[id_repeat] (mpc.py:142), indexed with the same j
             (mpc.py:583 reads q_plan, v_plan, a_plan, f_plan at one plan_step).
    With dt_nodes N = the horizon and n_interp sim_dt = the horizon these are `hermite_upsample(..)[1:n + 1]` and
    `np.take(.., id_repeat[:n])` to rounding; where the configured dt_nodes is rounded (N = 30: 0.0333) the host loop's
    linspace samples drift from (j + 1) sim_dt and this function follows the device's clock [decl]."""
    X, U, zoh = np.asarray(X, float), np.asarray(U, float), np.asarray(zoh)
    N, n = U.shape[-2], len(zoh)
    if X.shape[-2:] != (N + 1, 42) or U.shape[-1] != 30 or zoh.ndim != 1 or (n and (zoh.min() < 0 or zoh.max() >= N)):
        raise ValueError("plan_rows: need X [.., N+1, 42], U [.., N, 30] and hold indices in [0, N)")
    h = float(dt_nodes)
    t = (np.arange(n) + 1) * float(sim_dt)
    k = np.minimum(np.floor(t / h + 1e-9).astype(int), N - 1)
    s = ((t - k * h) / h)[:, None]
    h00, h10, h01, h11 = (1 + 2 * s) * (1 - s) ** 2, s * (1 - s) ** 2, s * s * (3 - 2 * s), s * s * (s - 1)
    q0, q1, v0, v1 = X[..., k, :18], X[..., k + 1, :18], X[..., k, 18:36], X[..., k + 1, 18:36]
    a0, a1 = U[..., np.maximum(k - 1, 0), :18], U[..., k, :18]
    q = h00 * q0 + h10 * h * v0 + h01 * q1 + h11 * h * v1
    v = h00 * v0 + h10 * h * a0 + h01 * v1 + h11 * h * a1
    hold = U[..., zoh, :]
    return q, v, hold[..., :18], hold[..., 18:].reshape(hold.shape[:-1] + (4, 3))


def base_ref_cnt_restricted(contact_locations, nom_height: float, height_offset: float = 0.0,
                            blend: float = 0.35) -> Tuple[np.ndarray, np.ndarray]:
    """Running and terminal base references of the contact-restricted mode (Raibert plan in hand): the base is sent
    between the centre of the first and the centre of the last COMPLETE set of planned foot locations.

    contact_locations [4, N+1, 3]: the plan, all-zero where a foot has no planned location yet.  The distinct location
    sets are taken in numpy's sorted order (`np.unique(.., axis=1)`), a set counts a foot when all three coordinates of
    that foot are non-zero, and "complete" means "as many feet as the best set has" -- the reference's bincount/argmax
    construction, quirks included: its sets are sorted by value, not by time, so "first"/"last" are the extremes of that
    order.  Running reference: 0.35 first + 0.65 last in x, y; terminal: the last centre; height as configured; everything
    else zero.  Pinned by tests/golden/cnt_restricted.npz (the reference's own outputs)."""
    loc = np.asarray(contact_locations, float)
    sets = np.unique(loc, axis=1)                                   # [4, n_sets, 3]
    feet_planned = np.all(sets != 0.0, axis=-1).sum(axis=0)         # per set: feet with a location
    if feet_planned.any():
        best = np.flatnonzero(feet_planned == feet_planned.max())
        first, last = sets[:, best[0]].mean(axis=0), sets[:, best[-1]].mean(axis=0)
    else:                                                           # nothing planned at all: first and last node as they are
        first, last = loc[:, 0].mean(axis=0), loc[:, -1].mean(axis=0)
    ref, ref_e = np.zeros(12), np.zeros(12)
    ref[:2] = blend * first[:2] + (1.0 - blend) * last[:2]
    ref_e[:2] = last[:2]
    ref[2] = ref_e[2] = nom_height + height_offset
    return ref, ref_e
