"""What tests/test_gpu_rollout_step.py judges the prepare and advance kernels of the centroidal rollout with (helper module, not
collected by pytest), in fp64 numpy:

  host_mpc            a `BatchedLocomotionMPC` of device None, for its golden-pinned host helpers (`build_problem`,
                      `plan_foot_locations`, `sim_step_rows`, `record_state`, `touch_down`, `increment_base_ref_position`)
  build_problem       `BatchedLocomotionMPC.build_problem` for ANY contact table [4, npc] and per-foot stance ratios: the window
                      and the touch-downs are read off the table (a touch-down is a 0 -> 1 step of a foot's row, the row taken
                      cyclically), where the host planner reads them off the tables it built from a gait configuration.  Pinned
                      against `build_problem` on the configured gaits by tests/test_rollout_step_reference.py.
  sim_rows_fp32       the per-step rows of `sim_step_rows` with every operation in float32: the rounding floor of the row formula
  ulps                distance of two float32 arrays in units in the last place
"""
import numpy as np

from iterative_learning_nmpc_amd.references import base_ref_vel_tracking

GRAVITY = 9.81


def widen(a):
    """the float64 array of the float32 nearest to `a`: inputs the device and the host read alike"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def host_mpc(batch, gait_name="trot", n_nodes=50, height_offset=0.0, footsteps=True, record_sim_steps=False):
    """A `BatchedLocomotionMPC` without a device: the controller's own constructor, host side alone."""
    from iterative_learning_nmpc_amd.mpc import BatchedLocomotionMPC
    return BatchedLocomotionMPC(batch, gait_name, n_nodes=n_nodes, device=None, height_offset=height_offset, footsteps=footsteps,
                                record_sim_steps=record_sim_steps, compute_timings=False)


def as_the_device_reads(m):
    """Round what a controller hands to the device as float32 -- model parameters, hip offsets, stance ratios, foot size -- in
    place, so that its host helpers compute in fp64 on the values the kernels read.  (The tables of the planners are built.)"""
    m.mp = widen(m.mp)
    m.raibert.offset_hip_b[:] = widen(m.raibert.offset_hip_b)
    m.config_gait.stance_ratio = widen(m.config_gait.stance_ratio)
    m.raibert.foot_size = float(widen(m.raibert.foot_size))
    return m


def contact_window(gait, node, n_nodes):
    """[4, n_nodes] contact flags from node `node` on, and the touch-down flags: a foot that stands where it swung one column
    earlier (cyclically; at the first node the column before it in the table)"""
    gait = np.asarray(gait)
    npc = gait.shape[1]
    cols = (node + np.arange(n_nodes)) % npc
    return gait[:, cols].astype(np.float64), (gait[:, cols] == 1) & (gait[:, (cols + npc - 1) % npc] == 0)


def foot_locations(gait, node, N, x, foot_pos, v_des, w_des, *, dt_nodes, period, stance_ratio, hip_offset, height_offset, foot_size):
    """[B, N+1, 4, 3]: `RaiberContactPlanner.get_locations` (stateless) for every touch-down of the window, then the stance
    anchoring of `plan_foot_locations` with its argmin (a foot that stands through the whole window is not anchored)."""
    x, foot_pos = np.asarray(x, float), np.asarray(foot_pos, float).reshape(-1, 4, 3)
    contacts, make = contact_window(gait, node, N + 1)
    B = x.shape[0]
    out = np.zeros((B, N + 1, 4, 3))
    for b in range(B):
        com_xy, com_z = x[b, :2], x[b, 2] - height_offset
        v_cmd, w_yaw = np.asarray(v_des[b][:2], float), float(w_des[b][2])
        cy, sy = np.cos(x[b, 3]), np.sin(x[b, 3])
        for f in range(4):
            locs = np.zeros((N + 1, 3))
            for k in np.flatnonzero(make[f]):
                t_touch = round(k * dt_nodes, 3)
                ratio = float(stance_ratio[f])
                t_stance = period * ratio
                off = np.array([cy * hip_offset[f][0] - sy * hip_offset[f][1], sy * hip_offset[f][0] + cy * hip_offset[f][1]])
                hip = com_xy + off + v_cmd * t_touch * (1 + ratio)
                lever = 0.5 * np.sqrt(max(com_z, 0.0) / GRAVITY) * v_cmd
                centrifugal = np.array([lever[1] * w_yaw, -lever[0] * w_yaw])
                locs[k:, :2] = hip + 0.1 * (v_cmd - x[b, 6:8]) + 0.5 * v_cmd * t_stance + centrifugal
                locs[k:, 2] = foot_size
            if contacts[f, 0]:
                locs[:int(np.argmin(contacts[f]))] = foot_pos[b, f]
            out[b, :, f] = locs
    return out


def build_problem(gait, node, N, x, v_des, w_des, ref_state, foot_pos, *, weight, t_horizon, nom_height, height_offset, footsteps,
                  period, stance_ratio, hip_offset, foot_size):
    """(yref [B, N, 24], yref_e [B, 12], params [B, N+1, 16]) of `BatchedLocomotionMPC.build_problem` for the contact table
    `gait` [4, npc] at node `node`; weight = -gz * mass, the weight the standing feet share."""
    x = np.asarray(x, float)
    B = x.shape[0]
    contacts, _ = contact_window(gait, node, N + 1)
    base_ref, base_ref_e = base_ref_vel_tracking(x, v_des, w_des, ref_state, t_horizon, nom_height, height_offset)
    params = np.zeros((B, N + 1, 16))
    params[:, :, :4] = contacts.T[None]
    if footsteps:
        params[:, :, 4:] = foot_locations(gait, node, N, x, foot_pos, v_des, w_des, dt_nodes=t_horizon / N, period=period,
                                          stance_ratio=stance_ratio, hip_offset=hip_offset, height_offset=height_offset,
                                          foot_size=foot_size).reshape(B, N + 1, 12)
    else:
        params[:, :, 4:] = np.asarray(foot_pos, float).reshape(B, 1, 12)
    n_stance = np.maximum(contacts[:, :N].sum(0), 1.0)
    yref = np.zeros((B, N, 24))
    yref[:, :, :12] = base_ref[:, None, :]
    yref[:, :, 14::3] = (contacts[:, :N].T * (weight / n_stance)[:, None])[None]
    return yref, base_ref_e, params


def _hermite32(y0, m0, y1, m1, h, s):
    one, two, three = np.float32(1.0), np.float32(2.0), np.float32(3.0)
    s2, om = s * s, one - s
    return (one + two * s) * om * om * y0 + s * om * om * h * m0 + s2 * (three - two * s) * y1 + s2 * (s - one) * h * m1


def _euler_rates32(xk):
    sy, cy, sx, cx = np.sin(xk[..., 4]), np.cos(xk[..., 4]), np.sin(xk[..., 5]), np.cos(xk[..., 5])
    wx, wy, wz = xk[..., 11], xk[..., 10], xk[..., 9]
    return np.stack([(sx * wy + cx * wz) / cy, cx * wy - sx * wz, wx + (sx * wy + cx * wz) * sy / cy], axis=-1)


def sim_rows_fp32(X, params, foot_pos, footsteps, *, dt_nodes, sim_dt, steps):
    """Columns 1..18 of the rows of `BatchedLocomotionMPC.sim_step_rows` [B, steps, 18] with the Hermite segments, the Euler
    rates and the finite-difference slopes evaluated in float32 (the segment and its parameter in fp64, rounded once): what
    single precision alone makes of the formula, with no kernel involved."""
    X, params, foot_pos = np.asarray(X, np.float32), np.asarray(params, np.float32), np.asarray(foot_pos, np.float32).reshape(-1, 4, 3)
    B, N = X.shape[0], X.shape[1] - 1
    h = np.float32(dt_nodes)
    out = np.zeros((B, steps, 18), np.float32)
    for j in range(steps):
        t = (j + 1) * sim_dt
        k = min(int(np.floor(t / dt_nodes + 1e-9)), N - 1)
        s = np.float32((t - k * dt_nodes) / dt_nodes)
        x0, x1 = X[:, k], X[:, k + 1]
        d0, d1 = _euler_rates32(x0), _euler_rates32(x1)
        pos = np.concatenate([_hermite32(x0[:, :3], x0[:, 6:9], x1[:, :3], x1[:, 6:9], h, s),
                              _hermite32(x0[:, 3:6], d0, x1[:, 3:6], d1, h, s)], axis=1)
        ka = max(k - 1, 0)
        m0, m1 = (X[:, ka + 1, 6:] - X[:, ka, 6:]) / h, (X[:, k + 1, 6:] - X[:, k, 6:]) / h
        vel = _hermite32(x0[:, 6:], m0, x1[:, 6:], m1, h, s)
        stands = (params[:, k, :4] > 0.5) & bool(footsteps)
        feet = np.where(stands[:, :, None], params[:, k, 4:].reshape(B, 4, 3), foot_pos)
        out[:, j] = np.concatenate([vel, pos[:, 2:6], (pos[:, None, :2] - feet[:, :, :2]).reshape(B, 8)], axis=1)
    return out


def ulps(a, b):
    """|a - b| in units in the last place of float32, entry by entry (int64): the distance of the two bit patterns on the
    ordered line of floats (+0 and -0 at distance 0); a NaN on either side is 2^40"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    def line(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.where(np.isnan(a) | np.isnan(b), np.int64(1) << 40, np.abs(line(a) - line(b)))
