"""References for the tests of the policy-driven rollout on the contact plant (nmpc_observe_batch, nmpc_policy_rollout_batch) --
TEST INFRASTRUCTURE ONLY, built on tests/contact_reference.py, tests/fd_reference.py, oracle/policy_oracle.py and
`trajectory_io` without touching any of them.

  row          the reference's 44-slot state row of a plant state: `convert_to_mujoco` and `state_row` of trajectory_io, with
               base_wrt_feet from `contact_reference.feet` -- the tree's own feet, the points the contact law pushes.
  normalise    the policy input made of a row and a goal: the fp64 expression of nmpc_assemble_batch.
  rollout_ref  the loop row -> normalise -> PolicyOracle.forward(train=False) -> contact_step_ref for one robot: in float64 over
               `fd_ref` it is the reference, in numpy float32 (a PolicyOracle of float32, `aba`) the measure of the number format.
  flags_ref    the fall predicates of a row, restated in numpy float32.
"""
import numpy as np

from iterative_learning_nmpc_amd import trajectory_io as tio
from tests import contact_reference as cr
from tests import fd_reference as fr

FLAG_SOLVER, FLAG_ROLL, FLAG_PITCH, FLAG_HEIGHT, FLAG_VEL_TRACKING, FLAG_COLLISION, FLAG_JOINT_LIMIT = 1, 2, 4, 8, 16, 32, 64
TERM_SHIFT = 8
GROUPS = dict(phase=slice(0, 1), v_lin=slice(1, 4), rates=slice(4, 7), joint_rates=slice(7, 19), z=slice(19, 20), quaternion=slice(20, 24),
              joints=slice(24, 36), base_wrt_feet=slice(36, 44))


def phase(t, period):
    """the recorded gait phase at time t: np.round(phase, 4)"""
    return float(np.round(np.fmod(t, period) / period, 4))


def row(m, q, v, phase, dtype=np.float64):
    """[phase, v_lin 3, body rates 3, joint rates 12, z, quaternion wxyz 4, joints 12, base_wrt_feet 8] of q, v [18] in the Euler
    layout.  dtype float32: the feet in float32 and the row rounded to float32 (rates and quaternion are made in fp64 from the
    fp32 state on the device too)."""
    t = np.dtype(dtype).type
    q, v = np.asarray(q, t), np.asarray(v, t)
    q_mj, v_mj = tio.convert_to_mujoco(q.astype(np.float64), v.astype(np.float64))
    pos = cr.feet(m, q, dtype=dtype)[0]
    base_wrt_feet = (q[:2] - pos[:, :2]).reshape(-1)
    assert base_wrt_feet.dtype == np.dtype(dtype)
    return tio.state_row(phase, v_mj, q_mj, base_wrt_feet).astype(t)


def normalise(state, goal, s_mean=None, s_std=None, s_first=1, dtype=np.float64):
    """[state_norm, goal]: columns [s_first, 44) are (s - mean) / std in fp64, the others raw.  dtype float32: of the row as
    float32 holds it, rounded to float32 -- nmpc_assemble_batch."""
    t = np.dtype(dtype).type
    x = np.asarray(state, t).astype(np.float64)
    if s_mean is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            x[s_first:] = (x[s_first:] - np.asarray(s_mean, np.float64)[s_first:]) / np.asarray(s_std, np.float64)[s_first:]
    return np.concatenate([x, np.asarray(goal, t).astype(np.float64)]).astype(t)


def rollout_ref(m, g, oracle, q, v, n_steps, dt, n_sub, goal, tau_ff=None, kp=20.0, kd=1.5, t0=0.0, period=0.5, s_mean=None, s_std=None,
                s_first=1, fd=fr.fd_ref, dtype=np.float64):
    """nmpc_policy_rollout_batch for one robot -> (S [n_steps, 44], A [n_steps, 12], q, v).  oracle: a PolicyOracle of `dtype`
    (eval mode: a row does not depend on its batch).  Observation k is at t0 + (k n_sub) float32(dt), as the library counts."""
    t = np.dtype(dtype).type
    assert oracle.dtype == dtype
    q, v = np.array(q, t), np.array(v, t)
    S, A = np.zeros((n_steps, 44), t), np.zeros((n_steps, 12), t)
    for k in range(n_steps):
        S[k] = row(m, q, v, phase(t0 + (k * n_sub) * float(np.float32(dt)), period), dtype)
        x = normalise(S[k], goal, s_mean, s_std, s_first, dtype)
        A[k] = oracle.forward(x[None], train=False)[0]
        assert A.dtype == np.dtype(dtype)
        q, v = cr.contact_step_ref(m, g, q, v, dt, n_sub, tau_ff, A[k], kp, kd, fd=fd, dtype=dtype)[:2]
    return S, A, q, v


def flags_ref(row, joints, collision_height):
    """The NMPC_ROLLOUT_FLAG_* bits a state raises, from its row (roll and pitch out of the quaternion) and its twelve joint
    angles, every comparison in float32: check_unsafe_state_v2 without the velocity tracking, and the joint limits in degrees."""
    f = np.float32
    r = np.asarray(row, f)
    z = r[19]
    w, x, y, zq = r[20:24]
    roll = np.arctan2(f(2) * (w * x + y * zq), f(1) - f(2) * (x * x + y * y))
    pitch = np.arcsin(np.clip(f(2) * (w * y - zq * x), f(-1), f(1)))
    lim = f(25.0) * f(0.017453292519943295)
    flags = 0
    if np.abs(roll) > lim:
        flags |= FLAG_ROLL
    if np.abs(pitch) > lim:
        flags |= FLAG_PITCH
    if z < f(0.18) or z > f(0.45):
        flags |= FLAG_HEIGHT
    if z < f(collision_height):
        flags |= FLAG_COLLISION
    if not np.abs(z) <= f(1e30):
        flags |= FLAG_SOLVER
    deg = np.asarray(joints, f).reshape(4, 3) * f(57.29577951308232)
    for hip, th, kn in deg:
        if not (f(-70) <= hip <= f(70)) or not (f(25) <= th <= f(115)) or not (f(-155) <= kn <= f(-60)):
            flags |= FLAG_JOINT_LIMIT
    return flags
