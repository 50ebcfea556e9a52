"""The two kernels around every solve of the device-resident centroidal rollout, tensor by tensor and entry by entry.

nmpc_rollout_prepare_kernel: one rollout call of one replan, then the problem tensors it wrote (yref, yref_e, params; read back with
nmpc_debug_read_centroidal_rollout_problem) against the host helpers in fp64 on the same float32-representable inputs --
`BatchedLocomotionMPC.build_problem` where the controller's defaults reach the case, tests/rollout_step_reference.py
(`build_problem` for any contact table, pinned by tests/test_rollout_step_reference.py) where they do not.
nmpc_rollout_advance_kernel: after that call X holds the plan the kernel read and the read-back its params, so the rows, the
flags and the advanced state are functions of known inputs; the solve is out of the comparison.

Bars (per entry, no norms, nothing left out):
  contact flags, copied entries, zeros, the heights, vg          0 ulp
  ref, ref_e, touch-down targets (fp64, rounded once to fp32)    <= 1 ulp of fp32 (the device's and numpy's sin / cos may differ in
                                                                 the last fp64 bit); 0 ulp in r[0], r[1], r[3] at the tie inputs
  force share cflag * weight / max(n, 1) (fp32 against fp64)     <= 1 ulp
  phase column of a row                                          0 ulp against np.round(.., 4) cast to fp32
  Hermite columns of a per-step row                              4 x the deviation of the fp32 numpy restatement of the formula
                                                                 (`sim_rows_fp32`) from the fp64 rows, per column
  the row of a per-replan call, x and foot_pos after the step    0 ulp
  ref_state after the step                                       <= 1 fp64 ulp per simulation step taken (40)
Measured on MI355X: every entry of yref, yref_e and params of every case below is 0 ulp from the host value, the force shares
included (a reference moved by 1e-7 relative in a hip offset, the weight, a stance ratio or the yaw is 2 - 3 ulp off and fails);
the device's per-step rows equal the fp32 numpy restatement bit for bit (the per-column figures stand in the docstring of
`test_per_step_rows_and_the_step`)."""
import ctypes
import types

import numpy as np
import pytest

from tests import rollout_step_reference as R
from tests.solve_helpers import dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
HIPS = R.widen([[0.23, 0.16], [0.23, -0.16], [-0.23, 0.16], [-0.23, -0.16]])          # the planner's hips (offsets 0.04, 0.02 added)
FOOT_SIZE = float(F32(0.0085))
PHASE = 0.375                                                                          # passed in with a per-replan row


def _mp(N):
    from iterative_learning_nmpc_amd.workloads import model_params
    return model_params(dt=1.0 / N)


WEIGHT = float(-R.widen(_mp(50))[5] * R.widen(_mp(50))[1])                            # -gz * mass of the float32 parameters, in fp64


def _solver(dev, N, B, gait):
    from iterative_learning_nmpc_amd.config import CostConfigFactory
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.workloads import MODEL_CENTROIDAL
    s = BatchedNmpcSolver(MODEL_CENTROIDAL, N, B, dev)
    s.set_contact_patterns(gait_sequence=gait)
    s.set_model_params(_mp(N))
    cost = CostConfigFactory.get("go2", "trot")
    s.set_cost_weights(np.concatenate([cost.W_base, cost.W_cnt_f_reg.ravel()]), cost.W_e_base, cost.reg_eps, cost.reg_eps_e)
    s.set_max_qp_iter(6)
    return s


def _cfg(gait, **kw):
    d = dict(n_replans=1, nodes_per_replan=1, replanning_steps=40, nodes_per_cycle=int(np.asarray(gait).shape[1]), start_node=0,
             first_solve=1, max_sqp_first=15, nlp_tol_first=0.01, nlp_tol=0.1, sim_dt=1.0e-3, time_horizon=1.0, nom_height=0.3,
             height_offset=0.0, push_start=0.0, push_duration=0.0, footsteps=1, record_sim_steps=0, hip_offset=HIPS.ravel().tolist(),
             stance_ratio=[0.5] * 4, nominal_period=0.5, foot_size=FOOT_SIZE, terminate_mask=0, collision_height=0.08)
    d.update(kw)
    return d


def _inputs(B, seed, pos_scale=1.0):
    """generic float32-representable inputs: positions of both signs, every angle, rate and command component non-zero"""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 12))
    x[:, :2] = rng.normal(0, pos_scale, (B, 2)); x[:, 2] = 0.3 + rng.normal(0, 0.02, B); x[:, 3] = rng.uniform(-3.0, 3.0, B)
    x[:, 4:6] = rng.normal(0, 0.05, (B, 2)); x[:, 6:] = rng.normal(0, 0.2, (B, 6))
    ref = np.zeros((B, 12)); ref[:, :2] = x[:, :2] + rng.normal(0, 0.05, (B, 2)); ref[:, 3:6] = rng.normal(0, 0.3, (B, 3))
    cy, sy = np.cos(x[:, 3]), np.sin(x[:, 3])
    foot = np.zeros((B, 4, 3))
    foot[:, :, 0] = x[:, None, 0] + cy[:, None] * HIPS[None, :, 0] - sy[:, None] * HIPS[None, :, 1]
    foot[:, :, 1] = x[:, None, 1] + sy[:, None] * HIPS[None, :, 0] + cy[:, None] * HIPS[None, :, 1]
    foot += rng.normal(0, 0.02, (B, 4, 3))
    return dict(x=R.widen(x), v_des=R.widen(rng.normal(0, 0.3, (B, 3))), w_des=R.widen(rng.normal(0, 0.3, (B, 3))), ref=R.widen(ref),
                foot=R.widen(foot))


def _problem(s, B):
    return tuple(np.stack(a) for a in zip(*(s.debug_centroidal_rollout_problem(b) for b in range(B))))


def _call(s, gait, inp, cfg, force=None):
    """one nmpc_rollout_batch call from `inp` (left as it is); -> what the call left, as numpy arrays, and the read-back"""
    B, N = inp["x"].shape[0], s.n_nodes
    x, foot = s.to_device(inp["x"]), s.to_device(inp["foot"].reshape(B, 12))
    v_des, w_des, ref = (s.to_device(inp[k], torch.float64) for k in ("v_des", "w_des", "ref"))
    X = torch.zeros(B, N + 1, 12, dtype=torch.float32, device=s.device)
    U = torch.zeros(B, N, 12, dtype=torch.float32, device=s.device)
    status = torch.zeros(B, dtype=torch.int32, device=s.device)
    S, failed = s.rollout(s.to_device(gait, torch.int8), x, v_des, w_des, ref, foot, None if force is None else s.to_device(force),
                          np.full(cfg["n_replans"], PHASE), X, U, status, **cfg)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dict(x=x, foot=foot, ref=ref, X=X, U=U, status=status, S=S, failed=failed).items()}
    return types.SimpleNamespace(problem=_problem(s, B), **out)


def _target_mask(gait, node, N):
    """[N+1, 4]: the foot locations that are Raibert targets (computed), the others being copies of foot_pos or zeros"""
    contacts, make = R.contact_window(gait, node, N + 1)
    seen = np.cumsum(make, axis=1) > 0
    for f in range(4):
        if contacts[f, 0]:
            seen[f, :int(np.argmin(contacts[f]))] = False
    return seen.T


def _exact_masks(B, N, targets=None, tie_rows=()):
    """the entries of (yref, yref_e, params) that must match bit for bit; targets: `_target_mask` (None: no footsteps)"""
    yref, yref_e, params = np.zeros((B, N, 24), bool), np.zeros((B, 12), bool), np.ones((B, N + 1, 16), bool)
    yref[:, :, [2, 4, 5, 6, 7, 8, 9, 10, 11]] = True                 # height, zeros, vg, the copied rates
    yref[:, :, 12:] = (np.arange(12) % 3 != 2)[None, None]           # the horizontal force references: zeros
    yref_e[:, [2, 4, 5, 8, 9, 10, 11]] = True
    for b in tie_rows:                                               # no sine or cosine behind these: the same fp64 operations
        yref[b, :, [0, 1, 3]] = True
        yref_e[b, [0, 1, 3]] = True
    if targets is not None:
        params[:, :, 4:] = ~np.repeat(targets, 3, axis=1)[None] | (np.arange(12) % 3 == 2)[None, None]
    return yref, yref_e, params


def _assert_problem(got, want, exact, what):
    worst = {}
    for name, g, w, ex in zip(("yref", "yref_e", "params"), got, want, exact):
        assert g.shape == w.shape == ex.shape, (what, name, g.shape, w.shape)
        w32 = w.astype(F32)
        d = R.ulps(g, w32)
        if name == "yref":                                           # a swinging foot's share: cflag = 0 times the share, a zero
            ex = ex.copy(); ex[:, :, 12:] |= w32[:, :, 12:] == 0
        worst[name] = (int(d.max()), int(d[ex].max()) if ex.any() else 0)
        bad = np.argwhere((d > 1) | (ex & (d > 0)))
        assert len(bad) == 0, (what, name, "entries off:", len(bad), "first:", bad[0].tolist(), float(g[tuple(bad[0])]),
                               float(w[tuple(bad[0])]), "ulps", int(d[tuple(bad[0])]))
    print(f"{what}: max ulps (all entries, exact entries) {worst}")
    return worst


def _table(name):
    m = R.host_mpc(1, name, 50)
    return m.contact_planner.gait_sequence.copy(), m.config_gait


TABLES = {
    # foot 0 stands through every window (not anchored: the argmin quirk), foot 1 never stands
    "stands_and_never": np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 1, 1], [0, 1, 1, 1, 0, 0]], np.int8),
    # at node 0: feet 0, 1 mid-swing with the table entry before node 0 across the wrap (swinging / standing there), foot 2 touches
    # down AT node 0 (its entry across the wrap swings), foot 3 stands since before the wrap
    "mid_swing_wrap": np.array([[0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 0, 0, 1, 1, 1]], np.int8),
    # column 2: all four feet in flight (share = weight / max(0, 1)); columns of one, two, three and four standing feet
    "flight": np.array([[1, 1, 0, 0, 1], [1, 0, 0, 1, 1], [1, 0, 0, 1, 0], [1, 1, 0, 0, 0]], np.int8),
}


def _reference(gait, node, N, inp, **kw):
    d = dict(weight=WEIGHT, t_horizon=1.0, nom_height=0.3, height_offset=0.0, footsteps=True, period=0.5, stance_ratio=[0.5] * 4,
             hip_offset=HIPS, foot_size=FOOT_SIZE)
    d.update(kw)
    return R.build_problem(gait, node, N, inp["x"], inp["v_des"], inp["w_des"], inp["ref"], inp["foot"], **d)


# ------------------------------------------------------------------------------------------------ the prepare kernel
@pytest.mark.parametrize("N", [1, 2, 7, 50, 127, 128])
def test_prepare_at_every_horizon_and_start_node(dev, N):
    """N = 128 fills the last slot of the LDS window (cflag[4 * 129]); N * 24 and (N + 1) * 16 that no multiple of 64 divides;
    start nodes 0, 1, npc - 1, npc, 3 npc + 5 wrap the trot table (npc = 25) on the first and on later window nodes.
    Measured: 0 ulp in every entry."""
    gait, _ = _table("trot")
    npc, B = gait.shape[1], 8
    s = _solver(dev, N, B, gait)
    for node in (0, 1, npc - 1, npc, 3 * npc + 5):
        inp = _inputs(B, 1000 * N + node)
        t = _call(s, gait, inp, _cfg(gait, start_node=node))
        _assert_problem(t.problem, _reference(gait, node, N, inp), _exact_masks(B, N, _target_mask(gait, node, N)), f"N={N} node={node}")


def test_a_horizon_past_the_window_is_refused_and_nothing_is_launched(dev):
    """N = 129: the entry point's own message, and S, x, X and failed keep what they held"""
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.solver import _cfg as cfg_struct
    gait, _ = _table("trot")
    B, N = 4, 129
    s = _solver(dev, N, B, gait)
    inp = _inputs(B, 5)
    x, foot = s.to_device(inp["x"]), s.to_device(inp["foot"].reshape(B, 12))
    v_des, w_des, ref = (s.to_device(inp[k], torch.float64) for k in ("v_des", "w_des", "ref"))
    X, U, S = (torch.full(shape, -7.0, dtype=torch.float32, device=dev) for shape in ((B, N + 1, 12), (B, N, 12), (B, 1, 19)))
    status, failed = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    c = cfg_struct(_lib.NmpcRolloutCfg, _cfg(gait))
    phase = np.zeros(1, F32)
    rc = s.lib.nmpc_rollout_batch(s._h, B, ctypes.byref(c), _lib.ptr(s.to_device(gait, torch.int8)), _lib.ptr(x), _lib.ptr(v_des),
                                  _lib.ptr(w_des), _lib.ptr(ref), _lib.ptr(foot), None, phase.ctypes.data_as(ctypes.c_void_p),
                                  _lib.ptr(X), _lib.ptr(U), _lib.ptr(S), _lib.ptr(status), _lib.ptr(failed), _lib.stream(dev))
    torch.cuda.synchronize()
    assert rc == -1 and s.lib.nmpc_last_error(s._h).decode() == "rollouts need N <= 128"
    assert (S == -7).all() and (X == -7).all() and (U == -7).all() and (failed == -7).all() and (status == -7).all()
    assert np.array_equal(x.cpu().numpy(), inp["x"].astype(F32)) and np.array_equal(ref.cpu().numpy(), inp["ref"])
    with pytest.raises(_lib.NmpcError, match="never run a rollout"):
        s.debug_centroidal_rollout_problem(0)
    with pytest.raises(_lib.NmpcError, match="index out of range"):
        s.debug_centroidal_rollout_problem(B)


def test_the_read_back_refuses_a_whole_body_handle(dev):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    from iterative_learning_nmpc_amd.workloads import MODEL_WHOLEBODY
    s = BatchedNmpcSolver(MODEL_WHOLEBODY, 10, 2, dev)
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(16 * 11 * 24, F32)
    rc = s.lib.nmpc_debug_read_centroidal_rollout_problem(s._h, 0, buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), buf.ctypes.data_as(fp))
    assert rc == -1 and b"needs the centroidal model" in s.lib.nmpc_last_error(s._h) and not buf.any()
    with pytest.raises(_lib.NmpcError):
        s.debug_rollout_problem(2)                                   # the whole-body read-back is as it was: b < B_max


@pytest.mark.parametrize("name", ["trot", "slow_trot", "stands_and_never", "mid_swing_wrap", "flight"])
def test_prepare_on_gait_tables(dev, name):
    """The configured tables and hand-written ones through `solver.rollout`, per-foot stance ratios that differ, against the
    restatement for any table: a foot standing through the window (not anchored) beside one that never stands; feet mid-swing at
    node 0 whose previous table entry lies across the wrap; a touch-down at node 0; a column with all four feet in flight.
    Measured: 0 ulp in every entry."""
    if name in TABLES:
        gait, period, nom_height, N = TABLES[name], 0.5, 0.3, 7                    # N > npc: the window wraps in itself
        ratios = R.widen([0.5, 0.63, 0.4, 0.7])
    else:
        gait, cg = _table(name)
        period, nom_height, N, ratios = cg.nominal_period, cg.nom_height, 50, R.widen(cg.stance_ratio)
    npc, B = gait.shape[1], 8
    s = _solver(dev, N, B, gait)
    reached = set()
    for node in (0, 1, npc - 1, npc, 3 * npc + 5):
        inp = _inputs(B, 77 + node)
        inp["x"][0, 2] = R.widen(-0.02)                                           # a base below the ground: the lever is clamped
        t = _call(s, gait, inp, _cfg(gait, start_node=node, stance_ratio=ratios.tolist(), nominal_period=period, nom_height=nom_height))
        want = _reference(gait, node, N, inp, period=period, stance_ratio=ratios, nom_height=nom_height)
        _assert_problem(t.problem, want, _exact_masks(B, N, _target_mask(gait, node, N)), f"{name} node={node}")
        contacts, make = R.contact_window(gait, node, N + 1)
        reached |= {"unanchored" for f in range(4) if contacts[f].all()} | {"never" for f in range(4) if not contacts[f].any()}
        reached |= {"touch_down_at_0" for f in range(4) if make[f, 0]} | {"flight" for k in range(N + 1) if not contacts[:, k].any()}
        reached |= {"swing_at_0_after_swing" for f in range(4) if not contacts[f, 0] and not gait[f, (node - 1) % npc]}
    assert {"stands_and_never": {"unanchored", "never"}, "mid_swing_wrap": {"touch_down_at_0", "swing_at_0_after_swing"},
            "flight": {"flight"}}.get(name, set()) <= reached, reached


TIE_YAWS = (0.25, 0.75, -0.25, 1.25, 2.75, 3.1, -3.1)                # the first five: exact binary ties of round(x, 1)
TIE_POS = (0.125, -0.375, 0.625, -0.875, 1.125, 2.375, -2.625)       # 0.005 k exactly representable: ties of np.round(x, 2)
TIE_V = ((0.25, 0.0, 0.0), (0.75, 0.25, -0.25), (-0.25, 0.75, 0.0), (0.0, -0.75, 0.25))     # R = 1: ties of np.round(R v, 1)


@pytest.mark.parametrize("gait_name,node,height_offset,footsteps",
                         [("trot", 0, 0.0, True), ("trot", 13, 0.05, True), ("slow_trot", 49, 0.05, True), ("trot", 7, 0.0, False)])
def test_prepare_through_the_controller(dev, gait_name, node, height_offset, footsteps):
    """`BatchedLocomotionMPC.open_loop_device` for one replan against its own `build_problem`, with current_opt_node,
    height_offset, v_des, w_des, base_ref_vel_tracking and foot_pos set directly.  Rows 0 .. 27: every tie yaw with every tie
    position and a tie command under an identity reference rotation -- r[0], r[1], r[3] and vg bit for bit; negative positions
    cross the clip bounds.  Rows 28 ..: generic, non-zero reference yaw, pitch and roll, bases below the ground, base velocity
    off the command, yaw rate non-zero.  footsteps = 0: params[:, :, 4:] is foot_pos repeated.
    Measured: 0 ulp in every entry."""
    from iterative_learning_nmpc_amd.mpc import BatchedLocomotionMPC
    n_tie, B = 28, 48
    inp = _inputs(B, 31 + node, pos_scale=1.5)
    for b in range(n_tie):
        inp["x"][b, 3] = R.widen(TIE_YAWS[b % 7])
        xy = np.array([TIE_POS[(b + b // 7) % 7], TIE_POS[(b + 3) % 7]])
        inp["foot"][b, :, :2] = R.widen(inp["foot"][b, :, :2] + (xy - inp["x"][b, :2]))      # the feet stay under the base
        inp["x"][b, :2] = xy
        inp["v_des"][b] = TIE_V[b % 4]
        inp["ref"][b, 3:6] = 0.0
    inp["x"][n_tie:n_tie + 4, 2] = R.widen(height_offset - 0.03)                  # below the ground
    mpc = R.as_the_device_reads(BatchedLocomotionMPC(B, gait_name, n_nodes=50, device=dev, height_offset=height_offset,
                                                     footsteps=footsteps, terminate_mask=0, compute_timings=False))
    mpc.current_opt_node = node
    mpc.v_des, mpc.w_des, mpc.base_ref_vel_tracking = inp["v_des"].copy(), inp["w_des"].copy(), inp["ref"].copy()
    mpc.foot_pos = inp["foot"].copy()
    want = mpc.build_problem(inp["x"])
    vg = want[0][:n_tie, 0, 6:9]
    assert np.array_equal(vg[0], [0.2, 0.0, 0.0]) and np.array_equal(vg[1], [0.8, 0.2, -0.2])      # the ties went to even
    mpc.open_loop_device(inp["x"], 0.04)
    torch.cuda.synchronize()
    gait = mpc.contact_planner.gait_sequence
    exact = _exact_masks(B, 50, _target_mask(gait, node, 50) if footsteps else None, tie_rows=range(n_tie))
    got = _problem(mpc.solver, B)
    _assert_problem(got, want, exact, f"{gait_name} node={node} height_offset={height_offset} footsteps={footsteps}")
    if not footsteps:
        assert np.array_equal(got[2][:, :, 4:], np.broadcast_to(inp["foot"].astype(F32).reshape(B, 1, 12), (B, 51, 12)))


def test_first_solve_warm_start(dev):
    """The cold start with the solve left out: X is the state repeated, U the force reference.  The skip mask of the solver does
    not reach a rollout (the rollout installs its own, failed & terminate_mask, and the prepare kernel leaves such a rollout
    alone as well), so the case runs the cold start with max_sqp_first = 0: `run_rollout` hands it to the solve as max_sqp, and
    the SQP loop of `launch_sqp` (nmpc_api.hip: `for (int it = 0; it < a.max_sqp; ++it)`, the only place that launches the
    linearisation and the QP kernel) then runs no iteration.  The advance kernel hands the unchanged plan on."""
    gait, _ = _table("trot")
    B, N = 8, 50
    s = _solver(dev, N, B, gait)
    inp = _inputs(B, 9)
    t = _call(s, gait, inp, _cfg(gait, start_node=3, max_sqp_first=0, nodes_per_replan=2))
    yref, _, _ = t.problem
    assert np.array_equal(t.X, np.broadcast_to(inp["x"].astype(F32)[:, None, :], (B, N + 1, 12)))
    assert np.array_equal(t.U, yref[:, :, 12:]) and np.abs(t.U[:, :, 2::3]).max() > 30.0
    want = _reference(gait, 3, N, inp)
    assert R.ulps(t.U, want[0][:, :, 12:].astype(F32)).max() <= 1
    assert (t.status == 0).all() and np.array_equal(t.x, inp["x"].astype(F32))    # plant = plan: the state it started from


# ------------------------------------------------------------------------------------------------ the advance kernel
def _start_states(B, seed):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 12)); x0[:, 2] = 0.3
    x0[:, :2] = rng.normal(0, 0.5, (B, 2)); x0[:, 3] = rng.uniform(-1.0, 1.0, B)
    x0[:, 4] = 0.3 * rng.choice([-1.0, 1.0], B); x0[:, 5] = 0.3 * rng.choice([-1.0, 1.0], B)
    x0[:, 6:9] = rng.normal(0, 0.3, (B, 3)); x0[:, 9:] = rng.normal(0, 1.0, (B, 3))
    return R.widen(x0)


@pytest.mark.parametrize("N", [25, 50, 125])
def test_per_step_rows_and_the_step(dev, N):
    """record_sim_steps = 1 at 1, 2 and 5 nodes per replan, roll and pitch of +-0.3 rad and body rates of order 1, a base push
    over the first interval, the start node one before a touch-down of the front left foot so that the touch-down lies inside
    the replan interval.  Replan 0 from a one-replan call; replan 1 (replan_index > 0 in the recorded phase; the centroidal
    harness has no clock across calls, so the index only grows inside a call) from a two-replan call whose first replan is bit
    for bit the one-replan call.  Every row against `sim_step_rows(X.double(), params, replan_index)`; x, foot_pos, ref_state
    after the step; failed against `state_row_flags` of the device's own rows.
    Measured on MI355X: max |row - fp64 row| per column, of the fp32 restatement (the floor; the bar is 4 x it) -- and of the device,
    which is the same figure in all 108 entries: its rows are the restatement bit for bit.  Cases N = 25, 50, 125, replan 0 / 1;
    the column's magnitude max |fp64 row| in brackets as a range over the cases.
      col  25/0    25/1    50/0    50/1    125/0   125/1    [magnitude]
       1   6.8e-08 1.2e-07 1.3e-07 1.1e-07 4.5e-08 4.5e-08  [0.51 .. 0.85]
       2   4.6e-08 3.0e-08 6.2e-08 6.0e-08 6.6e-08 9.0e-08  [0.20 .. 0.71]
       3   8.6e-08 8.9e-08 7.5e-08 8.3e-08 5.6e-08 3.4e-08  [0.37 .. 0.82]
       4   2.5e-07 2.6e-07 4.6e-07 3.1e-07 3.6e-07 2.2e-07  [1.87 .. 3.63]
       5   1.9e-07 2.0e-07 3.3e-07 2.5e-07 1.6e-07 2.4e-07  [1.99 .. 2.77]
       6   3.5e-07 3.6e-07 6.0e-07 7.6e-07 2.9e-07 2.6e-07  [2.40 .. 5.79]
       7   5.6e-08 5.7e-08 5.9e-08 6.1e-08 5.1e-08 4.3e-08  [0.32 .. 0.36]
       8   9.9e-08 1.5e-07 1.2e-07 1.3e-07 9.2e-08 7.1e-08  [0.76 .. 1.01]
       9   6.4e-08 6.2e-08 6.1e-08 5.2e-08 4.8e-08 4.0e-08  [0.30 .. 0.37]
      10   6.6e-08 4.2e-08 5.5e-08 4.1e-08 4.2e-08 3.6e-08  [0.27 .. 0.32]
      11   1.9e-07 1.7e-07 2.4e-07 1.4e-07 1.2e-07 1.4e-07  [0.34 .. 0.37]   (13, 15, 17: the same figures, magnitudes 0.22 .. 0.31)
      12   1.8e-07 1.7e-07 1.5e-07 9.7e-08 1.1e-07 1.2e-07  [0.24 .. 0.33]   (14, 16, 18: the same figures, magnitudes 0.16 .. 0.30)
    ref_state: at most 40 fp64 ulp (one per simulation step); x and foot_pos bit for bit."""
    from iterative_learning_nmpc_amd.mpc import BatchedLocomotionMPC, state_row_flags
    B = 8
    x0 = _start_states(B, N)
    force = R.widen(np.random.default_rng(N).uniform(-40, 40, (B, 3)))
    push = dict(start=0.0, duration=0.04, force=force)
    host = R.as_the_device_reads(R.host_mpc(B, "trot", N, footsteps=True, record_sim_steps=True))
    gait, npr, steps = host.contact_planner.gait_sequence, host.nodes_per_replan, host.replanning_steps
    node0 = int(np.flatnonzero((gait[0] == 1) & (np.roll(gait[0], 1) == 0))[0]) - 1          # front left touches down at window node 1
    v_des, w_des = R.widen(np.tile([0.3, 0.05, 0.0], (B, 1))), R.widen(np.tile([0.0, 0.0, 0.2], (B, 1)))
    ref0 = np.zeros((B, 12)); ref0[:, :2] = x0[:, :2]; ref0[:, 3] = x0[:, 3]
    foot0 = R.widen(x0[:, None, :3] * [1, 1, 0] + np.concatenate([HIPS, np.zeros((4, 1))], axis=1)[None])
    runs = {}
    for n_replans in (1, 2):
        mpc = R.as_the_device_reads(BatchedLocomotionMPC(B, "trot", n_nodes=N, device=dev, footsteps=True, record_sim_steps=True,
                                                         terminate_mask=0, compute_timings=False))
        mpc.current_opt_node = node0
        mpc.v_des, mpc.w_des, mpc.base_ref_vel_tracking, mpc.foot_pos = v_des.copy(), w_des.copy(), ref0.copy(), foot0.copy()
        S, _ = mpc.open_loop_device(x0, 0.04 * n_replans, push)
        torch.cuda.synchronize()
        runs[n_replans] = types.SimpleNamespace(S=S.cpu().numpy(), X=mpc.X.cpu().numpy(), x=mpc.x_final.cpu().numpy(), foot=mpc.foot_pos,
                                                ref=mpc.base_ref_vel_tracking, failed=mpc.failed.cpu().numpy(),
                                                params=_problem(mpc.solver, B)[2], status=mpc.status.cpu().numpy())
    one, two = runs[1], runs[2]
    assert one.S.shape == (B, steps, 19) and np.array_equal(two.S[:, :steps], one.S)       # the same first replan, bit for bit
    host.v_des, host.w_des = v_des, w_des
    table = []
    for index, run, foot_before, rows in ((0, one, foot0, one.S), (1, two, one.foot, two.S[:, steps:])):
        host.foot_pos = np.asarray(foot_before, np.float64).reshape(B, 4, 3)
        want = host.sim_step_rows(run.X.astype(np.float64), run.params.astype(np.float64), index)
        assert np.array_equal(rows[:, :, 0], want[:, :, 0].astype(F32)), index                # the phase, np.round(.., 4)
        if index == 1:
            assert want[0, 0, 0] == np.round(np.fmod((steps + 1) * 1e-3, 0.5) / 0.5, 4)        # ... counted from the rollout's start
        floor = R.sim_rows_fp32(run.X, run.params, foot_before, True, dt_nodes=host.dt_nodes, sim_dt=host.sim_dt, steps=steps)
        for c in range(1, 19):
            mag = np.abs(want[:, :, c]).max()
            fl = np.abs(floor[:, :, c - 1].astype(np.float64) - want[:, :, c]).max()
            dv = np.abs(rows[:, :, c].astype(np.float64) - want[:, :, c]).max()
            table.append((index, c, mag, fl, dv))
            assert dv <= 4.0 * fl, (index, c, mag, fl, dv)
        # the plan's foot where the foot stands at the segment, foot_pos otherwise: both kinds occur among the rows
        seg = np.minimum(np.floor((np.arange(steps) + 1) * 1e-3 / host.dt_nodes + 1e-9).astype(int), N - 1)
        assert index == 1 or (run.params[0, seg, 0] > 0.5).any() and not (run.params[0, seg, 0] > 0.5).all()
    print("replan column magnitude fp32-floor device:\n" + "\n".join(f"{i} {c:2d} {m:.3e} {f:.3e} {d:.3e}" for i, c, m, f, d in table))
    # after the step of replan 0: plant = plan at node nodes_per_replan, plus the push impulse in fp32
    want_x = one.X[:, npr].copy()
    want_x[:, 6:9] = want_x[:, 6:9] + force.astype(F32) * F32(0.04) / F32(_mp(N)[1])
    assert np.array_equal(one.x, want_x)
    stands = one.params[:, npr, :4] > 0.5
    want_foot = np.where(stands[:, :, None], one.params[:, npr, 4:].reshape(B, 4, 3), foot0.astype(F32))
    assert np.array_equal(one.foot.astype(F32).reshape(B, 4, 3), want_foot) and stands[:, 0].all() and not stands.all()
    assert (want_foot[:, 0] != foot0.astype(F32)[:, 0]).any()                                  # the front left foot did touch down
    host.base_ref_vel_tracking = ref0.copy()
    host.increment_base_ref_position(steps)
    assert (np.abs(one.ref - host.base_ref_vel_tracking) <= steps * np.spacing(np.abs(host.base_ref_vel_tracking))).all()
    assert np.array_equal(one.ref[:, [2, 4, 5, 6, 7, 8, 9, 10, 11]], ref0[:, [2, 4, 5, 6, 7, 8, 9, 10, 11]])
    for run in (one, two):
        solver_bit = np.where(np.isin(run.status, (1, 4)), 1, 0)
        assert np.array_equal(run.failed, state_row_flags(run.S, v_des) | solver_bit)


def test_one_row_per_replan_is_the_state_before_the_step(dev):
    """record_sim_steps = 0: the row is `record_state` of the state the replan starts from, cast to fp32, with the phase that was
    passed in -- bit for bit (the base-to-foot differences of float32 numbers round once on both sides)."""
    gait, _ = _table("trot")
    B, N = 8, 50
    s = _solver(dev, N, B, gait)
    inp = _inputs(B, 21)
    t = _call(s, gait, inp, _cfg(gait, start_node=4, nodes_per_replan=2))
    host = R.host_mpc(B, "trot", N)
    host.foot_pos = inp["foot"]
    want = host.record_state(inp["x"], 0.0)
    want[:, 0] = PHASE
    assert t.S.shape == (B, 1, 19) and np.array_equal(t.S[:, 0], want.astype(F32))
    assert np.array_equal(t.x, t.X[:, 2])


LIM = F32(25.0) * F32(0.017453292519943295)
# (slot of x, threshold, the side that raises the flag: +1 above / -1 below, the bit)
THRESHOLDS = [(5, LIM, +1, 2), (5, -LIM, -1, 2), (4, LIM, +1, 4), (4, -LIM, -1, 4), (2, F32(0.18), -1, 8), (2, F32(0.45), +1, 8),
              (2, F32(0.08), -1, 32 | 8), (6, F32(0.10), +1, 16), (6, F32(-0.10), -1, 16), (7, F32(0.10), +1, 16), (7, F32(-0.10), -1, 16)]


def _straddle(v_des, side):
    """the two adjacent float32 velocities whose distance from the float32 command v_des lies on either side of 0.10f, on the
    `side` of the command: (inside, outside).  The differences are exact in fp32 and in fp64, so which side each lies on is
    settled in fp64 here, with no fp32 subtraction of the test's own."""
    thr, vd = float(F32(0.10)), float(F32(v_des))
    v = F32(vd + side * thr)
    while side * (float(v) - vd) > thr:
        v = np.nextafter(v, F32(vd))
    while side * (float(np.nextafter(v, F32(side * np.inf))) - vd) <= thr:
        v = np.nextafter(v, F32(side * np.inf))
    out = np.nextafter(v, F32(side * np.inf))
    assert side * (float(v) - vd) <= thr < side * (float(out) - vd)
    return float(v), float(out)


@pytest.mark.parametrize("terminate", [False, True])
def test_flags_on_both_sides_of_every_threshold(dev, terminate):
    """Two replans, one row each.  Rows 1 ..: the first recorded row one fp32 step inside, on and outside each threshold -- roll and
    pitch at 25 degrees, z at 0.18 and 0.45, the collision height, |v - v_des| at 0.10 under a zero command; then four rows under
    the command (0.25, -0.125, 0) with the velocity on either side of 0.10 from it (the cast of v_des and the fp32 subtraction);
    the last two rows are clean and are pushed over the first interval, so that they cross the velocity threshold in replan 1
    only.  Every rollout has a yaw rate and a reference yaw, and the call starts one node before the touch-down of feet 0 and 3, so
    a rollout that advances changes its ref_state and its foot_pos.
    failed = `state_row_flags` of the device's own rows, and the bits of the first row are the expected ones.  With terminate_mask
    set: the stamp is 1 + replan_index (1 and 2 occur), a rollout stamped 1 repeats its row and keeps x, foot_pos and ref_state,
    one stamped 2 has advanced once, the others twice."""
    from iterative_learning_nmpc_amd.mpc import TERM_SHIFT, state_row_flags
    gait, _ = _table("trot")
    node0 = int(np.flatnonzero((gait[0] == 1) & (np.roll(gait[0], 1) == 0))[0]) - 1
    n_thr = 3 * len(THRESHOLDS)
    N, B = 50, 1 + n_thr + 4 + 2
    command, late = np.arange(1 + n_thr, 5 + n_thr), np.arange(5 + n_thr, B)
    inp = _inputs(B, 2)
    inp["x"][:] = 0.0; inp["x"][:, 2] = R.widen(0.3)
    inp["v_des"][:] = 0.0; inp["w_des"][:] = 0.0; inp["w_des"][:, 2] = 0.25
    inp["ref"][:] = 0.0; inp["ref"][:, 3] = 0.125
    inp["foot"] = R.widen(np.tile(np.concatenate([HIPS, np.zeros((4, 1))], axis=1)[None], (B, 1, 1)))
    expect = np.zeros(B, np.int64)
    for i, (slot, thr, side, bit) in enumerate(THRESHOLDS):
        away = F32(side * np.inf)
        for j, v in enumerate((np.nextafter(thr, -away), thr, np.nextafter(thr, away))):     # inside, on, outside
            inp["x"][1 + 3 * i + j, slot] = float(v)
            expect[1 + 3 * i + j] = bit if j == 2 else (8 if bit == 32 | 8 else 0)          # (0.08 lies below 0.18 anyhow)
    inp["v_des"][command] = [0.25, -0.125, 0.0]
    inp["x"][command, 6:8] = [0.25, -0.125]
    inp["x"][command[0], 6], inp["x"][command[1], 6] = _straddle(0.25, +1)
    inp["x"][command[2], 7], inp["x"][command[3], 7] = _straddle(-0.125, -1)
    expect[command] = [0, 16, 0, 16]
    force = np.zeros((B, 3)); force[late[0]] = [60.0, 0.0, 0.0]; force[late[1]] = [0.0, -60.0, 0.0]      # 60 N x 0.04 s / 15 kg = 0.16 m/s
    s = _solver(dev, N, B, gait)
    mask = 0xFE if terminate else 0                                  # every flag of a state (the solver's own bit aside)
    t = _call(s, gait, inp, _cfg(gait, n_replans=2, start_node=node0, nodes_per_replan=2, terminate_mask=mask, push_duration=0.04), force)
    x0, foot0 = inp["x"].astype(F32), inp["foot"].astype(F32).reshape(B, 12)
    assert t.S.shape == (B, 2, 19)
    assert np.array_equal(t.S[:, 0, 7:11], x0[:, 2:6]) and np.array_equal(t.S[:, 0, 1:3], x0[:, 6:8])
    r0, r1 = state_row_flags(t.S[:, :1], inp["v_des"]), state_row_flags(t.S[:, 1:], inp["v_des"])
    assert np.array_equal(r0, expect), (r0, expect)
    dead0 = (r0 & mask) != 0
    dead1 = ~dead0 & ((r1 & mask) != 0)
    live = ~dead0 & ~dead1
    assert np.array_equal(t.failed & 0xFE, np.where(dead0, r0, r0 | r1) & 0xFE), (t.failed, r0, r1)
    assert np.array_equal(t.failed >> TERM_SHIFT, np.where(dead0, 1, np.where(dead1, 2, 0)))      # stamped 1 + replan_index
    assert (r1[late] & 16).all() and not r0[late].any() and live[0]
    if terminate:
        assert np.array_equal(dead0, expect != 0) and dead1[late].all()
    else:
        assert live.all()
    # ref_state, foot_pos and x after no, one and two steps
    host = R.host_mpc(B, "trot", N)
    host.v_des, host.w_des = inp["v_des"], inp["w_des"]
    after = [inp["ref"].copy()]
    for _ in range(2):
        host.base_ref_vel_tracking = after[-1].copy()
        host.increment_base_ref_position(40)
        after.append(host.base_ref_vel_tracking.copy())
    assert (after[1][:, 3] != after[0][:, 3]).all() and (after[2][:, 3] != after[1][:, 3]).all()
    assert (after[1][command, :2] != after[0][command, :2]).all()
    for rows, steps_taken in ((dead0, 0), (dead1, 1), (live, 2)):
        want = after[steps_taken][rows]
        assert (np.abs(t.ref[rows] - want) <= 40 * steps_taken * np.spacing(np.abs(want))).all(), steps_taken
    assert np.array_equal(t.S[dead0, 1], t.S[dead0, 0]) and (t.S[~dead0, 1] != t.S[~dead0, 0]).any(axis=1).all()
    assert np.array_equal(t.x[dead0], x0[dead0]) and np.array_equal(t.foot[dead0], foot0[dead0])
    moved = (t.foot != foot0).reshape(B, 4, 3)
    assert moved[~dead0][:, [0, 3], 2].all() and not moved[:, [1, 2]].any()       # feet 0 and 3 touched down: at the plan's height
    assert np.array_equal(t.x[dead1][:, 2:6], t.S[dead1, 1, 7:11]) and np.array_equal(t.x[dead1][:, 6:], t.S[dead1, 1, 1:7])
    assert np.array_equal(t.x[live], t.X[live, 2], equal_nan=True)
