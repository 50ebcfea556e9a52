"""The articulated momentum model of the whole-body solve (nmpc_wb_set_momentum_model) on the device, against
tests/wb_momentum_reference.py (tied to the fp64 oracle and to central differences in tests/test_wb_momentum_reference.py).

Records      after one linearisation the momentum rows of the defect, d h_ang+ / d q, d h_ang+ / d f (the node records of the
             workspace) and the dense consistency record match reference (a) at the torque layer's bar,
             max(1e-5 of the largest |reference| of the group, 4 x the deviation of the float32-data reference from the fp64 one),
             on the tilted tree, with and without a folded warm-start shift, and with the base 100 m away in x and y against
             the reference AT HOME for the blocks the base position must not enter.
One step     max_sqp_iter = 1, max_qp_iter = 0, line_search = 0, precision 0 against reference (b), per problem and per slot
             group: relative L2 <= max(1e-5, 4 x floor), floor = the larger of the frozen fp32 oracle's own error in that group in
             the declared mode and the error of reference (b) fed with the float32-data quantities of (a); neither involves the
             device.  Measured tables: DESIGN.md 2.
Declared     a handle switched to the articulated mode and back gives the bits of a fresh handle (precision 0 and 3).
Single body  the articulated mode on a tree of one body equals the declared mode on the device within the bar above.
Policy       1 SQP x 6 IPM (the benchmark's policy) at B = 64, N = 30: statuses, bit reproducibility, independence of the batch.
             There is no reference for this policy: a property test only.
Refusals     the entry points that build x0 from the declared map, and the argument errors of the setter."""
import ctypes
import dataclasses

import numpy as np
import pytest

from iterative_learning_nmpc_amd import workloads as wl
from iterative_learning_nmpc_amd.workloads import quadruped_tree
from tests import parity_groups as pg
from tests import solve_helpers as sh
from tests import wb_momentum_reference as mr
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import held, layer

pytestmark = pytest.mark.gpu
GX, GU = pg.GROUPS[2]
H_POS = [36, 37, 40, 41, 44, 45]            # positions of the momentum states in the 48-wide defect (pos_of, nmpc_wb_layout.hpp)
R_D, R_HQ, R_HF = 0, 48, 96                 # offsets in the node record


@pytest.fixture(scope="module")
def problem():
    return mr.small_problem()


@pytest.fixture(scope="module")
def trees():
    return {"plain": mr.tree_model(quadruped_tree()), "tilted": mr.tree_model(quadruped_tree(seed=4, perturb=0.1)),
            "single": mr.tree_model(mr.single_body_tree())}


def one_step(w, dev, model="declared", m=None, precision=0, n_ipm=0, shift=0, B=None):
    s = sh.make_solver(w, w.B if B is None else B, dev, precision=precision, n_ipm=n_ipm)
    L = None
    if model == "articulated":
        L = layer(m)
        s.set_momentum_model("articulated", torque_layer=L)
    X, U, st, _ = sh.gpu_solve(s, w, shift=shift)
    return s, L, X, U, st


def node_blocks(w, X, U, m, data):
    """reference (a) of every stage of iterate X, U: defect of h [B, N, 6], d h_ang+ / d q [B, N, 3, 15], d h_ang+ / d f
    [B, N, 3, 12], and the scaled consistency rows [B, N+1, 6, 35] in the dense record's order"""
    B, N = w.B, w.N
    d, hq, hf, dc = np.zeros((B, N, 6)), np.zeros((B, N, 3, 15)), np.zeros((B, N, 3, 12)), np.zeros((B, N + 1, 6, 35))
    for b in range(B):
        for k in range(N + 1):
            term = k == N
            Wk = w.W_e if term else w.W
            n = mr.node(w.mp, X[b, k], None if term else U[b, k], w.params[b, k], w.yref_e[b] if term else w.yref[b, k], Wk,
                        "articulated", m, data)
            dc[b, k] = mr.reference_dense_consistency(n)[:, :35]
            if not term:
                xn = np.asarray(X[b, k + 1], np.float32 if data == "f32" else np.float64).astype(np.float64)
                d[b, k] = n["xn"][36:42] - xn[36:42]
                hq[b, k] = n["A"][39:42, 3:18]; hf[b, k] = n["B"][39:42, 18:30]
    return d, hq, hf, dc


def device_blocks(s, B, N):
    lay = s.debug_wb_layout()
    d, hq, hf, dc = np.zeros((B, N, 6)), np.zeros((B, N, 3, 15)), np.zeros((B, N, 3, 12)), np.zeros((B, N + 1, 6, 35))
    for b in range(B):
        for k in range(N + 1):
            dc[b, k] = s.debug_momentum(b, k)[1].reshape(6, 36)[:, :35]
            if k < N:
                rec = s.debug_workspace(b, lay["rec"] + k * lay["REC"], lay["REC"])
                d[b, k] = rec[R_D:R_D + 48][H_POS]
                hq[b, k] = rec[R_HQ:R_HQ + 48].reshape(3, 16)[:, :15]
                hf[b, k] = rec[R_HF:R_HF + 36].reshape(3, 12)
    return d, hq, hf, dc


@pytest.mark.parametrize("shift", (0, 1))
def test_records_match_the_reference_on_the_tilted_tree(dev, problem, trees, shift):
    w, m = problem, trees["tilted"]
    s, L, _, _, _ = one_step(w, dev, "articulated", m, shift=shift)
    got = device_blocks(s, w.B, w.N)
    Xs, Us = mr.oracle("f64").shift_warm_start(w.X, w.U, shift) if shift else (w.X, w.U)
    ref, f32 = node_blocks(w, Xs, Us, m, "f64"), node_blocks(w, Xs, Us, m, "f32")
    ok = [held(name, g, r, f) for name, g, r, f in zip(("defect h", "dh_ang/dq", "dh_ang/df", "consistency"), got, ref, f32)]
    assert all(ok)
    assert np.abs(ref[1]).max() > 0.1 and np.abs(ref[3][..., :33]).max() > 1.0      # the blocks are not trivially small


def test_records_do_not_see_the_base_position(dev, problem, trees):
    w, m = problem, trees["tilted"]
    far = dataclasses.replace(w, X=w.X.copy(), x0=w.x0.copy())
    far.X[:, :, 0:2] += 100.0; far.x0[:, 0:2] += 100.0
    s, L, _, _, _ = one_step(far, dev, "articulated", m)
    got = device_blocks(s, w.B, w.N)
    ref, f32 = node_blocks(w, w.X, w.U, m, "f64"), node_blocks(w, w.X, w.U, m, "f32")      # the reference at home
    ok = [held("defect h_ang", got[0][..., 3:], ref[0][..., 3:], f32[0][..., 3:])]
    ok += [held(name, g, r, f) for name, g, r, f in zip(("dh_ang/dq", "dh_ang/df", "consistency"), got[1:], ref[1:], f32[1:])]
    assert all(ok)


def floors(w, m_art):
    """the two floors of the one-step bar, per group: (X [groups], U [groups])"""
    o64, o32 = mr.oracle("f64"), mr.oracle("f32")
    X64, U64, _, _ = sh.oracle_solve(o64, w, n_ipm=0)
    X32, U32, _, _ = sh.oracle_solve(o32, w, n_ipm=0)
    Xr, Ur = mr.gn_step(w, "articulated", m_art)
    Xf, Uf = mr.gn_step(w, "articulated", m_art, data="f32")
    fx = np.maximum(pg.group_errors(X32, X64, GX)[0].max(0), pg.group_errors(Xf, Xr, GX)[0].max(0))
    fu = np.maximum(pg.group_errors(U32, U64, GU)[0].max(0), pg.group_errors(Uf, Ur, GU)[0].max(0))
    return (Xr, Ur), np.maximum(pg.NORTH_STAR, pg.F32_FACTOR * fx), np.maximum(pg.NORTH_STAR, pg.F32_FACTOR * fu)


def table(name, groups, e, bar):
    print(f"  {name}: " + "  ".join(f"{g} {e[:, j].max():.2e}/{bar[j]:.2e}" for j, g in enumerate(groups)))


@pytest.mark.parametrize("tree", ("plain", "tilted"))
def test_one_step_solve_matches_the_reference_per_problem_and_group(dev, problem, trees, tree):
    w, m = problem, trees[tree]
    (Xr, Ur), bx, bu = floors(w, m)
    _, L, X, U, _ = one_step(w, dev, "articulated", m)
    eX, eU = pg.group_errors(X, Xr, GX)[0], pg.group_errors(U, Ur, GU)[0]
    table(f"{tree} X (device max / bar)", GX, eX, bx); table(f"{tree} U (device max / bar)", GU, eU, bu)
    assert not pg.over_bar(eX, bx) and not pg.over_bar(eU, bu)


def test_single_body_tree_equals_the_declared_mode(dev, problem, trees):
    w = problem
    m1 = mr.tree_model(mr.single_body_tree(float(w.mp[1]), w.mp[2:5]))
    _, bx, bu = floors(w, m1)
    _, _, Xd, Ud, _ = one_step(w, dev)
    _, L, Xa, Ua, _ = one_step(w, dev, "articulated", m1)
    eX, eU = pg.group_errors(Xa, Xd, GX)[0], pg.group_errors(Ua, Ud, GU)[0]
    table("single body X (device max / bar)", GX, eX, bx); table("single body U (device max / bar)", GU, eU, bu)
    assert not pg.over_bar(eX, bx) and not pg.over_bar(eU, bu)


@pytest.mark.parametrize("precision", (0, 3))
def test_declared_mode_is_untouched_by_a_visit_to_the_articulated_mode(dev, problem, trees, precision):
    w = problem
    _, _, X0, U0, st0 = one_step(w, dev, precision=precision, n_ipm=6)
    s = sh.make_solver(w, w.B, dev, precision=precision, n_ipm=6)
    L = layer(trees["plain"])
    s.set_momentum_model("articulated", torque_layer=L)
    Xa, _, _, _ = sh.gpu_solve(s, w)
    s.set_momentum_model("declared")
    X1, U1, st1, _ = sh.gpu_solve(s, w)
    assert np.array_equal(X0.view(np.int32), X1.view(np.int32)) and np.array_equal(U0.view(np.int32), U1.view(np.int32))
    assert np.array_equal(st0, st1)
    assert not np.array_equal(Xa, X1)      # the visit did solve another model


def test_full_policy_properties(dev, trees):
    """1 SQP x 6 IPM at B = 64, N = 30 (B = 65 for the batch independence).  No reference exists for this policy."""
    w = wl.wholebody_trot(B=65, N=30, seed=3)
    s = sh.make_solver(w, 65, dev)
    L = layer(trees["plain"])
    s.set_momentum_model("articulated", torque_layer=L)
    cut = lambda n0, n1: dataclasses.replace(w, **{k: getattr(w, k)[n0:n1] for k in ("x0", "yref", "yref_e", "params", "X", "U")})      # noqa: E731
    # The benchmark leaves nlp_tol at 0.  There the QP kernel of either momentum model reports NMPC_STATUS_MAXITER (2) for a
    # healthy solve -- NMPC_STATUS_OK (0) is only given against a step tolerance -- and the benchmark counts NaN (1) and QP (4)
    # as failures.  So "every solve is healthy" is: every status is exactly MAXITER.  (The whole-body model takes full steps: it
    # refuses line_search = 1 in both modes, so the policy runs with the line search off, as the benchmark runs it.)
    X, U, st, _ = sh.gpu_solve(s, cut(0, 64))
    assert np.array_equal(st, np.full(64, 2, np.int32)) and np.isfinite(X).all() and np.isfinite(U).all()
    # the status channel itself: given a tolerance that any finite step meets, the same solves report NMPC_STATUS_OK, same bits
    s.set_nlp_tol(1e30)
    Xt, Ut, stt, _ = sh.gpu_solve(s, cut(0, 64))
    s.set_nlp_tol(0.0)
    assert np.array_equal(stt, np.zeros(64, np.int32))
    assert np.array_equal(X.view(np.int32), Xt.view(np.int32)) and np.array_equal(U.view(np.int32), Ut.view(np.int32))
    X2, U2, st2, _ = sh.gpu_solve(s, cut(0, 64))
    assert np.array_equal(X.view(np.int32), X2.view(np.int32)) and np.array_equal(U.view(np.int32), U2.view(np.int32))
    Xa, Ua, sta, _ = sh.gpu_solve(s, w)
    X1, U1, st1, _ = sh.gpu_solve(s, cut(64, 65))
    assert np.array_equal(Xa[:64].view(np.int32), X.view(np.int32))
    assert np.array_equal(Xa[64:].view(np.int32), X1.view(np.int32)) and np.array_equal(Ua[64:].view(np.int32), U1.view(np.int32))
    assert sta[64] == st1[0] == 2


def test_refusals(dev, problem, trees):
    from iterative_learning_nmpc_amd import _lib
    from tests import fd_reference as fr
    w = problem
    s = sh.make_solver(w, w.B, dev)
    lib = s.lib
    L = layer(trees["plain"])
    E_ARG, E_STATE = -1, -3
    # argument errors of the setter
    assert lib.nmpc_wb_set_momentum_model(s._h, L._h, 2) == E_ARG
    assert lib.nmpc_wb_set_momentum_model(s._h, None, 1) == E_ARG
    wc = wl.centroidal_trot(B=2, N=10)
    assert lib.nmpc_wb_set_momentum_model(sh.make_solver(wc, 2, dev)._h, L._h, 1) == E_ARG           # not model 2
    L23 = layer(fr.random_tree())
    assert lib.nmpc_wb_set_momentum_model(s._h, L23._h, 1) == E_ARG                                   # not 18 joints
    assert b"18" in lib.nmpc_last_error(s._h)
    t0 = {k: np.array(v, copy=True) for k, v in quadruped_tree().items()}
    t0["mass"] = np.zeros(18)
    L0 = layer(mr.tree_model(t0))
    assert lib.nmpc_wb_set_momentum_model(s._h, L0._h, 1) == E_ARG                                    # massless
    assert b"mass" in lib.nmpc_last_error(s._h)
    # the declared-map entry points in the articulated mode: refused on the host, before any argument is read
    assert s.momentum_model == "declared"      # a fresh solver says so
    s.set_momentum_model("articulated", torque_layer=L)
    # ... with real, minimal arguments through the Python layer: were the refusal ever to move behind the launches, this is a
    # failed assertion, not a stray pointer
    import torch
    from iterative_learning_nmpc_amd._lib import NmpcError
    B, N = w.B, w.N
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
    gait, peaks = torch.ones(4, 4, dtype=torch.int8, device=dev), z(4, 4, dtype=torch.int8)
    q = s.to_device(w.x0[:, :18]); v = z(B, 18)
    f64 = lambda *shape: z(*shape, dtype=torch.float64)                                        # noqa: E731
    fill = lambda struct, **kw: {f: kw.get(f, 1 if t is ctypes.c_int else 1.0) for f, t in struct._fields_}      # noqa: E731
    with pytest.raises(NmpcError, match="declared map"):
        s.wb_rollout(gait, peaks, [0], q, v, f64(B, 3), f64(B, 3), f64(B, 12), z(12), None, z(B, N + 1, 42), z(B, N, 30),
                     z(B, dtype=torch.int32), **fill(_lib.NmpcWbRolloutCfg, nodes_per_cycle=4, last_node=0, terminate_mask=0))
    cfg = fill(_lib.NmpcWbLabelCfg, nodes_per_cycle=4, terminate_mask=0); del cfg["n_rows"]
    with pytest.raises(NmpcError, match="declared map"):
        s.label_states(L, gait, peaks, z(1, dtype=torch.int32), z(1, dtype=torch.int32), q[:, None, :].contiguous(),
                       v[:, None, :].contiguous(), f64(B, 3), f64(B, 3), f64(B, 12), z(12), z(1, dtype=torch.int32), **cfg)
    # back in the declared mode the refusal is gone (the call then fails on its arguments instead)
    s.set_momentum_model("declared")
    assert s.momentum_model == "declared"
    with pytest.raises(ValueError):
        s.set_momentum_model("articulated")
    with pytest.raises(ValueError):
        s.set_momentum_model("rigid")


def test_facade_takes_the_momentum_of_the_tree(dev, trees):
    """`QuadrupedAcadosSolver(momentum_model="articulated")` at batch 1 through `LocomotionMPC`: x0's h is the tree's momentum
    (crba_reference) at the layer's bar, and `solve()` on the standing pose returns finite arrays with status 0.
    The standing pose is solved as the controller's first solve (N_SQP_FIRST = 15 iterations) with the force reference that
    lets the robot stand, `force_reference="gravity_share"` (with the reference's zero force reference the soft stance penalty
    lets the base sag: quadruped_solver.py).  Measured, SQP iterations until max|step| < nlp_tol, declared / articulated:
    gravity_share 7 / 7; zero 12 / 21 -- under the zero reference the articulated mode converges too, beyond the 15 of a first
    solve (status 2 at 15, 0 at 21)."""
    from iterative_learning_nmpc_amd import wholebody as wbm
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    from tests import crba_reference as cr
    m = trees["plain"]
    L = layer(m)
    mpc = LocomotionMPC(print_info=False, batch=1, device=dev, momentum_model="articulated", torque_layer=L,
                        force_reference="gravity_share")
    fs = mpc.solver
    assert fs.momentum_model == mpc.momentum_model == "articulated" and fs.dyn.torque_layer is L
    # a moving state: x0's h against the reference
    rng = np.random.default_rng(7)
    q = np.zeros(18); q[2] = 0.29; q[3:6] = rng.normal(0, 0.05, 3); q[6:] = wbm.Q_HOME + rng.normal(0, 0.1, 12)
    v = rng.normal(0, 0.3, 18)
    q, v = q.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)
    fs.init(*mpc.solver_inputs(q, v))
    h0 = fs.pack_problem()["x0"][0, 36:]
    ref, f32 = cr.crba(m, q, v)[2], cr.crba(m, q, v, np.float32)[2]
    assert held("x0 h", h0, ref, f32)
    assert np.abs(h0 - wbm.centroidal_momentum(q, v, 15.0, [0.11, 0.27, 0.33])).max() > 1e-2      # not the declared map's
    # the standing pose: one solve
    mpc.reset()
    q = np.zeros(18); q[2] = 0.30; q[6:] = wbm.Q_HOME
    mpc.set_convergence_on_first_iter()      # the first solve's policy, as `open_loop` sets it
    out = mpc.optimize(q, np.zeros(18))
    assert all(np.isfinite(a).all() for a in out)
    assert fs._device_solver().momentum_model == "articulated"
    assert int(np.asarray(fs.status).reshape(-1)[0]) == 0
    # the host-driven receding horizon runs in this mode (one replan, a few simulation steps)
    mpc.reset()
    assert np.isfinite(mpc.open_loop(q, np.zeros(18), 0.003)).all()
    # the device rollouts and labels build x0 from the declared map
    with pytest.raises(RuntimeError, match="declared map"):
        mpc.open_loop_device(q, np.zeros(18), 0.02)
    with pytest.raises(ValueError):
        LocomotionMPC(print_info=False, momentum_model="articulated")
