"""Solve parity per problem and per slot group (helper module, not collected by pytest).

The solve tests of test_gpu_parity.py, test_gpu_wholebody.py and test_gpu_run_sweep.py assert one relative L2 norm over the
X (or U) tensor of the whole batch.  That norm is carried by the large slots and by the many problems that are right: on
wholebody_trot(B = 64, N = 30) the batch norm of X is about 280 while one problem's Euler angles have norm 0.67, so an
error of 4e-3 relative in them passes the 1e-5 batch bar.  Here the error is taken per problem b and per slot group g over
the problem's whole horizon,

    e[b, g] = || A[b, :, g] - ref[b, :, g] ||_2 / || ref[b, :, g] ||_2          (float64)

against the fp64 oracle, and held under

    bar[g] = max(1e-5, 4 x max_b e32[b, g])

where e32 is the fp32 oracle's own error on the same inputs: 1e-5 is the project's north-star bar, 4 x the float32
restatement the rule of the torque-layer and policy-gradient tests.  Every problem and every group is asserted.

Shared by tests/test_gpu_solve_groups.py (device) and tests/test_parity_groups.py (CPU: partition, denominators, sensitivity).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from tests import solve_helpers
from tests.solve_helpers import rel as batch_rel  # noqa: F401  the figure of the batch-level solve tests: relative L2 over the whole tensor

NORTH_STAR = 1e-5          # BASELINE.json north_star: relative L2 on trajectories
F32_FACTOR = 4.0           # the standing factor on the float32 restatement's own error
DEN_FLOOR = 1e-3           # every per-problem group norm of the reference >= this share of the group's batch median

# Slot groups, name -> (first, one past last).  Centroidal: DESIGN.md 3.2, x = [r, (yaw, pitch, roll), rdot, body rates],
# u = f[4][3].  Whole body: WQ = 0 / WV = 18 / WH = 36 and WA = 0 / WF = 18 of csrc/nmpc_wb_model.hpp, q = [r, Euler, joints].
GROUPS = {
    1: (dict(pos=(0, 3), rpy=(3, 6), v=(6, 9), w=(9, 12)), dict(f=(0, 12))),
    2: (dict(r=(0, 3), eul=(3, 6), qj=(6, 18), vb=(18, 24), vj=(24, 36), h=(36, 42)), dict(ab=(0, 6), aj=(6, 18), f=(18, 30))),
}


def group_errors(A, ref, groups):
    """e[b, g] and the denominators den[b, g] = || ref[b, :, g] ||_2, groups in the order of the dict"""
    A, ref = np.asarray(A, np.float64), np.asarray(ref, np.float64)
    assert A.shape == ref.shape and A.ndim == 3
    B = A.shape[0]
    e, den = np.zeros((B, len(groups))), np.zeros((B, len(groups)))
    for j, (lo, hi) in enumerate(groups.values()):
        den[:, j] = np.linalg.norm(ref[:, :, lo:hi].reshape(B, -1), axis=1)
        e[:, j] = np.linalg.norm((A[:, :, lo:hi] - ref[:, :, lo:hi]).reshape(B, -1), axis=1) / np.maximum(den[:, j], 1e-300)
    return e, den


def bars(e32):
    """bar[g] from the fp32 oracle's errors e32[b, g] (or a stack [copy, b, g] of them)"""
    e32 = np.asarray(e32, np.float64)
    return np.maximum(NORTH_STAR, F32_FACTOR * e32.reshape(-1, e32.shape[-1]).max(axis=0))


def denominators_ok(den):
    """the condition on the inputs: no per-problem group norm of the reference vanishes against the batch's"""
    return bool((den >= DEN_FLOOR * np.median(den, axis=0, keepdims=True)).all() and (den > 0).all())


def over_bar(e, bar):
    """[(problem, group index)] of every entry over its bar (NaN counts as over)"""
    return [(int(b), int(g)) for b, g in zip(*np.nonzero(~(e <= bar[None, :])))]


def report(case, tensor, groups, e_gpu, e32, bar):
    """The table the tests print: per group the device's median and maximum over the batch, the fp32 oracle's, the bar and
    the worst problem.  e32 may be a stack over perturbed copies."""
    e32 = np.asarray(e32).reshape(-1, *np.asarray(e32).shape[-2:]).max(axis=0)
    lines = [f"{case}  {tensor}: group   gpu median / max      f32 median / max      bar       worst b"]
    for j, g in enumerate(groups):
        worst = int(np.nanargmax(np.where(np.isnan(e_gpu[:, j]), np.inf, e_gpu[:, j])))
        flag = "  OVER" if not e_gpu[worst, j] <= bar[j] else ""
        lines.append(f"{case}  {tensor}.{g:<4} {np.median(e_gpu[:, j]):9.2e} / {e_gpu[:, j].max():9.2e}   "
                     f"{np.median(e32[:, j]):9.2e} / {e32[:, j].max():9.2e}   {bar[j]:9.2e}   {worst}{flag}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    model: int
    recipe: str                 # which input recipe of `workload` below
    B: int
    N: int
    seed: int
    n_ipm: int
    sqp: int
    precision: int = 0          # BatchedNmpcSolver(precision=...)
    variants: Tuple = (None,)   # NMPC_QP_VARIANT values solved (the first is group-checked, the others equal it bit for bit)
    all_patterns: Tuple = (None,)   # set_contact_patterns(all_patterns=...) values solved, each group-checked
    shift: int = 0              # folded warm-start shift (oracle: shift_warm_start, then solve)
    floor_copies: int = 0       # fp32-oracle runs on inputs perturbed by one float32 ulp that join the floor (max over runs)
    sqp_cpu: int = 0            # CPU denominator test only: a cheaper SQP count (whole body, sqp >= 15), 0 = the case's own


_BOTH = ("resident", "lean")
CASES = (
    # centroidal headline shapes: B = 64 is the smallest batch at which the lane offset 51 b mod 64 of a problem's stages in
    # the linearisation's blocks of 64 takes every value; policies as test_centroidal_solve_parity
    Case("cen_trot_ipm0_sqp1", 1, "cen_trot", 64, 50, 0, 0, 1, variants=_BOTH),      # measured, group closest to its bar (device max / fp32 oracle max / bar): X.w 1.6e-5 / 1.7e-5 / 7.0e-5
    Case("cen_trot_ipm6_sqp1", 1, "cen_trot", 64, 50, 0, 6, 1, variants=_BOTH),      # X.v 5.8e-6 / 6.0e-6 / 2.4e-5 (X.w 1.5e-5 / 2.1e-5 / 8.5e-5)
    Case("cen_trot_ipm6_sqp3", 1, "cen_trot", 64, 50, 0, 6, 3, variants=_BOTH),      # X.pos 1.5e-5 / 9.2e-6 / 3.7e-5, X.w 3.7e-5 / 3.0e-5 / 1.2e-4: problem 31 in every group, for both
    Case("cen_trot_ipm6_sqp15", 1, "cen_trot", 64, 50, 0, 6, 15, variants=_BOTH),      # X.w 3.4e-6 / 3.0e-6 / 1.2e-5
    # binding friction pyramid (test_centroidal_active_friction)
    Case("cen_friction", 1, "cen_friction", 32, 50, 1, 6, 1),      # X.w 6.7e-5 / 5.8e-5 / 2.3e-4, U.f 2.1e-5 / 1.9e-5 / 7.5e-5 (problem 3)
    # every subset of the four feet, default kernel and all-patterns kernel (test_all_contact_patterns_kernel_...)
    Case("cen_patterns", 1, "cen_patterns", 24, 50, 23, 6, 1, all_patterns=(False, True)),      # X.w 9.4e-6 / 1.1e-5 / 4.5e-5 (default), X.rpy 6.0e-6 / 7.2e-6 / 2.9e-5 (all patterns)
    # ragged: beyond one stage per lane, and a short horizon with an odd batch
    Case("cen_ragged_b5_n70", 1, "cen_trot", 5, 70, 11, 6, 2),      # X.w 2.0e-6 / 3.6e-6 / 1.5e-5
    Case("cen_ragged_b3_n7", 1, "cen_trot", 3, 7, 11, 6, 2),      # X.w 3.6e-6 / 4.5e-6 / 1.8e-5
    # whole body: 31 b mod 64 takes every lane offset at B = 64; policies as test_wholebody_solve_parity
    Case("wb_trot_ipm0_sqp1", 2, "wb_trot", 64, 30, 0, 0, 1),      # U.f 5.5e-6 / 4.3e-6 / 1.7e-5 (U.ab 2.7e-5 / 2.3e-5 / 9.2e-5)
    Case("wb_trot_ipm6_sqp1", 2, "wb_trot", 64, 30, 0, 6, 1),      # U.ab 3.6e-5 / 2.2e-5 / 8.9e-5, X.h 2.8e-5 / 3.0e-5 / 1.2e-4
    Case("wb_trot_ipm6_sqp3", 2, "wb_trot", 64, 30, 0, 6, 3),      # U.ab 5.2e-6 / 4.9e-6 / 2.0e-5
    Case("wb_trot_ipm6_sqp15", 2, "wb_trot", 64, 30, 0, 6, 15, sqp_cpu=3),      # U.ab 5.3e-6 / 4.7e-6 / 1.9e-5
    # the shipped mixed-precision contraction (three-way split bf16)
    Case("wb_trot_precision3", 2, "wb_trot", 64, 30, 0, 6, 1, precision=3),      # U.ab 3.1e-5 / 2.2e-5 / 8.9e-5
    Case("wb_pyramid", 2, "wb_pyramid", 32, 30, 3, 6, 4),      # U.ab 5.0e-6 / 4.6e-6 / 1.8e-5
    Case("wb_patterns", 2, "wb_patterns", 48, 30, 13, 6, 2),      # X.h 1.5e-5 / 9.2e-6 / 3.7e-5
    # ragged, the reference's own horizon, either side of the LDS budget of the backward gains (43 | 44), lane = stage limit
    Case("wb_ragged_b3_n25", 2, "wb_trot", 3, 25, 7, 6, 2),      # X.eul 4.3e-6 / 2.8e-6 / 1.1e-5
    Case("wb_ragged_b2_n43", 2, "wb_trot", 2, 43, 7, 6, 2),      # U.aj 3.8e-6 / 3.4e-6 / 1.3e-5
    Case("wb_ragged_b2_n44", 2, "wb_trot", 2, 44, 7, 6, 2),      # U.aj 2.8e-6 / 2.5e-6 / 1.0e-5
    Case("wb_ragged_b2_n64", 2, "wb_trot", 2, 64, 7, 6, 2),      # U.aj 3.2e-6 / 3.7e-6 / 1.5e-5
    # folded warm-start shift of a previous solution (test_wholebody_warm_start_shift_folded)
    Case("wb_shift2", 2, "wb_shift", 16, 30, 5, 6, 1, shift=2),      # X.qj 3.2e-6 / 2.6e-6 / 1.0e-5
)


def workload(case, oracle64=None):
    """The case's inputs, by the recipes of the batch-level tests.  `wb_shift` needs the fp64 oracle: its warm start is the
    oracle's solution of the unshifted problem, rounded to float32 so that device and oracles read the same numbers."""
    from iterative_learning_nmpc_amd import workloads as wl
    B, N = case.B, case.N
    if case.recipe == "cen_trot":
        return wl.centroidal_trot(B=B, N=N, seed=case.seed)
    if case.recipe == "cen_friction":
        w = wl.centroidal_trot(B=B, N=N, seed=case.seed)
        w.mp[6] = 0.3
        return w
    if case.recipe == "cen_patterns":
        w = wl.centroidal_trot(B=B, N=N, seed=case.seed)
        rng = np.random.default_rng(7)
        flags = rng.integers(0, 2, size=(B, N + 1, 4)).astype(np.float32)
        flags[:, :, :][flags.sum(-1) == 0] = np.array([1, 0, 0, 1], np.float32)        # keep some support most of the time
        flags[:, ::7] = 0.0                                                              # ... and some flight stages
        w.params[:, :, 0:4] = flags
        n_st = np.maximum(flags[:, :N].sum(-1, keepdims=True), 1.0)
        fz = (-w.mp[5] * w.mp[1]) / n_st                                                 # weight shared by the stance feet
        for i in range(4):
            w.yref[:, :, 12 + 3 * i: 14 + 3 * i] = 0.0
            w.yref[:, :, 14 + 3 * i] = (fz[..., 0] * flags[:, :N, i]).astype(np.float32)
        w.U[:] = w.yref[:, :, 12:]
        assert len(np.unique((flags[:, :N] * np.array([1, 2, 4, 8])).sum(-1))) == 16
        return w
    if case.recipe in ("wb_trot", "wb_shift"):
        w = wl.wholebody_trot(B=B, N=N, seed=case.seed)
        if case.recipe == "wb_shift":
            X1, U1, st1, _ = oracle_solve(oracle64, dataclasses.replace(case, shift=0), w)
            assert (st1 == 2).all()
            w.X, w.U = X1.astype(np.float32).astype(np.float64), U1.astype(np.float32).astype(np.float64)
        return w
    if case.recipe == "wb_pyramid":
        w = wl.wholebody_trot(B=B, N=N, seed=case.seed)
        w.mp = w.mp.copy(); w.mp[6] = 0.15
        w.yref = w.yref.copy(); w.yref[:, :, 6] = 1.0
        return w
    if case.recipe == "wb_patterns":
        w = wl.wholebody_trot(B=B, N=N, seed=case.seed)
        rng = np.random.default_rng(5)
        c = (rng.random((B, N + 1, 4)) < 0.6).astype(np.float64)
        c[: B // 3] = w.params[: B // 3, :, :4]                                  # a third keeps its trot schedule
        w.params = w.params.copy()
        w.params[:, :, :4] = c
        w.params[:, :, 4:8] = 1.0 - c
        n_st = np.maximum(c[:, :N].sum(-1, keepdims=True), 1.0)
        w.U = w.U.copy(); w.yref = w.yref.copy()
        w.U[:, :, 18:] = 0.0
        w.U[:, :, 20::3] = c[:, :N] * (-w.mp[5] * w.mp[1]) / n_st
        w.yref[:, :, 52:64] = w.U[:, :, 18:]
        return w
    raise ValueError(case.recipe)


def oracle_solve(o, case, w, sqp=None):
    """(X, U, status, stats) of oracle `o` on the case: the warm start shifted first where the case folds a shift"""
    X, U = w.X, w.U
    if case.shift:
        X, U = o.shift_warm_start(X, U, case.shift)
    return solve_helpers.oracle_solve(o, w, X, U, max_sqp_iter=case.sqp if sqp is None else sqp, n_ipm=case.n_ipm)


def ulp_copy(w, k):
    """copy k of the inputs with x0, X and U moved by one float32 ulp of random sign (a second draw of float32 rounding)"""
    rng = np.random.default_rng(1000 + k)

    def nudge(a):
        a32 = np.asarray(a, np.float32)
        up = rng.integers(0, 2, a32.shape).astype(bool)
        return np.where(up, np.nextafter(a32, np.float32(np.inf)), np.nextafter(a32, np.float32(-np.inf))).astype(np.float64)
    return dataclasses.replace(w, x0=nudge(w.x0), X=nudge(w.X), U=nudge(w.U))


def floor_runs(oracle32, case, w, sqp=None):
    """[(X32, U32)]: the fp32 oracle on the case's inputs and on its `floor_copies` perturbed copies -- all of them are
    compared with the fp64 oracle on the unperturbed inputs"""
    runs = [oracle_solve(oracle32, case, w, sqp)[:2]]
    for k in range(case.floor_copies):
        runs.append(oracle_solve(oracle32, case, ulp_copy(w, k), sqp)[:2])
    return runs


def floors(runs, X64, U64, gx, gu):
    """e32 stacks [run, b, g] for X and U"""
    return (np.stack([group_errors(X, X64, gx)[0] for X, _ in runs]), np.stack([group_errors(U, U64, gu)[0] for _, U in runs]))
