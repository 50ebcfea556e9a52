"""The backward sweep of the centroidal QP kernel walks the horizon in runs of one contact pattern (a stage body is chosen once
per run, the stage in front of a touch-down is a run of its own, patterns without a static body form runs of the run-time
fallback).  Contact schedules that hit every edge of that run logic, each solved by the resident and the lean variant of the
default kernel and by the all-patterns kernel, against the fp64 oracle.

Tolerances are those of tests/test_gpu_parity.py: status equal and 1e-5 relative L2 on X (or 1.5 x the fp32 oracle's own error,
`within_tolerance`) and on U against the fp64 oracle, as test_centroidal_solve_parity; 3e-5 between the default and the
all-patterns kernel, as test_all_contact_patterns_kernel_matches_default_and_oracle.  Every schedule was first solved by the
fp64 oracle alone: no failed problem, finite trajectories (asserted again here, so the reference stays inside the comparison).
"""
import numpy as np
import pytest

from tests.solve_helpers import dev, gpu_solve, make_solver, oracle_solve, rel, within_tolerance  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


B = 8
# stance flags of the four feet, foot f = bit f of the pattern number (Centroidal::static_mask)
TROT_A, TROT_B, STANCE, FLIGHT, ONE_FOOT, THREE_FEET = 0b1001, 0b0110, 0b1111, 0b0000, 0b0001, 0b0111

# name -> pattern of stage 0 .. N-1 (the sweep walks them from the back)
SCHEDULES = {
    # one pattern throughout: a single run of odd / even length, a tail with and without a pair in front of it
    "one_pattern_n1": [TROT_A] * 1,
    "one_pattern_n2": [TROT_A] * 2,
    "one_pattern_n3": [TROT_A] * 3,
    "one_pattern_n8": [TROT_A] * 8,
    # another pattern at every stage: all runs have length 1
    "every_stage_differs_n5": [TROT_A, TROT_B, STANCE, TROT_A, TROT_B],
    # run lengths 2, 3, 1, 2: narrow-to-wide transitions (the stage in front of a touch-down, a run of its own) and wide-to-narrow
    "runs_2_3_1_2_n8": [TROT_A] * 2 + [STANCE] * 3 + [TROT_B] * 1 + [TROT_A] * 2,
    # patterns outside the default kernel's short list between static ones: runs of the run-time fallback
    "fallback_between_static_n8": [TROT_A] * 2 + [ONE_FOOT] * 2 + [STANCE] + [THREE_FEET] + [TROT_B] * 2,
    # flight in the middle and at the end of the horizon
    "flight_n8": [TROT_A] * 2 + [FLIGHT] * 2 + [TROT_B] * 2 + [FLIGHT] * 2,
    # a horizon beyond one stage per lane; the last run (stages 60..69) crosses stage 64
    "runs_across_64_n70": [TROT_A] * 12 + [TROT_B] * 12 + [STANCE] * 12 + [TROT_A] * 12 + [TROT_B] * 12 + [TROT_A] * 10,
}


def _workload(schedule):
    """centroidal_trot with the contact flags of `schedule` at every node (node N repeats the last stage) and the force
    reference and warm start that go with them: the weight shared by the stance feet.  A horizon below the headline's 50 is
    the first N stages of that workload (same time step; the gait planner has no nodes at a step of T / N for N = 1, 2)."""
    import dataclasses
    from iterative_learning_nmpc_amd import workloads as wl
    N = len(schedule)
    w = wl.centroidal_trot(B=B, N=max(N, 50), seed=31)
    if N < w.N:
        w = dataclasses.replace(w, N=N, yref=w.yref[:, :N].copy(), params=w.params[:, :N + 1].copy(),
                                X=w.X[:, :N + 1].copy(), U=w.U[:, :N].copy())
    pat = np.asarray(schedule + schedule[-1:])
    flags = ((pat[:, None] >> np.arange(4)) & 1).astype(np.float64)              # [N+1, 4]
    w.params[:, :, 0:4] = flags[None]
    share = (-w.mp[5] * w.mp[1]) / np.maximum(flags[:N].sum(-1), 1.0)
    w.yref[:, :, 12:] = 0.0
    w.yref[:, :, 14::3] = (share[:, None] * flags[:N])[None]
    w.U[:] = w.yref[:, :, 12:]
    return w


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_run_sweep_schedule(dev, oracle64, oracle32, monkeypatch, name):
    w = _workload(SCHEDULES[name])
    X64, U64, st64, _ = oracle_solve(oracle64, w)
    X32, U32, _, _ = oracle_solve(oracle32, w)
    # the reference itself solved the schedule: one SQP iteration without a tolerance ends as "iteration limit" (2), a
    # failed QP (4) or a NaN step (1) would not
    assert (st64 == 2).all() and np.isfinite(X64).all() and np.isfinite(U64).all()
    out = {}
    for variant in ("resident", "lean"):
        monkeypatch.setenv("NMPC_QP_VARIANT", variant)       # read by nmpc_create
        for allp in (False, True):
            s = make_solver(w, B, dev)
            assert s.set_contact_patterns(all_patterns=allp) == allp
            out[variant, allp] = gpu_solve(s, w)
    floor = rel(X32, X64)
    for key, (X, U, st, _) in out.items():
        eX, eU = rel(X, X64), rel(U, U64)
        print(f"{name} {key}: gpu-vs-f64 X {eX:.2e} U {eU:.2e}; f32-vs-f64 X {floor:.2e} U {rel(U32, U64):.2e}")
    for key, (X, U, st, _) in out.items():
        assert np.array_equal(st, st64), key
        assert within_tolerance(rel(X, X64), floor) and rel(U, U64) < 1e-5, (key, rel(X, X64), rel(U, U64), floor)
    for allp in (False, True):                                # resident against lean: bit for bit
        for a, b in zip(out["resident", allp], out["lean", allp]):
            assert np.array_equal(a, b), allp
    for variant in ("resident", "lean"):                      # default kernel against the all-patterns kernel
        assert rel(out[variant, True][0], out[variant, False][0]) < 3e-5
        assert rel(out[variant, True][1], out[variant, False][1]) < 3e-5
