"""Solve parity per problem and per slot group against the fp32 floor (tests/parity_groups.py).

The batch-level relative L2 of test_gpu_parity.py, test_gpu_wholebody.py and test_gpu_run_sweep.py is carried by the large
slots and by the many problems that are right.  The faults it cannot see are the ones this code can have: the linearisation
kernels run one thread per (problem, stage) in blocks of 64, so a problem's stages sit at another lane offset for every b
(51 b mod 64 at N = 50, 31 b mod 64 at N = 30); the QP kernels run one problem per wave; the momentum, base-rate and
Euler-angle slots are small against the joint and force slots.  Every case solves once on the device and once with each
oracle and asserts, for every problem b and every group g of X and of U,

    e_gpu[b, g] <= max(1e-5, 4 x max_b e32[b, g])

with e = relative L2 over the problem's horizon against the fp64 oracle and e32 the fp32 oracle's own (same inputs, same
run).  Status, iteration count and step length equal the fp64 oracle's per problem.  The table a case prints names the
worst problem of every group; measured maxima are quoted beside the cases in parity_groups.CASES and in DESIGN.md 2.
"""
import numpy as np
import pytest

from tests import parity_groups as pg
from tests.solve_helpers import dev, gpu_solve, make_solver  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", pg.CASES, ids=lambda c: c.name)
def test_solve_parity_per_problem_and_group(dev, oracle64, oracle32, monkeypatch, case):
    w = pg.workload(case, oracle64)
    gx, gu = pg.GROUPS[case.model]
    X64, U64, st64, stats64 = pg.oracle_solve(oracle64, case, w)
    # the reference solved the case (iteration limit, not a NaN step or a failed QP) and none of its group norms vanishes
    assert (st64 == 2).all() and np.isfinite(X64).all() and np.isfinite(U64).all()
    assert pg.denominators_ok(pg.group_errors(X64, X64, gx)[1]) and pg.denominators_ok(pg.group_errors(U64, U64, gu)[1])
    eX32, eU32 = pg.floors(pg.floor_runs(oracle32, case, w), X64, U64, gx, gu)
    barX, barU = pg.bars(eX32), pg.bars(eU32)

    out = {}
    for variant in case.variants:
        if variant is None:
            monkeypatch.delenv("NMPC_QP_VARIANT", raising=False)
        else:
            monkeypatch.setenv("NMPC_QP_VARIANT", variant)       # read by nmpc_create
        for allp in case.all_patterns:
            s = make_solver(w, case.B, dev, precision=case.precision, max_sqp_iter=case.sqp, n_ipm=case.n_ipm)
            if allp is not None:
                assert s.set_contact_patterns(all_patterns=allp) == allp
            out[variant, allp] = gpu_solve(s, w, shift=case.shift)

    failures = []
    for allp in case.all_patterns:                                # the tables first: a failing case prints all of them
        X, U, st, stats = out[case.variants[0], allp]
        tag = case.name if allp is None else f"{case.name}[all_patterns={allp}]"
        eX, eU = pg.group_errors(X, X64, gx)[0], pg.group_errors(U, U64, gu)[0]
        print(pg.report(tag, "X", gx, eX, eX32, barX))
        print(pg.report(tag, "U", gu, eU, eU32, barU))
        print(f"{tag}  batch figure: gpu X {pg.batch_rel(X, X64):.2e} U {pg.batch_rel(U, U64):.2e}")
        failures += [(tag, "X", list(gx)[g], b, eX[b, g], barX[g]) for b, g in pg.over_bar(eX, barX)]
        failures += [(tag, "U", list(gu)[g], b, eU[b, g], barU[g]) for b, g in pg.over_bar(eU, barU)]
    for allp in case.all_patterns:
        X, U, st, stats = first = out[case.variants[0], allp]
        for variant in case.variants[1:]:                         # resident against lean: bit for bit
            for a, b in zip(first, out[variant, allp]):
                assert np.array_equal(a, b), (variant, allp)
        assert np.array_equal(st, st64), allp
        assert np.array_equal(stats[:, 3], stats64[:, 3]), allp   # iteration count
        assert np.array_equal(stats[:, 2], stats64[:, 2]), allp   # step length
    assert not failures, failures
