"""The three entry points of csrc/nmpc_aux.hip.inc at the limits include/nmpc.h and the host guards state for them:
nmpc_riccati_batch at the edges of its 16x16 tile and with Bsz == B_max, nmpc_shift_warm_start at the last register slot
of its kernel, nmpc_tracking_error at the largest staging tile.  Comfortable shapes are in tests/test_gpu_parity.py.

References: the fp64 oracle for the Riccati sweep (bar below), the fp32 oracle bit for bit for the other two."""
import functools

import numpy as np
import pytest

from tests.solve_helpers import dense_lq, dev, rel  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE_FLOATS = 256      # one 16x16 tile; nmpc_riccati_kernel keeps 2 N of them per problem (K~', Acl~')


# ------------------------------------------------------------------------------- workspace of the Riccati entry
@pytest.mark.parametrize("B_max", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 3, 4, 50, 100, 256])
@pytest.mark.parametrize("model", [0, 1])
def test_workspace_holds_the_riccati_images(dev, model, N, B_max):
    """nmpc_riccati_kernel puts problem b at float b * 2 N * 256 of the handle's workspace, whatever the model, so a
    handle that accepts Bsz == B_max needs B_max * 2 N * 256 floats.  Creates handles only; nothing is launched.

    Before nmpc_create sized the workspace for this entry, the allocation was B_max times the solve layout alone:
    per problem 704, 1408, 1792, 18560, 36864, 93760 floats for the double integrator at these N against
    512, 1536, 2048, 25600, 51200, 131072 -- this test failed for model 0 from N = 3 up (model 1: 1472 floats at N = 1,
    4096 at N = 4, always above)."""
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    s = BatchedNmpcSolver(model, N, B_max, dev)
    need = B_max * 2 * N * TILE_FLOATS * 4
    print(f"model {model} N {N} B_max {B_max}: workspace {s.workspace_bytes} B, Riccati images {need} B")
    assert s.workspace_bytes >= need


# ------------------------------------------------------------------------------- Riccati at the tile's edges
RICCATI_B = 4
RICCATI_PERM = [2, 0, 3, 1]
# (handle's model, nx, nu, N)
RICCATI_CASES = [(1, 15, 16, 70),      # full tile, past 64 stages
                 (1, 15, 16, 256),     # full tile at the longest horizon
                 (1, 15, 1, 5),        # widest state, narrowest input
                 (1, 1, 16, 5),        # narrowest state, widest input
                 (1, 12, 12, 1),       # one stage
                 (0, 4, 2, 100),       # the layout the entry used to overrun (36864 floats per problem for 51200)
                 (1, 4, 2, 100)]       # the same problems on the layout that always fitted


@functools.lru_cache(maxsize=None)
def _riccati_case(nx, nu, N):
    """Four distinct problems of one shape (the generator of test_riccati_matches_oracle), their fp64 solutions and,
    per problem, the bar on (dX, dU).  Computed once per shape; nobody writes to it."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    lq = dense_lq(np.random.default_rng(nx * 100 + nu), RICCATI_B, nx, nu, N)
    ref, floor = [], []
    for b in range(RICCATI_B):
        r64, r32 = o64.riccati(*[a[b] for a in lq]), o32.riccati(*[a[b] for a in lq])
        assert r64["status"] == 0 and r32["status"] == 0
        floor.append((rel(r32["dX"], r64["dX"]), rel(r32["dU"], r64["dU"])))
        ref.append((r64["dX"], r64["dU"]))
    floor = np.array(floor)
    assert floor.max() < 1e-3, floor              # the problems are fp32-solvable: measured at most 8.7e-7, at (15, 16, N)
    return lq, ref, floor, np.maximum(2e-5, 4.0 * floor)


def _device_riccati(dev, model, N, lq):
    """(dX, dU, status) of the batch on a fresh handle with B_max == the batch"""
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    s = BatchedNmpcSolver(model, N, lq[0].shape[0], dev)
    dX, dU, st = s.riccati(*[s.to_device(a) for a in lq])
    torch.cuda.synchronize()
    return dX.cpu().numpy(), dU.cpu().numpy(), st.cpu().numpy()


def _riccati_parity(tag, dX, dU, case, problems):
    _, ref, floor, bar = case
    errs = np.array([(rel(dX[b], ref[b][0]), rel(dU[b], ref[b][1])) for b in problems])
    for b, e in zip(problems, errs):
        print(f"{tag} problem {b}: device dX {e[0]:.3g} dU {e[1]:.3g} | fp32 oracle dX {floor[b][0]:.3g} dU {floor[b][1]:.3g}"
              f" | bar dX {bar[b][0]:.3g} dU {bar[b][1]:.3g}")
    assert (errs < bar[list(problems)]).all(), (tag, errs, bar)


@pytest.mark.parametrize("model,nx,nu,N", RICCATI_CASES)
def test_riccati_parity_at_tile_edges(dev, model, nx, nu, N):
    """Bsz == B_max = 4 distinct problems against oracle64.riccati, relative L2 of dX and of dU per problem below
    max(2e-5, 4 x the fp32 oracle's own deviation from the fp64 one on the same inputs).

    Measured on the MI355X, worst problem of each case (device dX / dU | fp32 oracle dX / dU; the bar comes to 2e-5
    everywhere, four times the fp32 oracle staying below 3.5e-6):
      (15, 16, 70)    6.88e-7 / 8.34e-7 | 7.37e-7 / 8.65e-7
      (15, 16, 256)   6.67e-7 / 8.26e-7 | 7.38e-7 / 8.22e-7
      (15, 1, 5)      2.77e-7 / 2.59e-7 | 2.39e-7 / 2.57e-7
      (1, 16, 5)      3.26e-7 / 2.38e-7 | 2.46e-7 / 2.39e-7
      (12, 12, 1)     4.10e-7 / 4.59e-7 | 2.47e-7 / 4.55e-7
      (4, 2, 100)     3.00e-7 / 3.30e-7 | 3.08e-7 / 2.67e-7    on either handle, the same figures
    The horizon does not show: these closed loops are stable, the error does not grow with N."""
    case = _riccati_case(nx, nu, N)
    dX, dU, st = _device_riccati(dev, model, N, case[0])
    assert st.tolist() == [0] * RICCATI_B
    _riccati_parity(f"riccati model {model} ({nx}, {nu}, {N})", dX, dU, case, range(RICCATI_B))


@pytest.mark.parametrize("model,nx,nu,N", RICCATI_CASES)
def test_riccati_problem_reads_only_its_own_slice(dev, model, nx, nu, N):
    """The same batch in another order gives the same results in that order, bit for bit: what a problem computes does
    not depend on its batch slot, so it reads no other problem's K~', Acl~' images."""
    lq = _riccati_case(nx, nu, N)[0]
    dX, dU, st = _device_riccati(dev, model, N, lq)
    dXp, dUp, stp = _device_riccati(dev, model, N, [a[RICCATI_PERM] for a in lq])
    assert np.array_equal(dXp, dX[RICCATI_PERM]) and np.array_equal(dUp, dU[RICCATI_PERM])
    assert np.array_equal(stp, st[RICCATI_PERM])


@pytest.mark.parametrize("model,nx,nu,N", RICCATI_CASES)
def test_riccati_flags_indefinite_problem_in_last_slot(dev, model, nx, nu, N):
    """A negative-definite R at the last stage of the problem in the last batch slot (the slice that ends the
    workspace): that problem reports status 4, the others 0, with the results of the untouched batch bit for bit and
    so within the parity bar.  R = -1e3 I: R + B' Q_N B stays negative definite (B' Q_N B is below 30 for these
    draws); the fp64 oracle reports 4 for it as well."""
    from oracle.oracle import Oracle
    case = _riccati_case(nx, nu, N)
    lq = list(case[0])
    R = lq[1].copy()
    R[RICCATI_B - 1, N - 1] = -1e3 * np.eye(nu)
    lq[1] = R
    assert Oracle("f64").riccati(*[a[RICCATI_B - 1] for a in lq])["status"] == 4
    dX0, dU0, _ = _device_riccati(dev, model, N, case[0])
    dX, dU, st = _device_riccati(dev, model, N, lq)
    assert st.tolist() == [0] * (RICCATI_B - 1) + [4]
    others = range(RICCATI_B - 1)
    _riccati_parity(f"riccati indefinite last slot, model {model} ({nx}, {nu}, {N})", dX, dU, case, others)
    assert np.array_equal(dX[:-1], dX0[:-1]) and np.array_equal(dU[:-1], dU0[:-1])


# ------------------------------------------------------------------------------- shift kernel at its register limit
# nmpc_shift_kernel holds 16 elements per thread at 256 threads: N nx and N nu up to 4096 (host guard); shifts beyond N are N
@pytest.mark.parametrize("model,N,shifts", [(1, 341, (1, 340, 341, 400)),     # N nx = 4092: the last register slot in use
                                            (0, 1024, (1, 1023)),              # N nx = 4096 exactly
                                            (0, 1, (1,)),                      # shortest horizon
                                            (2, 64, (1, 63, 64))])             # the whole-body model's 18 kept inputs in the tail
def test_shift_at_the_register_limit(dev, oracle32, model, N, shifts):
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    B = 3
    s = BatchedNmpcSolver(model, N, B, dev)
    rng = np.random.default_rng(1000 * model + N)
    X = rng.normal(size=(B, N + 1, s.nx)).astype(np.float32)
    U = rng.normal(size=(B, N, s.nu)).astype(np.float32)
    for shift in shifts:
        Xd, Ud = s.to_device(X), s.to_device(U)
        s.warm_start_solver(Xd, Ud, shift)
        Xo, Uo = oracle32.shift_warm_start(X, U, shift)
        assert np.array_equal(Xd.cpu().numpy(), Xo), shift
        assert np.array_equal(Ud.cpu().numpy(), Uo), shift


@pytest.mark.parametrize("model,N", [(1, 342), (0, 1025)])
def test_shift_refuses_one_stage_beyond_the_limit(dev, model, N):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.solver import BatchedNmpcSolver
    B = 3
    s = BatchedNmpcSolver(model, N, B, dev)
    assert N * s.nx > 4096 >= (N - 1) * s.nx
    rng = np.random.default_rng(N)
    X = rng.normal(size=(B, N + 1, s.nx)).astype(np.float32)
    U = rng.normal(size=(B, N, s.nu)).astype(np.float32)
    Xd, Ud = s.to_device(X), s.to_device(U)
    with pytest.raises(_lib.NmpcError, match=r"\(-1\).*too long"):         # NMPC_E_ARG
        s.warm_start_solver(Xd, Ud, 1)
    torch.cuda.synchronize()
    assert np.array_equal(Xd.cpu().numpy(), X) and np.array_equal(Ud.cpu().numpy(), U)


# ------------------------------------------------------------------------------- tracking error at the staging tile's limit
@pytest.mark.parametrize("B,T,ns", [(3, 5, 127),      # 128 rows x 127 floats = 65,024 B of LDS, the largest accepted
                                    (2, 3, 126),      # even ns: padded to a row stride of 127
                                    (1, 300, 2),      # T > 128: a block spans no row boundary of S_nom
                                    (130, 1, 3),      # T = 1: every row of a block wraps
                                    (7, 37, 44)])     # T divides neither 128 nor the row count
def test_tracking_error_at_the_staging_limit(dev, oracle32, B, T, ns):
    from iterative_learning_nmpc_amd.solver import tracking_error
    rng = np.random.default_rng(1000 * B + T)
    Snom = rng.normal(0, 1, (T, ns)).astype(np.float32)
    S = (Snom[None] + rng.normal(0, 0.62, (B, T, ns))).astype(np.float32)
    S[:, :, 0] += 100.0
    ref = oracle32.tracking_error(S, Snom)
    Sd, Snd = torch.from_numpy(S).to(dev), torch.from_numpy(Snom).to(dev)
    err, wgt = tracking_error(Sd, Snd)
    assert np.array_equal(err.cpu().numpy(), ref)
    assert np.array_equal(wgt.cpu().numpy(), np.where(ref > 4.0, 5.0, 1.0).astype(np.float32))
    assert np.array_equal(tracking_error(Sd, Snd, with_weights=False).cpu().numpy(), ref)
    # a threshold that IS one of the errors: that row and everything below it weigh 1, everything above the other weight
    thr = float(np.sort(ref.ravel())[ref.size // 2])
    err2, wgt2 = tracking_error(Sd, Snd, threshold=thr, ood_weight=3.5)
    assert np.array_equal(err2.cpu().numpy(), ref)
    assert np.array_equal(wgt2.cpu().numpy(), np.where(ref > np.float32(thr), 3.5, 1.0).astype(np.float32))
    assert (ref == np.float32(thr)).any()


def test_tracking_error_refuses_a_row_beyond_the_staging_tile(dev):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd.solver import tracking_error
    S, Snom = torch.zeros(2, 3, 128, device=dev), torch.zeros(3, 128, device=dev)
    with pytest.raises(_lib.NmpcError, match=r"\(-1\).*staging tile"):      # NMPC_E_ARG: 128 x 129 floats > 64 KB
        tracking_error(S, Snom)


def test_tracking_error_threshold_is_strict(dev, oracle32):
    """err == threshold keeps weight 1, one ulp above takes ood_weight.  Row (0, 1) differs from the nominal row in one
    non-phase column by 4.0 exactly (4.5 - 0.5): err = sqrt(16) = 4 = the threshold.  Its twin (1, 1) differs by
    4 + 2^-21: the square rounds to 16 + 2^-18, its root to 4 + 2^-21, the float after 4.  The fp32 oracle confirms both."""
    from iterative_learning_nmpc_amd.solver import tracking_error
    B, T, ns = 2, 3, 5
    Snom = np.random.default_rng(0).normal(0, 1, (T, ns)).astype(np.float32)
    Snom[:, 2] = 0.5
    S = np.tile(Snom, (B, 1, 1))
    S[:, :, 0] += 100.0                                  # the phase column does not count
    S[0, 1, 2] = 4.5
    S[1, 1, 2] = np.nextafter(np.float32(4.5), np.float32(5.0))
    ref = oracle32.tracking_error(S, Snom)
    above = np.nextafter(np.float32(4.0), np.float32(5.0))
    assert ref[0, 1] == np.float32(4.0) and ref[1, 1] == above and S[1, 1, 2] - Snom[1, 2] == above
    err, wgt = tracking_error(torch.from_numpy(S).to(dev), torch.from_numpy(Snom).to(dev), threshold=4.0, ood_weight=5.0)
    assert np.array_equal(err.cpu().numpy(), ref)
    expect = np.ones((B, T), np.float32)
    expect[1, 1] = 5.0
    assert np.array_equal(wgt.cpu().numpy(), expect)
