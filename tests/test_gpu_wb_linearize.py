"""The whole-body linearisation's records and the QP prologue's Hessian images on the device, node by node, in the declared
momentum model, against the frozen oracle's per-node hooks (tests/wb_record_layout.py).

Every case solves with max_sqp_iter = 1.  In such a solve the linearisation kernel is the only writer of the node records
(`rec`) and of the compact Jacobian records (`js`), and the `store_tile` of the QP kernel's prologue is the only writer of the Q~
images (`qt`): behind the prologue the QP kernel reads `recs` and `Qimg` and never stores to them (nmpc_wb_qp.hip.inc; its one
other store to `js` is inside the NMPC_WB_STAMPS timing build).  The three regions of a problem are read whole, one
`debug_workspace` call per region.

(a) Records   every block of every node against the fp64 oracle under the project's standing bar taken PER NODE,
                  err[b, k] <= max(1e-5 max|ref[b, k]|, 4 max over the batch |f32[b, k] - ref[b, k]|),
              f32 the float32-data reference; a block whose reference is all zero at a node is exact zeros there.
              The active mask: the kernel writes it only for a solve with interior-point iterations (n_ipm > 0), so the solve
              with n_ipm = 0 has the word 0, and a second solve with n_ipm = 1 has the oracle's `act` bits -- and every other
              word of the three regions as before.
(b) Index paths   folded shifts 1, N - 1, N against oracle64.shift_warm_start + reference; yref [B, ny] against per-stage copies.
(c) Foot-placement rows   weights on: rows 22..29 under the bar; weights back to zero: exact zeros, the regions of a fresh handle.
(d) Hessian images   precisions 0..3: same records; images against a float64 contraction of the device's own record by exactly
              the products of the path, |Q - Q_ref| <= 34 2^-24 sum_rows |Js Js| + 2^-24 |Q_ref| (32 contracted rows and the two
              additions, float32 accumulation at its worst); precisions 0 and 3 also against the oracle's Js'Js under bar (a).
(e) Skip      a skipped problem's regions keep their bits.

Shapes (threads of the linearisation = B (N + 1), blocks of 64): lanes 5 x 30 = 155 threads, two full blocks and a ragged one,
terminal nodes on lanes 30, 61, 28, 59, 26; short 67 x 4: the problem changes every 5 lanes; limit 2 x 64: node 64 beyond
lane = stage; tiny 3 x 7: 24 threads.  Measured maxima: DESIGN.md 2.
"""
import dataclasses
import functools

import numpy as np
import pytest

from tests import solve_helpers as sh
from tests import wb_momentum_reference as mr
from tests import wb_record_checks as C
from tests import wb_record_layout as L
from tests.solve_helpers import dev  # noqa: F401
from tests.wb_record_checks import (CASES, NODE_BLOCKS, STAGE_BLOCKS, ZERO_BLOCKS, device_blocks, held_per_node, lane_of, read_regions,
                                    same_bits, workload)

pytestmark = pytest.mark.gpu
U24 = C.U24


# ---------------------------------------------------------------------------------------------------------------- device
def solve_once(w, dev, precision=0, shift=0, s=None, n_ipm=0):
    """(solver, (rec, js, qt), stats) after one solve of `w` with max_sqp_iter = 1"""
    if s is None:
        s = sh.make_solver(w, w.B, dev, precision=precision, max_sqp_iter=1, n_ipm=n_ipm)
    _, _, _, stats = sh.gpu_solve(s, C.writable(w), shift=shift)
    return s, read_regions(s, w.B, w.N), stats


_BASE = {}


def base(name, dev):
    """the case's solve at precision 0 with n_ipm = 0 on a fresh handle, once per module"""
    if name not in _BASE:
        _BASE[name] = solve_once(workload(name), dev)
    return _BASE[name]


# ---------------------------------------------------------------------------------------------------------- reference
@functools.lru_cache(maxsize=None)
def reference(name, shift=0, foot_placement=0.0, yref_per_stage=True, data="f64"):
    """(blocks {name: [B, N or N+1, m]}, act [B, N, 16], act words [B, N], Q~ [B, N+1, 46, 46]) of the case from the oracle's
    hooks in `data` precision; shift > 0: the warm start shifted first by the fp64 oracle"""
    w = workload(name, foot_placement)
    if not yref_per_stage:
        w = dataclasses.replace(w, yref=w.yref[:, 0])
    X, U = mr.oracle("f64").shift_warm_start(w.X, w.U, shift) if shift else (w.X, w.U)
    B, N = w.B, w.N
    reg, reg_e = w.meta.get("reg", 1e-6), w.meta.get("reg_e", 1e-5)
    z = lambda *s: np.zeros((B,) + s)      # noqa: E731
    d, hq, hf, cdt, r, c, act = z(N, 48), z(N, 3, 16), z(N, 3, 12), z(N, 4), z(N, 32), z(N, 16), z(N, 16)
    gq, cost, Js, Q, words = z(N + 1, 36), z(N + 1, 1), z(N + 1, 30, 46), z(N + 1, 46, 46), np.zeros((B, N), np.uint32)
    for b in range(B):
        for k in range(N + 1):
            n = L.node(w, b, k, X, U, data)
            rr = L.reference_record(n, None if k == N else X[b, k + 1])
            gq[b, k], cost[b, k, 0], Js[b, k] = rr["gq"], rr["cost"], L.reference_rows(n)
            Q[b, k] = L.reference_q(n, reg_e if k == N else reg)
            if k < N:
                assert L.cdt_agree(n)
                d[b, k], hq[b, k], hf[b, k], cdt[b, k], r[b, k], c[b, k] = rr["d"], rr["hq"], rr["hf"], rr["cdt"], rr["r"], rr["c"]
                act[b, k], words[b, k] = n["act"] != 0, rr["act"]
    out = C.record_blocks(d, hq, hf, cdt, r, c, act)
    out.update(gq=gq, cost=cost)
    out.update(C.js_blocks(Js))
    return out, act, words, Q


def check_records(case, regions, stats, refs64, refs32, N, expect_act_word):
    """every assertion of (a) on the regions of one solve"""
    return C.check_records(case, regions, stats, refs64, refs32, N, expect_act_word, np.float32(workload(case.split("+")[0]).mp[0]))


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", list(CASES))
def test_records_match_the_oracle_node_by_node(dev, name):
    w = workload(name)
    B, N, patterns = CASES[name]
    s, regions, stats = base(name, dev)
    refs64, refs32 = reference(name), reference(name, data="f32")
    check_records(name, regions, stats, refs64, refs32, N, expect_act_word=False)
    # the inputs reach what the case is for: no block of the reference is trivially small, every block of threads has swing
    # and stance feet, and the terminal nodes sit on the lanes the shape promises
    ref = refs64[0]
    for blk in STAGE_BLOCKS + NODE_BLOCKS:
        if blk not in ZERO_BLOCKS and not blk.startswith("placement"):
            assert np.abs(ref[blk]).max() > 1e-3, blk
    assert np.abs(ref["placement"]).max() == 0.0
    if patterns:
        c = w.params[:, :, :4].reshape(-1, 4)
        for t0 in range(0, len(c), 64):
            assert (c[t0:t0 + 64] > 0.5).any() and (c[t0:t0 + 64] < 0.5).any()
    if name == "lanes":
        assert [lane_of(b, N, N) for b in range(B)] == [30, 61, 28, 59, 26]
        assert {lane_of(b, k, N) for b in range(B) for k in range(N + 1)} == set(range(64))
    # the active mask is the oracle's, bit for bit, once the solve has an interior point; nothing else moves
    s.set_max_qp_iter(1)
    _, again, _ = solve_once(w, dev, s=s)
    s.set_max_qp_iter(0)
    words = refs64[2]
    assert np.array_equal(again[0][:, :-1, L.R_ACT].view(np.uint32), words) and (words != 0).any()
    masked = again[0].copy()
    masked[:, :-1, L.R_ACT] = regions[0][:, :-1, L.R_ACT]
    assert same_bits(masked, regions[0]) and same_bits(again[1], regions[1]) and same_bits(again[2], regions[2])


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", ("lanes", "tiny"))
def test_folded_shift_reads_through_the_index_map(dev, name):
    w = workload(name)
    N = w.N
    s = sh.make_solver(w, w.B, dev, max_sqp_iter=1, n_ipm=0)
    for shift in (1, N - 1, N):
        _, regions, stats = solve_once(w, dev, shift=shift, s=s)
        refs64, refs32 = reference(name, shift), reference(name, shift, data="f32")
        check_records(f"{name}+{shift}", regions, stats, refs64, refs32, N, expect_act_word=False)
        # the exposed tail: forces zero (so c and the force rows of r see zeros), accelerations kept
        Xs, Us = mr.oracle("f64").shift_warm_start(w.X, w.U, shift)
        assert (Us[:, N - shift:, 18:] == 0).all() and np.array_equal(Us[:, N - shift:, :18], w.U[:, N - shift:, :18])
        assert (regions[0][:, N - shift:N, L.R_C:L.R_C + 16] == 0).all()
    assert not same_bits(regions[0], base(name, dev)[1][0])


@pytest.mark.parametrize("name", ("lanes", "tiny"))
def test_one_yref_row_is_its_per_stage_copies(dev, name):
    w = workload(name)
    row = dataclasses.replace(w, yref=np.ascontiguousarray(w.yref[:, 0]))
    copies = dataclasses.replace(w, yref=np.ascontiguousarray(np.repeat(w.yref[:, :1], w.N, axis=1)))
    _, r_row, st_row = solve_once(row, dev)
    _, r_cop, st_cop = solve_once(copies, dev)
    assert all(same_bits(a, b) for a, b in zip(r_row, r_cop)) and same_bits(st_row, st_cop)
    assert not same_bits(r_row[0], base(name, dev)[1][0])          # the case's own references differ from stage to stage
    refs64, refs32 = reference(name, yref_per_stage=False), reference(name, yref_per_stage=False, data="f32")
    check_records(name, r_row, st_row, refs64, refs32, w.N, expect_act_word=False)


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_foot_placement_rows_and_their_way_back_to_zeros(dev):
    name = "lanes"
    w0, wf = workload(name), workload(name, 1.0e3)
    N = w0.N
    s, regions, stats = solve_once(wf, dev)
    refs64, refs32 = reference(name, foot_placement=1.0e3), reference(name, foot_placement=1.0e3, data="f32")
    got = device_blocks(regions[0], regions[1], refs64[1])
    for blk in STAGE_BLOCKS + NODE_BLOCKS:
        assert not held_per_node(name + " fp", blk, got[blk], refs64[0][blk], refs32[0][blk], N), blk
    assert np.abs(refs64[0]["placement"]).max() > 1.0 and np.abs(refs64[0]["residual"][..., 10:]).max() > 1e-2
    assert (np.abs(regions[1][..., L.POS_SLOTS]).max(-1) > 0).all()
    # weights back to zero on the same handle: exact zeros again, and everything a fresh handle has
    s.set_cost_weights(w0.W, w0.W_e, w0.meta.get("reg", 1e-6), w0.meta.get("reg_e", 1e-5))
    _, back, stats_back = solve_once(w0, dev, s=s)
    _, fresh, stats_fresh = base(name, dev)
    assert (back[1][..., L.POS_SLOTS].view(np.int32) == 0).all() and (fresh[1][..., L.POS_SLOTS].view(np.int32) == 0).all()
    assert same_bits(back[1], fresh[1]) and same_bits(back[0], fresh[0]) and same_bits(back[2], fresh[2]) and same_bits(stats_back, stats_fresh)


# ------------------------------------------------------------------------------------------------------------------ (d)
def q_of(qt, term, width=48):
    return L.unpack_q(qt, term, width)


@pytest.mark.parametrize("precision", (0, 1, 2, 3))
def test_hessian_images_are_the_contraction_of_the_record(dev, precision):
    name = "lanes"
    w = workload(name)
    B, N = w.B, w.N
    _, base_regions, _ = base(name, dev)
    rec, js, qt = base_regions if precision == 0 else solve_once(w, dev, precision=precision)[1]
    # the split happens in registers: the records do not know the precision
    assert same_bits(rec, base_regions[0]) and same_bits(js, base_regions[1])
    if precision:
        assert not same_bits(qt, base_regions[2])
    reg, reg_e = w.meta.get("reg", 1e-6), w.meta.get("reg_e", 1e-5)
    share, worst, Qdev = 0.0, None, np.zeros((B, N + 1, 46, 46))
    for b in range(B):
        for k in range(N + 1):
            term = k == N
            Qref, absprod = L.device_q_reference(js[b, k], rec[b, k, L.R_GQ:L.R_GQ + 36], w.W_e if term else w.W, reg_e if term else reg, precision)
            bound = 34 * U24 * absprod + U24 * np.abs(Qref)
            images = [q_of(qt[b, k], False)] if not term else list(q_of(qt[b, k], True))      # terminal: mirrored lower, and all nine as stored
            for Q48 in images:
                assert (Q48[L.NO_STATE, :] == 0).all() and (Q48[:, L.NO_STATE] == 0).all(), (b, k)
                assert Q48[L.HX, L.HX] == 0
                e = np.abs(Q48[:46, :46] - Qref)
                over = e > bound
                assert not over.any(), f"(b, k, lane) = ({b}, {k}, {lane_of(b, k, N)}): (row, col, error, bound) {[(int(r), int(c), float(e[r, c]), float(bound[r, c])) for r, c in np.argwhere(over)[:6]]}"
                ratio = np.where(bound > 0, e / np.where(bound > 0, bound, 1.0), 0.0).max()
                if ratio > share:
                    share, worst = float(ratio), (b, k, lane_of(b, k, N))
            if term:
                assert not np.array_equal(images[1][:16, 16:], np.zeros((16, 30)))      # the upper tiles are stored
            Qdev[b, k] = images[0][:46, :46]
    print(f"  precision {precision}: largest share of the accumulation bound {share:.3f} at (b, k, lane) = {worst}")
    if precision in (0, 3):
        Q64, Q32 = reference(name)[3], reference(name, data="f32")[3]
        P, q, v = L.POS, np.arange(18), np.arange(18, 36)
        groups = {"Q[q, q]": (q, q), "Q[v, q]": (v, q), "Q[v, v]": (v, v), "Q[h, x]": (P[36:], P), "gradient": (P, np.array([L.HX]))}
        over = {}
        for g, (r, c) in groups.items():
            pick = lambda Q: Q[:, :, r][:, :, :, c].reshape(B, N + 1, -1)      # noqa: E731
            bad = held_per_node(f"p{precision}", g, pick(Qdev), pick(Q64), pick(Q32), N)
            if bad:
                over[g] = bad[:8]
        assert not over, over
        assert np.abs(Q64[:, :, :36, :36]).max() > 1.0


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_a_skipped_problem_keeps_its_regions(dev):
    import torch
    name = "tiny"
    w = workload(name)
    s, before, _ = solve_once(w, dev)
    moved = dataclasses.replace(w, X=(w.X + 0.01).astype(np.float32).astype(np.float64))
    flags = torch.zeros(w.B, dtype=torch.int32, device=dev)
    flags[1] = 1
    s.set_skip(flags, 1)
    _, after, _ = solve_once(moved, dev, s=s)
    s.set_skip(None)
    for a, b in zip(after, before):
        assert same_bits(a[1], b[1])
        assert not same_bits(a[0], b[0]) and not same_bits(a[2], b[2])      # its neighbours were solved anew
