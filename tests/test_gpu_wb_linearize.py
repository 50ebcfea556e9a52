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

from iterative_learning_nmpc_amd import workloads as wl
from tests import parity_groups as pg
from tests import solve_helpers as sh
from tests import wb_momentum_reference as mr
from tests import wb_record_layout as L
from tests.solve_helpers import dev  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = {"lanes": (5, 30, True), "short": (67, 4, True), "limit": (2, 64, False), "tiny": (3, 7, False)}      # B, N, random patterns
H_POS = [36, 37, 40, 41, 44, 45]
D_PAD = [38, 39, 42, 43, 46, 47]
U24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def workload(name, foot_placement=0.0):
    """the case's inputs, never written to afterwards: wholebody_trot (with the contact patterns of parity_groups' wb_patterns
    where the case has them), N(0, 0.02) on every slot of X and N(0, 0.5) on every slot of U, everything rounded to float32 so
    that device and oracles read the same numbers"""
    B, N, patterns = CASES[name]
    seed = 20 + list(CASES).index(name)
    if patterns:
        w = pg.workload(pg.Case(name, 2, "wb_patterns", B, N, seed, 0, 1))
    else:
        w = wl.wholebody_trot(B=B, N=N, seed=seed)
    if foot_placement > 0.0:
        wf = wl.wholebody_trot(B=B, N=N, seed=seed, foot_placement=foot_placement)
        assert np.array_equal(wf.x0, w.x0)
        yref, yref_e = w.yref.copy(), w.yref_e.copy()
        yref[:, :, 82:90], yref_e[:, 58:66] = wf.yref[:, :, 82:90], wf.yref_e[:, 58:66]
        w = dataclasses.replace(w, W=wf.W, W_e=wf.W_e, yref=yref, yref_e=yref_e)
    rng = np.random.default_rng(seed + 100)
    X = w.X + rng.normal(0, 0.02, w.X.shape)
    U = w.U + rng.normal(0, 0.5, w.U.shape)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)                # noqa: E731
    w = dataclasses.replace(w, mp=f32(w.mp), x0=f32(w.x0), yref=f32(w.yref), yref_e=f32(w.yref_e), params=f32(w.params), X=f32(X),
                            U=f32(U), W=f32(w.W), W_e=f32(w.W_e))
    for a in (w.mp, w.x0, w.yref, w.yref_e, w.params, w.X, w.U, w.W, w.W_e):
        a.setflags(write=False)
    return w


# ---------------------------------------------------------------------------------------------------------------- device
def read_regions(s, B, N):
    """(rec [B, N+1, 228], js [B, N+1, 388], qt [B, N+1, 2304]) float32: one debug_workspace call per problem and region"""
    lay = s.debug_wb_layout()
    assert lay["REC"] == L.REC
    sizes = {"rec": L.REC, "js": L.CJ_FLOATS, "qt": L.QT_FLOATS}
    return tuple(np.stack([s.debug_workspace(b, lay[r], (N + 1) * n).reshape(N + 1, n) for b in range(B)]) for r, n in sizes.items())


def solve_once(w, dev, precision=0, shift=0, s=None, n_ipm=0):
    """(solver, (rec, js, qt), stats) after one solve of `w` with max_sqp_iter = 1"""
    if s is None:
        s = sh.make_solver(w, w.B, dev, precision=precision, max_sqp_iter=1, n_ipm=n_ipm)
    fields = ("x0", "yref", "yref_e", "params", "X", "U")          # (writable copies: the cached workload's arrays are read-only)
    _, _, _, stats = sh.gpu_solve(s, dataclasses.replace(w, **{k: np.array(getattr(w, k)) for k in fields}), shift=shift)
    return s, read_regions(s, w.B, w.N), stats


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


_BASE = {}


def base(name, dev):
    """the case's solve at precision 0 with n_ipm = 0 on a fresh handle, once per module"""
    if name not in _BASE:
        _BASE[name] = solve_once(workload(name), dev)
    return _BASE[name]


# ------------------------------------------------------------------------------------------------------------- blocks
STAGE_BLOCKS = ("defect q", "defect v", "defect h", "defect padding", "dh_ang/dq", "dh_ang/dq column 15", "dh_ang/df", "dt c", "r",
                "r padding", "c", "c active")
# the contact rows per foot (a swing foot's are exact zeros), their q columns c (Jd + [z] p_gain J_z) split into the rows x, y --
# d/dt J alone -- and the row z, where p_gain J_z is fifty times larger and would set the scale of the block
JS_BLOCKS = tuple(f"{g} foot {f}" for g in ("contact J", "contact Jd xy", "contact Jd z", "contact residual") for f in range(4)) + \
    ("swing", "consistency", "placement", "residual")
NODE_BLOCKS = ("gq", "cost") + JS_BLOCKS
# blocks whose reference is zero by design (the others must be non-trivial in every case)
ZERO_BLOCKS = ("defect padding", "dh_ang/dq column 15", "r padding")


def _js_blocks(Js):
    """Js [..., 30, 46] -> {group: [..., m]}"""
    flat = lambda a: a.reshape(a.shape[:-2] + (-1,))      # noqa: E731
    out = {}
    for f in range(4):
        out[f"contact J foot {f}"] = flat(Js[..., 3 * f:3 * f + 3, 18:36])
        out[f"contact Jd xy foot {f}"] = flat(Js[..., 3 * f:3 * f + 2, 0:18])
        out[f"contact Jd z foot {f}"] = Js[..., 3 * f + 2, 0:18]
        out[f"contact residual foot {f}"] = Js[..., 3 * f:3 * f + 3, L.HX]
    out["swing"] = flat(Js[..., 12:16, 0:18])
    out["consistency"] = flat(np.delete(Js[..., 16:22, :], L.HX, axis=-1))
    out["placement"] = flat(Js[..., 22:30, 0:18])
    out["residual"] = Js[..., 12:, L.HX]
    return out


def _record_blocks(d, hq, hf, cdt, r, c, actbits):
    return {"defect q": d[..., 0:18], "defect v": d[..., 18:36], "defect h": d[..., H_POS], "defect padding": d[..., D_PAD],
            "dh_ang/dq": hq[..., :15].reshape(hq.shape[:-2] + (45,)), "dh_ang/dq column 15": hq[..., 15], "dh_ang/df": hf.reshape(hf.shape[:-2] + (36,)),
            "dt c": cdt, "r": r[..., :30], "r padding": r[..., 30:], "c": c, "c active": c * actbits}


def device_blocks(rec, js, act):
    """the device's blocks {name: [B, N or N+1, m]} (float64); act [B, N, 16]: the oracle's active rows"""
    st = rec[:, :-1].astype(np.float64)
    out = _record_blocks(st[..., L.R_D:L.R_D + 48], st[..., L.R_HQ:L.R_HQ + 48].reshape(st.shape[:2] + (3, 16)),
                         st[..., L.R_HF:L.R_HF + 36].reshape(st.shape[:2] + (3, 12)), st[..., L.R_CDT:L.R_CDT + 4],
                         st[..., L.R_R:L.R_R + 32], st[..., L.R_C:L.R_C + 16], act)
    out["gq"] = rec[..., L.R_GQ:L.R_GQ + 36].astype(np.float64)
    out["cost"] = rec[..., L.R_COST:L.R_COST + 1].astype(np.float64)
    out.update(_js_blocks(L.unpack_js(js)))
    return out


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
    out = _record_blocks(d, hq, hf, cdt, r, c, act)
    out.update(gq=gq, cost=cost)
    out.update(_js_blocks(Js))
    return out, act, words, Q


def lane_of(b, k, N):
    return int((b * (N + 1) + k) % 64)


def held_per_node(case, name, got, ref, f32, N, table=None):
    """the bar of (a) on block `name`, arrays [B, K, m]: [] or the [(b, k, lane, error, bar)] over it"""
    err = np.abs(got - ref).max(-1)
    scale = np.abs(ref).max(-1)
    floor = np.abs(f32 - ref).max()
    bar = np.maximum(1e-5 * scale, 4.0 * floor)
    zero = (scale == 0.0) & (np.abs(f32).max(-1) == 0.0)
    bar = np.where(zero, 0.0, bar)                          # a block whose reference is all zero at a node: exact zeros
    bad = ~(err <= bar)
    wb, wk = np.unravel_index(np.argmax(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), err * 1e300)), err.shape)
    line = (f"  {case:<6} {name:<26} device {err.max():.2e}  float32 reference {floor:.2e}  scale {scale.max():.2e}  "
            f"bar {max(1e-5 * scale.max(), 4.0 * floor):.2e}  closest (b, k, lane) = ({wb}, {wk}, {lane_of(wb, wk, N)})")
    print(line)
    if table is not None:
        table.append(line)
    return [(int(b), int(k), lane_of(b, k, N), float(err[b, k]), float(bar[b, k])) for b, k in zip(*np.nonzero(bad))]


def check_records(case, regions, stats, refs64, refs32, N, expect_act_word):
    """every assertion of (a) on the regions of one solve"""
    rec, js, _ = regions
    ref, act, words, _ = refs64
    f32 = refs32[0]
    got = device_blocks(rec, js, act)
    over = {}
    for name in STAGE_BLOCKS + NODE_BLOCKS:
        bad = held_per_node(case, name, got[name], ref[name], f32[name], N)
        if bad:
            over[name] = bad[:8]
    assert not over, f"{case}: blocks over their bar, name -> [(b, k, lane, error, bar)]: {over}"
    # the exact words
    st = rec[:, :-1]
    assert np.array_equal(st[..., L.R_ACT].view(np.uint32), words if expect_act_word else np.zeros_like(words))
    dt = np.float32(workload(case.split("+")[0]).mp[0])
    assert (st[..., L.R_ZERO].view(np.int32) == 0).all() and (st[..., L.R_DT] == dt).all() and (st[..., L.R_DT2] == dt * dt).all()
    assert (js[..., L.CJ_PADDING].view(np.int32) == 0).all()
    # the sum of the node costs is the solve's cost figure, to the rounding of a float32 sum of N + 1 terms in any order
    costs = rec[..., L.R_COST].astype(np.float64)
    assert (np.abs(costs.sum(1) - stats[:, 0]) <= (N + 1) * U24 * np.abs(costs).sum(1)).all(), (costs.sum(1), stats[:, 0])
    return got


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
