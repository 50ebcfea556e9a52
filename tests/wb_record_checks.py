"""What the node-by-node record tests of the whole-body family share -- TEST INFRASTRUCTURE ONLY (helper module, not collected by
pytest): tests/test_gpu_wb_linearize.py (the declared momentum model) and tests/test_gpu_wb_linearize_articulated.py (the
articulated one) read the same regions, cut them into the same blocks and hold them to the same per-node bar.

  workload            the cases' inputs (shapes in CASES), rounded to float32, read-only
  read_regions        rec, js, qt of every problem (one debug_workspace call per problem and region)
  *_BLOCKS            the block tables; device_blocks / record_blocks / js_blocks cut records into them
  held_per_node       the bar  err[b, k] <= max(1e-5 max|ref[b, k]|, 4 max over the batch |f32 - ref|)  on one block
  check_records       every assertion on the regions of one solve

In the articulated mode the consistency rows live in the dense consistency record `dcons` (csrc/nmpc_wb_momentum.hpp): the
functions take it as an optional argument, and the block `consistency` is then its six rows of 35 slots.
"""
import dataclasses
import functools

import numpy as np

from iterative_learning_nmpc_amd import workloads as wl
from tests import parity_groups as pg
from tests import wb_record_layout as L

CASES = {"lanes": (5, 30, True), "short": (67, 4, True), "limit": (2, 64, False), "tiny": (3, 7, False)}      # B, N, random patterns
H_POS = [36, 37, 40, 41, 44, 45]
D_PAD = [38, 39, 42, 43, 46, 47]
U24 = 2.0 ** -24
PER_PROBLEM = ("x0", "yref", "yref_e", "params", "X", "U")


@functools.lru_cache(maxsize=None)
def workload(name, foot_placement=0.0, first=None):
    """the case's inputs, never written to afterwards: wholebody_trot (with the contact patterns of parity_groups' wb_patterns
    where the case has them), N(0, 0.02) on every slot of X and N(0, 0.5) on every slot of U, everything rounded to float32 so
    that device and oracles read the same numbers.  first: only the first so many problems of the case"""
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
    if first is not None:
        w = dataclasses.replace(w, **{k: np.ascontiguousarray(getattr(w, k)[:first]) for k in PER_PROBLEM})
        assert w.B == first
    for a in (w.mp, w.x0, w.yref, w.yref_e, w.params, w.X, w.U, w.W, w.W_e):
        a.setflags(write=False)
    return w


def writable(w):
    """`w` with writable copies of its per-problem arrays (the cached workload's are read-only)"""
    return dataclasses.replace(w, **{k: np.array(getattr(w, k)) for k in PER_PROBLEM})


# ---------------------------------------------------------------------------------------------------------------- device
def read_regions(s, B, N):
    """(rec [B, N+1, 228], js [B, N+1, 388], qt [B, N+1, 2304]) float32: one debug_workspace call per problem and region"""
    lay = s.debug_wb_layout()
    assert lay["REC"] == L.REC
    sizes = {"rec": L.REC, "js": L.CJ_FLOATS, "qt": L.QT_FLOATS}
    return tuple(np.stack([s.debug_workspace(b, lay[r], (N + 1) * n).reshape(N + 1, n) for b in range(B)]) for r, n in sizes.items())


def read_momentum(s, B, N):
    """(mrec [B, N+1, 228], dcons [B, N+1, 216]) float32 of a handle in the articulated mode: one debug_momentum call per node"""
    mrec, dcons = np.zeros((B, N + 1, L.MR_FLOATS), np.float32), np.zeros((B, N + 1, L.DC_FLOATS), np.float32)
    for b in range(B):
        for k in range(N + 1):
            mrec[b, k], dcons[b, k] = s.debug_momentum(b, k)
    return mrec, dcons


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


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


def js_blocks(Js, dense=None):
    """Js [..., 30, 46] -> {group: [..., m]}; dense [..., 6, 36]: the dense consistency record, which is then the block
    `consistency` (35 slots of each row) in place of the rows 16..21 of Js"""
    flat = lambda a: a.reshape(a.shape[:-2] + (-1,))      # noqa: E731
    out = {}
    for f in range(4):
        out[f"contact J foot {f}"] = flat(Js[..., 3 * f:3 * f + 3, 18:36])
        out[f"contact Jd xy foot {f}"] = flat(Js[..., 3 * f:3 * f + 2, 0:18])
        out[f"contact Jd z foot {f}"] = Js[..., 3 * f + 2, 0:18]
        out[f"contact residual foot {f}"] = Js[..., 3 * f:3 * f + 3, L.HX]
    out["swing"] = flat(Js[..., 12:16, 0:18])
    out["consistency"] = flat(np.delete(Js[..., 16:22, :], L.HX, axis=-1)) if dense is None else flat(dense[..., :35])
    out["placement"] = flat(Js[..., 22:30, 0:18])
    out["residual"] = Js[..., 12:, L.HX]
    return out


def record_blocks(d, hq, hf, cdt, r, c, actbits):
    return {"defect q": d[..., 0:18], "defect v": d[..., 18:36], "defect h": d[..., H_POS], "defect padding": d[..., D_PAD],
            "dh_ang/dq": hq[..., :15].reshape(hq.shape[:-2] + (45,)), "dh_ang/dq column 15": hq[..., 15], "dh_ang/df": hf.reshape(hf.shape[:-2] + (36,)),
            "dt c": cdt, "r": r[..., :30], "r padding": r[..., 30:], "c": c, "c active": c * actbits}


def device_blocks(rec, js, act, dcons=None):
    """the device's blocks {name: [B, N or N+1, m]} (float64); act [B, N, 16]: the oracle's active rows; dcons [B, N+1, 216]:
    the dense consistency records of the articulated mode"""
    st = rec[:, :-1].astype(np.float64)
    out = record_blocks(st[..., L.R_D:L.R_D + 48], st[..., L.R_HQ:L.R_HQ + 48].reshape(st.shape[:2] + (3, 16)),
                        st[..., L.R_HF:L.R_HF + 36].reshape(st.shape[:2] + (3, 12)), st[..., L.R_CDT:L.R_CDT + 4],
                        st[..., L.R_R:L.R_R + 32], st[..., L.R_C:L.R_C + 16], act)
    out["gq"] = rec[..., L.R_GQ:L.R_GQ + 36].astype(np.float64)
    out["cost"] = rec[..., L.R_COST:L.R_COST + 1].astype(np.float64)
    if dcons is None:
        out.update(js_blocks(L.unpack_js(js)))
    else:
        out.update(js_blocks(L.unpack_js_art(js, dcons), dcons.astype(np.float64).reshape(dcons.shape[:-1] + (6, L.DC_ROW))))
    return out


def lane_of(b, k, N):
    return int((b * (N + 1) + k) % 64)


def held_per_node(case, name, got, ref, f32, N, table=None):
    """the per-node bar on block `name`, arrays [B, K, m]: [] or the [(b, k, lane, error, bar)] over it"""
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


def check_records(case, regions, stats, refs64, refs32, N, expect_act_word, dt, dcons=None):
    """every assertion on the records of one solve: regions (rec, js, ...), refs (blocks, act, act words, ...) of the fp64 and
    the float32-data reference, dt the model's time step as the device holds it (float32)"""
    rec, js = regions[0], regions[1]
    ref, act, words = refs64[:3]
    f32 = refs32[0]
    got = device_blocks(rec, js, act, dcons)
    over = {}
    for name in STAGE_BLOCKS + NODE_BLOCKS:
        bad = held_per_node(case, name, got[name], ref[name], f32[name], N)
        if bad:
            over[name] = bad[:8]
    assert not over, f"{case}: blocks over their bar, name -> [(b, k, lane, error, bar)]: {over}"
    # the exact words
    st = rec[:, :-1]
    assert np.array_equal(st[..., L.R_ACT].view(np.uint32), words if expect_act_word else np.zeros_like(words))
    assert (st[..., L.R_ZERO].view(np.int32) == 0).all() and (st[..., L.R_DT] == dt).all() and (st[..., L.R_DT2] == dt * dt).all()
    assert (js[..., L.CJ_PADDING].view(np.int32) == 0).all()
    if dcons is not None:
        assert (dcons.reshape(dcons.shape[:-1] + (6, L.DC_ROW))[..., 35].view(np.int32) == 0).all()
    # the sum of the node costs is the solve's cost figure, to the rounding of a float32 sum of N + 1 terms in any order
    costs = rec[..., L.R_COST].astype(np.float64)
    assert (np.abs(costs.sum(1) - stats[:, 0]) <= (N + 1) * U24 * np.abs(costs).sum(1)).all(), (costs.sum(1), stats[:, 0])
    return got
