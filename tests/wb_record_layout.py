"""The records of the whole-body family restated in Python -- TEST INFRASTRUCTURE ONLY (helper module, not collected by pytest).

A restatement of csrc/nmpc_wb_layout.hpp, written from the header's comments and formulas and tied to its static_assert values in
tests/test_wb_record_layout.py: where a state sits in the 48-wide homogeneous vector, the compact record of the scaled residual
Jacobian Js = sqrt(W) [J | res] (388 floats, `cj_index`), the node record of the linearisation (228 floats, `R_*`) and the tile
images of Q~ (nine 16 x 16 tiles, column-major).  On top of it the references the device tests compare with:

  unpack_js / pack_js     compact record <-> Js [30, 46] in column positions
  unpack_js_art / pack_js_art   the same in the articulated mode (csrc/nmpc_wb_momentum.hpp, restated below: `MR_*`, `DC_*`,
                          `CJ_ART`, `cj_index_art`): the consistency rows 16..21 come from the dense consistency record
  unpack_q                tile images -> Q~ (symmetrised from the lower tiles for a running node)
  node                    tests/wb_momentum_reference.node (the frozen oracle's per-node hooks) of node (b, k) of a workload,
                          with what the record needs beside it (inputs, weights, pyramid rows)
  reference_rows          the oracle's Js [ny, 43] -> the kernel's 30 dense rows and 46 column positions
  reference_record        every block of the node record from the oracle's quantities
  reference_q             the oracle's Q~ = Js'Js + reg I with the gradient in row and column HX
  bf16_split, contract    the four arithmetic paths of the QP kernel's prologue in float64, on a record
"""
import numpy as np

from tests import wb_momentum_reference as mr

NX, NU, NP, NG, NY, NYE = 42, 30, 20, 16, 90, 66
WQ, WV, WH, WA, WF = 0, 18, 36, 0, 18
RY_BASE, RY_JOINT, RY_ACC, RY_SWING, RY_FREG, RY_CNT, RY_CONS, RY_POS = 0, 12, 36, 48, 52, 64, 76, 82
RE_BASE, RE_JOINT, RE_SWING, RE_CNT, RE_CONS, RE_POS = 0, 12, 36, 40, 52, 58
NJR = 30                      # dense residual rows: contact 0..11, swing 12..15, consistency 16..21, foot placement 22..29

HX, XW, XP = 38, 46, 48       # the homogeneous coordinate, positions in use, positions of three tiles


def pos_of(s):
    return s if s < 36 else 32 + 4 * (1 + (s - 36) // 2) + ((s - 36) & 1)


def state_at(p):
    if p < 36:
        return p
    return 36 + 2 * ((p - 36) >> 2) + (p & 1) if (p < XW and (p & 3) < 2) else -1


POS = np.array([pos_of(s) for s in range(NX)])             # position of every state
NO_STATE = [p for p in range(XP) if state_at(p) < 0 and p != HX]      # 39, 42, 43, 46, 47

CJ_FOOT = 88
CJ_CONS = 4 * CJ_FOOT
CJ_FLOATS = CJ_CONS + 36
CJ_PADDING = [CJ_FOOT * f + 67 for f in range(4)] + [CJ_CONS + 33, CJ_CONS + 34, CJ_CONS + 35]


def xi_col(f, c):
    return c if c < 6 else 6 + 3 * f + (c - 6)


def xi_slot(f, qi):
    if qi < 6:
        return qi
    return 6 + (qi - 6 - 3 * f) if 6 + 3 * f <= qi < 9 + 3 * f else -1


def cj_index(row, col):
    """record index of element (row, column POSITION) of Js, or -1 for a structural zero"""
    if row < 12:
        f, i = divmod(row, 3)
        if col == HX:
            return CJ_FOOT * f + 54 + i
        if col < 18:
            c = xi_slot(f, col)
            return -1 if c < 0 else CJ_FOOT * f + 6 * c + i
        if col < 36:
            c = xi_slot(f, col - 18)
            return -1 if c < 0 else CJ_FOOT * f + 6 * c + 3 + i
        return -1
    if row < 16:
        f = row - 12
        if col == HX:
            return CJ_FOOT * f + 66
        if col < 18:
            c = xi_slot(f, col)
            return -1 if c < 0 else CJ_FOOT * f + 57 + c
        return -1
    if row < 19:
        i = row - 16
        if col == pos_of(WH + i):
            return CJ_CONS + 3 * i
        if col == WV + i:
            return CJ_CONS + 3 * i + 1
        return CJ_CONS + 3 * i + 2 if col == HX else -1
    if row < 22:
        i = row - 19
        if col == pos_of(WH + 3 + i):
            return CJ_CONS + 9 + 2 * i
        if col == HX:
            return CJ_CONS + 10 + 2 * i
        if WQ + 3 <= col < WQ + 6:
            return CJ_CONS + 15 + 3 * (col - WQ - 3) + i
        if WV + 3 <= col < WV + 6:
            return CJ_CONS + 24 + 3 * (col - WV - 3) + i
        return -1
    if row < 30:
        f, i = divmod(row - 22, 2)
        if col == HX:
            return CJ_FOOT * f + 68 + 10 * i + 9
        if col < 18:
            c = xi_slot(f, col)
            return -1 if c < 0 else CJ_FOOT * f + 68 + 10 * i + c
        return -1
    return -1


CJ = np.array([[cj_index(r, c) for c in range(XW)] for r in range(NJR)])      # the map as a table [30, 46]
CJ_ROWS, CJ_COLS = np.nonzero(CJ >= 0)
CJ_SLOTS = CJ[CJ_ROWS, CJ_COLS]
# the 80 record slots of the foot-placement rows 22..29
POS_SLOTS = np.array([CJ_FOOT * f + 68 + j for f in range(4) for j in range(20)])

# ---- csrc/nmpc_wb_momentum.hpp: what the articulated momentum model adds
# the momentum record of a node: A_g [6][18], dh_dq [6][18], A_g v [6], com from the origin of the base frame [3]
MR_AG, MR_DH, MR_AGV, MR_COM, MR_FLOATS = 0, 108, 216, 222, 228
# the dense consistency record of a node: six rows of [q_3..q_17 (15) | v (18) | own h slot | HX | padding]
DC_ROW, DC_V, DC_H, DC_RES = 36, 15, 33, 34
DC_FLOATS = 6 * DC_ROW
CJ_ART = CJ_FLOATS + 4        # where the QP prologue keeps the dense record in its record buffer, behind the zero slot
LDU = 36                      # the record buffer is the 32 elimination columns of this stride (csrc/nmpc_wb_layout.hpp)


def cj_index_art(row, col):
    """record-buffer index of element (row, column POSITION) of Js in the articulated mode, or -1 for a structural zero"""
    if row < 16 or row >= 22:
        return cj_index(row, col)
    i = row - 16
    base = CJ_ART + DC_ROW * i
    if col == HX:
        return base + DC_RES
    if col == pos_of(WH + i):
        return base + DC_H
    if WQ + 3 <= col < WQ + 18:
        return base + (col - WQ - 3)
    if WV <= col < WV + 18:
        return base + DC_V + (col - WV)
    return -1


CJA = np.array([[cj_index_art(r, c) for c in range(XW)] for r in range(NJR)])      # the articulated map as a table [30, 46]
_DENSE = np.zeros((NJR, XW), bool)
_DENSE[16:22] = CJA[16:22] >= 0
DC_ROWS, DC_COLS = np.nonzero(_DENSE)                      # positions of Js that live in the dense record ...
DC_SLOTS = CJA[DC_ROWS, DC_COLS] - CJ_ART                  # ... and their slots in it
_COMPACT = (CJA >= 0) & ~_DENSE
CA_ROWS, CA_COLS = np.nonzero(_COMPACT)                    # positions that stay in the compact record (rows 0..15, 22..29)
CA_SLOTS = CJA[CA_ROWS, CA_COLS]

# the node record (float offsets)
R_D, R_HQ, R_HF, R_CDT, R_R, R_C, R_ACT, R_COST, R_ZERO, R_DT, R_GQ, R_DT2, REC = 0, 48, 96, 132, 136, 168, 184, 185, 186, 187, 188, 224, 228

# tile images: element (row, col) of tile (i, j) at (3 i + j) 256 + 16 col + row
XT, IMG = 3, 256
QT_FLOATS = XT * XT * IMG


def unpack_js(record):
    """[..., 388] compact record -> Js [..., 30, 46] in column positions (float64)"""
    record = np.asarray(record)
    Js = np.zeros(record.shape[:-1] + (NJR, XW))
    Js[..., CJ_ROWS, CJ_COLS] = record[..., CJ_SLOTS]
    return Js


def pack_js(Js):
    """the inverse of unpack_js: [..., 30, 46] -> [..., 388], zeros in the padding slots"""
    Js = np.asarray(Js)
    record = np.zeros(Js.shape[:-2] + (CJ_FLOATS,), Js.dtype)
    record[..., CJ_SLOTS] = Js[..., CJ_ROWS, CJ_COLS]
    return record


def unpack_js_art(js_record, dcons):
    """[..., 388] compact record and [..., 216] dense consistency record -> Js [..., 30, 46] in column positions (float64):
    rows 0..15 and 22..29 through cj_index, rows 16..21 from the dense record"""
    js_record, dcons = np.asarray(js_record), np.asarray(dcons)
    Js = np.zeros(js_record.shape[:-1] + (NJR, XW))
    Js[..., CA_ROWS, CA_COLS] = js_record[..., CA_SLOTS]
    Js[..., DC_ROWS, DC_COLS] = dcons[..., DC_SLOTS]
    return Js


def pack_js_art(Js):
    """the inverse of unpack_js_art: [..., 30, 46] -> ([..., 388], [..., 216]); zeros in the padding slots, in slot 35 of every
    dense row and in the 36 consistency slots of the compact record, which this mode does not use"""
    Js = np.asarray(Js)
    record = np.zeros(Js.shape[:-2] + (CJ_FLOATS,), Js.dtype)
    dcons = np.zeros(Js.shape[:-2] + (DC_FLOATS,), Js.dtype)
    record[..., CA_SLOTS] = Js[..., CA_ROWS, CA_COLS]
    dcons[..., DC_SLOTS] = Js[..., DC_ROWS, DC_COLS]
    return record, dcons


def unpack_q(images, term, width=XW):
    """[2304] tile images of one node -> Q~ [width, width] (float64; width 48 keeps the two unused positions).  A running node
    has its lower tiles only: the strict upper tiles are filled with their transposes.  For the terminal node all nine tiles
    are read as stored, and the return value is (Q with its lower tiles mirrored, Q as stored)."""
    t = np.asarray(images, np.float64).reshape(XT, XT, 16, 16)               # [i, j, col, row]
    stored = t.transpose(0, 3, 1, 2).reshape(XP, XP)                         # [16 i + row, 16 j + col]
    Q = stored.copy()
    for i in range(XT):
        for j in range(i + 1, XT):
            Q[16 * i:16 * i + 16, 16 * j:16 * j + 16] = stored[16 * j:16 * j + 16, 16 * i:16 * i + 16].T
    if term:
        return Q[:width, :width], stored[:width, :width]
    return Q[:width, :width]


# ---------------------------------------------------------------------------------------------------------- references
def node(w, b, k, X, U, data="f64", momentum="declared", m=None):
    """reference quantities of node k of problem b of workload `w` at the iterate (X, U): wb_momentum_reference.node in the
    momentum model `momentum` (tree `m` for the articulated one), plus the inputs the record is built from"""
    term = k == w.N
    yr = w.yref_e[b] if term else (w.yref[b, k] if w.yref.ndim == 3 else w.yref[b])
    Wk = np.asarray(w.W_e if term else w.W, np.float64)
    n = mr.node(w.mp, X[b, k], None if term else U[b, k], w.params[b, k], yr, Wk, momentum, m, data)
    dt_ = np.float64 if data == "f64" else np.float32
    n.update(term=term, W=Wk, mp=np.asarray(w.mp, np.float64), p=np.asarray(w.params[b, k], np.float64))
    if not term:
        n["u"] = np.asarray(U[b, k], dt_).astype(np.float64)
        G, h, act = mr.oracle(data).constraints(2, w.mp, w.params[b, k])
        n.update(G=G.astype(np.float64), h=h.astype(np.float64), act=act)
    return n


def _dense_rows(term):
    r_ct, r_sw, r_cs, r_ps = (RE_CNT, RE_SWING, RE_CONS, RE_POS) if term else (RY_CNT, RY_SWING, RY_CONS, RY_POS)
    return np.concatenate([r_ct + np.arange(12), r_sw + np.arange(4), r_cs + np.arange(6), r_ps + np.arange(8)])


def reference_rows(n):
    """the oracle's Js [ny, 43] (rows in W order, columns [x; 1]) -> the kernel's dense rows [30, 46] in column positions"""
    rows = n["Js"][_dense_rows(n["term"])]
    out = np.zeros((NJR, XW))
    out[:, POS] = rows[:, :NX]
    out[:, HX] = rows[:, NX]
    return out


def reference_record(n, X_next=None):
    """every block of the node record from the oracle's quantities of node `n`; X_next: the next node's state (a stage).
    dict: d [48] (defect by position), hq [3, 16], hf [3, 12], cdt [4], r [32], c [16], act (int), cost, gq [36]; the terminal
    node has cost and gq only."""
    W, res = n["W"], n["res"]
    g = W * res
    gq = np.concatenate([g[RY_BASE:RY_BASE + 6], g[RY_JOINT:RY_JOINT + 12], g[RY_BASE + 6:RY_BASE + 12], g[RY_JOINT + 12:RY_JOINT + 24]])
    out = dict(gq=gq, cost=0.5 * float(np.sum(n["Js"][:, NX] ** 2)))
    if n["term"]:
        return out
    d = np.zeros(XP)
    d[POS] = n["xn"] - np.asarray(X_next, np.float64)
    hq = np.zeros((3, 16))
    hq[:, :15] = n["A"][39:42, 3:18]
    r = np.zeros(32)
    r[6:18] = g[RY_ACC:RY_ACC + 12]
    r[18:30] = g[RY_FREG:RY_FREG + 12]
    act = 0
    for j in range(NG):
        act |= int(n["act"][j] != 0) << j
    out.update(d=d, hq=hq, hf=n["B"][39:42, 18:30].copy(), cdt=np.array([n["B"][36, 18 + 3 * f] for f in range(4)]),
               r=r, c=n["G"] @ n["u"] - n["h"], act=act)
    return out


def cdt_agree(n):
    """the three entries dt c_f of each foot in B (rows h_lin x, y, z) are one number: the record keeps one"""
    B = n["B"]
    return all(B[36, 18 + 3 * f] == B[37, 19 + 3 * f] == B[38, 20 + 3 * f] for f in range(4))


def state_weights(W):
    """weight of the diagonal residuals (base, joint) on the states 0..35: the kernel's wdiag"""
    return np.concatenate([W[RY_BASE:RY_BASE + 6], W[RY_JOINT:RY_JOINT + 12], W[RY_BASE + 6:RY_BASE + 12], W[RY_JOINT + 12:RY_JOINT + 24]])


def reference_q(n, reg):
    """the oracle's Q~ [46, 46]: Jx' W Jx + reg I on the state positions (every row of the cost: the dense rows of
    reference_rows plus the diagonal rows), the gradient Jx' W res in row and column HX, zero at (HX, HX)"""
    Js = n["Js"]
    H = Js.T @ Js                                  # [43, 43] over [x; 1]
    Q = np.zeros((XW, XW))
    Q[np.ix_(POS, POS)] = H[:NX, :NX] + reg * np.eye(NX)
    Q[POS, HX] = H[:NX, NX]
    Q[HX, POS] = H[NX, :NX]
    return Q


# ------------------------------------------------------------------------------------------- the contraction's four paths
def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even: v_cvt_pk_bf16_f32, to_bf16x4 of csrc/nmpc_tile.hpp), as float32"""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32)


def bf16_split(J):
    """(hi, mid, lo) of float32 J as the prologue forms them: hi = bf16(J), mid = bf16(J - hi), lo = bf16((J - hi) - mid), the
    differences in float32 (exact)"""
    J = np.asarray(J, np.float32)
    hi = bf16_round(J)
    r1 = J - hi
    mid = bf16_round(r1)
    return hi, mid, bf16_round(r1 - mid)


def contract(Js, precision):
    """Js'Js [46, 46] in float64 from exactly the products path `precision` of the prologue forms, Js float32 [30, 46]"""
    Js = np.asarray(Js, np.float32)
    if precision == 0:
        J = Js.astype(np.float64)
        return J.T @ J
    h, m, lo = (a.astype(np.float64) for a in bf16_split(Js))
    if precision == 1:
        return h.T @ h
    if precision == 2:
        return h.T @ h + h.T @ m + m.T @ h
    return lo.T @ h + h.T @ lo + m.T @ m + m.T @ h + h.T @ m + h.T @ h


def device_q_reference(js_record, gq, Wk, reg, precision, dcons=None):
    """(Q_ref [46, 46], sum_rows |Js[row, r] Js[row, c]| [46, 46]) of a node from the DEVICE's own records: path `precision` of
    the contraction, + (wdiag + reg) on the state positions (one float32 sum, as the kernel holds it), + gq in row and column
    HX, (HX, HX) = 0.  dcons: the node's dense consistency record -- the articulated mode, whose rows 16..21 come from it"""
    if dcons is None:
        Js = unpack_js(np.asarray(js_record, np.float32)).astype(np.float32)
    else:
        Js = unpack_js_art(np.asarray(js_record, np.float32), np.asarray(dcons, np.float32)).astype(np.float32)
    Q = contract(Js, precision)
    wd = np.zeros(NX, np.float32)
    wd[:36] = state_weights(np.asarray(Wk, np.float32))
    Q[POS, POS] += (wd + np.float32(reg)).astype(np.float64)
    Q[:36, HX] += np.asarray(gq, np.float64)
    Q[HX, :36] += np.asarray(gq, np.float64)
    Q[HX, HX] = 0.0
    A = np.abs(Js.astype(np.float64))
    return Q, A.T @ A

