"""tests/wb_record_layout.py against the layout header's own anchors, against itself, and against the fp64 oracle's structure
(CPU only).

Anchors      the static_assert values of csrc/nmpc_wb_layout.hpp hold for the restatement.
Map          cj_index is injective where it is >= 0; its values and the documented padding slots partition range(388);
             pack_js o unpack_js is the identity.
Structure    on 240 random nodes (stage and terminal, random contact flags, p_gain in [0, 50], foot-placement weights on and
             off) every non-zero of the fp64 oracle's dense rows sits where cj_index >= 0, and the positions the oracle makes
             non-zero are EXACTLY the map's positions less the zeros the model itself states (below).
             Count: the map has 381 positions (388 floats - 7 padding: the header's figure); the oracle shows 288 of them.  The
             other 93 are slots of the dense 3 x 9 foot Jacobian blocks the record stores whole: d p_f / d r = I (off-diagonal
             zeros; its time derivative zero) and d z_f / d yaw = 0, in the contact rows (16 per foot), the swing rows (3 per
             foot) and the foot-placement rows (2 per row), plus d L_z / d yaw = 0 of the angular consistency row.  No position
             of the oracle is missing from the map.
Articulated  the restatement of csrc/nmpc_wb_momentum.hpp: cj_index_art reproduces the header's five static_assert lines, is
             cj_index outside rows 16..21 and maps each of those rows one to one onto 35 slots of the dense consistency record (slot
             35 of a row is never addressed); pack_js_art o unpack_js_art is the identity; on 240 random nodes of the tilted tree
             no non-zero of the fp64 reference's dense rows lies outside cj_index_art >= 0, and every one of the 210 dense slots is
             non-zero at some node but the 9 the model makes zero: the angular rows in the columns v_0..v_2 -- the momentum about
             the centre of mass does not change with a translation of the whole tree, k x z - com x (m z) = 0 with k = m com --
             where the reference shows its own rounding (< 1e-12) and nothing else.
Sensitivity  one Jacobian entry scaled by 1 + 1e-4 moves exactly its block of reference_record / reference_rows by more than
             the bar of tests/test_gpu_wb_linearize.py.
"""
import numpy as np
import pytest

from iterative_learning_nmpc_amd import workloads as wl
from tests import wb_momentum_reference as mr
from tests import wb_record_layout as L
from tests.torque_helpers import bar


def test_anchors_of_the_header():
    assert [L.pos_of(s) for s in range(36, 42)] == [36, 37, 40, 41, 44, 45]
    assert all(L.pos_of(s) == s for s in range(36))
    assert L.state_at(40) == 38 and L.state_at(45) == 41 and L.state_at(L.HX) == -1 and L.state_at(39) == -1 and L.state_at(46) == -1
    assert all(L.state_at(L.pos_of(s)) == s for s in range(42))
    assert L.NO_STATE == [39, 42, 43, 46, 47]
    assert (L.HX - 32) >> 2 == 1 and (L.HX - 32) & 3 == 2
    assert L.cj_index(0, 0) == 0
    assert L.cj_index(5, 27) == 88 + 39 + 2
    assert L.cj_index(4, 6) == -1
    assert L.cj_index(13, L.HX) == 88 + 66
    assert L.cj_index(17, L.pos_of(37)) == 352 + 3
    assert L.cj_index(20, 22) == 352 + 28
    assert L.cj_index(29, 2) == 3 * 88 + 80
    assert (L.CJ_FOOT, L.CJ_CONS, L.CJ_FLOATS, L.REC) == (88, 352, 388, 228) and L.CJ_FLOATS % 4 == 0
    assert all(L.xi_slot(f, L.xi_col(f, c)) == c for f in range(4) for c in range(9))
    # the tail of the record (the kernel's static_assert) and the blocks in their order, none overlapping
    assert L.R_ACT % 4 == 0 and L.R_COST == L.R_ACT + 1 and L.R_ZERO == L.R_ACT + 2 and L.R_DT == L.R_ACT + 3 and L.R_DT2 % 4 == 0
    ends = [(L.R_D, 48), (L.R_HQ, 48), (L.R_HF, 36), (L.R_CDT, 4), (L.R_R, 32), (L.R_C, 16), (L.R_ACT, 4), (L.R_GQ, 36), (L.R_DT2, 1)]
    assert all(a + n <= b for (a, n), (b, _) in zip(ends[:-1], ends[1:])) and ends[-1][0] + 1 <= L.REC


def test_map_is_a_partition_of_the_record():
    assert len(L.CJ_SLOTS) == len(set(L.CJ_SLOTS.tolist())) == 381                        # injective
    assert sorted(L.CJ_SLOTS.tolist() + L.CJ_PADDING) == list(range(L.CJ_FLOATS))        # with the padding: every float once
    assert all(L.cj_index(r, c) == -1 for r in range(30) for c in L.NO_STATE if c < L.XW)
    assert all(L.cj_index(30 + r, c) == -1 for r in range(2) for c in range(L.XW))        # rows 30, 31 of the second K tile
    rng = np.random.default_rng(0)
    rec = rng.normal(size=(3, L.CJ_FLOATS)).astype(np.float32)
    rec[:, L.CJ_PADDING] = 0.0
    assert np.array_equal(L.pack_js(L.unpack_js(rec).astype(np.float32)), rec)
    Js = L.unpack_js(rec)
    assert np.array_equal(L.unpack_js(L.pack_js(Js)), Js) and np.count_nonzero(Js[0]) == 381
    assert sorted(L.POS_SLOTS.tolist()) == sorted(L.CJ[22:30][L.CJ[22:30] >= 0].tolist())


def test_unpack_q_reads_the_tile_order():
    img = np.zeros(L.QT_FLOATS, np.float32)
    full = np.arange(48 * 48, dtype=np.float64).reshape(48, 48)
    for i in range(3):
        for j in range(3):
            for col in range(16):
                for row in range(16):
                    img[(i * 3 + j) * 256 + col * 16 + row] = full[16 * i + row, 16 * j + col]
    Q, stored = L.unpack_q(img, True, 48)
    assert np.array_equal(stored, full)
    assert np.array_equal(np.tril(Q), np.tril(full)) and np.array_equal(Q[16:, :16], Q[:16, 16:].T) and np.array_equal(Q[32:, 16:32], Q[16:32, 32:].T)
    assert np.array_equal(L.unpack_q(img, False), Q[:46, :46])


def model_zeros():
    """the positions of the dense rows that the MODEL makes zero whatever the state (module docstring), from the structure of
    the foot Jacobian J_f = d p_f / d [r, theta, ql_f] -- d p / d r = I, d/dt of it zero, z_f independent of yaw -- and of
    L = R I_b E thetadot, whose z component does not depend on yaw"""
    Z = np.zeros((30, 46), bool)
    for f in range(4):
        for i in range(3):
            for c in range(3):
                Z[3 * f + i, L.WQ + c] = not (i == 2 and c == 2)        # c (Jd + [i == 2] p_gain J_z): Jd = 0, J_z = e_z
                Z[3 * f + i, L.WV + c] = i != c                          # c J: identity
            Z[3 * f + 2, [L.WQ + 3, L.WV + 3]] = True                    # yaw does not move z
        Z[12 + f, [0, 1, 3]] = True                                      # swing row: peak J_z
        for i in range(2):
            Z[22 + 2 * f + i, [c for c in range(3) if c != i]] = True    # placement rows: J_x, J_y
    Z[21, L.WQ + 3] = True
    return Z


@pytest.fixture(scope="module")
def sampled_nodes():
    """240 random nodes as (fp64 node, float32-data node) of wb_momentum_reference.node, a `term` flag added"""
    return sample_nodes()


def sample_nodes(momentum="declared", m=None, datas=("f64", "f32")):
    rng = np.random.default_rng(12)
    B = 8
    ws = [wl.wholebody_trot(B=B, N=10, seed=2, foot_placement=fp) for fp in (0.0, 1.0e3)]
    out = []
    for it in range(120):
        w = ws[it % 2]
        b = it % B
        x = (w.x0[b] + rng.normal(0, 0.1, 42)).astype(np.float32).astype(np.float64)
        p = w.params[b, it % 11].copy()
        c = (rng.random(4) < 0.6).astype(float)
        if it < 4:
            c[:] = it % 2
        p[:4], p[4:8] = c, 1.0 - c
        p[8:] = rng.normal(0, 0.1, 12)
        mp = w.mp.copy()
        mp[8] = rng.uniform(0.0, 50.0)
        for term in (False, True):
            u = None if term else rng.normal(0, 5.0, 30).astype(np.float32).astype(np.float64)
            yr, Wk = (w.yref_e[b], w.W_e) if term else (w.yref[b, 0], w.W)
            pair = []
            for data in datas:
                n = mr.node(mp, x, u, p, yr, Wk, momentum, m, data)
                n.update(term=term, W=np.asarray(Wk, np.float64), weighted=it % 2 == 1, p=p, mp=mp)
                if not term:
                    G, h, act = mr.oracle(data).constraints(2, mp, p)
                    n.update(u=u, G=G.astype(np.float64), h=h.astype(np.float64), act=act)
                pair.append(n)
            out.append(tuple(pair))
    return out


def test_structure_is_the_oracles(sampled_nodes):
    assert len(sampled_nodes) >= 200
    seen = np.zeros((30, 46), bool)
    for n, _ in sampled_nodes:
        nz = np.abs(L.reference_rows(n)) > 0
        outside = nz & (L.CJ < 0)
        assert not outside.any(), f"the oracle has non-zeros the map drops (row, column position): {np.argwhere(outside).tolist()}"
        if not n["weighted"]:
            assert not nz[22:30].any()
        seen |= nz
        # nothing of the dense rows' Jacobian lives outside reference_rows: the other rows are the diagonal and input rows
        rest = np.delete(n["Js"], L._dense_rows(n["term"]), axis=0)
        assert all(np.count_nonzero(r[:42]) <= 1 for r in rest)
    mapped, zeros = L.CJ >= 0, model_zeros()
    assert not (zeros & ~mapped).any()
    dead = mapped & ~seen
    print(f"\nstructural positions: the map {mapped.sum()} (header: 381), the oracle {seen.sum()}, the model's own zeros {zeros.sum()}")
    # no dead slot beyond the zeros the model states, and none of those is ever non-zero: the oracle's structure, exactly
    assert np.array_equal(dead, zeros), f"(row, column position) mapped, never non-zero, not a model zero: {np.argwhere(dead & ~zeros).tolist()};" \
                                        f" model zeros seen non-zero: {np.argwhere(zeros & seen).tolist()}"
    assert (mapped.sum(), seen.sum(), zeros.sum()) == (381, 288, 93)


# ------------------------------------------------------------------------------------------------- the articulated mode
def test_anchors_of_the_momentum_header():
    A, c, HX, WV, WH, pos_of = L.cj_index_art, L.cj_index, L.HX, L.WV, L.WH, L.pos_of
    assert (L.MR_AG, L.MR_DH, L.MR_AGV, L.MR_COM, L.MR_FLOATS) == (0, 108, 216, 222, 228)
    assert L.MR_FLOATS % 4 == 0 and L.MR_COM + 3 <= L.MR_FLOATS
    assert (L.DC_ROW, L.DC_V, L.DC_H, L.DC_RES, L.DC_FLOATS) == (36, 15, 33, 34, 216) and L.DC_FLOATS % 4 == 0
    assert L.CJ_ART == L.CJ_FLOATS + 4 == 392
    assert L.CJ_ART + L.DC_FLOATS <= 32 * L.LDU and L.DC_FLOATS <= 64 * 4          # the record buffer, one 16 B piece per lane
    # the five static_assert lines of cj_index_art, value for value
    assert A(0, 0) == c(0, 0) and A(13, HX) == c(13, HX) and A(29, 2) == c(29, 2)
    assert A(16, 0) == -1 and A(16, 3) == L.CJ_ART and A(18, 17) == L.CJ_ART + 2 * L.DC_ROW + 14
    assert A(19, WV) == L.CJ_ART + 3 * L.DC_ROW + L.DC_V and A(21, WV + 17) == L.CJ_ART + 5 * L.DC_ROW + L.DC_V + 17
    assert A(17, pos_of(WH + 1)) == L.CJ_ART + L.DC_ROW + L.DC_H and A(17, pos_of(WH)) == -1 and A(21, HX) == L.CJ_ART + 5 * L.DC_ROW + L.DC_RES
    assert A(20, pos_of(WH + 4)) == L.CJ_ART + 4 * L.DC_ROW + L.DC_H and A(20, 39) == -1


def test_articulated_map_is_the_compact_one_with_dense_consistency_rows():
    outside = [r for r in range(32) if r < 16 or r >= 22]
    assert all(L.cj_index_art(r, c) == L.cj_index(r, c) for r in outside for c in range(L.XP))
    assert np.array_equal(np.delete(L.CJA, np.arange(16, 22), axis=0), np.delete(L.CJ, np.arange(16, 22), axis=0))
    for i in range(6):
        slots = [L.cj_index_art(16 + i, c) for c in range(L.XP) if L.cj_index_art(16 + i, c) >= 0]
        assert sorted(slots) == [L.CJ_ART + 36 * i + j for j in range(35)], i      # one to one onto 35 slots; slot 35 never
        assert all(L.cj_index_art(16 + i, c) == -1 for c in L.NO_STATE + [0, 1, 2])
        assert all(L.cj_index_art(16 + i, L.pos_of(L.WH + j)) == -1 for j in range(6) if j != i)
    assert sorted(L.DC_SLOTS.tolist()) == [36 * i + j for i in range(6) for j in range(35)]
    # no compact slot of the consistency rows is addressed, and every other compact slot is, once
    assert sorted(L.CA_SLOTS.tolist() + L.CJ_PADDING[:4] + list(range(L.CJ_CONS, L.CJ_FLOATS))) == list(range(L.CJ_FLOATS))
    rng = np.random.default_rng(1)
    rec, dc = rng.normal(size=(3, L.CJ_FLOATS)).astype(np.float32), rng.normal(size=(3, L.DC_FLOATS)).astype(np.float32)
    rec[:, L.CJ_PADDING[:4] + list(range(L.CJ_CONS, L.CJ_FLOATS))] = 0.0
    dc.reshape(3, 6, 36)[:, :, 35] = 0.0
    Js = L.unpack_js_art(rec, dc)
    back = L.pack_js_art(Js.astype(np.float32))
    assert np.array_equal(back[0], rec) and np.array_equal(back[1], dc)
    assert np.array_equal(L.unpack_js_art(*L.pack_js_art(Js)), Js) and np.count_nonzero(Js[0]) == 381 - 33 + 210
    # the rows outside 16..21 are unpack_js's
    assert np.array_equal(np.delete(Js, np.arange(16, 22), axis=-2), np.delete(L.unpack_js(rec), np.arange(16, 22), axis=-2))


def articulated_model_zeros():
    """the positions of the dense consistency rows that the MODEL makes zero whatever the state: the angular rows in the columns
    of the three translations of the base -- column j of A_g about the centre of mass is k x z - com x (m z) with k = m com for a
    translation of the whole tree along z"""
    Z = np.zeros((30, 46), bool)
    Z[19:22, L.WV:L.WV + 3] = True
    return Z


def test_articulated_structure_is_the_references():
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    m = mr.tree_model(quadruped_tree(seed=4, perturb=0.1))
    nodes = sample_nodes("articulated", m, ("f64",))
    assert len(nodes) == 240 and {n["term"] for n, in nodes} == {False, True}
    largest = np.zeros((30, 46))
    for n, in nodes:
        R = np.abs(L.reference_rows(n))
        outside = (R > 0) & (L.CJA < 0)
        assert not outside.any(), f"the reference has non-zeros the map drops (row, column position): {np.argwhere(outside).tolist()}"
        # the dense record's order holds the same numbers
        dc = mr.reference_dense_consistency(n)
        assert np.array_equal(L.pack_js_art(L.reference_rows(n))[1].reshape(6, 36), dc) and (dc[:, 35] == 0).all()
        largest = np.maximum(largest, R)
    mapped, zeros = L.CJA >= 0, articulated_model_zeros()
    assert not (zeros & ~mapped).any()
    dense = np.zeros((30, 46), bool)
    dense[16:22] = mapped[16:22]
    live = dense & (largest > 1e-6)
    print(f"\ndense consistency slots: the map {dense.sum()}, the reference {live.sum()}, the model's own zeros {zeros.sum()}, "
          f"largest |reference| there {largest[zeros].max():.1e}, smallest of the largest elsewhere {largest[dense & ~zeros].min():.1e}")
    assert np.array_equal(dense & ~live, zeros), np.argwhere((dense & ~live) ^ zeros).tolist()
    assert largest[zeros].max() < 1e-12
    assert (dense.sum(), live.sum(), zeros.sum()) == (210, 201, 9)
    # outside the consistency rows the two modes have one structure: what test_structure_is_the_oracles states
    assert not ((largest > 0) & ~mapped).any()


def test_cdt_is_one_number_per_foot(sampled_nodes):
    assert all(L.cdt_agree(n) for n, _ in sampled_nodes if not n["term"])


def _blocks(n, xnext):
    r = L.reference_record(n, xnext)
    rows = L.reference_rows(n)
    r.update(contact_J=rows[:12, 18:36], contact_Jd=rows[:12, :18], swing=rows[12:16, :18], consistency=np.delete(rows[16:22], L.HX, axis=1),
             placement=rows[22:30, :18], residual=rows[:, L.HX])
    return r


@pytest.mark.parametrize("which", ("hq", "hf", "cdt", "contact_Jd", "contact_J", "consistency"))
def test_one_scaled_entry_moves_exactly_its_block(sampled_nodes, which):
    n, n32 = next((a, b) for a, b in sampled_nodes if not a["term"] and a["p"][:4].sum() == 4 and not a["weighted"])
    xnext = n["xn"] + 0.01
    clean, f32 = _blocks(n, xnext), _blocks(n32, xnext)
    m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in n.items()}
    if which == "hq":
        blk = m["A"][39:42, 3:18]
    elif which == "hf":
        blk = m["B"][39:42, 18:30]
    elif which == "cdt":
        blk = m["B"][36:37, 18:19]
    else:
        rows = {"contact_Jd": (L.RY_CNT, 12, 0, 18), "contact_J": (L.RY_CNT, 12, 18, 36), "consistency": (L.RY_CONS, 6, 0, 42)}[which]
        blk = m["Js"][rows[0]:rows[0] + rows[1], rows[2]:rows[3]]
    i = np.unravel_index(np.argmax(np.abs(blk)), blk.shape)
    blk[i] *= 1.0 + 1e-4                                     # a view: the node's own array
    moved = _blocks(m, xnext)
    for k in clean:
        diff = np.abs(np.asarray(moved[k], np.float64) - np.asarray(clean[k], np.float64)).max()
        if k == which:
            assert diff > bar(np.asarray(clean[k]), np.asarray(f32[k])), (k, diff)
        else:
            assert diff == 0.0, (k, diff)
