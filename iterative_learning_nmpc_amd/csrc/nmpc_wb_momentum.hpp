// nmpc_wb_momentum.hpp -- the second momentum model of the whole-body family (NMPC_WB_MOMENTUM_ARTICULATED): sizes,
// offsets and index maps of what the articulated mode adds to nmpc_wb_layout.hpp -- the per-node momentum record that the torque
// family's momentum pass writes (nmpc_torque_centroidal.hip.inc) and the linearisation reads, the dense consistency record that the
// linearisation writes and the QP kernel's prologue gathers, and the argument block both kernels take beside WbArgs.  No kernel and
// no arithmetic on data, as nmpc_wb_layout.hpp; the declared mode uses nothing of this file.
#pragma once
#include "nmpc_wb_layout.hpp"

namespace nmpc {
namespace wb {

// ---- the momentum record of a node: the tree's centroidal quantities at (q, v) of the node (float offsets) ------------------------
//   A_g [6][18] (rows: linear 3, angular about the centre of mass 3; world axes), dh_dq = d(A_g v)/dq at fixed v [6][18],
//   A_g v [6], and the centre of mass FROM THE ORIGIN OF THE BASE FRAME (the first frame of the tree that carries mass; model 2's
//   base position r = q[0..2] is where that frame sits), world axes.  d com / d q_j is the linear row block of A_g over the mass.
constexpr int MR_AG = 0, MR_DH = 108, MR_AGV = 216, MR_COM = 222, MR_FLOATS = 228;
static_assert(MR_FLOATS % 4 == 0 && MR_COM + 3 <= MR_FLOATS, "records are whole 16 B pieces");

// ---- the dense consistency record of a node: the six sqrt(W)-scaled rows h - A_g(q) v - yref of Js -------------------------------
//   row i, floats 36 i ..:  [j] column q_(3+j), j < 15 (-sw dh_dq);  [15 + j] column v_j, j < 18 (-sw A_g);  [33] column h_i (sw);
//                           [34] column HX (the scaled residual);  ([35] padding)
constexpr int DC_ROW = 36, DC_V = 15, DC_H = 33, DC_RES = 34, DC_FLOATS = 6 * DC_ROW;
static_assert(DC_FLOATS % 4 == 0, "records are whole 16 B pieces");
// where the QP kernel's prologue keeps the dense consistency record in its record buffer: behind the compact record and its zero slot
constexpr int CJ_ART = CJ_FLOATS + 4;
static_assert(CJ_ART + DC_FLOATS <= 32 * LDU && DC_FLOATS <= 64 * 4, "record buffer: the dense consistency record is one 16 B piece per lane");

// record-buffer index of element (row, column POSITION) of Js in the articulated mode, or -1 for a structural zero: the
// consistency rows 16..21 are dense over q_3..q_17, v_0..v_17, their own momentum slot and HX; every other row is cj_index's
__host__ __device__ constexpr int cj_index_art(int row, int col) {
    if (row < 16 || row >= 22) return cj_index(row, col);
    const int i = row - 16, base = CJ_ART + DC_ROW * i;
    if (col == HX) return base + DC_RES;
    if (col == pos_of(WH + i)) return base + DC_H;
    if (col >= WQ + 3 && col < WQ + 18) return base + (col - WQ - 3);
    if (col >= WV && col < WV + 18) return base + DC_V + (col - WV);
    return -1;
}
static_assert(cj_index_art(0, 0) == cj_index(0, 0) && cj_index_art(13, HX) == cj_index(13, HX) && cj_index_art(29, 2) == cj_index(29, 2), "cj_index_art");
static_assert(cj_index_art(16, 0) == -1 && cj_index_art(16, 3) == CJ_ART && cj_index_art(18, 17) == CJ_ART + 2 * DC_ROW + 14, "cj_index_art");
static_assert(cj_index_art(19, WV) == CJ_ART + 3 * DC_ROW + DC_V && cj_index_art(21, WV + 17) == CJ_ART + 5 * DC_ROW + DC_V + 17, "cj_index_art");
static_assert(cj_index_art(17, pos_of(WH + 1)) == CJ_ART + DC_ROW + DC_H && cj_index_art(17, pos_of(WH)) == -1 && cj_index_art(21, HX) == CJ_ART + 5 * DC_ROW + DC_RES, "cj_index_art");
static_assert(cj_index_art(20, pos_of(WH + 4)) == CJ_ART + 4 * DC_ROW + DC_H && cj_index_art(20, 39) == -1, "cj_index_art");

// what the kernels of the articulated mode take beside WbArgs: the handle-owned buffers of the mode and the mass of the tree
struct WbArtArgs {
    const float* mrec;      // dev [B][N+1][MR_FLOATS]: the momentum records of this iteration (the momentum pass)
    float* dcons;           // dev [B][N+1][DC_FLOATS]: the dense consistency records (linearisation -> QP kernel)
    float m_tree;           // total mass of the tree
};

}  // namespace wb
}  // namespace nmpc
