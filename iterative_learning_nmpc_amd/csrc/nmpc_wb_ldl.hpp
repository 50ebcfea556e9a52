// nmpc_wb_ldl.hpp -- LDL' of the 30 x 30 input Hessian Huu of a whole-body stage, applied to [Huu | I] in column layout
// (lane = column): 4 x 4 panels factorised on wave-uniform values, the row groups below on v_mfma_f32_4x4x1 with A broadcast.
// Instantiated per contact pattern by the backward sweep of nmpc_wb_qp_kernel (nmpc_wb.hip).
#pragma once
#include "nmpc_wb_model.hpp"

// every a*b + c of the elimination is an fmaf or an MFMA (as in nmpc_wb.hip, which includes this file behind the same pragma)
#pragma clang fp contract(off)

namespace nmpc {
namespace wb {

// Coupling mask of the inputs at a stage: the accelerations always couple (bits 0..17); the three force components of a
// foot couple only while the foot stands -- a swing foot has a zero column in B~, no active pyramid row and a diagonal
// cost, so its row and column of Huu are exactly diagonal: its multipliers are exact zeros and nothing below it changes.
// The elimination is instantiated for the contact patterns of a trot (the two diagonal pairs, four-foot stance, flight)
// with those rows and pivots left out at compile time (160 of the 435 multipliers of a two-foot stage), and for the full
// mask, which is valid for every pattern.
__host__ __device__ constexpr unsigned coupling_mask(unsigned stance) {
    unsigned m = 0x3FFFFu;
    for (int f = 0; f < 4; ++f) m |= ((stance >> f) & 1u) ? (0x7u << (WF + 3 * f)) : 0u;
    return m;
}
// ---- the elimination, with its rank-1 updates on the matrix pipe ----------------------------------------------------------
// Register file: row i of [Huu | I] in register i & 3 of Xq[i >> 2] (lane = column).  v_mfma_f32_4x4x1_16b_f32 is sixteen 4 x 4
// outer products, D[v][lane] = C[v][lane] + A[lane 4 (lane / 4) + v] B[lane], and with its A-broadcast control (cbsz = 4,
// abid = g) all sixteen blocks take the A operand of block g: D[v][lane] = C[v][lane] + A[lane 4g + v] B[lane].  Huu is symmetric
// and stays so under the elimination, so the multiplier of row i under pivot J, M[i][J], is what the scaled pivot row y_J holds
// in LANE i: with A = y_J and B = -y_J ONE two-pass instruction updates the four rows of group g in all 64 columns -- no
// broadcast, no data movement -- where a scalar form spends four v_readlane and four v_fma.
// The pivots themselves are a dependent chain (pivot -> v_rsq -> multiplier -> next pivot): the four of a panel are factorised on
// wave-uniform values (ldl_panel), the row groups below the panel take them as four MFMAs each (ldl_trailing;
// tools/probes/mfma4x4x1.hip checks the operand layout on the device).
// Every cross-lane read of the elimination is a bcast() (the v_readlane builtin), so the compiler sees it and places the wait
// states.  Hand-written v_readlane in inline assembly, which this elimination once had, needs a leading s_nop: gfx950 wants a
// wait state between a VALU write of a VGPR and a v_readlane of it, the hazard recognizer does not look into inline assembly,
// and the scheduler is free to sink the last FMA in front of the asm block to just before it (found as a run-to-run varying
// 5e-5 error after an unrelated edit had changed the schedule).
constexpr int LDL_ROWS = 32, LDL_GROUPS = LDL_ROWS / 4;
// the pivots `panel` (bit jj: pivot 4P + jj is coupled) applied to the row groups G .. LDL_GROUPS-1
template <int P, int G, unsigned MASK>
__device__ __forceinline__ void ldl_trailing(f32x4 (&Xq)[LDL_GROUPS], const float (&ny)[4]) {
    if constexpr (G < LDL_GROUPS) {
        if constexpr (((MASK >> (4 * G)) & 0xFu) != 0u) {      // not a group of decoupled inputs only (or past the last row)
            constexpr unsigned panel = (MASK >> (4 * P)) & 0xFu;
            if constexpr (panel & 1u) Xq[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(Xq[P][0], ny[0], Xq[G], 4, G, 0);
            if constexpr (panel & 2u) Xq[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(Xq[P][1], ny[1], Xq[G], 4, G, 0);
            if constexpr (panel & 4u) Xq[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(Xq[P][2], ny[2], Xq[G], 4, G, 0);
            if constexpr (panel & 8u) Xq[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(Xq[P][3], ny[3], Xq[G], 4, G, 0);
        }
        ldl_trailing<P, G + 1, MASK>(Xq, ny);
    }
}
// One panel: the 4 x 4 diagonal block of the panel's rows (ten numbers, lanes 4P .. 4P+3 of the four registers) is factorised on
// wave-uniform values -- pivot -> v_rsq -> multiplier -> next pivot, three operations per pivot and no cross-lane move on the
// chain -- and the four rows follow it as y_c = (x_c - sum_{k<c} l_ck y_k) / sqrt(d_c); then the row groups below, on the matrix pipe.
template <int P, unsigned MASK>
__device__ __forceinline__ void ldl_panel(f32x4 (&Xq)[LDL_GROUPS], bool& ok, const float (&rs_free)[12]) {
    if constexpr (P < LDL_GROUPS) {
        constexpr int J0 = 4 * P;
        constexpr unsigned pm = (MASK >> J0) & 0xFu;          // coupled rows of the panel (rows past NU - 1 have no bit)
        float blk[4][4], l[4][4], rs[4] = {1.0f, 1.0f, 1.0f, 1.0f}, ny[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c)
                blk[r][c] = (((pm >> r) & 1u) && ((pm >> c) & 1u)) ? bcast(Xq[P][r], J0 + c) : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if ((pm >> c) & 1u) {
                float d = blk[c][c];
#pragma unroll
                for (int k = 0; k < c; ++k)
                    if ((pm >> k) & 1u) d = fmaf(-l[c][k], l[c][k], d);
                ok = ok && (d > 0.0f);
                rs[c] = __builtin_amdgcn_rsqf(d);
#pragma unroll
                for (int r = c + 1; r < 4; ++r)
                    if ((pm >> r) & 1u) {
                        float t = blk[r][c];
#pragma unroll
                        for (int k = 0; k < c; ++k)
                            if ((pm >> k) & 1u) t = fmaf(-l[r][k], l[c][k], t);
                        l[r][c] = t * rs[c];
                    }
            } else if (J0 + c < NU) {
                // a decoupled input (a force component of a swing foot): nothing of B~'P~B~ or of the barrier reaches its pivot, which
                // is the constant W_f_reg + reg -- its 1 / sqrt comes from the kernel's prologue (rs_free: the same v_rsq of the same
                // bits) instead of a v_readlane -> v_rsq on the elimination's dependent chain
                rs[c] = rs_free[J0 + c >= WF ? J0 + c - WF : 0];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (J0 + c < NU) {
                float v = Xq[P][c];
                if ((pm >> c) & 1u) {
#pragma unroll
                    for (int k = 0; k < c; ++k)
                        if ((pm >> k) & 1u) v = fmaf(-l[c][k], Xq[P][k], v);
                }
                v *= rs[c];
                Xq[P][c] = v;
                ny[c] = -v;
            }
        ldl_trailing<P, P + 1, MASK>(Xq, ny);
        ldl_panel<P + 1, MASK>(Xq, ok, rs_free);
    }
}

}  // namespace wb
}  // namespace nmpc
