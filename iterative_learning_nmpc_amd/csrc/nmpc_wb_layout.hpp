// nmpc_wb_layout.hpp -- sizes, offsets and index maps of the whole-body family (nmpc_wb.hip): where a state sits in the 48-wide
// homogeneous vector, the compact record of the scaled residual Jacobian, the per-node record of the linearisation, the
// argument block of the two kernels, the rows of the diagonal residuals, the workspace of a problem and the LDS of the QP kernel.  No kernel and no arithmetic on
// data: what only needs a size or an offset (the host layer, the rollout kernels, the debug entry points) needs this header alone.
#pragma once
#include "nmpc_wb_model.hpp"

namespace nmpc {
namespace wb {

// Positions of the states in the 48-wide homogeneous vector x~ (three tiles of 16).  States 0..35 (q, v_0..v_17) sit at their own
// index: tiles 0, 1 and slots 0..3 of tile 2.  The six momentum states sit at slots 4, 5, 8, 9, 12, 13 of tile 2 and the
// homogeneous coordinate at slot 6: registers 0 and 1 of lane rows 1..3 in the accumulator layout.  A product that contracts over
// tile row 2 against an operand whose only non-zero rows are momentum rows (the dense part of N~ = A~ - I and of B~) then needs
// contraction steps 0 and 1 only: 34 of 196 MFMAs of a backward stage less than with the states in their own order.
constexpr int HX = 38;                 // position of the homogeneous coordinate of x~ = [dx; 1]
constexpr int XW = 46;                 // positions in use: 0..45
__host__ __device__ constexpr int pos_of(int s) { return s < 36 ? s : 32 + 4 * (1 + (s - 36) / 2) + ((s - 36) & 1); }      // s < 42
__host__ __device__ constexpr int state_at(int p) {      // -1: padding or the homogeneous coordinate
    return p < 36 ? p : (p < XW && (p & 3) < 2) ? 36 + 2 * ((p - 36) >> 2) + (p & 1) : -1;
}
static_assert(pos_of(36) == 36 && pos_of(37) == 37 && pos_of(38) == 40 && pos_of(39) == 41 && pos_of(40) == 44 && pos_of(41) == 45, "momentum slots");
static_assert(state_at(40) == 38 && state_at(45) == 41 && state_at(HX) == -1 && state_at(39) == -1 && state_at(46) == -1, "momentum slots");
constexpr int HXQ = (HX - 32) >> 2, HXR = (HX - 32) & 3;      // lane row and register of row HX in tile row 2
static_assert(HXR == 2, "the homogeneous row is register 2 of its lane row");

// ---- the scaled residual Jacobian Js = sqrt(W) [J | res] of a node, COMPACT -------------------------------------------------------
// Js is 30 x 46 and the record keeps 381 of its positions: the 288 the model can make non-zero and, because the 3 x 9 foot Jacobian
// blocks are stored whole, 93 that it never does (d p_f / d r = I and its zero time derivative, d z_f / d yaw = 0, d L_z / d yaw = 0;
// tests/test_wb_record_layout.py counts both against the oracle).  As a dense tile image (6 KB per node, each thread of the linearisation scattering
// its ~440 dword stores over its own image) it cost 0.6 of the linearisation's 0.78 ms per launch; it is now a 388-float record
// in the order the linearisation produces it, written in 16 B pieces, and the QP kernel's prologue gathers its operand tiles
// from the record through a per-lane index map (cj_index) -- the way the stage sweeps synthesise N~ and B~.
//   foot f, floats 88 f ..:  contact rows 3f+i (i < 3):  [6 c + i]      column q(xi_c)       c < 9  (xi = [r, theta, ql_f])
//                                                        [6 c + 3 + i]  column v(xi_c)
//                                                        [54 + i]       column HX (the scaled residual)
//                            swing row 12+f:             [57 + c], [66] column HX            ([67] padding)
//                            placement rows 22+2f+i:     [68 + 10 i + c], [68 + 10 i + 9] column HX
//   consistency, floats 352 ..:  rows 16+i: [3 i] h_lin_i, [3 i + 1] v_i, [3 i + 2] HX;  rows 19+i: [9 + 2 i] h_ang_i, [10 + 2 i] HX,
//                                [15 + 3 a + i] theta_a, [24 + 3 a + i] thetadot_a            ([33..35] padding)
constexpr int CJ_FOOT = 88, CJ_CONS = 4 * CJ_FOOT, CJ_FLOATS = CJ_CONS + 36;
static_assert(CJ_FLOATS % 4 == 0, "records are whole 16 B pieces");
__host__ __device__ constexpr int xi_slot(int f, int qi) {      // inverse of xi_col: slot of coordinate qi in xi_f, or -1
    return qi < 6 ? qi : (qi >= 6 + 3 * f && qi < 9 + 3 * f) ? 6 + (qi - 6 - 3 * f) : -1;
}
// record index of element (row, column POSITION) of Js, or -1 for a structural zero
__host__ __device__ constexpr int cj_index(int row, int col) {
    if (row < 12) {
        const int f = row / 3, i = row % 3;
        if (col == HX) return CJ_FOOT * f + 54 + i;
        if (col < 18) { const int c = xi_slot(f, col); return c < 0 ? -1 : CJ_FOOT * f + 6 * c + i; }
        if (col < 36) { const int c = xi_slot(f, col - 18); return c < 0 ? -1 : CJ_FOOT * f + 6 * c + 3 + i; }
        return -1;
    }
    if (row < 16) {
        const int f = row - 12;
        if (col == HX) return CJ_FOOT * f + 66;
        if (col < 18) { const int c = xi_slot(f, col); return c < 0 ? -1 : CJ_FOOT * f + 57 + c; }
        return -1;
    }
    if (row < 19) {
        const int i = row - 16;
        return col == pos_of(WH + i) ? CJ_CONS + 3 * i : col == WV + i ? CJ_CONS + 3 * i + 1 : col == HX ? CJ_CONS + 3 * i + 2 : -1;
    }
    if (row < 22) {
        const int i = row - 19;
        if (col == pos_of(WH + 3 + i)) return CJ_CONS + 9 + 2 * i;
        if (col == HX) return CJ_CONS + 10 + 2 * i;
        if (col >= WQ + 3 && col < WQ + 6) return CJ_CONS + 15 + 3 * (col - WQ - 3) + i;
        if (col >= WV + 3 && col < WV + 6) return CJ_CONS + 24 + 3 * (col - WV - 3) + i;
        return -1;
    }
    if (row < 30) {
        const int f = (row - 22) / 2, i = (row - 22) % 2;
        if (col == HX) return CJ_FOOT * f + 68 + 10 * i + 9;
        if (col < 18) { const int c = xi_slot(f, col); return c < 0 ? -1 : CJ_FOOT * f + 68 + 10 * i + c; }
        return -1;
    }
    return -1;
}
static_assert(cj_index(0, 0) == 0 && cj_index(5, 18 + 9) == CJ_FOOT + 6 * 6 + 3 + 2 && cj_index(4, 6) == -1 && cj_index(13, HX) == CJ_FOOT + 66, "cj_index");
static_assert(cj_index(17, pos_of(WH + 1)) == CJ_CONS + 3 && cj_index(20, WV + 4) == CJ_CONS + 24 + 3 + 1 && cj_index(29, 2) == CJ_FOOT * 3 + 68 + 10 + 2, "cj_index");
constexpr int XT = 3, UT = 2;          // 16-wide tiles of the state (48) and input (32) dimensions
constexpr int JT = 2;                  // K tiles of the dense residual Jacobian (22 rows)
constexpr int IMG = TILE;              // floats of one tile image (column-major 16x16)
constexpr int QT_FLOATS = XT * XT * IMG, KT_FLOATS = UT * XT * IMG;

// per-node record written by the linearisation (float offsets)
constexpr int R_D = 0;                 // defect d, by POSITION: [48], zero where no state sits
constexpr int R_HQ = 48;               // d h_ang+ / d q[3..17]: [3][16]
constexpr int R_HF = 96;               // d h_ang+ / d f: [3][12]
constexpr int R_CDT = 132;             // dt c_i: d h_lin+ / d f_i = cdt_i I
constexpr int R_R = 136;               // input gradient r[30] (+2)
constexpr int R_C = 168;               // friction pyramid values c = G u - h [16]
constexpr int R_ACT = 184, R_COST = 185;
constexpr int R_ZERO = 186, R_DT = 187, R_DT2 = 224;   // constants the tile synthesis reads like any other entry
constexpr int R_GQ = 188;              // gradient of the diagonal residuals on x[0..35]
constexpr int REC = 228;

struct WbArgs {
    ModelParams mp;
    float W[NY], We[NYE];
    float reg, reg_e;
    int N, B;
    int max_sqp, n_ipm, yref_per_stage, it, shift;
    int precision;      // 0: fp32; 1: bf16 residual Jacobian, J'WJ on the bf16 matrix pipe; 2: split bf16 (hi + lo); 3: hi + mid + lo
    int pos_rows;       // 1: some foot-placement weight (W / W_e rows RY_POS.., RE_POS..) is non-zero
    float nlp_tol, mu0, sigma, s_min, gamma, tau_min;
    const float* x0;
    const float* yref;
    const float* yref_e;
    const float* params;
    float* X;
    float* U;
    int* status;
    float* stats;
    float* ws;
    const int* skip;    // nullptr, or dev [B] flag words: a problem with skip[b] & skip_mask != 0 is left untouched (nmpc_set_skip)
    int skip_mask;
};

__host__ __device__ inline int r4(int n) { return (n + 3) & ~3; }
__device__ __forceinline__ int shifted_node(int k, int shift, int N) { return (k >= 1 && k <= N - shift) ? k + shift : k; }
__device__ __forceinline__ bool shifted_stage_valid(int k, int shift, int N) { return k < N - shift; }

// arrays of the lane = stage phases, feature-major [feature][stage], odd stage stride
struct StageArr {
    int NS, dX, dU, dXp, dUp, sv, lv, total;
    __host__ __device__ explicit StageArr(int N) {
        NS = (N + 1) | 1;
        int o = 0;
        dX = o;  o += r4(NX * NS);
        dU = o;  o += r4(NU * NS);
        dXp = o; o += r4(NX * NS);
        dUp = o; o += r4(NU * NS);
        sv = o;  o += r4(NG * NS);
        lv = o;  o += r4(NG * NS);
        total = o;
    }
};
// workspace of one problem (float offsets)
struct WsLayout {
    size_t rec, js, qt, kt, arr, flag, stride;
    __host__ __device__ explicit WsLayout(int N) {
        size_t o = 0;
        rec = o; o += (size_t)(N + 1) * REC;
        js = o;  o += (size_t)(N + 1) * CJ_FLOATS;
        qt = o;  o += (size_t)(N + 1) * QT_FLOATS;
        kt = o;  o += (size_t)N * KT_FLOATS;
        arr = o; o += StageArr(N).total;
        flag = o; o += 4;
        stride = (o + 63) & ~(size_t)63;
#ifdef WB_T_ODD_STRIDE       // timing build: an odd number of 256 B units per problem (do the problems' images camp on memory channels?)
        if (((stride / 64) & 1) == 0) stride += 64;
#endif
    }
};

// ---- the diagonal residuals (base, joint) sit on the states s < 36: their weight, stage and terminal, and their row of yref ------
__device__ __forceinline__ float wdiag(const WbArgs& a, int s, bool term) {
    const int i = (s < 6) ? RY_BASE + s : (s < 18) ? RY_JOINT + (s - 6) : (s < 24) ? RY_BASE + 6 + (s - 18) : RY_JOINT + 12 + (s - 24);
    return term ? a.We[i] : a.W[i];        // base and joint rows have the same offsets in W and W_e
}
__device__ __forceinline__ int yref_of_state(int s) {
    return (s < 6) ? RY_BASE + s : (s < 18) ? RY_JOINT + (s - 6) : (s < 24) ? RY_BASE + 6 + (s - 18) : RY_JOINT + 12 + (s - 24);
}

// ---- the LDS of the QP kernel (float offsets) ----------------------------------------------------------------------------------
constexpr int LDU = 36;      // LDS column stride of the 32-row elimination columns (Huu | H~ux -> W | Y)
constexpr int LDH = 52;      // LDS column stride of the 48-row transposition buffer of H~xx
constexpr int IPMW = 57;     // LDS row of a stage's barrier-modified input terms: rt[30] at 0, Rf[4][5] at 32
constexpr int IPM_RF = 32;

constexpr int KLD = 20;                      // LDS column stride of a gain tile K~' (conflict-free 16 B row reads)
constexpr int KBUF = UT * XT * 16 * KLD;     // the six tiles of one stage
struct WbLds {
    int colU, hbuf, recb, ipm, klds, n_klds, total;
    __host__ __device__ explicit WbLds(int N) {
        int o = 0;
        colU = o; o += NG * 0 + 32 * LDU;
        hbuf = o; o += 48 * LDH;
        recb = o; o += 256;
        ipm = o;  o += r4(N * IPMW);
        // the gains of the LAST stages of a backward sweep (the first of the forward sweep) stay in the LDS -- as many as fit next to
        // three other waves of the CU (160 KB / 4): the forward sweep starts without a trip to memory and those images never leave the CU
        klds = o;
        n_klds = (o + 2 * KBUF) * 4 <= 40 * 1024 ? 2 : (o + KBUF) * 4 <= 40 * 1024 ? 1 : 0;
        if (n_klds > N) n_klds = N;
        o += n_klds * KBUF;
        total = o;
    }
};

}  // namespace wb
}  // namespace nmpc
