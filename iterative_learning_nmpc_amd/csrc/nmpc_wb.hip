// nmpc_wb.hip -- batched NMPC solve of the whole-body model (nx = 42, nu = 30) on gfx950: a blocked Riccati /
// interior-point kernel family beside the 16x16 single-tile family of nmpc_solve.hip (nmpc_linearize.hip.inc, nmpc_qp.hip.inc).
//
// Replaces, for the problem the reference actually solves (q18 + v18 + h6 | a18 + f12, solver.py:88-92,405-418),
// the per-step solve  QuadrupedAcadosSolver.solve -> acados SQP / HPIPM  (solver.py:396-403).  Two kernels per
// SQP iteration, as in the tile family (nmpc_linearize.hip.inc, nmpc_qp.hip.inc):
//   nmpc_wb_linearize_kernel  one thread per (problem, node): foot kinematics with first and second
//        derivatives, dynamics defect and its non-trivial Jacobian blocks, the scaled dense residual Jacobian
//        Js = sqrt(W) [J | res] of the swing / contact / consistency rows as a compact record (cj_index), gradients of the
//        diagonal residuals, friction-pyramid values.
//   nmpc_wb_qp_kernel  one problem per wavefront, 48x48 homogeneous stage matrices as 3x3 tiles of 16x16 fp32 in
//        the accumulator layout of v_mfma_f32_16x16x4_f32 (nmpc_tile.hpp: X'Y on registers, no data movement):
//        prologue   Q~_k = Js'Js + diag  -- the Gauss-Newton J'WJ contraction -- on the matrix pipe, per node; the operand tiles
//                   gathered from the node's compact record through the LDS
//        phase R    backward sweep: P~A~ (A~ = I + N~), P~B~, H~ux, Huu, H~xx -- the integrator's identity blocks as lane / row
//                   shifts, the momentum rows (registers 0, 1 of tile row 2: pos_of) as two-step MFMA products; LDL' of the
//                   30x30 Huu in column layout (lane = column) applied to [Huu | I] -> W: 4x4 panels factorised on wave-uniform
//                   values, rank-1 updates of the row groups below on v_mfma_f32_4x4x1 with A broadcast (ldl_panel);
//                   Y = W H~ux, P~+ = H~xx - Y'Y, K~' = -Y'W on MFMA tiles
//        phase F    forward sweep: du = K~ dx~ row-per-lane (gain tiles -> LDS -> rows), dx+ from the model's sparse structure
//        phase I    interior point on the friction pyramids, lane = stage, barrier terms G'DG / G'v in closed form
//        phase S    step, status, write-back (warm-start shift folded in as an index map)
// Stage data that does not fit the LDS (Q~, K~' images, 6 + 6 KB per stage and sweep) streams through an HBM workspace;
// the per-stage record, the elimination columns, the transposition buffer and the gains of the last two stages live in the LDS
// (37.8 KB at N = 30: four waves per CU).  DESIGN.md 5b has the measurements behind every choice.
// The family by file: nmpc_wb_model.hpp (the model), nmpc_wb_layout.hpp (sizes, offsets, index maps, argument block: no kernel),
// nmpc_wb_momentum.hpp (records and index map of the articulated momentum model), nmpc_wb_linearize.hip.inc (the linearisation
// kernel), nmpc_wb_ldl.hpp (the LDL' elimination), nmpc_wb_qp.hip.inc (the QP kernel) and this file: the wave helpers only the QP
// kernel uses.  The two kernel files are compiled once per momentum model (WB_ART).  This file includes the others and is what
// nmpc_api.hip includes.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "../../include/nmpc.h"
#include "nmpc_wb_model.hpp"

// Contraction off from here on (as in the QP kernel of nmpc_qp.hip.inc), for every file of the family: every intended a*b + c is an
// fmaf or an MFMA; what the backend would fuse on its own depends on the instantiation.
#pragma clang fp contract(off)

#include "nmpc_wb_layout.hpp"
#include "nmpc_wb_momentum.hpp"
// both kernels of the family once per momentum model: WB_ART = 0 the declared model (the kernels as they were), 1 the articulated one
#define WB_ART 0
#include "nmpc_wb_linearize.hip.inc"
#undef WB_ART
#define WB_ART 1
#include "nmpc_wb_linearize.hip.inc"
#undef WB_ART
#include "nmpc_wb_ldl.hpp"

namespace nmpc {
namespace wb {

// a lane shift inside the 16-lane rows (DPP row_shr:n = 0x110 + n: lane i reads lane i - n; row_shl:n = 0x100 + n: lane i + n);
// lanes whose source falls outside their row read 0
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// the same, for the lanes of bank 0 (lanes 0..3 of every row) only; the others read 0
template <int CTRL>
__device__ __forceinline__ float dpp_row_bank0(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0x1, true));
}
// sum over the 16 lanes of a lane row, in every lane of it (the first four steps of wave_reduce)
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_row<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_row<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_row<0x141>(v);     // row_half_mirror
    v += dpp_row<0x140>(v);     // row_mirror
    return v;
}
// lane row q (16 lanes) of the result takes lane row q + 1 of `a`, the last lane row takes lane row 0 of `b`: the rows 4(q+1)..
// of a tile column, continued into the next tile, moved up by one quad (ds_bpermute: the LDS crossbar, no LDS memory)
// (one crossbar move: the lane row that nobody reads `a` from -- row 0 -- offers `b` instead)
__device__ __forceinline__ float rows_up(float a, float b, int up_addr, bool first_row) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(up_addr, __float_as_int(first_row ? b : a)));
}
__device__ __forceinline__ bool n_tile_nonzero(int k, int j) { return !((k == 0 && j == 0) || (k == 1 && j == 0) || (k == 1 && j == 1)); }
__device__ __forceinline__ bool b_tile_nonzero(int k, int j) { return !(k == 0 && j == 1); }

// Diagnostic build (-DNMPC_WB_STAMPS, tools/wb_stamps.py): cycle counters of the segments of a backward stage and of
// the phases, summed per wave and left in the first Js record of the problem.  The production kernel has no stamp.
#ifdef NMPC_WB_STAMPS
#define WB_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t1_ = __builtin_readcyclecounter(); \
                         st_acc[i] += t1_ - st_t0; st_t0 = t1_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define WB_STAMP(i)
#endif

#define WB_ART 0
#include "nmpc_wb_qp.hip.inc"
#undef WB_ART
#define WB_ART 1
#include "nmpc_wb_qp.hip.inc"
#undef WB_ART

}  // namespace wb
}  // namespace nmpc
