// nmpc_solve_layout.hpp -- what the host and the other kernel files read of the 16x16 tile family (nmpc_solve.hip): the argument
// block, the warm-start shift map, the stage images and their per-lane offsets, the workspace and LDS layouts.  No kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/nmpc.h"
#include "nmpc_models.hpp"
#include "nmpc_sweep.hpp"

namespace nmpc {

struct SolveArgs {
    ModelParams mp;
    float W[32];    // stage weights [nx+nu]
    float rs_free[16];   // 1/sqrt(W_u + reg): row scale of an input that is decoupled at a stage
    float We[16];   // terminal weights [nx]
    float reg, reg_e;
    int N, B;
    int max_sqp, n_ipm, line_search, yref_per_stage;
    int it;               // SQP iteration this launch pair belongs to
    int shift;            // warm-start shift folded into this launch pair's reads of X, U (0: none)
    float nlp_tol, mu0, sigma, s_min, gamma, tau_min, rho;
    const float* x0;
    const float* yref;
    const float* yref_e;
    const float* params;
    float* X;
    float* U;
    int* status;
    float* stats;
    float* ws;            // workspace, WsLayout per problem
    float* dbg;           // diagnostic builds: [B][8] phase cycle counts, else unused
    const int* skip;      // nullptr, or dev [B] flag words: a problem with skip[b] & skip_mask != 0 is left untouched
    int skip_mask;        // (terminated rollouts, nmpc_set_skip)
};

__device__ __forceinline__ bool skipped(const SolveArgs& a, int b) { return a.skip && (a.skip[b] & a.skip_mask) != 0; }

__host__ __device__ inline int round4(int n) { return (n + 3) & ~3; }

// Warm-start shift as an index map (solver.py:304-322, same result as nmpc_shift_kernel): node 0 and
// the last `shift` nodes of X keep their values, nodes 1..N-shift take those `shift` nodes later; U
// moves up by `shift` stages and its tail is zero.  With it the shift costs no launch and no pass
// over memory: the kernels of the first SQP iteration read the previous solution through the map.
__device__ __forceinline__ int shifted_node(int k, int shift, int N) {
    return (k >= 1 && k <= N - shift) ? k + shift : k;
}
__device__ __forceinline__ bool shifted_stage_valid(int k, int shift, int N) { return k < N - shift; }

// Compact stage images in the workspace (tile strides are multiples of 128 B so an image starts
// on a cache line).  Images hold logical indices; the slot layout of the tiles (nmpc_tile.hpp)
// exists only in registers and in the column index of the K~/Acl~ rows:
//   A~ : columns 0..nx (A | d), rows 0..nx-1, column-major, column stride SA = round4(nx) floats
//        (row HS = e_HS is synthesised at load)
//   B~ : columns 0..nu-1, rows 0..nx-1, same column stride
//   K~ : rows 0..nu-1 of [K kff], row-major, 16 floats per row indexed by slot (what the forward
//        sweep multiplies with); rows padded to a multiple of 3
//   Acl~: rows 0..nx-1 of A~ + B~K~, same format
template <class M>
struct TileGeom {
    static_assert(M::NX <= 12 && M::NU <= 12, "slot layout: at most 12 states and 12 inputs");
    static constexpr int SA = (M::NX + 3) & ~3;                       // column stride of A~/B~ images
    static constexpr int RQ = SA / 4;                                 // row quads stored per column
    static constexpr int KQ = (M::NU + 2) / 3;                        // row triples of a K~ image
    static constexpr int CQ = (M::NX + 2) / 3;                        // row triples of an Acl~ image
    static constexpr int A_FLOATS = (((M::NX + 1) * SA) + 31) & ~31;
    static constexpr int B_FLOATS = ((M::NU * SA) + 31) & ~31;
    static constexpr int K_FLOATS = ((3 * KQ * TS) + 31) & ~31;
    static constexpr int C_FLOATS = ((3 * CQ * TS) + 31) & ~31;
};

typedef float f32x3u __attribute__((ext_vector_type(3), aligned(4)));

// Per-lane byte offsets into a stage image, computed once per kernel.  Every access of the stage
// sweeps is  uniform image base + lane offset + immediate  (ld_f32/st_f32): no per-access address
// arithmetic in the VALU.  Loads come in two halves so that a prefetch stays a prefetch: the raw
// load is issued a stage ahead (clamped in-bounds addresses), *_fix masks the padding when the tile
// is consumed.  (Masking at the load would make the wave wait for it on the spot.)
// Lane (q, c) of a tile holds row slots 4q..4q+3 = logical rows 3q..3q+2 (+ padding) of column slot c.
template <class M>
struct ImageLane {
    using G = TileGeom<M>;
    unsigned a_off, b_off, t_off;   // A~ and B~ (three consecutive rows of a column), B~' (3 dwords)
    bool a_ok, b_ok, t_ok;
    __device__ __forceinline__ void init(int lane) {
        const int q = lane >> 4, c = lane & 15;
        const int jc = (c == HS) ? M::NX : index_of(c);       // logical column of A~ (d sits at HS)
        a_ok = (jc >= 0) && (jc <= M::NX) && (3 * q < M::NX);
        b_ok = (index_of(c) >= 0) && (index_of(c) < M::NU) && (3 * q < M::NX);
        a_off = 4u * ((a_ok ? jc : 0) * G::SA + (a_ok ? 3 * q : 0));
        b_off = 4u * ((b_ok ? index_of(c) : 0) * G::SA + (b_ok ? 3 * q : 0));
        // element (slot(u), slot(x)) of B~' is B~[x][u]: image column u = 3q+r, row x
        t_ok = (index_of(c) >= 0) && (index_of(c) < M::NX) && (3 * q < M::NU);
        t_off = 4u * ((t_ok ? 3 * q : 0) * G::SA + (t_ok ? index_of(c) : 0));
    }
    __device__ __forceinline__ f32x4 load3(const float* img, unsigned off) const {
        const f32x3u v = *reinterpret_cast<const f32x3u*>(reinterpret_cast<const char*>(img) + (size_t)off);
        return f32x4{v[0], v[1], v[2], 0.0f};
    }
    __device__ __forceinline__ f32x4 load_A(const float* img) const { return load3(img, a_off); }
    __device__ __forceinline__ f32x4 load_B(const float* img) const { return load3(img, b_off); }
    __device__ __forceinline__ f32x4 load_Bt(const float* img) const {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = ld_f32(img, t_off, 4 * r * G::SA);
        o[3] = 0.0f;
        return o;
    }
    // masks of the raw loads: rows/columns beyond the model's dimensions are zero; A~[HS][HS] = 1
    __device__ __forceinline__ f32x4 fix_A(f32x4 v, int lane) const {
        const int q = lane >> 4, c = lane & 15;
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = (a_ok && 3 * q + r < M::NX) ? v[r] : 0.0f;
        o[3] = (q == 0 && c == HS) ? 1.0f : 0.0f;
        return o;
    }
    __device__ __forceinline__ f32x4 fix_B(f32x4 v, int lane) const {
        const int q = lane >> 4;
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = (b_ok && 3 * q + r < M::NX) ? v[r] : 0.0f;
        o[3] = 0.0f;
        return o;
    }
    __device__ __forceinline__ f32x4 fix_Bt(f32x4 v, int lane) const {
        const int q = lane >> 4;
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = (t_ok && 3 * q + r < M::NU) ? v[r] : 0.0f;
        o[3] = 0.0f;
        return o;
    }
};
// Row-major store of the logical rows of an accumulator-layout tile (registers 0..2 of the first NQ
// quads), 16 floats per row, into the image of stage k of an image array.  Lanes of the other quads
// write to the array's scratch image (slot N) instead, so the store needs no branch.  `off` walks
// down with the stage.
struct RowStoreLane {
    unsigned off, step;
    __device__ __forceinline__ void init(int lane, int nq, int image_floats, int k_first, int k_scratch) {
        const int q = lane >> 4, c = lane & 15;
        const bool valid = q < nq;
        off = 4u * ((valid ? k_first : k_scratch) * image_floats + (valid ? 3 * q * TS : 0) + c);
        step = valid ? 4u * image_floats : 0u;
    }
    __device__ __forceinline__ void store(float* images, f32x4 v) {
#pragma unroll
        for (int r = 0; r < 3; ++r) st_f32(images, off, 4 * r * TS, v[r]);
        off -= step;
    }
};

// Arrays of the lane = stage phases (trajectories, steps, slacks, multipliers).  Two layouts:
//   LDS (resident variant): FEATURE-major, [feature][stage] with an odd stage stride NS, so consecutive lanes touch
//       consecutive banks;
//   workspace (lean variant): STAGE-major, [stage][16]: the lane that owns a stage moves its whole row with three or
//       four 16 B accesses (a feature-major row costs one 4 B access per feature: 100 instead of 35 memory instructions
//       per lane and interior-point iteration), and the forward sweep's row stores of a stage land in one cache line.
// Offsets in floats from the start of the group; nX/nU/nG = extent of a state / input / constraint-row array for the
// element-wise passes (padding of the stage-major rows is zero and stays zero).
template <class M>
struct StageArrays {
    int NS;   // feature-major: stage stride (odd, >= N+1)
    int nX, nU, nG;
    int Xs, Us, dX, dU, dXp, dUp, sv, lv, total;
    __host__ __device__ StageArrays(int N, bool stage_major) {
        NS = (N + 1) | 1;
        nX = stage_major ? (N + 1) * TS : M::NX * NS;
        nU = stage_major ? (N + 1) * TS : M::NU * NS;
        nG = stage_major ? (N + 1) * TS : M::NG * NS;
        int o = 0;
        Xs = o;  o += round4(nX);
        Us = o;  o += round4(nU);
        dX = o;  o += round4(nX);
        dU = o;  o += round4(nU);
        dXp = o; o += round4(nX);
        dUp = o; o += round4(nU);
        sv = o;  o += round4(nG);
        lv = o;  o += round4(nG);
        o += 4;                                   // sink for the idle lanes of the forward sweep
        total = o;
    }
};

// Workspace of one problem (float offsets): stage images A~[N], B~[N], K~[N+1], Acl~[N+1]
// (the extra slot is scratch for the software pipeline), then what the linearisation hands to the
// QP kernel: gradients q[N+1][nx], r[N][nu], constraint values c[N][ng], masks, stage costs, and
// the problem's "finished" flag.
template <class M>
struct WsLayout {
    size_t At, Bt, Kt, Ct, q, r, c, act, umk, cost, flag, lean, stride;
    __host__ __device__ explicit WsLayout(int N) {
        size_t o = 0;
        At = o; o += (size_t)N * TileGeom<M>::A_FLOATS;
        Bt = o; o += (size_t)N * TileGeom<M>::B_FLOATS;
        Kt = o; o += (size_t)(N + 1) * TileGeom<M>::K_FLOATS;
        Ct = o; o += (size_t)(N + 1) * TileGeom<M>::C_FLOATS;
        q = o; o += round4((N + 1) * M::NX);
        r = o; o += round4(N * M::NU);
        c = o; o += round4(N * M::NG);
        act = o; o += round4(N);
        umk = o; o += round4(N);
        cost = o; o += round4(N + 1);
        flag = o; o += 4;
        lean = o; o += StageArrays<M>(N, true).total;     // lane = stage arrays of the lean-LDS kernel variant (stage-major)
        stride = (o + 63) & ~(size_t)63;
    }
};
constexpr int N_LANE_STAGES = 4;   // horizon limit of the lane = stage loops: N <= 256
// true if nmpc_qp_kernel<M, LEAN, ..> linearises its problem itself (then nmpc_linearize_kernel is not launched)
__host__ __device__ constexpr bool qp_linearizes_itself(bool lean, int N) { return lean && N < 64; }

// LDS layout of one problem.  Two variants of the QP kernel:
//   resident (LEAN = false): stage arrays + sweep operands + run schedule + conversion tiles, 39.9 KB at N = 50 ->
//       4 waves per CU, one per SIMD: the choice while the batch fits that many waves (B <= 1024 on an MI355X);
//   lean (LEAN = true): the stage arrays live in the workspace (stage-major rows), 17.8 KB -> 8 waves per CU, two per
//       SIMD: the choice for larger batches (the second wave fills the first one's dependency stalls: 2.7 M solves/s
//       at B = 8192 against 2.3 M), for horizons whose resident layout does not fit the LDS, and NMPC_QP_VARIANT=lean.
// Same arithmetic in the same order: results are bit-identical (tests/test_gpu_parity.py).  DESIGN.md 7.
template <class M, bool LEAN>
struct Lds {
    int arr, qv, rv, gsq, gvt, act, umk, runs, conv, dx0, total;   // float offsets
    __host__ __device__ explicit Lds(int N) {
        const int NS = (N + 1) | 1;
        int o = 0;
        arr = o; o += LEAN ? 0 : StageArrays<M>(N, false).total;
        // sweep operands are STAGE-major, 16 floats per stage: the four tile registers of a lane
        // are one 16 B read (only the stage sweeps touch them after they are written)
        qv = o;  o += (N + 1) * TS;
        rv = o;  o += N * TS;
        gsq = o; o += N * TS;                     // barrier terms of the interior-point iterate, 2 x 16 floats per stage:
        gvt = o; o += N * TS;                     // eight numbers per foot (M::foot_terms), or sqrt(D) | v/sqrt(D) by row
        act = o; o += round4(NS);
        umk = o; o += round4(NS);
        runs = o; o += LEAN ? 0 : round4(N + 1);  // run-length schedule of the backward sweep (resident): at most N runs and the end word
        conv = o; o += CONV_FLOATS;
        dx0 = o; o += LEAN ? TS : 0;              // lean: x0 - X[0], read at the start of every forward sweep
        total = o;
    }
};

}  // namespace nmpc
