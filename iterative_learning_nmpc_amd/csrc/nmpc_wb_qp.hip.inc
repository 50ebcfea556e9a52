// nmpc_wb_qp.hip.inc -- the QP kernel of the whole-body family (see nmpc_wb.hip, which includes this file behind its helpers,
// inside namespace nmpc::wb, once per momentum model).  WB_ART = 0: the declared model, nmpc_wb_qp_kernel, whose text is what it
// was before the second model existed.  WB_ART = 1: the articulated model (nmpc_wb_momentum.hpp), nmpc_wb_qp_art_kernel -- the
// prologue also loads the node's dense consistency record `m.dcons` into the record buffer and gathers the consistency rows of Js
// through cj_index_art; nothing behind the prologue differs.

// QP + step of one SQP iteration: one problem per wavefront.
#if WB_ART
__global__ __launch_bounds__(64, 1) void nmpc_wb_qp_art_kernel(const WbArgs a, const WbArtArgs m) {
#else
__global__ __launch_bounds__(64, 1) void nmpc_wb_qp_kernel(const WbArgs a) {
#endif
#ifdef NMPC_WB_STAMPS
    unsigned long long st_t0 = __builtin_readcyclecounter(), st_acc[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    if (a.skip && (a.skip[b] & a.skip_mask) != 0) return;
    const int lane = lane_id();
    const int q4 = lane >> 4, c = lane & 15;
    const int N = a.N;
    const WsLayout wl(N);
    float* ws = a.ws + (size_t)b * wl.stride;
    int* flag = reinterpret_cast<int*>(ws + wl.flag);
    if (a.it > 0 && flag[0]) return;
    const WbLds L(N);
    const StageArr SA(N);
    const int NS = SA.NS;
    float* arr = ws + wl.arr;
    float* dX = arr + SA.dX;   float* dU = arr + SA.dU;
    float* dXp = arr + SA.dXp; float* dUp = arr + SA.dUp;
    float* sv = arr + SA.sv;   float* lv = arr + SA.lv;
    float* colU = smem + L.colU; float* hbuf = smem + L.hbuf;
    float* recb = smem + L.recb; float* ipm = smem + L.ipm; float* klds = smem + L.klds;
    const float* recs = ws + wl.rec;
    float* Qimg = ws + wl.qt;
    float* Kimg = ws + wl.kt;
    float* Xg = a.X + (size_t)b * (N + 1) * NX;
    float* Ug = a.U + (size_t)b * N * NU;
    const float* x0 = a.x0 + (size_t)b * NX;
    const ModelParams& mp = a.mp;
    const float dt = mp.dt;
#define AT(arr_, k_, i_) (arr_)[(i_) * NS + (k_)]
    auto phase_sync = [&]() { __threadfence_block(); wave_sync(); };

    // ---------------------------------------------------------------- prologue: Q~_k = Js'Js + diag (+ gradient)
    // the Gauss-Newton contraction J'WJ of the dense residual rows on the matrix pipe
    float qdiag[XT], qdiag_e[XT];      // diagonal element this lane may hold in tile (I, I): weight + reg
#pragma unroll
    for (int i = 0; i < XT; ++i) {
        const int row = 16 * i + c;
        const bool mine = (c >> 2) == q4 && state_at(row) >= 0;
        qdiag[i] = mine ? (row < 36 ? wdiag(a, row < 36 ? row : 0, false) : 0.0f) + a.reg : 0.0f;
        qdiag_e[i] = mine ? (row < 36 ? wdiag(a, row < 36 ? row : 0, true) : 0.0f) + a.reg_e : 0.0f;
    }
    // The compact Jacobian record and the gradient entries of node k + 1 are requested while node k is contracted (one node per
    // iteration with its loads at the top waited a full memory latency per node).  A node's record goes through the LDS: two
    // 16 B pieces per lane in, then every lane gathers the 24 elements of its six operand tiles at precomputed indices (cj_index;
    // structural zeros read a slot that holds zero).
    float* const cjbuf = colU;                      // CJ_FLOATS + the zero slot; the elimination's columns are not in use yet
    constexpr int CJ_ZERO = CJ_FLOATS;
    static_assert(CJ_FLOATS + 4 <= 32 * LDU && CJ_FLOATS <= 2 * 64 * 4, "record buffer");
    int jIdx[JT][XT][4];
#pragma unroll
    for (int t = 0; t < JT; ++t)
#pragma unroll
        for (int j = 0; j < XT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#if WB_ART
                const int ci = cj_index_art(16 * t + 4 * q4 + r, 16 * j + c);
#else
                const int ci = cj_index(16 * t + 4 * q4 + r, 16 * j + c);
#endif
                jIdx[t][j][r] = ci >= 0 ? ci : CJ_ZERO;
            }
    if (lane == 0) *reinterpret_cast<f32x4*>(cjbuf + CJ_ZERO) = zero4();
    const bool cj_second = 4 * (lane + 64) < CJ_FLOATS;      // the record is 97 pieces: lanes 0..32 carry a second one
    f32x4 cjA, cjB, gcol_n[XT];
#if WB_ART
    const bool cj_dense = 4 * lane < DC_FLOATS;              // the dense consistency record is 54 pieces: one for each of lanes 0..53
    f32x4 cjC;
#endif
    float grow_n[XT];
    auto request_node = [&](int k) {
        const float* js = ws + wl.js + (size_t)k * CJ_FLOATS;
        const float* rec = recs + (size_t)k * REC;
        cjA = *reinterpret_cast<const f32x4*>(js + 4 * lane);
        cjB = *reinterpret_cast<const f32x4*>(js + (cj_second ? 4 * (lane + 64) : 0));
#if WB_ART
        cjC = *reinterpret_cast<const f32x4*>(m.dcons + ((size_t)b * (N + 1) + k) * DC_FLOATS + (cj_dense ? 4 * lane : 0));
#endif
        // gradient of the diagonal residuals: column HX (lanes c == 10 of tile column 2) and row HX
#pragma unroll
        for (int i = 0; i < XT; ++i) {
            const int row0 = 16 * i + 4 * q4;
            gcol_n[i] = *reinterpret_cast<const f32x4*>(rec + R_GQ + (row0 < 36 ? row0 : 0));
        }
#pragma unroll
        for (int j = 0; j < XT; ++j) { const int col = 16 * j + c; grow_n[j] = rec[R_GQ + (col < 36 ? col : 0)]; }
    };
    request_node(0);
    for (int k = 0; k <= N; ++k) {
        const bool term = (k == N);
        f32x4 J[JT][XT], gcol[XT];
        float grow[XT];
        *reinterpret_cast<f32x4*>(cjbuf + 4 * lane) = cjA;
        if (cj_second) *reinterpret_cast<f32x4*>(cjbuf + 4 * (lane + 64)) = cjB;
#if WB_ART
        if (cj_dense) *reinterpret_cast<f32x4*>(cjbuf + CJ_ART + 4 * lane) = cjC;
#endif
#pragma unroll
        for (int i = 0; i < XT; ++i) { gcol[i] = gcol_n[i]; grow[i] = grow_n[i]; }
        request_node(k < N ? k + 1 : N);
        wave_sync();
#pragma unroll
        for (int t = 0; t < JT; ++t)
#pragma unroll
            for (int j = 0; j < XT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) J[t][j][r] = cjbuf[jIdx[t][j][r]];
        wave_sync();      // (the next node's record is written behind these reads: the LDS serves a wave in order)
        // mixed precision (BASELINE configs[4]): the scaled Jacobian rounded to bf16 -- or split into a bf16 head and a
        // bf16 tail, J = hi + lo -- and contracted on the bf16 matrix pipe with fp32 accumulation
        // (v_mfma_f32_16x16x16_bf16: one instruction per 16 residual rows where fp32 takes four steps); the accumulator
        // layout of a tile is that instruction's operand layout (nmpc_tile.hpp).  Everything downstream stays fp32.
        s16x4 Jh[JT][XT], Jm[JT][XT], Jl[JT][XT];
        if (a.precision != 0) {
            auto widen = [](s16x4 v) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = __uint_as_float(((unsigned)(unsigned short)v[r]) << 16);
                return o;
            };
#pragma unroll
            for (int t = 0; t < JT; ++t)
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    Jh[t][j] = to_bf16x4(J[t][j]);
                    const f32x4 r1 = J[t][j] - widen(Jh[t][j]);          // exact: the head's 8 bits leave a 16-bit remainder
                    Jm[t][j] = to_bf16x4(r1);                            // precision 2 calls this part "lo"
                    Jl[t][j] = to_bf16x4(r1 - widen(Jm[t][j]));          // precision 3 only: J = hi + mid + lo to 24 bits
                }
        }
        // diagonal, gradient column / row, and store -- called right behind the products of each precision branch, so
        // that the MFMA results are consumed in the block that produced them
        auto finish = [&](int i, int j, f32x4 acc) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * q4 + r, col = 16 * j + c;
                float v = acc[r];
                if (i == j && r == (c & 3)) v += term ? qdiag_e[i] : qdiag[i];      // row == col <=> r == c - 4q
                if (col == HX && row < 36) v += gcol[i][r];
                if (row == HX && col < 36) v += grow[j];
                if (row == HX && col == HX) v = 0.0f;
                acc[r] = v;
            }
            store_tile(Qimg + (size_t)k * QT_FLOATS + (i * XT + j) * IMG, lane, acc);
        };
        if (a.precision == 0) {
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    if (j > i && !term) continue;      // the sweep reads the lower tiles of a running node, all nine of the terminal one
                    f32x4 acc = zero4();
#pragma unroll
                    for (int t = 0; t < JT; ++t) acc = xty(J[t][i], J[t][j], acc);
                    finish(i, j, acc);
                }
        } else if (a.precision != 3) {
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    if (j > i && !term) continue;      // the sweep reads the lower tiles of a running node, all nine of the terminal one
                    f32x4 acc = zero4();
#pragma unroll
                    for (int t = 0; t < JT; ++t) {
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jh[t][i], Jh[t][j], acc, 0, 0, 0);
                        if (a.precision == 2) {      // (hi + lo)'(hi + lo) without the lo'lo term (2^-16 of the product)
                            acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jh[t][i], Jm[t][j], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jm[t][i], Jh[t][j], acc, 0, 0, 0);
                        }
                    }
                    finish(i, j, acc);
                }
        } else {
            // three-way split: J = hi + mid + lo carries the 24 bits of the fp32 Jacobian; of the nine products the six of
            // relative size >= 2^-16 are formed (mid'lo, lo'mid, lo'lo are below fp32 rounding), smallest first, each
            // bf16 x bf16 product exact in the fp32 accumulator: the Hessian differs from the fp32 contraction by
            // accumulation order only.  Six instructions of K = 16 per 16 residual rows against four fp32 steps of K = 4.
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    if (j > i && !term) continue;      // the sweep reads the lower tiles of a running node, all nine of the terminal one
                    f32x4 acc = zero4();
#pragma unroll
                    for (int t = 0; t < JT; ++t) {
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jl[t][i], Jh[t][j], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jh[t][i], Jl[t][j], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jm[t][i], Jm[t][j], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < JT; ++t) {
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jm[t][i], Jh[t][j], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jh[t][i], Jm[t][j], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < JT; ++t)
                        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(Jh[t][i], Jh[t][j], acc, 0, 0, 0);
                    finish(i, j, acc);
                }
        }
    }
    WB_STAMP(12);
    // cost, active rows, cold start of the interior point: s = max(-c, s_min), lam = mu0 / s
    float cost_l = 0.0f, mu_l = 0.0f;
    int nact_l = 0;
    unsigned my_act = 0u;
    for (int k = lane; k <= N; k += 64) cost_l += recs[(size_t)k * REC + R_COST];     // (N = 64: node 64 has no lane of its own)
    float s_init[NG], l_init[NG], c_init[NG], r_init[NU];      // (the first sweep's barrier terms are formed from these, below)
    {
        const float* rec = recs + (size_t)(lane < N ? lane : 0) * REC;
        if (lane < N) {
            my_act = reinterpret_cast<const unsigned*>(rec)[R_ACT];
            nact_l = __popc(my_act);
            mu_l = a.mu0 * (float)nact_l;
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) r_init[i] = rec[R_R + i];
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            c_init[j] = rec[R_C + j];
            s_init[j] = fmaxf(-c_init[j], a.s_min);
            l_init[j] = a.mu0 * fast_rcp(s_init[j]);
            if (lane < N) { AT(sv, lane, j) = s_init[j]; AT(lv, lane, j) = l_init[j]; }
        }
    }
    const float cost = wave_sum(cost_l);
    const int n_act = (int)(wave_sum((float)nact_l) + 0.5f);
    float mu_sum = wave_sum(mu_l);
    const bool use_ipm = (a.n_ipm > 0) && (n_act > 0);
    const int n_sweeps = use_ipm ? a.n_ipm : 1;
    phase_sync();

    // barrier-modified input terms of stage `lane`, lane = stage: rt = r + G'(tau/s + lam + D c), Rf = G'DG per foot
    // barrier-modified input terms of stage `lane` into its LDS row, from the stage's slacks, multipliers, constraint values and
    // input gradient in registers
    auto ipm_terms = [&](float tau, const float (&sj)[NG], const float (&lj)[NG], const float (&cj)[NG], const float (&rr)[NU]) {
        if (lane < N) {
            float* row = ipm + lane * IPMW;
#pragma unroll
            for (int i = 0; i < WF; ++i) row[i] = rr[i];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                float D[4], v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool on = use_ipm && ((my_act >> (4 * f + j)) & 1u);
                    const float s = sj[4 * f + j], l = lj[4 * f + j];
                    const float is = fast_rcp(s);
                    D[j] = on ? l * is : 0.0f;
                    v[j] = on ? tau * is + l + l * is * cj[4 * f + j] : 0.0f;
                }
                row[WF + 3 * f + 0] = rr[WF + 3 * f + 0] + (v[0] - v[1]);
                row[WF + 3 * f + 1] = rr[WF + 3 * f + 1] + (v[2] - v[3]);
                row[WF + 3 * f + 2] = rr[WF + 3 * f + 2] - mp.mu * ((v[0] + v[1]) + (v[2] + v[3]));
                row[IPM_RF + 5 * f + 0] = D[0] + D[1];
                row[IPM_RF + 5 * f + 1] = D[2] + D[3];
                row[IPM_RF + 5 * f + 2] = mp.mu * mp.mu * ((D[0] + D[1]) + (D[2] + D[3]));
                row[IPM_RF + 5 * f + 3] = -mp.mu * (D[0] - D[1]);
                row[IPM_RF + 5 * f + 4] = -mp.mu * (D[2] - D[3]);
            }
        }
    };

    if (lane < N) ipm[lane * IPMW + IPMW - 1] = 0.0f;
    // the weight-derived constants of the backward sweep (loads from the argument block: once per kernel, unlike the index maps)
    float rdiag_w[UT][4], rs_free_w[12];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < UT; ++i) {
            const int uu = 16 * i + 4 * q4 + r;
            float w = 0.0f;
            if (uu >= 6 && uu < 18) w = a.W[RY_ACC + (uu >= 6 && uu < 18 ? uu - 6 : 0)];
            if (uu >= WF && uu < NU) w = a.W[RY_FREG + (uu >= WF && uu < NU ? uu - WF : 0)];
            rdiag_w[i][r] = (uu == 16 * i + c && uu < NU) ? w + a.reg : 0.0f;
        }
#pragma unroll
    for (int i = 0; i < 12; ++i) rs_free_w[i] = __builtin_amdgcn_rsqf((a.W[RY_FREG + i] + a.reg) + 0.0f);
    // barrier terms of the first sweep, from the registers of the cold start (read back from memory they cost a store -> load trip)
    ipm_terms(use_ipm ? fmaxf(a.sigma * mu_sum / (float)n_act, a.tau_min) : 0.0f, s_init, l_init, c_init, r_init);
    wave_sync();
    bool qp_ok = true;
    // What a backward sweep starts from -- terminal P~ (nine tiles), the records of stages N-1 and N-2, the lower Q~ tiles of stage
    // N-1 -- is the same for every sweep of a call and is requested at the top of the interior-point phase BEFORE it, so that the
    // sweep does not open with a memory latency.
    f32x4 P[XT][XT], Qn[XT][XT], rec_first, rec_pref;
    auto request_sweep = [&]() {
#pragma unroll
        for (int i = 0; i < XT; ++i)
#pragma unroll
            for (int j = 0; j < XT; ++j) P[i][j] = load_tile(Qimg + (size_t)N * QT_FLOATS + (i * XT + j) * IMG, lane);
        rec_first = *reinterpret_cast<const f32x4*>(recs + (size_t)(N - 1) * REC + (4 * lane < REC ? 4 * lane : 0));
        rec_pref = *reinterpret_cast<const f32x4*>(recs + (size_t)(N > 1 ? N - 2 : 0) * REC + (4 * lane < REC ? 4 * lane : 0));
#pragma unroll
        for (int i = 0; i < XT; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) Qn[i][j] = load_tile(Qimg + (size_t)(N - 1) * QT_FLOATS + (i * XT + j) * IMG, lane);
    };
    request_sweep();
    for (int ii = 0; ii < n_sweeps; ++ii) {
        const float tau = use_ipm ? fmaxf(a.sigma * mu_sum / (float)n_act, a.tau_min) : 0.0f;
        // Everything below that is derived from the lane index -- the index maps of the tile synthesis, LDS addresses of the layout
        // changes, masks -- is recomputed at the top of every sweep from a copy of the lane index the optimiser cannot see through:
        // ~150 integer operations per sweep.  Computed once per kernel (where loop-invariant code motion puts them) these ~100
        // registers stay live through the forward sweep and the interior-point phase, which then keep their own working set --
        // the gain rows of the next two stages -- in the accumulation registers and move every element back before use.
        int lane_opaque = lane;
        asm volatile("" : "+v"(lane_opaque));
        const int lane = lane_opaque, q4 = lane >> 4, c = lane & 15;
        // per-lane constants of the tile synthesis: every element of N~ = A~ - I, B~, R~ and S~ is ONE LDS read at a
        // precomputed index -- into the stage record (defect, momentum Jacobians, or one of its constant slots 0, dt, dt^2)
        // or into the stage's row of barrier-modified input terms.  (Lane predicates instead of indices cost an SGPR pair
        // per element and tile: the loop-invariant masks spilled 626 SGPRs into VGPR lanes.)
        constexpr int NT = 6, BT = 5;
        // non-zero tiles of N~: (0,1) (0,2) (1,2) (2,0) (2,1) (2,2) ; of B~: (0,0) (1,0) (1,1) (2,0) (2,1)
        int nIdx[NT][4], bIdx[BT][4], rIdx[4], sIdx[UT][4];
        float rdiag[UT][4];
        {
            constexpr int nt_i[NT] = {0, 0, 1, 2, 2, 2}, nt_j[NT] = {1, 2, 2, 0, 1, 2};
            constexpr int bt_i[BT] = {0, 1, 1, 2, 2}, bt_j[BT] = {0, 0, 1, 0, 1};
    #pragma unroll
            for (int t = 0; t < NT; ++t)
    #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * nt_i[t] + 4 * q4 + r, col = 16 * nt_j[t] + c;
                    int idx = R_ZERO;
                    if (row < 18 && col == row + 18) idx = R_DT;
                    const int sr = state_at(row);
                    if (col == HX && sr >= 0) idx = R_D + row;
                    if (sr >= 39 && sr < 42 && col >= 3 && col < 18) idx = R_HQ + (sr - 39) * 16 + (col - 3);
                    nIdx[t][r] = idx;
                }
    #pragma unroll
            for (int t = 0; t < BT; ++t)
    #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bt_i[t] + 4 * q4 + r, uc = 16 * bt_j[t] + c;
                    int idx = R_ZERO;
                    if (uc < 18 && row == uc) idx = R_DT2;
                    // (dt at (v_16, a_16), (v_17, a_17) of tile (2,1) is applied without the matrix pipe, so that the tile's only non-zero
                    //  rows are momentum rows: contraction steps 0, 1)
                    if (uc < 18 && row == uc + 18 && !(bt_i[t] == 2 && bt_j[t] == 1)) idx = R_DT;
                    if (uc >= WF && uc < NU) {
                        const int f = uc - WF, sr = state_at(row);
                        if (sr >= 36 && sr < 39 && sr - 36 == f % 3) idx = R_CDT + f / 3;
                        if (sr >= 39 && sr < 42) idx = R_HF + (sr - 39) * 12 + f;
                    }
                    bIdx[t][r] = idx;
                }
            // input-cost tile (1,1): the barrier block of the foot, and the diagonal W_acc / W_cnt_f_reg + reg of (0,0), (1,1)
    #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ur = 16 + 4 * q4 + r, uc = 16 + c;
                int idx = IPMW - 1;                                  // a slot that holds zero
                if (ur >= WF && ur < NU && uc >= WF && uc < NU) {
                    const int fr = ur - WF, fc = uc - WF;
                    if (fr / 3 == fc / 3) {
                        const int ar = fr % 3, ac = fc % 3;
                        const int sel = (ar == ac) ? ar : (ar + ac == 2) ? 3 : (ar + ac == 3) ? 4 : -1;
                        if (sel >= 0) idx = IPM_RF + 5 * (fr / 3) + sel;
                    }
                }
                rIdx[r] = idx;
    #pragma unroll
                for (int i = 0; i < UT; ++i) {
                    const int uu = 16 * i + 4 * q4 + r;
                    rdiag[i][r] = rdiag_w[i][r];
                    sIdx[i][r] = (c == HX - 32 && uu < NU) ? uu : IPMW - 1;      // S~: the input gradient rides in column HX
                }
            }
        }
        // constants of the identity blocks of B~ (see the backward stage): dt^2, on columns 0, 1 of a tile, on rows 0, 1 of a tile
        // 1 / sqrt of the pivot of a decoupled force input, by component: Huu[j][j] = (W_f_reg + reg) + 0 there (see ldl_panel)
        float rs_free[12];
    #pragma unroll
        for (int i = 0; i < 12; ++i) rs_free[i] = rs_free_w[i];
        const float dt2 = dt * dt;
        const float dt2_c01 = (c < 2) ? dt2 : 0.0f, dt_c01 = (c < 2) ? dt : 0.0f;
        const int up_addr = 4 * ((lane + 16) & 63);
        const int down_addr = 4 * ((lane + 48) & 63);               // the lane one lane row (16 lanes) before this one
        const float dt_qn0 = (q4 > 0) ? dt : 0.0f;
        const bool first_row = lane < 16;
        const int x16_addr = 4 * (lane ^ 16), x32_addr = 4 * (lane ^ 32);
        const float dt_q0 = (q4 == 0) ? dt : 0.0f;
        const bool hx_col = (c == HX - 32), hx_row = (q4 == HXQ);     // HX = 38: column 6 of tile column 2; row 6 of tile row 2 = lane row 1, register 2
        // where this lane finds, in the stage record, the defects of its columns (one per tile column) ...
        int dcolIdx[XT];
    #pragma unroll
        for (int kk = 0; kk < XT; ++kk) dcolIdx[kk] = R_D + 16 * kk + c;      // (the record holds zeros where no state sits)
        float dt2_r01[4];
    #pragma unroll
        for (int r = 0; r < 4; ++r) dt2_r01[r] = (4 * q4 + r < 2) ? dt2 : 0.0f;

        // ------------------------------------------------------------ phase R: backward sweep
        // (terminal P~, the records of stages N-1 and N-2 and the Q~ tiles of stage N-1 were requested by request_sweep())
        // record of stage N-1 into the LDS; each stage prefetches the next one's (global -> registers -> LDS)
        *reinterpret_cast<f32x4*>(recb + 4 * lane) = rec_first;
        // The record of stage k-1 is requested in the middle of stage k+1, next to the Q~ tiles -- BEFORE that stage's K~ stores.
        // vmcnt retires in order: requested at the top of stage k (behind the six K~ stores of stage k+1), waiting for it meant
        // waiting for those stores to reach memory, every stage (s_waitcnt vmcnt(0) in the middle of the stage).
        wave_sync();
        // Q~ tiles (lower ones) are requested one and a half stages ahead of their use: for stage k-1 in the middle of
        // stage k.  (A timing build that reads one cache-resident image instead of each stage's own ran 10 % faster:
        // requested at the top of their own stage, the 6 KB did not arrive by the time H needs them.)
        WB_STAMP(21);          // terminal tiles, first record and Q~ tiles requested
        for (int k = N - 1; k >= 0; --k) {
            const int kn = k > 0 ? k - 1 : 0;
            WB_STAMP(19);      // the loop's back edge
            // prefetch: next record, this stage's Q~ tiles were requested ... (Q of stage k is loaded here; the
            // loads are issued first and consumed after the P~A~, P~B~ products)
            const f32x4 rec_next = rec_pref;
            f32x4 Q[XT][XT];
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) Q[i][j] = Qn[i][j];
            const float* rk = recb;
            const float* ik = ipm + k * IPMW;
            // contact pattern of the stage from the record's dt c_f (wave-uniform; read now: the record is replaced mid-stage)
            const unsigned pat = __builtin_amdgcn_readfirstlane((rk[R_CDT] > 0.0f ? 1u : 0u) | (rk[R_CDT + 1] > 0.0f ? 2u : 0u) |
                                                                (rk[R_CDT + 2] > 0.0f ? 4u : 0u) | (rk[R_CDT + 3] > 0.0f ? 8u : 0u));
            WB_STAMP(0);
            // ---- synthesise N~ = A~ - I and B~ tiles from the record (one LDS read per element)
            f32x4 Nt[XT][XT], Bt[XT][UT];
            {
                constexpr int nt_i[NT] = {0, 0, 1, 2, 2, 2}, nt_j[NT] = {1, 2, 2, 0, 1, 2};
                constexpr int bt_i[BT] = {0, 1, 1, 2, 2}, bt_j[BT] = {0, 0, 1, 0, 1};
                Nt[0][0] = Nt[1][0] = Nt[1][1] = zero4();
                Bt[0][1] = zero4();
                Nt[0][1] = Nt[0][2] = Nt[1][2] = Nt[2][2] = zero4();       // (their products are formed without the matrix pipe, see below)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (nt_j[t] != 2 && nt_i[t] == 2) {      // the dense tiles: momentum rows against q (2,0), (2,1)
#pragma unroll
                        for (int r = 0; r < 4; ++r) Nt[nt_i[t]][nt_j[t]][r] = rk[nIdx[t][r]];
                    }
#pragma unroll
                for (int t = 0; t < BT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Bt[bt_i[t]][bt_j[t]][r] = rk[bIdx[t][r]];
            }
            // the defect of the stage: by column of this lane (P~ d) and by row quad of this lane (d'(P~A~)); d[42], d[43] are zero
            float dcol[XT], drow[XT][4];
#pragma unroll
            for (int kk = 0; kk < XT; ++kk) {
                dcol[kk] = rk[dcolIdx[kk]];
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(rk + R_D + 16 * kk + 4 * q4);
#pragma unroll
                for (int r = 0; r < 4; ++r) drow[kk][r] = d4[r];
            }
            WB_STAMP(1);
            // ---- P~A~ = P~ + P~N~ ,  P~B~
            // Where a tile of N~ or B~ holds nothing but the integrator's identities -- N~(0,1): dt at (q_r, v_r); B~(.,0): dt^2 at
            // (q_c, a_c) and dt at (v_c, a_c) -- the product with P~ is a COLUMN SHIFT of P~ by 18 = 16 + 2 columns: a lane shift
            // by two inside the 16-lane rows of the accumulator layout (DPP row_shr / row_shl, no matrix instruction).  Every
            // output element has the same non-zero terms in the same order as the MFMA chain had (its other terms were exact
            // zeros), so the results are bit-identical: 48 of the 132 MFMAs of this segment become 48 VALU operations.
            f32x4 PA[XT][XT], PB[XT][UT];
#pragma unroll
            for (int i = 0; i < XT; ++i) {
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    f32x4 acc = P[i][j];
                    if (j == 1) {            // kk = 0: (P~ N~)[:, 18 + c] = dt P~[:, c], c <= 13
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(dt, dpp_row<0x112>(P[i][0][r]), acc[r]);      // row_shr:2
                    }
                    if (j == 2) {
                        // the tiles N~(.,2) hold dt at (q_14..q_17, v_14..v_17) -- column shifts as above -- and the defect d in the
                        // homogeneous column: (P~ N~)[:, HX] = P~ d, one column from a contraction over all 42 states.  On the
                        // matrix pipe that column costs 36 MFMAs per stage; here every lane multiplies its row quad of P~ with the
                        // defects of its columns (three fma per register) and the 16 lanes of a row add up (four DPP steps)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            acc[r] = __builtin_fmaf(dt, dpp_row<0x10E>(P[i][0][r]), acc[r]);              // row_shl:14: columns 14, 15 -> 32, 33
                            acc[r] = __builtin_fmaf(dt, dpp_row_bank0<0x112>(P[i][1][r]), acc[r]);        // row_shr:2, lanes 2, 3: columns 16, 17 -> 34, 35
                            float t = P[i][0][r] * dcol[0];
                            t = __builtin_fmaf(P[i][1][r], dcol[1], t);
                            t = __builtin_fmaf(P[i][2][r], dcol[2], t);
                            t = row_sum16(t);
                            acc[r] += hx_col ? t : 0.0f;
                        }
                    }
#pragma unroll
                    for (int kk = 0; kk < XT; ++kk)
                        if (n_tile_nonzero(kk, j) && !(kk == 0 && j == 1) && j != 2) {
                            static_assert(XT == 3, "the dense tiles of N~ are those of tile row 2");
                            if (kk == 2) acc = xty01(P[kk][i], Nt[kk][j], acc);      // momentum rows only: steps 0, 1
                        }
                    PA[i][j] = acc;
                }
                {   // j = 0 (inputs a_0..a_15): (P~ B~)[:, a_c] = dt^2 P~[:, c] + dt P~[:, 18 + c]
                    f32x4 acc;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float t = dt2 * P[i][0][r];
                        t = __builtin_fmaf(dt, dpp_row<0x102>(P[i][1][r]), t);      // row_shl:2: columns 18..31 of P~ onto lanes 0..13
                        t = __builtin_fmaf(dt, dpp_row<0x11E>(P[i][2][r]), t);      // row_shr:14: columns 32, 33 onto lanes 14, 15
                        acc[r] = t;
                    }
                    PB[i][0] = acc;
                }
                {   // j = 1 (a_16, a_17, f): B~(1,1) holds nothing but dt^2 at (q_16, a_16), (q_17, a_17) -- columns 16, 17 of P~ in
                    // place, scaled; the rest (dt at v_16, v_17 and the wrench map of the forces) is the tile B~(2,1)
                    f32x4 acc;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        acc[r] = dt2_c01 * P[i][1][r];
                        acc[r] = __builtin_fmaf(dt_c01, dpp_row<0x102>(P[i][2][r]), acc[r]);      // dt at (v_16, a_16), (v_17, a_17): columns 34, 35 onto lanes 0, 1
                    }
                    PB[i][1] = xty01(P[2][i], Bt[2][1], acc);      // the wrench map of the forces: momentum rows only
                }
            }
            WB_STAMP(2);
            // ---- H~ux = S~ + B~'(P~A~) (stays in registers) ,  Huu = R~ + B~'(P~B~)  -> LDS columns
            // (products are written step by step over several output tiles at once: a dependent fp32 MFMA waits 40
            //  cycles for its accumulator, an independent one issues after 32 -- tools/wb_stamps.py)
            f32x4 Hux[UT][XT], Huu[UT][UT];
#pragma unroll
            for (int i = 0; i < UT; ++i) {
#pragma unroll
                for (int j = 0; j < XT; ++j) {
                    Hux[i][j] = zero4();
                    if (j == 2) {   // S~: the input gradient rides in column HX
#pragma unroll
                        for (int r = 0; r < 4; ++r) Hux[i][j][r] = ik[sIdx[i][r]];
                    }
                }
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    Huu[i][j] = zero4();
                    if (i == j) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) Huu[i][j][r] = rdiag[i][r] + (i == 1 ? ik[rIdx[r]] : 0.0f);
                    }
                }
                // kk = i: B~(i,i) is dt^2 on its diagonal (all of it for i = 0, rows a_16, a_17 for i = 1) -- B~(i,i)' X is X scaled
                // in place, the first term of every element as in the MFMA chain it replaces
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sc = (i == 0) ? dt2 : dt2_r01[r];
#pragma unroll
                    for (int j = 0; j < XT; ++j) Hux[i][j][r] = __builtin_fmaf(sc, PA[i][j][r], Hux[i][j][r]);
#pragma unroll
                    for (int j = 0; j <= i; ++j) Huu[i][j][r] = __builtin_fmaf(sc, PB[i][j][r], Huu[i][j][r]);
                }
                if (i == 0) {
                    // kk = 1, 2 for the inputs a_0..a_15: B~(1,0), B~(2,0) hold nothing but dt at (v_c, a_c) -- row 18 + c of X onto
                    // row c.  In the accumulator layout rows 18 + 4q + r are registers 2, 3 of the same lane (r = 0, 1) and
                    // registers 0, 1 one lane row (16 lanes) further on (r = 2, 3; the last lane row takes rows 32, 33 from tile
                    // row 2): one crossbar move per such register, no matrix instruction
#pragma unroll
                    for (int j = 0; j < XT; ++j) {
                        Hux[0][j][0] = __builtin_fmaf(dt, PA[1][j][2], Hux[0][j][0]);
                        Hux[0][j][1] = __builtin_fmaf(dt, PA[1][j][3], Hux[0][j][1]);
                        Hux[0][j][2] = __builtin_fmaf(dt, rows_up(PA[1][j][0], PA[2][j][0], up_addr, first_row), Hux[0][j][2]);
                        Hux[0][j][3] = __builtin_fmaf(dt, rows_up(PA[1][j][1], PA[2][j][1], up_addr, first_row), Hux[0][j][3]);
                    }
                    Huu[0][0][0] = __builtin_fmaf(dt, PB[1][0][2], Huu[0][0][0]);
                    Huu[0][0][1] = __builtin_fmaf(dt, PB[1][0][3], Huu[0][0][1]);
                    Huu[0][0][2] = __builtin_fmaf(dt, rows_up(PB[1][0][0], PB[2][0][0], up_addr, first_row), Huu[0][0][2]);
                    Huu[0][0][3] = __builtin_fmaf(dt, rows_up(PB[1][0][1], PB[2][0][1], up_addr, first_row), Huu[0][0][3]);
                }
                if (i == 1) {
                    // kk = 2, inputs a_16, a_17: dt at (v_16, a_16), (v_17, a_17) -- rows 34, 35 of X (registers 2, 3 of lane row 0 of tile
                    // row 2) onto rows a_16, a_17 (registers 0, 1 of lane row 0)
#pragma unroll
                    for (int j = 0; j < XT; ++j) {
                        Hux[1][j][0] = __builtin_fmaf(dt_q0, PA[2][j][2], Hux[1][j][0]);
                        Hux[1][j][1] = __builtin_fmaf(dt_q0, PA[2][j][3], Hux[1][j][1]);
                    }
#pragma unroll
                    for (int j = 0; j <= 1; ++j) {
                        Huu[1][j][0] = __builtin_fmaf(dt_q0, PB[2][j][2], Huu[1][j][0]);
                        Huu[1][j][1] = __builtin_fmaf(dt_q0, PB[2][j][3], Huu[1][j][1]);
                    }
                }
#pragma unroll
                for (int kk = 0; kk < XT; ++kk)
                    if (b_tile_nonzero(kk, i) && kk != i && i != 0) {
                        static_assert(XT == 3, "the one dense tile of B~ left for the matrix pipe is (2,1): momentum rows, steps 0, 1");
#pragma unroll
                        for (int st = 0; st < 2; ++st) {
#pragma unroll
                            for (int j = 0; j < XT; ++j) Hux[i][j] = mfma4(Bt[kk][i][st], PA[kk][j][st], Hux[i][j]);
#pragma unroll
                            for (int j = 0; j <= i; ++j) Huu[i][j] = mfma4(Bt[kk][i][st], PB[kk][j][st], Huu[i][j]);
                        }
                    }
                // lower tiles only; lane L > j of the elimination reads row j of column L (upper triangle), so the
                // off-diagonal tile is written a second time, transposed, into the (0,1) position
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    *reinterpret_cast<f32x4*>(colU + (16 * j + c) * LDU + 16 * i + 4 * q4) = Huu[i][j];
                    if (i != j) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) colU[(16 * i + 4 * q4 + r) * LDU + 16 * j + c] = Huu[i][j][r];
                    }
                }
            }
            WB_STAMP(3);
            // ---- H = Q~ + P~A~ + N~'(P~A~), lower tiles only; the upper ones and the symmetrisation of the diagonal
            // tiles come back transposed from the LDS: H~xx is symmetric bit for bit
            f32x4 H[XT][XT];
            // registers 2, 3 of tile row 0 of P~A~, one lane row back (lane row 0 reads lane row 3): rows q_2.. onto rows v_2.. of tile row 1
            // and rows q_14, q_15 onto v_14, v_15 of tile row 2 -- one crossbar move per register serves both
            float pa_dn2[XT], pa_dn3[XT];
#pragma unroll
            for (int j = 0; j < XT; ++j) {
                pa_dn2[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(down_addr, __float_as_int(PA[0][j][2])));
                pa_dn3[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(down_addr, __float_as_int(PA[0][j][3])));
            }
#pragma unroll
            for (int i = 0; i < XT; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) H[i][j] = Q[i][j] + PA[i][j];
                if (i == 2) {
                    // N~(.,2)'(P~A~): rows v_14..v_17 = dt x rows q_14..q_17 of P~A~ (quad 3 of tile row 0 and quad 0 of tile row 1 onto
                    // quad 0 of tile row 2), and the homogeneous row = d'(P~A~): every lane adds up its row quads against the
                    // defects of its rows (twelve fma per column tile), the four lane rows of a column meet through the crossbar
#pragma unroll
                    for (int j = 0; j < XT; ++j) {
                        const float v14 = pa_dn2[j], v15 = pa_dn3[j];
                        H[2][j][0] = __builtin_fmaf(dt_q0, v14, H[2][j][0]);
                        H[2][j][1] = __builtin_fmaf(dt_q0, v15, H[2][j][1]);
                        H[2][j][2] = __builtin_fmaf(dt_q0, PA[1][j][0], H[2][j][2]);
                        H[2][j][3] = __builtin_fmaf(dt_q0, PA[1][j][1], H[2][j][3]);
                        float t = 0.0f;
#pragma unroll
                        for (int kk = 0; kk < XT; ++kk)
#pragma unroll
                            for (int r = 0; r < 4; ++r) t = __builtin_fmaf(drow[kk][r], PA[kk][j][r], t);
                        t += __int_as_float(__builtin_amdgcn_ds_bpermute(x16_addr, __float_as_int(t)));
                        t += __int_as_float(__builtin_amdgcn_ds_bpermute(x32_addr, __float_as_int(t)));
                        H[2][j][2] += hx_row ? t : 0.0f;
                    }
                } else {
                    if (i == 1) {
                        // N~(0,1)'(P~A~): N~(0,1) holds nothing but dt at (q_c, v_c), c < 14 -- rows v_c = 18 + c of H take dt x row c of P~A~:
                        // rows 4q, 4q+1 of tile row 0 onto rows 4q+2, 4q+3 of tile row 1 (registers 0, 1 -> 2, 3 of the same lane), rows
                        // 4q+2, 4q+3 onto rows 4(q+1), 4(q+1)+1 (registers 2, 3 -> 0, 1 one lane row further on: one crossbar move each)
#pragma unroll
                        for (int j = 0; j <= 1; ++j) {
                            const float d2 = pa_dn2[j], d3 = pa_dn3[j];
                            H[1][j][0] = __builtin_fmaf(dt_qn0, d2, H[1][j][0]);
                            H[1][j][1] = __builtin_fmaf(dt_qn0, d3, H[1][j][1]);
                            H[1][j][2] = __builtin_fmaf(dt, PA[0][j][0], H[1][j][2]);
                            H[1][j][3] = __builtin_fmaf(dt, PA[0][j][1], H[1][j][3]);
                        }
                    }
#pragma unroll
                    for (int kk = 0; kk < XT; ++kk)
                        if (n_tile_nonzero(kk, i) && kk == 2) {      // tile row 2 of N~: momentum rows only, contraction steps 0, 1
#pragma unroll
                            for (int st = 0; st < 2; ++st)
#pragma unroll
                                for (int j = 0; j <= i; ++j) H[i][j] = mfma4(Nt[kk][i][st], PA[kk][j][st], H[i][j]);
                        }
                }
#pragma unroll
                for (int j = 0; j <= i; ++j) *reinterpret_cast<f32x4*>(hbuf + (16 * j + c) * LDH + 16 * i + 4 * q4) = H[i][j];
            }
            // next stage's record replaces this one's (all of its reads are issued above)
            *reinterpret_cast<f32x4*>(recb + 4 * lane) = rec_next;
            wave_sync();
            WB_STAMP(4);
            // ---- LDL' of Huu in column layout applied to the identity: W = D^-1/2 L^-1
            // lanes 0..31: column `lane` of Huu; lanes 32..63: column lane-32 of I; row i in register i & 3 of Xq[i >> 2] (ldl_panel).
            // The right-hand side H~ux is NOT carried through the elimination (as a second column per lane the compiler split it into
            // a pass of its own and parked all 435 multipliers in spilled SGPRs for it): Y = W H~ux is formed on the matrix pipe below.
            f32x4 Xq[LDL_GROUPS];
            {
                const bool is_h = lane < 32;
                const float* pu = colU + (is_h ? lane : 0) * LDU;
#pragma unroll
                for (int i4 = 0; i4 < LDL_GROUPS; ++i4) {
                    const f32x4 vu = *reinterpret_cast<const f32x4*>(pu + 4 * i4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 4 * i4 + r;
                        Xq[i4][r] = (i < NU) ? (is_h ? vu[r] : ((lane - 32 == i) ? 1.0f : 0.0f)) : 0.0f;
                    }
                }
            }
            bool ok = true;
            {
                if (pat == 0x9u) ldl_panel<0, coupling_mask(0x9u)>(Xq, ok, rs_free);
                else if (pat == 0x6u) ldl_panel<0, coupling_mask(0x6u)>(Xq, ok, rs_free);
                else if (pat == 0x0u) ldl_panel<0, coupling_mask(0x0u)>(Xq, ok, rs_free);
                else ldl_panel<0, coupling_mask(0xFu)>(Xq, ok, rs_free);
            }
            qp_ok = qp_ok && ok;
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) Qn[i][j] = load_tile(Qimg + (size_t)
#ifdef WB_T_ONEQ      // timing build: every stage reads the Q~ tiles of stage 0 (cache-resident; results are wrong)
                                                    (a.B < 0 ? kn : 0)
#else
                                                    kn
#endif
                                                    * QT_FLOATS + (i * XT + j) * IMG, lane);
            rec_pref = *reinterpret_cast<const f32x4*>(recs + (size_t)(k > 1 ? k - 2 : 0) * REC + (4 * lane < REC ? 4 * lane : 0));
            WB_STAMP(5);
            // transposed tiles: Ht[i][j] = (lower tile (i,j))', i >= j
            f32x4 Ht[XT][XT];
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const float* ph = hbuf + (16 * j + 4 * q4) * LDH + 16 * i + c;      // element (4q+r, c) of the transpose = H[16i+c][16j+4q+r]
                    Ht[i][j] = f32x4{ph[0], ph[LDH], ph[2 * LDH], ph[3 * LDH]};
                }
            wave_sync();
            // W columns back into the LDS (lanes 32..63 -> column lane-32), then as tiles: W and W'
            {
                float* pw = colU + (lane >= 32 ? lane - 32 : 0) * LDU;
#pragma unroll
                for (int i4 = 0; i4 < 8; ++i4) {
                    f32x4 vw;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 4 * i4 + r;
                        vw[r] = (i < NU) ? Xq[i4][r] : 0.0f;
                    }
                    if (lane >= 32) *reinterpret_cast<f32x4*>(pw + 4 * i4) = vw;
                }
            }
            wave_sync();
            f32x4 Wt[UT][UT], WT[UT][UT];      // W[i][j] (rows 16i.., columns 16j..) and its transpose W'[j][i] = WT[i][j]
#pragma unroll
            for (int i = 0; i < UT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    Wt[i][j] = *reinterpret_cast<const f32x4*>(colU + (16 * j + c) * LDU + 16 * i + 4 * q4);
                    const float* pt = colU + (16 * j + 4 * q4) * LDU + 16 * i + c;      // element (4q+r, c) of W[i][j]' = W[16i+c][16j+4q+r]
                    WT[i][j] = f32x4{pt[0], pt[LDU], pt[2 * LDU], pt[3 * LDU]};
                }
            Wt[0][1] = zero4();
            wave_sync();
            WB_STAMP(6);
            // Y = W H~ux:  Y[i][j] = sum_{kk <= i} W[i][kk] H~ux[kk][j] = sum xty(W[i][kk]', H~ux[kk][j])
            f32x4 Y[UT][XT];
#pragma unroll
            for (int i = 0; i < UT; ++i)
#pragma unroll
                for (int j = 0; j < XT; ++j) Y[i][j] = zero4();
#pragma unroll
            for (int kk = 0; kk < UT; ++kk)
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int i = kk; i < UT; ++i)
#pragma unroll
                        for (int j = 0; j < XT; ++j) Y[i][j] = mfma4(WT[i][kk][st], Hux[kk][j][st], Y[i][j]);
            WB_STAMP(7);
            // ---- P~+ = H~xx - Y'Y (lower tiles; the upper ones are their transposes through the LDS) ,  K~ = -W'Y
            f32x4 nY[UT][XT];
#pragma unroll
            for (int i = 0; i < UT; ++i)
#pragma unroll
                for (int j = 0; j < XT; ++j) nY[i][j] = -Y[i][j];
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) P[i][j] = (i == j) ? 0.5f * (H[i][j] + Ht[i][j]) : H[i][j];
#pragma unroll
            for (int kk = 0; kk < UT; ++kk)
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int i = 0; i < XT; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) P[i][j] = mfma4(nY[kk][i][st], Y[kk][j][st], P[i][j]);
            WB_STAMP(16);      // P~+ products
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (c == HX - 32 && 32 + 4 * q4 + r == HX) P[2][2][r] = 0.0f;
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j) *reinterpret_cast<f32x4*>(hbuf + (16 * j + c) * LDH + 16 * i + 4 * q4) = P[i][j];
            wave_sync();
#pragma unroll
            for (int i = 0; i < XT; ++i)
#pragma unroll
                for (int j = 0; j < i; ++j) {
                    const float* ph = hbuf + (16 * j + 4 * q4) * LDH + 16 * i + c;
                    P[j][i] = f32x4{ph[0], ph[LDH], ph[2 * LDH], ph[3 * LDH]};
                }
            WB_STAMP(17);      // mirror of P~+ through the LDS
            {
                f32x4 Kt[UT][XT];
#pragma unroll
                for (int i = 0; i < UT; ++i)
#pragma unroll
                    for (int j = 0; j < XT; ++j) Kt[i][j] = zero4();
#pragma unroll
                for (int kk = 0; kk < UT; ++kk)
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int i = 0; i <= kk; ++i)                                   // W is lower triangular
#pragma unroll
                            for (int j = 0; j < XT; ++j) Kt[i][j] = mfma4(nY[kk][j][st], Wt[kk][i][st], Kt[i][j]);      // K~' tiles: states x inputs
#pragma unroll
                for (int i = 0; i < UT; ++i)
#pragma unroll
                    for (int j = 0; j < XT; ++j) {
#ifdef WB_T_NOKSTORE     // timing build (tools/ab_wb.sh): no gain stores -- results are wrong, the time tells what the stores cost
                        if (a.B < 0)
#endif
                        if (k >= L.n_klds) store_tile(Kimg + (size_t)k * KT_FLOATS + (i * XT + j) * IMG, lane, Kt[i][j]);
                        else *reinterpret_cast<f32x4*>(klds + k * KBUF + ((i * XT + j) * 16 + c) * KLD + 4 * q4) = Kt[i][j];
                    }
            }
            WB_STAMP(18);      // K~ products and stores
        }
        WB_STAMP(8);
        phase_sync();
        // ------------------------------------------------------------ phase F: forward sweep
        // du = K~ dx~ row per lane, dx+ from the model's sparse structure -- with dx~ and the force part of du WAVE-UNIFORM in
        // scalar registers (v_readlane broadcasts) and the two lane-shifted terms of the kinematic rows through one crossbar
        // move: no LDS round trip on the stage-to-stage chain (the version that kept dx~, du in the LDS spent 4.4 k cycles
        // per stage in three dependent write -> fence -> read trips; this one is bit-identical to it).  Gain tiles are
        // requested three stages ahead (registers -> LDS -> rows), the stage record two stages ahead (registers -> LDS).
        float* oX = use_ipm ? dXp : dX;
        float* oU = use_ipm ? dUp : dU;
        // lanes are POSITIONS of x~ (pos_of): lane p holds dx of the state that sits there, lane HX the homogeneous 1, the others 0
        const int sl = state_at(lane);
        float xcur = 0.0f;
        if (sl >= 0) xcur = x0[sl >= 0 ? sl : 0] - Xg[sl >= 0 ? sl : 0];          // node 0 is not moved by the warm-start shift
        if (lane == HX) xcur = 1.0f;
        if (sl >= 0) AT(oX, 0, sl) = xcur;
        float* const rbuf[2] = {recb, hbuf + 1024};         // stage records, double-buffered (hbuf is free in this phase)
        // The gain images K~' (states x inputs) come in as TILES -- six 16 B loads per lane and stage, every one a contiguous KiB
        // across the wave -- two stages before the stage that writes them into the LDS (column stride 20 floats: conflict-free),
        // where every lane reads its row of K~ (a column of K~') a stage later.  A lane reading its row straight from memory
        // (twelve 16 B loads, 64 B apart between lanes: 64 separate lines per instruction) kept the CU's address path busy for
        // most of a stage with all four waves in this phase, and a deeper prefetch made that worse, not better.
        static_assert(KBUF <= 32 * LDU + 1024 && 1024 + 256 <= 48 * LDH, "gain tiles and the second record buffer fit the elimination's LDS");
        float* const kbuf = colU;                           // (spans colU and the head of hbuf: both free in this phase)
        const unsigned rec_lane = (4 * lane < REC) ? 4 * lane : 0;
        auto load_rec = [&](int k) { return *reinterpret_cast<const f32x4*>(recs + (size_t)(k < N ? k : N - 1) * REC + rec_lane); };
        *reinterpret_cast<f32x4*>(rbuf[0] + 4 * lane) = load_rec(0);
        f32x4 rec_ahead = load_rec(1);                      // the record of stage k + 1 while stage k runs
        wave_sync();
        const int urow = lane < NU ? lane : 0;
        auto load_ktiles = [&](int k, f32x4 (&t)[UT * XT]) {
            const float* Kk = Kimg + (size_t)(k < N ? k : N - 1) * KT_FLOATS;
#pragma unroll
            for (int i = 0; i < UT * XT; ++i) t[i] = load_tile(Kk + i * IMG, lane);
        };
        auto put_ktiles = [&](const f32x4 (&t)[UT * XT]) {
#pragma unroll
            for (int i = 0; i < UT * XT; ++i) *reinterpret_cast<f32x4*>(kbuf + (i * 16 + c) * KLD + 4 * q4) = t[i];
        };
        const int krow_off = ((urow >> 4) * XT * 16 + (urow & 15)) * KLD;      // tiles (urow >> 4, 0..2), column urow & 15
        auto get_krow = [&](const float* buf, float (&row)[48]) {
            const float* krow = buf + krow_off;
#pragma unroll
            for (int j4 = 0; j4 < 12; ++j4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(krow + (j4 >> 2) * 16 * KLD + 4 * (j4 & 3));
#pragma unroll
                for (int r = 0; r < 4; ++r) row[4 * j4 + r] = v[r];
            }
        };
        const int fi = sl >= 0 ? sl : 0;
        const int hr = (fi >= 39) ? fi - 39 : 0, lr = (fi >= 36 && fi < 39) ? fi - 36 : 0;
        const int x_addr = 4 * (lane < 18 ? lane + 18 : (lane < 36 ? lane - 18 : lane));      // q rows take dx of their v row, v rows du of their q row
        // tiles on their way: requested two stages before their LDS write.  ktA holds those of the even stages, ktB of the odd ones;
        // the first n_klds stages find their gains in the LDS where the backward sweep left them
        f32x4 ktA[UT * XT], ktB[UT * XT];
        const int KL = L.n_klds;                            // 0, 1 or 2
        if (KL == 0) {
            load_ktiles(0, ktA);
            load_ktiles(1, ktB);
            put_ktiles(ktA);
            load_ktiles(2, ktA);
        } else if (KL == 1) {
            load_ktiles(1, ktB);
            load_ktiles(2, ktA);
        } else {
            load_ktiles(2, ktA);
            load_ktiles(3, ktB);
        }
        wave_sync();
        // What the interior-point phase reads that this sweep does not write -- slacks, multipliers, constraint values, the input
        // gradient of the next sweep's barrier terms, lane = stage -- is requested three stages before the sweep ends: the phase then
        // opens with its inputs in registers instead of a trip to memory (7 k cycles per sweep).
        const bool ipm_more = ii + 1 < n_sweeps;
        const int ipm_k = lane < N ? lane : 0;
        float ipm_s[NG], ipm_l[NG], ipm_c[NG], ipm_rr[NU];
#pragma unroll
        for (int j = 0; j < NG; ++j) ipm_s[j] = ipm_l[j] = ipm_c[j] = 0.0f;
#pragma unroll
        for (int i = 0; i < NU; ++i) ipm_rr[i] = 0.0f;
        auto request_ipm_inputs = [&]() {
            const unsigned k4 = 4u * (unsigned)ipm_k;
            const float* rec = recs + (size_t)ipm_k * REC;
#pragma unroll
            for (int j = 0; j < NG; ++j) { ipm_c[j] = rec[R_C + j]; ipm_s[j] = ld_f32(sv + j * NS, k4, 0); ipm_l[j] = ld_f32(lv + j * NS, k4, 0); }
#pragma unroll
            for (int i = 0; i < NU; ++i) ipm_rr[i] = ipm_more ? rec[R_R + i] : 0.0f;
        };
        const int ipm_request_stage = N > 3 ? N - 3 : 0;
        auto fwd_stage = [&](int k, f32x4 (&kt)[UT * XT]) {      // kt: the tiles of stage k + 1, refilled with those of k + 3
            if (use_ipm && k == ipm_request_stage) request_ipm_inputs();
            const float* rk = rbuf[k & 1];
            const f32x4 rec_next = rec_ahead;                // stage k + 1's record, requested a stage ago
            rec_ahead = load_rec(k + 2);
            // what this lane needs of the stage record (not on the dependent chain: the record has been in the LDS for a stage)
            const float d_i = rk[R_D + (lane < 48 ? lane : 0)];      // (the record's defect is stored by position)
            f32x4 hq4[4], hf4[3];
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) hq4[v4] = *reinterpret_cast<const f32x4*>(rk + R_HQ + hr * 16 + 4 * v4);
#pragma unroll
            for (int v4 = 0; v4 < 3; ++v4) hf4[v4] = *reinterpret_cast<const f32x4*>(rk + R_HF + hr * 12 + 4 * v4);
            const f32x4 cd = *reinterpret_cast<const f32x4*>(rk + R_CDT);
            float row[48];
            get_krow(k < KL ? klds + k * KBUF : kbuf, row);
            float dxs[XW];
#pragma unroll
            for (int j = 0; j < XW; ++j) dxs[j] = bcast(xcur, j);
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
            for (int j4 = 0; j4 < 12; ++j4) {
                a0 = fmaf(row[4 * j4], dxs[4 * j4], a0);
                a1 = fmaf(row[4 * j4 + 1], dxs[4 * j4 + 1], a1);
                if (4 * j4 + 2 < XW) a2 = fmaf(row[4 * j4 + 2 < XW ? 4 * j4 + 2 : 0], dxs[4 * j4 + 2 < XW ? 4 * j4 + 2 : 0], a2);
                if (4 * j4 + 3 < XW) a3 = fmaf(row[4 * j4 + 3 < XW ? 4 * j4 + 3 : 0], dxs[4 * j4 + 3 < XW ? 4 * j4 + 3 : 0], a3);
            }
            const float du = (a0 + a1) + (a2 + a3);
            WB_STAMP(13);
            if (lane < NU) AT(oU, k, lane) = du;
            float duf[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) duf[j] = bcast(du, WF + j);
            const float other = __int_as_float(__builtin_amdgcn_ds_bpermute(x_addr, __float_as_int(lane >= 18 ? xcur : du)));
            float xn = xcur + d_i;
            // kinematic rows: q+ = q + dt v + dt^2 a, v+ = v + dt a
            const float t_q = dt * other + dt * dt * du;
            const float t_v = dt * other;
            xn += (fi < 18) ? t_q : (fi < 36) ? t_v : 0.0f;
            // momentum rows 36..41 (every lane runs the code on a clamped row; six lanes keep the result):
            // linear rows: sum_f cdt_f duf[3f + i-36]; angular rows: Hq[i-39] . dx[3..17] + Hf[i-39] . duf
            float acc_a = 0.0f, acc_l = 0.0f;
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * v4 + r < 15) acc_a = fmaf(hq4[v4][r], dxs[3 + 4 * v4 + r], acc_a);
#pragma unroll
            for (int v4 = 0; v4 < 3; ++v4)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc_a = fmaf(hf4[v4][r], duf[4 * v4 + r], acc_a);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const float sel = lr == 0 ? duf[3 * f] : lr == 1 ? duf[3 * f + 1] : duf[3 * f + 2];
                acc_l = fmaf(cd[f], sel, acc_l);
            }
            xn += (fi >= 39) ? acc_a : (fi >= 36) ? acc_l : 0.0f;
            WB_STAMP(14);
            if (sl >= 0) AT(oX, k + 1, sl) = xn;
            xcur = (sl >= 0) ? xn : (lane == HX ? 1.0f : 0.0f);
            *reinterpret_cast<f32x4*>(rbuf[(k + 1) & 1] + 4 * lane) = rec_next;
            if (k + 1 >= KL) {
                put_ktiles(kt);                              // (this stage's row reads were issued before: the LDS serves a wave in order)
                load_ktiles(k + 3, kt);
            }
            wave_sync();
            WB_STAMP(15);
        };
        {
            int k = 0;
            for (; k + 2 <= N; k += 2) {
                fwd_stage(k, ktB);
                fwd_stage(k + 1, ktA);
            }
            if (k < N) fwd_stage(k, ktB);
        }
        phase_sync();
        WB_STAMP(9);
        // ------------------------------------------------------------ phase I: interior-point update, lane = stage
        // Everything the phase reads from memory is requested in one go at its top -- its own inputs, the first pieces of the
        // step blend, the input gradient of the next sweep's barrier terms -- and nothing in it waits for a store: written
        // serially (load, compute, store, fence, load ...) the phase took six memory latencies per sweep, 15 % of the kernel
        // (tools/wb_stamps.py, slot 20).  Addresses are uniform base + lane offset (one VGPR for all of them).
        if (use_ipm) {
            const bool more = ipm_more;
            const bool live = lane < N;
            const int k = ipm_k;
            const unsigned k4 = 4u * (unsigned)k;
            float duf[12], g[NG];
            float (&s)[NG] = ipm_s; float (&l)[NG] = ipm_l; float (&cc)[NG] = ipm_c; float (&rr)[NU] = ipm_rr;
#pragma unroll
            for (int i = 0; i < 12; ++i) duf[i] = ld_f32(dUp + (WF + i) * NS, k4, 0);
            // step <- step + ap (new step - step): [dX | dU] and [dXp | dUp] have the same layout (StageArr), one pass over both
            // in 16 B pieces, nine pieces per lane in flight
            const int nvec = (SA.dXp - SA.dX) >> 2;
            f32x4* d4 = reinterpret_cast<f32x4*>(dX);
            const f32x4* n4 = reinterpret_cast<const f32x4*>(dXp);
            constexpr int BL = 9;      // N <= 30: the whole blend in one round (559 pieces)
            f32x4 dv[BL], nv[BL];
            auto blend_request = [&](int i0) {
#pragma unroll
                for (int u = 0; u < BL; ++u) {
                    const int i = i0 + 64 * u;
                    const int ic = i < nvec ? i : i0;
                    nv[u] = n4[ic];
                    dv[u] = (ii == 0) ? zero4() : d4[ic];
                }
            };
            blend_request(lane);
            request_sweep();
            gdot(mp, duf, g);
            // (the steps ds, dl are formed twice -- for the step lengths and for the update -- rather than kept: 32 registers)
            float rp = 0.0f, rd = 0.0f;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                const float is = fast_rcp(s[j]);
                const float dsj = -(g[j] + cc[j]) - s[j];
                const float dlj = tau * is - l[j] - l[j] * is * dsj;
                const bool on = live && ((my_act >> j) & 1u);
                rp = on ? fmaxf(rp, -dsj * is) : rp;
                rd = on ? fmaxf(rd, -dlj * __builtin_amdgcn_rcpf(l[j])) : rd;
            }
            WB_STAMP(22);      // inputs arrived, step lengths per lane
            const float rpm = wave_max(rp), rdm = wave_max(rd);
            const float ap = rpm > a.gamma ? a.gamma / rpm : 1.0f;
            const float ad = rdm > a.gamma ? a.gamma / rdm : 1.0f;
            float m_l = 0.0f;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                const float is = fast_rcp(s[j]);
                const float dsj = -(g[j] + cc[j]) - s[j];
                const float dlj = tau * is - l[j] - l[j] * is * dsj;
                const bool on = live && ((my_act >> j) & 1u);
                s[j] += on ? ap * dsj : 0.0f;
                l[j] += on ? ad * dlj : 0.0f;
                m_l += on ? s[j] * l[j] : 0.0f;
            }
            if (live) {
#pragma unroll
                for (int j = 0; j < NG; ++j) { st_f32(sv + j * NS, k4, 0, s[j]); st_f32(lv + j * NS, k4, 0, l[j]); }
            }
            mu_sum = wave_sum(m_l);
            WB_STAMP(23);      // reductions, update, slack / multiplier stores
            for (int i0 = lane; i0 < nvec; i0 += 64 * BL) {
#pragma unroll
                for (int u = 0; u < BL; ++u) {
                    const int i = i0 + 64 * u;
                    if (i < nvec) d4[i] = dv[u] + ap * (nv[u] - dv[u]);
                }
                if (i0 + 64 * BL < nvec) blend_request(i0 + 64 * BL);
            }
            // (no fence here: the next reader of dX, dU across lanes is the step phase, behind its own phase_sync; the slacks and
            //  multipliers are read back by the lane that wrote them)
            if (more) {
                ipm_terms(fmaxf(a.sigma * mu_sum / (float)n_act, a.tau_min), s, l, cc, rr);
                wave_sync();
            }
        } else {
            request_sweep();
        }
        WB_STAMP(20);      // interior-point update of this sweep
    }
    WB_STAMP(10);
    phase_sync();
    // ---------------------------------------------------------------- phase S: step
    float sn_l = 0.0f;
    bool bad_l = false;
    for (int k = lane; k <= N; k += 64) {
        for (int i = 0; i < NX; ++i) { const float v = AT(dX, k, i); bad_l = bad_l || !(fabsf(v) <= 1e30f); sn_l = fmaxf(sn_l, fabsf(v)); }
        if (k < N)
            for (int i = 0; i < NU; ++i) { const float v = AT(dU, k, i); bad_l = bad_l || !(fabsf(v) <= 1e30f); sn_l = fmaxf(sn_l, fabsf(v)); }
    }
    const float stepn = wave_max(sn_l);
    const bool bad = __any(bad_l);
    int status = NMPC_STATUS_MAXITER;
    bool finished = false;
    if (bad) { status = NMPC_STATUS_NAN; finished = true; }
    else if (!qp_ok) { status = NMPC_STATUS_QP; finished = true; }
    else if (a.nlp_tol > 0.0f && stepn < a.nlp_tol) { status = NMPC_STATUS_OK; finished = true; }
    // new iterate = previous one (read through the warm-start shift) + step; all reads before the first write
    if (!bad || a.shift > 0) {
        constexpr int PRE = 8;
        const float sc = bad ? 0.0f : 1.0f;
        const int n_x = (N + 1) * NX, n_u = N * NU;
        for (int base = 0; base < n_x; base += 64 * PRE) {
            float v[PRE];
#pragma unroll
            for (int uu = 0; uu < PRE; ++uu) {
                const int e = base + 64 * uu + lane, ec = e < n_x ? e : 0;
                const int k = ec / NX, i = ec - k * NX;
                v[uu] = Xg[ec + (shifted_node(k, a.shift, N) - k) * NX] + (bad ? 0.0f : sc * AT(dX, k, i));
            }
            if (a.shift > 0) phase_sync();      // a shifted read may be another lane's write target
#pragma unroll
            for (int uu = 0; uu < PRE; ++uu) {
                const int e = base + 64 * uu + lane;
                if (e < n_x) Xg[e] = v[uu];
            }
            if (a.shift > 0) phase_sync();
        }
        for (int base = 0; base < n_u; base += 64 * PRE) {
            float v[PRE];
#pragma unroll
            for (int uu = 0; uu < PRE; ++uu) {
                const int e = base + 64 * uu + lane, ec = e < n_u ? e : 0;
                const int k = ec / NU, i = ec - k * NU;
                const bool okk = a.shift == 0 || shifted_stage_valid(k, a.shift, N);
                const float t = Ug[ec + (okk ? a.shift * NU : 0)];
                v[uu] = ((okk || i < WF) ? t : 0.0f) + (bad ? 0.0f : sc * AT(dU, k, i));
            }
            if (a.shift > 0) phase_sync();
#pragma unroll
            for (int uu = 0; uu < PRE; ++uu) {
                const int e = base + 64 * uu + lane;
                if (e < n_u) Ug[e] = v[uu];
            }
            if (a.shift > 0) phase_sync();
        }
    }
#ifdef NMPC_WB_STAMPS
    WB_STAMP(11);
    if (lane == 0) for (int i = 0; i < 24; ++i) (ws + wl.js)[i] = (float)st_acc[i];
#endif
    if (lane == 0) {
        flag[0] = finished ? 1 : 0;
        if (a.status) a.status[b] = status;
        if (a.stats) {
            a.stats[4 * b + 0] = cost;
            a.stats[4 * b + 1] = stepn;
            a.stats[4 * b + 2] = 1.0f;
            a.stats[4 * b + 3] = (float)(a.it + 1);
        }
    }
#undef AT
}
