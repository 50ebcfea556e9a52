// nmpc_qp.hip.inc -- the QP kernel of the tile family (included by nmpc_solve.hip): the stamp macros of the diagnostic build, the
// element-wise pass, the barrier tiles and nmpc_qp_kernel.
namespace nmpc {

// Diagnostic build only (-DNMPC_STAMPS, tools/phase_shares.py): per-phase cycle counters written to
// a buffer of their own; the production kernel contains no stamp.
#ifdef NMPC_STAMPS
#define STAMP_DECL unsigned long long st_t0 = __builtin_readcyclecounter(), st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; \
    StageStamps sst = {0, {0, 0, 0, 0, 0, 0, 0, 0}}
#define SST_PASS , sst
#define SST_TILES(i) SST(i)
#define STAMP(i) do { const unsigned long long st_t1 = __builtin_readcyclecounter(); st_acc[i] += st_t1 - st_t0; st_t0 = st_t1; } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define SST_PASS
#define SST_TILES(i)
#endif

// Element-wise pass over n floats, lane-strided, with PRE loads per lane in flight before the first
// result is stored: ld(i) computes the value of element i from its loads, st(i, v) consumes it.
// (In the lean variant these are memory round trips; a plain loop would serialise them, since the
// compiler must assume that a store may alias the next iteration's loads.)
template <int PRE, class Load, class Store>
__device__ __forceinline__ void batched(int n, int lane, Load&& ld, Store&& st) {
    for (int base = 0; base < n; base += 64 * PRE) {
        float v[PRE];
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int i = base + 64 * u + lane;
            v[u] = ld(i < n ? i : 0);
        }
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int i = base + 64 * u + lane;
            if (i < n) st(i, v[u]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The barrier part of a stage's cost tiles (NextCost in nmpc_qp_kernel), one form per instantiation of the kernel.  b0, b1: the
// lane's two 16 B reads of the stage's barrier rows; Rn, Sn: the tiles R and S~ = [0 r] they are added to.
//   FOOT: the rows hold the terms ready, b0 = {xx, yy, zz, xz}, b1 = {G'v x, G'v y, G'v z, yz} of the foot of this lane's row
//   quad (Centroidal::foot_terms).  mx / my / mz are 1 where the lane's column is the x / y / z force of that foot (it then
//   takes entries of the foot's block of G'DG), mh where it is the homogeneous column (which takes G'v), else 0; at most one
//   of a lane is 1, so each register takes ONE add: R + block entry, r + G'v.  Multipliers rather than select masks: a mask
//   is an SGPR pair, and the stage bodies already spill scalars (measured: the same terms picked with selects cost the
//   headline 5.6 %).  x.1 + y is x + y and x.0 + y is y bit for bit, the sign of a zero aside, which no sum here keeps.
//   Otherwise: the rows hold sqrt(D) and vt = v/sqrt(D); with Gs = sqrt(D).G the tile T = Gs'[Gs | vt] holds G'DG in its
//   columns < nu and G'v in column nx (the Gauss-Newton contraction of the barrier): ONE product on the matrix pipe, step(i)
//   its K step i in fp32, or one bf16 instruction (BF16B); finish() splits it onto R and S~.
// Same sums on the same bits in the two fp32 forms.
template <bool FOOT, bool BF16B>
struct BarrierTiles;
template <bool BF16B>
struct BarrierTiles<true, BF16B> {
    float mx, my, mz, mh;
    __device__ __forceinline__ void build(f32x4 b0, f32x4 b1, bool, f32x4& Rn, f32x4& Sn) {
        Rn[0] = __builtin_fmaf(b0[3], mz, __builtin_fmaf(b0[0], mx, Rn[0]));
        Rn[1] = __builtin_fmaf(b1[3], mz, __builtin_fmaf(b0[1], my, Rn[1]));
        Rn[2] = __builtin_fmaf(b0[2], mz, __builtin_fmaf(b1[3], my, __builtin_fmaf(b0[3], mx, Rn[2])));
#pragma unroll
        for (int r = 0; r < 3; ++r) Sn[r] = __builtin_fmaf(b1[r], mh, Sn[r]);
    }
    __device__ __forceinline__ void step(int) {}
    __device__ __forceinline__ void finish(bool, f32x4&, f32x4&) {}
};
template <bool BF16B>
struct BarrierTiles<false, BF16B> {
    f32x4 Gc;            // this lane's registers of the constraint matrix G (rows: constraints)
    f32x4 Gs, Vt, Tb;
    __device__ __forceinline__ void build(f32x4 b0, f32x4 b1, bool hx_col, f32x4&, f32x4&) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Gs[r] = Gc[r] * b0[r];                  // rows >= ng: Gc = 0
            Vt[r] = hx_col ? b1[r] : Gs[r];         // [Gs | vt]
        }
        Tb = zero4();
    }
    __device__ __forceinline__ void step(int i) {
        if constexpr (!BF16B) Tb = __builtin_amdgcn_mfma_f32_16x16x4f32(Gs[i], Vt[i], Tb, 0, 0, 0);
        else if (i == 0) Tb = xty_bf16(Gs, Vt);
    }
    __device__ __forceinline__ void finish(bool hx_col, f32x4& Rn, f32x4& Sn) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Rn[r] += hx_col ? 0.0f : Tb[r];     // columns >= nu of Tb are zero
            Sn[r] += hx_col ? Tb[r] : 0.0f;
        }
    }
};

// ------------------------------------------------------------------------------------------------
// QP + step of one SQP iteration: one problem per wavefront.
// LEAN: LDS layout variant (Lds).  BF16B: the barrier product Gs'[Gs | vt] on the bf16 matrix pipe
// (nmpc_dims.precision = 1, BASELINE configs[4]); everything else stays fp32.
// ALLV: the stage loop dispatches over every static variant the model lists (all contact patterns);
// otherwise over the model's short list (common_variant) with the run-time fallback for the rest.
// Two kernels rather than one loop with everything: measured, the mere presence of the other
// variants in the kernel costs the common ones 2.5 % (code layout, register allocation).
// Registers: 234 VGPRs (resident) / 256 with 16 values in scratch, none of them in a stage loop (lean); no AGPRs
// (profiles/r02_isa_resources.md).  The resident variant is pinned to ONE wave per SIMD (amdgpu_waves_per_eu): its LDS image lets
// four waves onto a CU, and with two allowed per SIMD the hardware co-locates them and leaves SIMDs idle once a batch runs in
// rounds (measured 1.91 M instead of 2.30 M solves/s at B = 8192).  build.sh passes -amdgpu-mfma-vgpr-form so that the MFMAs keep
// their VGPR operands.  What kept both variants above 256 registers until round 2 was the interior-point phase, not the sweeps:
// its loads were interleaved with their uses; a stage's rows are now requested up front (ld_row / st_row).
// Floating-point contraction is OFF in the body of this kernel (the tile algebra in nmpc_sweep.hpp / nmpc_tile.hpp is MFMA and
// explicit fma; this is about the lane = stage arithmetic) and every a*b + c that is meant as one operation is written as fmaf:
// left to the compiler, which products get fused into the following add depends on the instantiation -- the resident and the
// lean variant, compiled from the same expressions, came out 1e-5 apart after an unrelated change to their loads.
#pragma clang fp contract(off)
#ifndef NMPC_RES_WAVES
#define NMPC_RES_WAVES 1      // diagnostic builds (tools/occupancy_probe.py) compile the resident variant for two waves per SIMD
#endif
template <class M, bool LEAN, bool BF16B, bool ALLV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LEAN ? 2 : NMPC_RES_WAVES, LEAN ? 2 : NMPC_RES_WAVES)))
void nmpc_qp_kernel(const SolveArgs a) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NG = M::NG, NY = NX + NU;
    using G = TileGeom<M>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    if (skipped(a, b)) return;                   // e.g. a terminated rollout: X, U, status stay as they are
    const int lane = lane_id();
    const int q4 = lane >> 4, c = lane & 15;
    const int N = a.N;
    const WsLayout<M> wl(N);
    float* ws = a.ws + (size_t)b * wl.stride;
    int* flag = reinterpret_cast<int*>(ws + wl.flag);
    if (a.it > 0 && flag[0]) return;             // finished in an earlier iteration
    const Lds<M, LEAN> L(N);
    const StageArrays<M> SA_(N, LEAN);
    const int NS = SA_.NS;
    // the stage arrays: LDS in the resident variant, workspace in the lean one (same code either way;
    // the variant is a template parameter so that every pointer has ONE address space)
    float* arr = LEAN ? ws + wl.lean : smem + L.arr;
    float* Xs = arr + SA_.Xs;   float* Us = arr + SA_.Us;
    float* dX = arr + SA_.dX;   float* dU = arr + SA_.dU;
    float* dXp = arr + SA_.dXp; float* dUp = arr + SA_.dUp;
    float* sv = arr + SA_.sv;   float* lv = arr + SA_.lv;
    float* idle_sink = arr + SA_.total - 4;
    float* qv = smem + L.qv;   float* rv = smem + L.rv;
    float* gsq = smem + L.gsq; float* gvt = smem + L.gvt;
    // Barrier terms of a stage as the stage sweep reads them.  FOOT (fp32 barrier of a model with the closed form per foot, one
    // wave per SIMD): quad f of gsq / gvt holds the first / second four numbers of foot f (M::foot_terms) -- G'DG and G'v ready
    // to add, built where every stage has a lane of its own (put_foot_terms).  Otherwise (bf16 barrier product, double
    // integrator, lean variant): sqrt(D) and v/sqrt(D) by constraint row, and the sweep forms the product Gs'[Gs | vt] on the
    // matrix pipe.  Lean keeps the product: with a second wave to fill the stage body's stalls it was never exposed, and the
    // terms built lane = stage cost that variant 4.7 % at B = 8192 (its update phase spills: 16 -> 56 registers in scratch).
    // The two are bit-identical (same chain, see foot_terms), as the variants have to be.
    constexpr bool FOOT = M::FOOT_TERMS && !BF16B && !LEAN;
    // Input: the stage's active rows, slacks s, multipliers lam, constraint values c and the barrier parameter tau:
    //   D = lam/s, sq = sqrt(D), vt = (tau/s + lam + D c)/sqrt(D), exact zeros in inactive rows -- the same arithmetic as
    // the by-row loops of the product path.  Foot by foot: four rows, eight numbers, two stores.
    // (The row's five lines stand three times: here, in front of the first sweep and at the end of phase I.  One __forceinline__
    // function for them was tried site by site and changed the code each time: here 4457 of 15 999 lines of the resident Centroidal
    // kernel, in the pre-sweep loop 57-87 lines of the DoubleIntegrator kernels, in phase I 16 lines of the lean Centroidal ones.)
    auto put_foot_terms = [&](int k, unsigned am, const float (&s)[NG], const float (&l)[NG], const float (&cc)[NG], float tau_k) {
        if constexpr (FOOT) {
            static_assert(!FOOT || (NG == 16 && NU == 12), "foot terms: four feet, quad f of the tiles = foot f");
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                float sq[NG] = {}, vt[NG] = {}, t[8];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int j = M::row_of(f, jj);
                    const bool on = (am >> j) & 1u;
                    const float is = fast_rcp(s[j]);
                    const float D = l[j] * is;
                    const float rs = __builtin_amdgcn_rsqf(D);
                    sq[j] = on ? D * rs : 0.0f;
                    vt[j] = on ? __builtin_fmaf(D, cc[j], __builtin_fmaf(tau_k, is, l[j])) * rs : 0.0f;
                }
                M::foot_terms(a.mp, f, sq, vt, t);
                *reinterpret_cast<f32x4*>(gsq + k * TS + 4 * f) = f32x4{t[0], t[1], t[2], t[3]};
                *reinterpret_cast<f32x4*>(gvt + k * TS + 4 * f) = f32x4{t[4], t[5], t[6], t[7]};
            }
        }
    };
    // ordering point between phases that exchange data between lanes: LDS traffic of a single wave
    // is ordered by issue; the workspace needs the stores drained first
    auto phase_sync = [&]() {
        if constexpr (LEAN) __threadfence_block();
        wave_sync();
    };
    unsigned* actm = reinterpret_cast<unsigned*>(smem + L.act);
    unsigned* umask = reinterpret_cast<unsigned*>(smem + L.umk);
    float* conv = smem + L.conv;
#define AT(arr, k, i) (arr)[LEAN ? (k) * TS + (i) : (i) * NS + (k)]
    // the row of stage k of a stage array (12 or 16 features): 16 B accesses in the stage-major layout
    auto ld_row = [&](const float* arr_, int k, auto& out) {
        constexpr int n = (int)(sizeof(out) / sizeof(float));
        if constexpr (LEAN) {
#pragma unroll
            for (int g = 0; g < (n + 3) / 4; ++g) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(arr_ + k * TS + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g + r < n) out[4 * g + r] = v[r];
            }
        } else {
#pragma unroll
            for (int i = 0; i < n; ++i) out[i] = AT(arr_, k, i);
        }
    };
    auto st_row = [&](float* arr_, int k, const auto& in) {     // (the padding of a stage-major row is rewritten as zero)
        constexpr int n = (int)(sizeof(in) / sizeof(float));
        if constexpr (LEAN) {
#pragma unroll
            for (int g = 0; g < (n + 3) / 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (4 * g + r < n) ? in[4 * g + r < n ? 4 * g + r : 0] : 0.0f;
                *reinterpret_cast<f32x4*>(arr_ + k * TS + 4 * g) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < n; ++i) AT(arr_, k, i) = in[i];
        }
    };

    float* Xg = a.X + (size_t)b * (N + 1) * NX;
    float* Ug = a.U + (size_t)b * N * NU;
    const float* pg = a.params + (size_t)b * (N + 1) * NP;
    const float* yr = a.yref + (size_t)b * (a.yref_per_stage ? (size_t)N * NY : (size_t)NY);
    const float* yre = a.yref_e + (size_t)b * NX;
    const float* x0 = a.x0 + (size_t)b * NX;
    float* At = ws + wl.At;
    float* Bt = ws + wl.Bt;
    float* Kt = ws + wl.Kt;   // transposed images of K~ (N + 1 scratch slot)
    float* Ct = ws + wl.Ct;   // transposed images of Acl~ = A~ + B~K~ (N + 1)

    // Two-wave variant, horizon within one wave: the problem's linearisation runs here, lane = node, instead of in a kernel of
    // its own (the host leaves that launch out: qp_linearizes_itself).  With a second wave on the SIMD to fill its latency this is
    // +2 % per solve call at B = 8192; alone on the SIMD it is not (measured -0.6 % at B = 1024: the resident variant keeps the
    // separate kernel).  Scratch: the region of the sweep operands, which the prologue below fills.
    if constexpr (LEAN) {
        if (qp_linearizes_itself(LEAN, N)) {
            static_assert(LIN_LDS_FLOATS <= 4 * TS * 20, "scratch of the fused linearisation");
            linearize_node<M>(a, lane <= N, b, lane, smem + L.qv);
            __threadfence_block();
            wave_sync();
        }
    }
    for (int i = 4 * lane; i < L.conv; i += 256)                // padding entries stay finite
        *reinterpret_cast<f32x4*>(smem + i) = zero4();
    if constexpr (LEAN)
        for (int i = 4 * lane; i < SA_.total; i += 256) *reinterpret_cast<f32x4*>(arr + i) = zero4();
    phase_sync();
    // Stream the problem into the LDS through registers, PRE floats per lane and array at a time,
    // with the loads of ALL arrays in flight before the first is used (an element-wise copy loop
    // pays one memory round trip per 64 floats -- some thirty in a row for a horizon of 50).
    constexpr int PRE = 13;
    auto fetch = [&](const float* src, int total, int base, float (&v)[PRE]) {
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int e = base + 64 * u + lane;
            v[u] = src[e < total ? e : 0];
        }
    };
    // X and U of the previous solve, read through the warm-start shift (a.shift = 0: identity)
    auto fetch_x = [&](int base, float (&v)[PRE]) {
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int e = base + 64 * u + lane, ec = e < (N + 1) * NX ? e : 0;
            const int k = ec / NX;
            v[u] = Xg[ec + (shifted_node(k, a.shift, N) - k) * NX];
        }
    };
    auto fetch_u = [&](int base, float (&v)[PRE]) {
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int e = base + 64 * u + lane, ec = e < N * NU ? e : 0;
            const bool ok = a.shift == 0 || shifted_stage_valid(ec / NU, a.shift, N);
            const float t = Ug[ec + (ok ? a.shift * NU : 0)];
            v[u] = ok ? t : 0.0f;
        }
    };
    auto drain = [&](int total, int base, const float (&v)[PRE], auto&& sink) {
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const int e = base + 64 * u + lane;
            if (e < total) sink(e, v[u]);
        }
    };
    auto put_x = [&](int e, float v) { const int k = e / NX; AT(Xs, k, e - k * NX) = v; };
    auto put_q = [&](int e, float v) { const int k = e / NX; qv[k * TS + slot_of(e - k * NX)] = v; };   // by slot
    auto put_u = [&](int e, float v) { const int k = e / NU; AT(Us, k, e - k * NU) = v; };
    auto put_r = [&](int e, float v) { const int k = e / NU; rv[k * TS + slot_of(e - k * NU)] = v; };
    auto put_c = [&](int e, float cj) {                        // c = G u - h at the linearisation point
        const int k = e / NG, j = e - k * NG;
        const float s = fmaxf(-cj, a.s_min);
        AT(sv, k, j) = s;
        AT(lv, k, j) = a.mu0 * fast_rcp(s);
    };
    const int n_x = (N + 1) * NX, n_u = N * NU, n_c = N * NG;
    const int n_max = n_x > n_c ? n_x : n_c;
    for (int base = 0; base < n_max; base += 64 * PRE) {
        float vx[PRE], vq[PRE], vu[PRE], vr[PRE], vc[PRE];
        fetch_x(base, vx);
        fetch(ws + wl.q, n_x, base, vq);
        fetch_u(base, vu);
        fetch(ws + wl.r, n_u, base, vr);
        fetch(ws + wl.c, n_c, base, vc);
        drain(n_x, base, vx, put_x);
        drain(n_x, base, vq, put_q);
        drain(n_u, base, vu, put_u);
        drain(n_u, base, vr, put_r);
        drain(n_c, base, vc, put_c);
    }
    float* dx0s = smem + L.dx0;
    if constexpr (LEAN) {
        if (lane < NX) dx0s[lane] = x0[lane] - Xg[lane];      // node 0 is a fixed point of the shift map
    }
    float cost_l = 0.0f, mu_l = 0.0f;
    int nact_l = 0;
    for (int k = lane; k <= N; k += 64) {
        cost_l += ws[wl.cost + k];
        if (k < N) {
            const unsigned am = reinterpret_cast<const unsigned*>(ws + wl.act)[k];
            actm[k] = am;
            // coupling mask of the stage, with the index of its static variant (+1; 0 = none) on top:
            // the stage loop then dispatches on one shift instead of recomputing the index every stage
            const unsigned um = reinterpret_cast<const unsigned*>(ws + wl.umk)[k];
            // bit 24: stage k-1 (the next one of the backward sweep, whose barrier product is built in this stage's
            // body) has active constraint rows in MFMA steps that this stage's pattern does not have
            const unsigned um_prev = reinterpret_cast<const unsigned*>(ws + wl.umk)[k > 0 ? k - 1 : 0];
            const unsigned wider = (k > 0 && (M::barrier_steps(um_prev) & ~M::barrier_steps(um)) != 0u) ? 1u : 0u;
            umask[k] = um | ((unsigned)(M::static_index(um) + 1) << 16) | (wider << 24);
            nact_l += __popc(am);
            mu_l += a.mu0 * (float)__popc(am);      // s * (mu0 / s) per active row
        }
    }
    // per-lane weights of "its" column (slot layout: column slot c holds logical index ic, HS the
    // homogeneous coordinate)
    const int ic = index_of(c);
    const bool c_is_x = ic >= 0 && ic < NX, c_is_u = ic >= 0 && ic < NU;
    const float wq_c = c_is_x ? a.W[c_is_x ? ic : 0] + a.reg : 0.0f;
    const float wr_c = c_is_u ? a.W[NX + (c_is_u ? ic : 0)] + a.reg : 0.0f;
    const float we_c = c_is_x ? a.We[c_is_x ? ic : 0] + a.reg_e : 0.0f;
    // per-lane constants of the stage sweeps: which element of q / r / sqrt(D) / v each of the
    // lane's four tile registers takes (a clamped LDS feature index and a 0/1 mask), so that the
    // cost tiles of a stage are built with unconditional loads and selects (no branches)
    SweepLane sl;
    sl.init(conv, lane, HS, a.rs_free);
    f32x4 Qc, Rc;                // constant parts: diag(Wx)+reg, diag(Wu)+reg
    bool qm[4], rm[4];           // masks: the register takes an element of q / r
    BarrierTiles<FOOT, BF16B> bt;    // per-lane constants of the barrier, one form per instantiation
    if constexpr (FOOT) {
        bt.mx = (c == 4 * q4) ? 1.0f : 0.0f; bt.my = (c == 4 * q4 + 1) ? 1.0f : 0.0f;
        bt.mz = (c == 4 * q4 + 2) ? 1.0f : 0.0f; bt.mh = (c == HS) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * q4 + r, ir = index_of(row);      // row slot and its logical index
        const bool r_is_x = ir >= 0 && ir < NX, r_is_u = ir >= 0 && ir < NU;
        Qc[r] = (row == c && r_is_x) ? wq_c : 0.0f;
        Rc[r] = (row == c && r_is_u) ? wr_c : 0.0f;
        qm[r] = (c == HS && r_is_x) || (row == HS && c_is_x);
        rm[r] = (c == HS && r_is_u);
        if constexpr (!FOOT) bt.Gc[r] = (row < NG && c_is_u) ? M::G(a.mp, row < NG ? row : 0, c_is_u ? ic : 0) : 0.0f;
    }
    const bool is_hx_col = (c == HS);
    phase_sync();
    // Run-length schedule of the backward sweeps: the stages N-1 .. 0 as runs of ONE stage body, so that the sweep picks a
    // body once per run and the loop over a run's stages holds nothing but that body.  A run word is
    //   top (bits 0..8: first stage of the run + 1) | length (bits 9..17) | key (bits 18..22: run_key);  the end word is 0.
    // The stage in front of a touch-down (bit 24 of its mask word: the body of the widest pattern) is a run of its own;
    // masks without a static body form runs of the run-time fallback, which takes the mask of each stage.
    // Built once per launch: the masks do not change over the interior-point sweeps.
    constexpr int WIDEST = M::static_index((NU < 32) ? ((1u << NU) - 1u) : 0xFFFFFFFFu);
    constexpr unsigned KEY_DYNAMIC = ALLV ? 16u : 4u;
    auto run_key = [&](unsigned w) -> unsigned {
        const int vi = ((w >> 24) & 1u) ? WIDEST : (int)((w >> 16) & 0x1Fu) - 1;
        if constexpr (ALLV) {
            return (vi >= 0 && vi < 16 && vi < M::N_STATIC_MASKS) ? (unsigned)vi : KEY_DYNAMIC;
        } else {
            unsigned key = KEY_DYNAMIC;
#pragma unroll
            for (int j = 3; j >= 0; --j)
                if (M::common_variant(j) >= 0 && vi == M::common_variant(j)) key = (unsigned)j;
            return key;
        }
    };
    unsigned* runs = reinterpret_cast<unsigned*>(smem + L.runs);
    if constexpr (!LEAN) {       // (the lean variant dispatches per stage, see the sweep)
        int n_runs = 0;
        for (int base = ((N - 1) >> 6) << 6; base >= 0; base -= 64) {      // lane = stage, the top 64 stages first
            const int k = base + lane;
            const bool valid = k < N;
            const unsigned w = umask[valid ? k : N - 1], w_above = umask[k + 1 < N ? k + 1 : N - 1];
            const unsigned key = run_key(w);
            const bool first = valid && (k == N - 1 || key != run_key(w_above) || (((w | w_above) >> 24) & 1u) != 0u);
            const unsigned long long m = __ballot(first);
            const unsigned long long above = (lane < 63) ? (m >> (lane + 1)) : 0ull;
            if (first) runs[n_runs + __popcll(above)] = (key << 18) | (unsigned)(k + 1);
            n_runs += __popcll(m);
        }
        if (lane == 0) runs[n_runs] = 0u;
        wave_sync();
        for (int i = lane; i < n_runs; i += 64) {      // length of a run: down to the top of the next one
            const unsigned w = runs[i], w_next = runs[i + 1];
            runs[i] = w | (((w & 0x1FFu) - (w_next & 0x1FFu)) << 9);
        }
        wave_sync();
    }

    int status = NMPC_STATUS_MAXITER;
    bool finished = false;
    STAMP_DECL;
    float cost = 0.0f, stepn = 0.0f, alpha = 1.0f;
    // phase S of the lean variant with one node per lane (see there): the node's rows of X, U in registers
    const bool rows_in_regs = LEAN && N < 64;
    const int kx_s = lane <= N ? lane : 0, ku_s = lane < N ? lane : 0;
    float xr[LEAN ? NX : 1], ur[LEAN ? NU : 1];
    {
        cost = wave_sum(cost_l);
        const int n_act = (int)(wave_sum((float)nact_l) + 0.5f);
        STAMP(0);
        // ------------------------------------------------------------ QP: interior point loop
        const bool use_ipm = (a.n_ipm > 0) && (n_act > 0);
        const int n_sweeps = use_ipm ? a.n_ipm : 1;
        bool qp_ok = true;
        float mu_sum = wave_sum(mu_l);          // sum of s.lam over the active rows
        const bool one_stage_per_lane = N <= 64;
        // step <- step + ap (new step - step), both trajectories
        auto blend = [&](float ap) {
            batched<10>(SA_.nX, lane, [&](int i) { const float d = dX[i]; return __builtin_fmaf(ap, dXp[i] - d, d); },
                        [&](int i, float v) { dX[i] = v; });
            batched<10>(SA_.nU, lane, [&](int i) { const float d = dU[i]; return __builtin_fmaf(ap, dUp[i] - d, d); },
                        [&](int i, float v) { dU[i] = v; });
        };
        for (int ii = 0; ii < n_sweeps; ++ii) {
            float tau = 0.0f;
            if (use_ipm) {
                // barrier coefficients of this iteration, lane = stage:
                //   D = lam/s, gsq = sqrt(D), gvt = (tau/s + lam + D c)/sqrt(D)
                // so that the stage sweep only builds Gs = gsq.G and Vt = gvt.e_nx (no divides there) -- or, FOOT, the
                // barrier terms themselves (put_foot_terms)
                tau = fmaxf(a.sigma * mu_sum / (float)n_act, a.tau_min);
                // (with N <= 64 the update phase of the previous iteration has already written them)
                if (ii == 0 || !one_stage_per_lane)
                for (int k = lane; k < N; k += 64) {
                    const unsigned am = actm[k];
                    float uk[NU], gk[NG], sk[NG], lk[NG];
                    ld_row(Us, k, uk);
                    ld_row(sv, k, sk);
                    ld_row(lv, k, lk);
                    M::gdot(a.mp, uk, gk);
                    if constexpr (FOOT) {
#pragma unroll
                        for (int j = 0; j < NG; ++j) gk[j] -= M::h(a.mp, j);      // c = G u - h
                        put_foot_terms(k, am, sk, lk, gk, tau);
                    } else {
#pragma unroll
                        for (int j = 0; j < NG; ++j) {
                            const bool on = (am >> j) & 1u;
                            const float s = sk[j], l = lk[j], cj = gk[j] - M::h(a.mp, j);
                            const float is = fast_rcp(s);
                            const float D = l * is;
                            const float rs = __builtin_amdgcn_rsqf(D);
                            gsq[k * TS + j] = on ? D * rs : 0.0f;
                            gvt[k * TS + j] = on ? __builtin_fmaf(D, cj, __builtin_fmaf(tau, is, l)) * rs : 0.0f;
                        }
                    }
                }
                phase_sync();
            }
            STAMP(1);
            // -------------------------------------------------------- phase R: backward sweep
            f32x4 P;
            {   // terminal: P~ = [diag(We)+reg_e, q_N; q_N', 0]
                const float qc = c_is_x ? qv[N * TS + c] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * q4 + r, ir = index_of(row);
                    const bool r_is_x = ir >= 0 && ir < NX;
                    float v = 0.0f;
                    if (row == c && r_is_x) v = we_c;
                    if (c == HS && r_is_x) v = qv[N * TS + row];
                    if (row == HS && c_is_x) v = qc;
                    P[r] = v;
                }
            }
            // Backward sweep.  The wave is alone on its SIMD at B = 1024, so nothing else hides
            // latency: stage images are prefetched one stage ahead and the cost tiles of the next
            // stage are built inside the current one.
            auto sweep = [&](auto ipm_tag) {
                constexpr bool IPM = decltype(ipm_tag)::value;
                // The additive cost tiles of a stage (NextCost of backward_stage): Q~ = [Q q; q' 0], S~ = [0 r], R, and on R and
                // S~ the barrier terms G'DG and G'v in the form of this instantiation (BarrierTiles): ready from the lane = stage
                // phase (put_foot_terms) and added in build() -- no matrix instruction, nothing to wait for -- or as one product,
                // mfma(i), that finish() folds in.
                struct NextCost {
                    f32x4 Qn, Sn, Rn;
                    const float *qrow, *rrow, *sqrow, *vtrow;   // 16 B of this lane's row quad of q, r and the two barrier rows
                    const float* qcol;                          // q at this lane's column slot
                    const bool *qm, *rm;
                    f32x4 Qc, Rc;
                    bool hx_col;
                    BarrierTiles<FOOT, BF16B> bt;
                    f32x4 q4v, r4v, sq4, vt4;
                    float qcv;
                    __device__ __forceinline__ void fetch() {
                        q4v = *reinterpret_cast<const f32x4*>(qrow);
                        r4v = *reinterpret_cast<const f32x4*>(rrow);
                        qcv = *qcol;
                        if constexpr (IPM) {
                            sq4 = *reinterpret_cast<const f32x4*>(sqrow);
                            vt4 = *reinterpret_cast<const f32x4*>(vtrow);
                        }
                    }
                    __device__ __forceinline__ void build() {
                        Rn = Rc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            Qn[r] = Qc[r] + (qm[r] ? (hx_col ? q4v[r] : qcv) : 0.0f);
                            Sn[r] = rm[r] ? r4v[r] : 0.0f;
                        }
                        if constexpr (IPM) bt.build(sq4, vt4, hx_col, Rn, Sn);
                    }
                    __device__ __forceinline__ void mfma(int i) {
                        if constexpr (IPM) bt.step(i);
                    }
                    __device__ __forceinline__ void finish() {
                        if constexpr (IPM) bt.finish(hx_col, Rn, Sn);
                    }
                };
                auto next_cost = [&](int kk) {
                    NextCost nc;
                    nc.qrow = qv + kk * TS + 4 * q4; nc.rrow = rv + kk * TS + 4 * q4;
                    nc.sqrow = gsq + kk * TS + 4 * q4; nc.vtrow = gvt + kk * TS + 4 * q4;
                    nc.qcol = qv + kk * TS + c;
                    nc.qm = qm; nc.rm = rm;
                    nc.Qc = Qc; nc.Rc = Rc; nc.bt = bt; nc.hx_col = is_hx_col;
                    return nc;
                };
                ImageLane<M> il;
                il.init(lane);
                RowStoreLane ks, cs;
                ks.init(lane, G::KQ, G::K_FLOATS, N - 1, N);
                cs.init(lane, G::CQ, G::C_FLOATS, N - 1, N);
                f32x4 A0 = il.fix_A(il.load_A(At + (size_t)(N - 1) * G::A_FLOATS), lane);
                f32x4 B0 = il.fix_B(il.load_B(Bt + (size_t)(N - 1) * G::B_FLOATS), lane);
                f32x4 T0 = il.fix_Bt(il.load_Bt(Bt + (size_t)(N - 1) * G::B_FLOATS), lane);
                f32x4 Qt, St, Rt;
                {   // prologue: cost tiles of stage N-1
                    NextCost nc = next_cost(N - 1);
                    nc.fetch();
                    nc.build();
#pragma unroll
                    for (int i = 0; i < 4; ++i) nc.mfma(i);
                    nc.finish();
                    Qt = nc.Qn; St = nc.Sn; Rt = nc.Rn;
                }
                int lane_zero = 0;
                asm volatile("" : "+v"(lane_zero));
                // (The stage body and the dispatch over the static patterns stand twice below.  Tried against the parent's instruction
                // stream, tools/asm_identity.py: one dispatch_pattern<M, ALLV>(index or key, f) for both loops left ten instantiations
                // the same and changed the two resident short-list kernels of Centroidal, 2028 of 15 999 and 1818 of 16 065 lines (SGPR
                // spill slots), in four forms; one stage body for both loops, parameterised by whether it reads a run-time mask,
                // changed all twelve, 1902 to 11 963 lines.  DESIGN.md 7.)
                // Two stage loops, chosen by measurement (DESIGN.md 7): one wave per SIMD (resident) walks the horizon in runs of one
                // contact pattern; two waves per SIMD (lean) keep the dispatch per stage -- there the other wave hides it, and the
                // run loops measured 3.0 % slower at B = 8192.
                if constexpr (LEAN) {
                    unsigned cm = umask[N - 1];
                    for (int k = N - 1; k >= 0; --k) {
    #ifdef NMPC_STAMPS
                        sst.t0 = __builtin_readcyclecounter();
    #endif
                        // next stage's images and coupling mask: issued first, consumed by the register
                        // rotation at the end of this stage -- by then only this stage's K~/Acl~ stores are
                        // younger (vmcnt retires in order), so neither the loads nor the stores stall the sweep
                        const int kn = (k > 0) ? k - 1 : 0;
    #ifdef QP_T_ONEIMG      // timing build (tools/qp_traffic_timing.sh): every stage reads the images of stage 0 (cache-resident) -- results are wrong
                        const int ki = (a.B < 0) ? kn : 0;
    #else
                        const int ki = kn;
    #endif
                        const f32x4 A1 = il.load_A(At + (size_t)ki * G::A_FLOATS);
                        const f32x4 B1 = il.load_B(Bt + (size_t)ki * G::B_FLOATS);
                        const f32x4 T1 = il.load_Bt(Bt + (size_t)ki * G::B_FLOATS);
                        // (read through an offset the compiler cannot see is uniform: the value stays in a
                        // VGPR until the end of the stage instead of being scalarised, and waited for, here)
                        const unsigned cm_next = umask[kn + lane_zero];
                        f32x4 Kk, Acl;
                        NextCost sh = next_cost(kn);
                        // a static body holds the barrier-product steps of its own stance feet only: exact zeros elsewhere
                        // while the next stage's pattern is the same or narrower.  The rare stage before a touch-down
                        // (bit 24 of the mask word) runs the body of the widest pattern instead -- valid for any pattern
                        // (it eliminates every pivot for real), all four steps, and no extra code on the common path
                        auto run = [&](auto mask_tag) {
                            constexpr unsigned MK = decltype(mask_tag)::value;
                            constexpr unsigned STEPS = (IPM && !FOOT && !BF16B && MK != DYNAMIC_MASK) ? M::barrier_steps(MK) : 0xFu;
                            return backward_stage<NU, MK, true, ALLV, STEPS, LEAN ? 0 : 2>(P, A0, B0, T0, Qt, St, Rt, conv, sl, lane,
                                                                            cm & 0xFFFFu, Kk, Acl, sh SST_PASS);
                        };
                        bool ok = true;
                        // one static variant per mask: the model's short list as a chain (ALLV = false), or
                        // every listed variant through a decision tree; any other mask takes the run-time fallback
    #define NMPC_VARIANT(I)                                                                                   \
        case I:                                                                                               \
            if constexpr (I < M::N_STATIC_MASKS)                                                              \
                ok = run(std::integral_constant<unsigned, M::static_mask(I < M::N_STATIC_MASKS ? I : 0)>{}); \
            else ok = run(std::integral_constant<unsigned, DYNAMIC_MASK>{});                                  \
            break;
    #define NMPC_COMMON(J) (M::common_variant(J) >= 0 && vi == M::common_variant(J))
    #define NMPC_RUN_COMMON(J) run(std::integral_constant<unsigned, M::static_mask(M::common_variant(J) >= 0 ? M::common_variant(J) : 0)>{})
                        const int vi = ((cm >> 24) & 1u) ? WIDEST : (int)((cm >> 16) & 0x1Fu) - 1;
                        if constexpr (!ALLV) {
                            if (NMPC_COMMON(0)) ok = NMPC_RUN_COMMON(0);
                            else if (NMPC_COMMON(1)) ok = NMPC_RUN_COMMON(1);
                            else if (NMPC_COMMON(2)) ok = NMPC_RUN_COMMON(2);
                            else if (NMPC_COMMON(3)) ok = NMPC_RUN_COMMON(3);
                            else ok = run(std::integral_constant<unsigned, DYNAMIC_MASK>{});
                        } else {
                            switch (vi) {
                                NMPC_VARIANT(0) NMPC_VARIANT(1) NMPC_VARIANT(2) NMPC_VARIANT(3)
                                NMPC_VARIANT(4) NMPC_VARIANT(5) NMPC_VARIANT(6) NMPC_VARIANT(7)
                                NMPC_VARIANT(8) NMPC_VARIANT(9) NMPC_VARIANT(10) NMPC_VARIANT(11)
                                NMPC_VARIANT(12) NMPC_VARIANT(13) NMPC_VARIANT(14) NMPC_VARIANT(15)
                                default: ok = run(std::integral_constant<unsigned, DYNAMIC_MASK>{});
                            }
                        }
    #undef NMPC_VARIANT
    #undef NMPC_COMMON
    #undef NMPC_RUN_COMMON
                        qp_ok = ok && qp_ok;
    #ifdef QP_T_NOSTORE     // timing build: no gain stores -- results are wrong, the time tells what the stores cost
                        if (a.B < 0)
    #endif
                        {
                        ks.store(Kt, Kk);      // gain tiles of this stage, read by the forward sweep
                        cs.store(Ct, Acl);
                        }
                        A0 = il.fix_A(A1, lane);
                        B0 = il.fix_B(B1, lane);
                        T0 = il.fix_Bt(T1, lane);
                        Qt = sh.Qn; St = sh.Sn; Rt = sh.Rn;
                        cm = __builtin_amdgcn_readfirstlane(cm_next);
                        SST_TILES(5);
                    }
                } else {
                    // The stages of one run (run-length schedule of the prologue): top-1 down to top-len, all with the body of
                    // MK.  A static body holds the barrier-product steps of its own stance feet only: exact zeros elsewhere
                    // while the next stage's pattern is the same or narrower -- inside a run it is the same, behind its last
                    // stage it is narrower, since the stage before a touch-down is a run of the widest pattern's body (valid
                    // for any pattern: it eliminates every pivot for real, all four steps).
                    auto run_stages = [&](auto mask_tag, int top, int len) {
                        constexpr unsigned MK = decltype(mask_tag)::value;
                        constexpr bool DYN = (MK == DYNAMIC_MASK);
                        constexpr unsigned STEPS = (IPM && !FOOT && !BF16B && !DYN) ? M::barrier_steps(MK) : 0xFu;
                        unsigned cm = 0u;       // coupling mask of the stage: the fallback body alone reads it
                        if constexpr (DYN) cm = __builtin_amdgcn_readfirstlane(umask[top - 1]);
                        for (int k = top - 1; k >= top - len; --k) {
#ifdef NMPC_STAMPS
                            sst.t0 = __builtin_readcyclecounter();
#endif
                            // next stage's images: issued first, consumed by the register rotation at the end of this
                            // stage -- by then only this stage's K~/Acl~ stores are younger (vmcnt retires in order), so
                            // neither the loads nor the stores stall the sweep
                            const int kn = (k > 0) ? k - 1 : 0;
#ifdef QP_T_ONEIMG      // timing build (tools/qp_traffic_timing.sh): every stage reads the images of stage 0 (cache-resident) -- results are wrong
                            const int ki = (a.B < 0) ? kn : 0;
#else
                            const int ki = kn;
#endif
                            const f32x4 A1 = il.load_A(At + (size_t)ki * G::A_FLOATS);
                            const f32x4 B1 = il.load_B(Bt + (size_t)ki * G::B_FLOATS);
                            const f32x4 T1 = il.load_Bt(Bt + (size_t)ki * G::B_FLOATS);
                            // (the fallback's next mask: read through an offset the compiler cannot see is uniform, so the
                            // value stays in a VGPR until the end of the stage instead of being scalarised, and waited for, here)
                            unsigned cm_next = 0u;
                            if constexpr (DYN) cm_next = umask[kn + lane_zero];
                            f32x4 Kk, Acl;
                            NextCost sh = next_cost(kn);
                            const bool ok = backward_stage<NU, MK, true, ALLV, STEPS, LEAN ? 0 : 2>(P, A0, B0, T0, Qt, St, Rt, conv, sl, lane,
                                                                                                 cm & 0xFFFFu, Kk, Acl, sh SST_PASS);
                            qp_ok = ok && qp_ok;
#ifdef QP_T_NOSTORE     // timing build: no gain stores -- results are wrong, the time tells what the stores cost
                            if (a.B < 0)
#endif
                            {
                            ks.store(Kt, Kk);      // gain tiles of this stage, read by the forward sweep
                            cs.store(Ct, Acl);
                            }
                            A0 = il.fix_A(A1, lane);
                            B0 = il.fix_B(B1, lane);
                            T0 = il.fix_Bt(T1, lane);
                            Qt = sh.Qn; St = sh.Sn; Rt = sh.Rn;
                            if constexpr (DYN) cm = __builtin_amdgcn_readfirstlane(cm_next);
                            SST_TILES(5);
                        }
                    };
                    // one static body per key: the model's short list (ALLV = false) or every listed variant; the run word
                    // of the next run is requested when a run starts and waited for when it ends
#define NMPC_VARIANT(I)                                                                                                 \
        case I:                                                                                                             \
            if constexpr (I < M::N_STATIC_MASKS)                                                                            \
                run_stages(std::integral_constant<unsigned, M::static_mask(I < M::N_STATIC_MASKS ? I : 0)>{}, top, len);    \
            else run_stages(std::integral_constant<unsigned, DYNAMIC_MASK>{}, top, len);                                    \
            break;
#define NMPC_COMMON(J) (M::common_variant(J) >= 0 && key == J##u)
#define NMPC_RUN_COMMON(J) run_stages(std::integral_constant<unsigned, M::static_mask(M::common_variant(J) >= 0 ? M::common_variant(J) : 0)>{}, top, len)
                    unsigned rw = __builtin_amdgcn_readfirstlane(runs[0]);
                    for (int r = 1; (rw & 0x1FFu) != 0u; ++r) {
                        const unsigned rw_next = runs[r + lane_zero];
                        const int top = (int)(rw & 0x1FFu), len = (int)((rw >> 9) & 0x1FFu);
                        const unsigned key = rw >> 18;
                        if constexpr (!ALLV) {
                            if (NMPC_COMMON(0)) NMPC_RUN_COMMON(0);
                            else if (NMPC_COMMON(1)) NMPC_RUN_COMMON(1);
                            else if (NMPC_COMMON(2)) NMPC_RUN_COMMON(2);
                            else if (NMPC_COMMON(3)) NMPC_RUN_COMMON(3);
                            else run_stages(std::integral_constant<unsigned, DYNAMIC_MASK>{}, top, len);
                        } else {
                            switch (key) {
                                NMPC_VARIANT(0) NMPC_VARIANT(1) NMPC_VARIANT(2) NMPC_VARIANT(3)
                                NMPC_VARIANT(4) NMPC_VARIANT(5) NMPC_VARIANT(6) NMPC_VARIANT(7)
                                NMPC_VARIANT(8) NMPC_VARIANT(9) NMPC_VARIANT(10) NMPC_VARIANT(11)
                                NMPC_VARIANT(12) NMPC_VARIANT(13) NMPC_VARIANT(14) NMPC_VARIANT(15)
                                default: run_stages(std::integral_constant<unsigned, DYNAMIC_MASK>{}, top, len);
                            }
                        }
                        rw = __builtin_amdgcn_readfirstlane(rw_next);
                    }
#undef NMPC_VARIANT
#undef NMPC_COMMON
#undef NMPC_RUN_COMMON
                }
            };
            if (use_ipm) sweep(std::true_type{}); else sweep(std::false_type{});
            __threadfence_block();          // K~/Acl~ images: stored above, read by other lanes below
            wave_sync();
            STAMP(2);
            // -------------------------------------------------------- phase F: forward sweep
            // dx~+ = Acl~ dx~ , du = K~ dx~ as ONE row-per-lane mat-vec: lane i < nx holds row i of
            // Acl~ (the stored image is row-major, columns by slot), lane 16+j row j of K~; dx~ is
            // wave-uniform (SGPRs, refreshed by v_readlane).  13 FMAs + 12 readlanes per stage -- fp32
            // MFMA and VALU do not overlap on a SIMD, so the 16-column MFMA mat-vec cost 8x32 cycles.
            // Rows are prefetched FWD_PF stages ahead (a stage is shorter than an L2 miss).
            float* oX = use_ipm ? dXp : dX;
            float* oU = use_ipm ? dUp : dU;
            float vs[NX];
            if constexpr (LEAN) {      // (the same difference, kept in the LDS: X lives in the workspace)
#pragma unroll
                for (int i = 0; i < NX; ++i) vs[i] = dx0s[i];
                if (lane < NX) AT(oX, 0, lane) = dx0s[lane];
            } else {
#pragma unroll
                for (int i = 0; i < NX; ++i) vs[i] = x0[i] - AT(Xs, 0, i);
                if (lane < NX) AT(oX, 0, lane) = x0[lane] - AT(Xs, 0, lane);
            }
            constexpr int FWD_PF = 4, RQ4 = slot_of(NX - 1) / 4 + 1;
            const bool is_x = lane < NX, is_u = (lane >= 16 && lane < 16 + NU);
            // row of this lane in the image of stage 0, as a byte offset from the workspace base
            unsigned rowoff = 4u * (unsigned)((is_x ? wl.Ct : wl.Kt) + (is_x ? lane : is_u ? lane - 16 : 0) * TS);
            const unsigned rowstep = 4u * (is_x ? G::C_FLOATS : G::K_FLOATS);
            float* dst = is_x ? &AT(oX, 1, lane) : is_u ? &AT(oU, 0, lane - 16) : idle_sink;
            const int dstep = (is_x || is_u) ? (LEAN ? TS : 1) : 0;
            // the used floats of a row: quad 0 (three states and the homogeneous slot) as a 16 B load,
            // the other quads as 12 B loads (a load with dead elements lets the allocator reuse them at
            // once -- which means a wait on the load in flight)
            auto load_row = [&](unsigned off, f32x4 (&row)[RQ4]) {
                row[0] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(ws) + (size_t)off);
#pragma unroll
                for (int g = 1; g < RQ4; ++g) {
                    const f32x3u v = *reinterpret_cast<const f32x3u*>(reinterpret_cast<const char*>(ws) + (size_t)off + 16 * g);
                    row[g] = f32x4{v[0], v[1], v[2], 0.0f};
                }
            };
            f32x4 ring[FWD_PF][RQ4];
#pragma unroll
            for (int j = 0; j < FWD_PF; ++j) load_row(rowoff + (unsigned)((j < N) ? j : N - 1) * rowstep, ring[j]);
            const unsigned rowlast = rowoff + (unsigned)(N - 1) * rowstep;
            rowoff += FWD_PF * rowstep;        // next row to prefetch
            // one stage: consume a ring slot, then refill it with the row FWD_PF stages ahead (the
            // refill comes after the last use, so old and new value share registers and the loop
            // carries no copies -- a copy of fresh load data would put a full wait into every stage)
            auto fwd_stage = [&](int k, f32x4 (&slot)[RQ4]) {
                // four accumulator chains: a dependent v_fmac issues only every ~11 cycles, four chains
                // keep the 4-cycle issue rate (tools/ubench/ubench_dpp.hip).  asm: left to itself the
                // compiler re-associates the sum and, worse, re-schedules the ring refills around it.
                float acc = slot[0][HS], acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;   // slot HS: times dx~[HS] = 1
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    const float e = slot[slot_of(i) >> 2][slot_of(i) & 3];
                    float& ac = (i & 3) == 0 ? acc : (i & 3) == 1 ? acc1 : (i & 3) == 2 ? acc2 : acc3;
                    asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(ac) : "s"(vs[i]), "v"(e));
                }
                acc = (acc + acc1) + (acc2 + acc3);
#ifdef QP_T_ONEIMG
                load_row((a.B < 0) ? rowoff : rowlast, slot);
#else
                load_row(rowoff < rowlast ? rowoff : rowlast, slot);
#endif
                rowoff += rowstep;
                dst[k * dstep] = acc;
#pragma unroll
                for (int i = 0; i < NX; ++i) vs[i] = bcast(acc, i);
                __builtin_amdgcn_sched_barrier(0);   // keep each refill inside its own stage
            };
            int k0 = 0;
            for (; k0 + FWD_PF <= N; k0 += FWD_PF) {     // whole groups: one straight-line body
#pragma unroll
                for (int j = 0; j < FWD_PF; ++j) fwd_stage(k0 + j, ring[j]);
            }
#pragma unroll
            for (int j = 0; j < FWD_PF - 1; ++j)          // the last N % FWD_PF stages
                if (k0 + j < N) fwd_stage(k0 + j, ring[j]);
            phase_sync();
            STAMP(3);
            // -------------------------------------------------------- phase I: IPM update
            if (use_ipm && one_stage_per_lane) {
                // Lane = stage, everything of the stage in registers: step direction
                //   ds = -(G du+ + c) - s ,  dlam = tau/s - lam - (lam/s) ds ,
                // fraction to the boundary  alpha = min(1, gamma / max(-d./.))  (one division per wave),
                // update, complementarity sum, and the barrier coefficients of the next iteration.
                const bool live = lane < N;
                const int k = live ? lane : 0;
                float du[NU], g[NG], uk[NU], cc[NG], s[NG], l[NG], ds[NG], dl[NG];
                ld_row(dUp, k, du);
                ld_row(Us, k, uk);
                ld_row(sv, k, s);
                ld_row(lv, k, l);
                // lean variant: the blend of the step with the new one rides in this phase (the stage's rows, requested
                // here, used once the step length is known) instead of two element-wise passes over the workspace
                const int kx = (lane <= N) ? lane : 0;
                float dxo[LEAN ? NX : 1], dxn[LEAN ? NX : 1], duo[LEAN ? NU : 1];
                if constexpr (LEAN) { ld_row(dX, kx, dxo); ld_row(dXp, kx, dxn); ld_row(dU, k, duo); }
                M::gdot(a.mp, du, g);
                M::gdot(a.mp, uk, cc);          // c = G u - h at the linearisation point
                const unsigned am = live ? actm[k] : 0u;
                float rp = 0.0f, rd = 0.0f;
#pragma unroll
                for (int j = 0; j < NG; ++j) {
                    cc[j] -= M::h(a.mp, j);
                    const float is = fast_rcp(s[j]);
                    ds[j] = -(g[j] + cc[j]) - s[j];
                    dl[j] = __builtin_fmaf(-(l[j] * is), ds[j], __builtin_fmaf(tau, is, -l[j]));
                    const bool on = (am >> j) & 1u;
                    rp = on ? fmaxf(rp, -ds[j] * is) : rp;
                    rd = on ? fmaxf(rd, -dl[j] * __builtin_amdgcn_rcpf(l[j])) : rd;
                }
                const float rpm = wave_max(rp), rdm = wave_max(rd);
                const float ap = rpm > a.gamma ? a.gamma / rpm : 1.0f;
                const float ad = rdm > a.gamma ? a.gamma / rdm : 1.0f;
                float m_l = 0.0f;
#pragma unroll
                for (int j = 0; j < NG; ++j) {
                    const bool on = (am >> j) & 1u;
                    s[j] = on ? __builtin_fmaf(ap, ds[j], s[j]) : s[j];
                    l[j] = on ? __builtin_fmaf(ad, dl[j], l[j]) : l[j];
                    m_l = on ? __builtin_fmaf(s[j], l[j], m_l) : m_l;
                }
                if (live) { st_row(sv, k, s); st_row(lv, k, l); }
                mu_sum = wave_sum(m_l);
                if constexpr (LEAN) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) dxo[i] = __builtin_fmaf(ap, dxn[i] - dxo[i], dxo[i]);
#pragma unroll
                    for (int i = 0; i < NU; ++i) duo[i] = __builtin_fmaf(ap, du[i] - duo[i], duo[i]);
                    if (lane <= N) st_row(dX, kx, dxo);
                    if (live) st_row(dU, k, duo);
                    if (N == 64 && lane < NX) {            // node 64 has no lane of its own
                        const float d = AT(dX, 64, lane);
                        AT(dX, 64, lane) = __builtin_fmaf(ap, AT(dXp, 64, lane) - d, d);
                    }
                } else {
                    blend(ap);
                }
                if (ii + 1 < n_sweeps && live) {
                    const float tau_n = fmaxf(a.sigma * mu_sum / (float)n_act, a.tau_min);
                    if constexpr (FOOT) {
                        put_foot_terms(k, am, s, l, cc, tau_n);
                    } else {
                        float sq[NG], vt[NG];
#pragma unroll
                        for (int j = 0; j < NG; ++j) {
                            const bool on = (am >> j) & 1u;
                            const float is = fast_rcp(s[j]);
                            const float D = l[j] * is;
                            const float rs = __builtin_amdgcn_rsqf(D);
                            sq[j] = on ? D * rs : 0.0f;
                            vt[j] = on ? __builtin_fmaf(D, cc[j], __builtin_fmaf(tau_n, is, l[j])) * rs : 0.0f;
                        }
#pragma unroll
                        for (int j = 0; j < NG; ++j) { gsq[k * TS + j] = sq[j]; gvt[k * TS + j] = vt[j]; }
                    }
                }
                phase_sync();
            } else if (use_ipm) {
                float ap_l = 1.0f, ad_l = 1.0f;
                // long horizons (several stages per lane): the same update in two passes.  (Both load du, uk and form g, cc: one
                // helper for that changed the four resident Centroidal kernels, 114 to 572 lines, in two forms.)
                // ds = -(G du+ + c) - s ;  dlam = tau/s - lam - (lam/s) ds   (recomputed in the
                // second pass rather than kept in runtime-indexed arrays, which would go to scratch)
                auto step_dir = [&](int k, int j, const float (&g)[NG], const float (&cc)[NG], float& s, float& l, float& dsj, float& dlj) {
                    s = AT(sv, k, j); l = AT(lv, k, j);
                    const float is = fast_rcp(s);
                    dsj = -(g[j] + cc[j]) - s;
                    dlj = __builtin_fmaf(-(l * is), dsj, __builtin_fmaf(tau, is, -l));
                };
                for (int k = lane; k < N; k += 64) {
                    float du[NU], g[NG], uk[NU], cc[NG];
#pragma unroll
                    for (int i = 0; i < NU; ++i) { du[i] = AT(dUp, k, i); uk[i] = AT(Us, k, i); }
                    M::gdot(a.mp, du, g);
                    M::gdot(a.mp, uk, cc);          // c = G u - h, recomputed (kept out of LDS)
#pragma unroll
                    for (int j = 0; j < NG; ++j) cc[j] -= M::h(a.mp, j);
                    const unsigned am = actm[k];
#pragma unroll
                    for (int j = 0; j < NG; ++j) {
                        float s, l, dsj, dlj;
                        step_dir(k, j, g, cc, s, l, dsj, dlj);
                        const bool on = (am >> j) & 1u;
                        if (on && dsj < 0.0f) ap_l = fminf(ap_l, -a.gamma * s / dsj);
                        if (on && dlj < 0.0f) ad_l = fminf(ad_l, -a.gamma * l / dlj);
                    }
                }
                const float ap = wave_min(ap_l), ad = wave_min(ad_l);
                float m_l = 0.0f;
                for (int k = lane; k < N; k += 64) {
                    float du[NU], g[NG], uk[NU], cc[NG];
#pragma unroll
                    for (int i = 0; i < NU; ++i) { du[i] = AT(dUp, k, i); uk[i] = AT(Us, k, i); }
                    M::gdot(a.mp, du, g);
                    M::gdot(a.mp, uk, cc);          // c = G u - h, recomputed (kept out of LDS)
#pragma unroll
                    for (int j = 0; j < NG; ++j) cc[j] -= M::h(a.mp, j);
                    const unsigned am = actm[k];
#pragma unroll
                    for (int j = 0; j < NG; ++j) {
                        float s, l, dsj, dlj;
                        step_dir(k, j, g, cc, s, l, dsj, dlj);
                        const bool on = (am >> j) & 1u;
                        s = on ? __builtin_fmaf(ap, dsj, s) : s;
                        l = on ? __builtin_fmaf(ad, dlj, l) : l;
                        AT(sv, k, j) = s;
                        AT(lv, k, j) = l;
                        if (on) m_l = __builtin_fmaf(s, l, m_l);
                    }
                }
                mu_sum = wave_sum(m_l);
                blend(ap);
                phase_sync();
            }
        }
        STAMP(4);
        // ------------------------------------------------------------ phase S: step
        float sn_l = 0.0f;
        bool bad_l = false;
        auto step_norm = [&](int, float v) {
            bad_l = bad_l || !(fabsf(v) <= 1e30f);
            sn_l = fmaxf(sn_l, fabsf(v));
        };
        // lean variant, one node per lane: the node's rows go through registers once -- norm, step and the store to the
        // caller's X, U -- instead of six element-wise passes over the workspace (each a memory round trip)
        float dxr[LEAN ? NX : 1], dur[LEAN ? NU : 1];
        if constexpr (LEAN) {
            if (rows_in_regs) {
                ld_row(dX, kx_s, dxr); ld_row(Xs, kx_s, xr); ld_row(dU, ku_s, dur); ld_row(Us, ku_s, ur);
#pragma unroll
                for (int i = 0; i < NX; ++i) step_norm(0, lane <= N ? dxr[i] : 0.0f);
#pragma unroll
                for (int i = 0; i < NU; ++i) step_norm(0, lane < N ? dur[i] : 0.0f);
            }
        }
        if (!rows_in_regs) {
            batched<10>(SA_.nX, lane, [&](int i) { return dX[i]; }, step_norm);
            batched<10>(SA_.nU, lane, [&](int i) { return dU[i]; }, step_norm);
        }
        stepn = wave_max(sn_l);
        const bool bad = __any(bad_l);
        if (bad) { status = NMPC_STATUS_NAN; finished = true; }
        alpha = 1.0f;
        if (a.line_search && !bad) {
            // l1 merit: cost + rho * (|x0 - X0| + sum |defects| + sum max(0, G u - h))
            auto merit = [&](float al) -> float {
                float m_l = 0.0f;
                for (int k = lane; k < N; k += 64) {
                    float x[NX], u[NU], xn[NX], p[NP > 0 ? NP : 1];
#pragma unroll
                    for (int i = 0; i < NX; ++i) x[i] = __builtin_fmaf(al, AT(dX, k, i), AT(Xs, k, i));
#pragma unroll
                    for (int i = 0; i < NU; ++i) u[i] = __builtin_fmaf(al, AT(dU, k, i), AT(Us, k, i));
#pragma unroll
                    for (int i = 0; i < NP; ++i) p[i] = pg[(size_t)k * NP + i];
                    M::step(a.mp, x, u, p, xn);
                    const float* yk = yr + (a.yref_per_stage ? (size_t)k * NY : 0);
                    float viol = 0.0f, cst = 0.0f;
#pragma unroll
                    for (int i = 0; i < NX; ++i) {
                        const float e = x[i] - yk[i];
                        cst += 0.5f * a.W[i] * e * e;
                        viol += fabsf(xn[i] - __builtin_fmaf(al, AT(dX, k + 1, i), AT(Xs, k + 1, i)));
                    }
#pragma unroll
                    for (int i = 0; i < NU; ++i) {
                        const float e = u[i] - yk[NX + i];
                        cst += 0.5f * a.W[NX + i] * e * e;
                    }
                    if (a.n_ipm > 0) {
                        float g[NG];
                        M::gdot(a.mp, u, g);
                        const unsigned am = M::active_mask(a.mp, p);
#pragma unroll
                        for (int j = 0; j < NG; ++j)
                            if ((am >> j) & 1u) viol += fmaxf(g[j] - M::h(a.mp, j), 0.0f);
                    }
                    m_l += cst + a.rho * viol;
                }
                if (lane < NX) {
                    const float xe = __builtin_fmaf(al, AT(dX, N, lane), AT(Xs, N, lane));
                    const float e = xe - yre[lane];
                    m_l += 0.5f * a.We[lane] * e * e;
                    m_l += a.rho * fabsf(x0[lane] - __builtin_fmaf(al, AT(dX, 0, lane), AT(Xs, 0, lane)));
                }
                return wave_sum(m_l);
            };
            const float m0 = merit(0.0f);
            for (int t = 0; t < 6; ++t) {
                const float m1 = merit(alpha);
                if (m1 < m0 || t == 5) break;
                alpha *= 0.5f;
            }
        }
        if (!bad) {
            if (rows_in_regs) {
                if constexpr (LEAN) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) xr[i] = __builtin_fmaf(alpha, dxr[i], xr[i]);
#pragma unroll
                    for (int i = 0; i < NU; ++i) ur[i] = __builtin_fmaf(alpha, dur[i], ur[i]);
                }
            } else {
                batched<10>(SA_.nX, lane, [&](int i) { return __builtin_fmaf(alpha, dX[i], Xs[i]); }, [&](int i, float v) { Xs[i] = v; });
                batched<10>(SA_.nU, lane, [&](int i) { return __builtin_fmaf(alpha, dU[i], Us[i]); }, [&](int i, float v) { Us[i] = v; });
                phase_sync();
            }
            if (!qp_ok) { status = NMPC_STATUS_QP; finished = true; }
            else if (a.nlp_tol > 0.0f && stepn < a.nlp_tol) { status = NMPC_STATUS_OK; finished = true; }
        }
    }
    // a NaN step leaves the iterate of the previous iteration -- which, in a call that folded a warm-start shift into its
    // first iteration, is the SHIFTED previous solution: it is written back so that the caller's node bookkeeping
    // (last_node already advanced) and the trajectory stay aligned
    if (status != NMPC_STATUS_NAN || a.shift > 0) {
        if (rows_in_regs) {
            if constexpr (LEAN) {
                if (lane <= N) {
#pragma unroll
                    for (int i = 0; i < NX; ++i) Xg[lane * NX + i] = xr[i];
                }
                if (lane < N) {
#pragma unroll
                    for (int i = 0; i < NU; ++i) Ug[lane * NU + i] = ur[i];
                }
            }
        } else {
            batched<10>((N + 1) * NX, lane, [&](int e) { const int k = e / NX; return AT(Xs, k, e - k * NX); },
                        [&](int e, float v) { Xg[e] = v; });
            batched<10>(N * NU, lane, [&](int e) { const int k = e / NU; return AT(Us, k, e - k * NU); },
                        [&](int e, float v) { Ug[e] = v; });
        }
    }
    STAMP(5);
#ifdef NMPC_STAMPS
    if (lane == 0 && a.dbg) {
        for (int i = 0; i < 8; ++i) a.dbg[16 * b + i] = (float)st_acc[i];
        for (int i = 0; i < 8; ++i) a.dbg[16 * b + 8 + i] = (float)sst.acc[i];
    }
#endif
    if (lane == 0) {
        flag[0] = finished ? 1 : 0;
        if (a.status) a.status[b] = status;
        if (a.stats) {
            a.stats[4 * b + 0] = cost;
            a.stats[4 * b + 1] = stepn;
            a.stats[4 * b + 2] = alpha;
            a.stats[4 * b + 3] = (float)(a.it + 1);
        }
    }
#undef AT
}

}  // namespace nmpc
