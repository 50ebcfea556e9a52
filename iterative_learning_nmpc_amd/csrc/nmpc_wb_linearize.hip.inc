// nmpc_wb_linearize.hip.inc -- the linearisation kernel of the whole-body family: one thread per (problem, node) evaluates the
// model (nmpc_wb_model.hpp) at the current iterate and writes the node's record and its compact Jacobian record
// (nmpc_wb_layout.hpp) for the QP kernel.  Included by nmpc_wb.hip, behind its contraction pragma and nmpc_wb_layout.hpp.
#pragma clang fp contract(off)

namespace nmpc {
namespace wb {

// Linearisation: thread t <-> (problem b, node k), k = N is the terminal node.
#ifndef WB_LIN_WAVES
#define WB_LIN_WAVES 1
#endif
// The file is compiled once per momentum model (nmpc_wb.hip includes it twice): WB_ART = 0 is the declared model and gives
// nmpc_wb_linearize_kernel, whose text is what it was before the second model existed; WB_ART = 1 is the articulated model
// (nmpc_wb_momentum.hpp; DESIGN.md 3.2) and gives nmpc_wb_linearize_art_kernel -- the consistency rows and the momentum rows of
// the dynamics take the tree's centroidal quantities from the node's momentum record `m.mrec`, and the consistency rows go,
// dense, into `m.dcons`.
#if WB_ART
__global__ __launch_bounds__(64, WB_LIN_WAVES) void nmpc_wb_linearize_art_kernel(const WbArgs a, const WbArtArgs m) {
#else
__global__ __launch_bounds__(64, WB_LIN_WAVES) void nmpc_wb_linearize_kernel(const WbArgs a) {
#endif
    const int N = a.N;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)a.B * (N + 1)) return;
    const int b = (int)(t / (N + 1)), k = (int)(t - (long long)b * (N + 1));
    const WsLayout wl(N);
    float* ws = a.ws + (size_t)b * wl.stride;
    if (a.it > 0 && reinterpret_cast<const int*>(ws + wl.flag)[0]) return;
    if (a.skip && (a.skip[b] & a.skip_mask) != 0) return;
    const bool term = (k == N);
    const ModelParams& mp = a.mp;
    const float dt = mp.dt;
    const float* Xg = a.X + (size_t)b * (N + 1) * NX;
    const float* Ug = a.U + (size_t)b * N * NU;
    // alignments the vectoriser may rely on (a lane is a node: every access of this kernel is strided across the wave, so its
    // cost is the number of memory instructions -- 16 B pieces of the record instead of 210 dword stores, 8 B pieces of x, u, yref).
    // Workspace: 256 B; caller's arrays: 8 B (x, u, references: rows of 42, 30, 90 / 66 floats) and 16 B (parameters), checked by
    // the C-ABI (nmpc_api.hip, launch_wb).
    float* rec = static_cast<float*>(__builtin_assume_aligned(ws + wl.rec + (size_t)k * REC, 16));
    float* js = ws + wl.js + (size_t)k * CJ_FLOATS;
#if WB_ART
    // the node's momentum record (read where it is used): the tree's mass and centre of mass in place of the declared body's
    const float* mr = static_cast<const float*>(__builtin_assume_aligned(m.mrec + (size_t)t * MR_FLOATS, 16));
    const float com[3] = {mr[MR_COM], mr[MR_COM + 1], mr[MR_COM + 2]};
#endif

    float x[NX], u[NU], p[NP];
    const float* xk = static_cast<const float*>(__builtin_assume_aligned(Xg + (size_t)shifted_node(k, a.shift, N) * NX, 8));
#pragma unroll
    for (int i = 0; i < NX; i += 2) { const f32x2 v = *reinterpret_cast<const f32x2*>(xk + i); x[i] = v[0]; x[i + 1] = v[1]; }
    const int ks = term ? 0 : k;
    {
        // warm-start shift as an index map; in the exposed tail the contact forces are zero and the accelerations keep the
        // previous solution's values at that stage (solver.py:316-322 moves a[:, :n_warm_start] and zeroes f[:, n_warm_start:])
        const bool ok = (a.shift == 0) || shifted_stage_valid(ks, a.shift, N);
        const float* uk = static_cast<const float*>(__builtin_assume_aligned(Ug + (size_t)(ok ? ks + a.shift : ks) * NU, 8));
#pragma unroll
        for (int i = 0; i < NU; i += 2) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(uk + i);
            u[i] = (ok || i < WF) ? v[0] : 0.0f; u[i + 1] = (ok || i + 1 < WF) ? v[1] : 0.0f;
        }
    }
    const float* pg = static_cast<const float*>(__builtin_assume_aligned(a.params + ((size_t)b * (N + 1) + k) * NP, 16));
    static_assert(NX % 2 == 0 && NU % 2 == 0 && NY % 2 == 0 && NYE % 2 == 0 && NP % 4 == 0 && REC % 4 == 0, "row alignments");
#pragma unroll
    for (int i = 0; i < NP; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pg + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) p[i + r] = v[r];
    }
    const int ny = term ? NYE : NY;
    const float* yr = static_cast<const float*>(__builtin_assume_aligned(
        term ? a.yref_e + (size_t)b * NYE
             : a.yref + (size_t)b * (a.yref_per_stage ? (size_t)N * NY : (size_t)NY) + (a.yref_per_stage ? (size_t)k * NY : 0), 8));
    const float* Wv = term ? a.We : a.W;
    const int r_sw = term ? RE_SWING : RY_SWING, r_ct = term ? RE_CNT : RY_CNT, r_cs = term ? RE_CONS : RY_CONS;
    const int r_ps = term ? RE_POS : RY_POS;
    (void)ny;

    // ---- kinematics
    BaseRot br;
    {
        const float th[3] = {x[WQ + 3], x[WQ + 4], x[WQ + 5]}, thd[3] = {x[WV + 3], x[WV + 4], x[WV + 5]};
        base_rotation<true>(th, thd, br);
    }
    float cost = 0.0f;
    // a run of the node's compact Jacobian record (layout: cj_index), from registers, in 16 B pieces
    float* cj = static_cast<float*>(__builtin_assume_aligned(js, 16));
    auto put_cj = [&](int off, int n, const float* v) {
#pragma unroll
        for (int i = 0; i < n; i += 4) *reinterpret_cast<f32x4*>(cj + off + i) = f32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
    };

    // a run of the record, from registers, in 16 B pieces (`off` a multiple of four)
    auto put_rec = [&](int off, const auto& v) {
        constexpr int n = (int)(sizeof(v) / sizeof(float));
        static_assert(n % 4 == 0, "record runs are whole 16 B pieces");
#pragma unroll
        for (int i = 0; i < n; i += 4) *reinterpret_cast<f32x4*>(rec + off + i) = f32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
    };
    float tau_acc[3] = {0.f, 0.f, 0.f}, F[3] = {0.f, 0.f, 0.f};
    float hfr[36], cdt[4] = {0.f, 0.f, 0.f, 0.f};      // d h_ang+ / d f [3][12] and dt c_f of the record
#pragma unroll
    for (int i = 0; i < 36; ++i) hfr[i] = 0.0f;
    float hq[3][15];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 15; ++j) hq[i][j] = 0.0f;

#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const float ql[3] = {x[WQ + 6 + 3 * f], x[WQ + 7 + 3 * f], x[WQ + 8 + 3 * f]};
        const float wl3[3] = {x[WV + 6 + 3 * f], x[WV + 7 + 3 * f], x[WV + 8 + 3 * f]};
        Leg lg;
        leg_kin<true>(mp, f, ql, wl3, lg);
        // world position, Jacobian J (3x9 wrt xi = [r, theta, ql]) and its time derivative Jd
        float Rb[3];
        mv(br.R, lg.b, Rb);
        const float pz = x[WQ + 2] + Rb[2];
        float J[3][9], Jd[3][9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) { J[i][c] = (i == c) ? 1.0f : 0.0f; Jd[i][c] = 0.0f; }
#pragma unroll
        for (int aa = 0; aa < 3; ++aa) {
            float t0[3], t1[3], t2[3];
            mv(br.Ra[aa], lg.b, t0);
            mv(br.Rad[aa], lg.b, t1);
            mv(br.Ra[aa], lg.bd, t2);
#pragma unroll
            for (int i = 0; i < 3; ++i) { J[i][3 + aa] = t0[i]; Jd[i][3 + aa] = t1[i] + t2[i]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float jc[3] = {lg.Jb.m[c], lg.Jb.m[3 + c], lg.Jb.m[6 + c]};
            const float jdc[3] = {lg.Jbd.m[c], lg.Jbd.m[3 + c], lg.Jbd.m[6 + c]};
            float t0[3], t1[3], t2[3];
            mv(br.R, jc, t0);
            mv(br.Rd, jc, t1);
            mv(br.R, jdc, t2);
#pragma unroll
            for (int i = 0; i < 3; ++i) { J[i][6 + c] = t0[i]; Jd[i][6 + c] = t1[i] + t2[i]; }
        }
        const float cf = p[f], peak = p[4 + f], ppz = p[8 + 3 * f + 2];
        // foot-placement rows (pos_cost, solver.py:128-137,272-273): world x, y of the foot - planned location.  Weight 0
        // outside the contact-restricted mode: the rows are then exact zeros in the image and are not rewritten
        // (a.pos_rows, wave-uniform; nmpc_set_weights has the image cleared when the rows go from weighted to unweighted)
        float fb[CJ_FOOT];      // this foot's part of the compact Jacobian record
        fb[67] = 0.0f;
        if (a.pos_rows) {
            const float px[2] = {x[WQ] + Rb[0], x[WQ + 1] + Rb[1]};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float w = Wv[r_ps + 2 * f + i], sw = sqrtf(w);
                const float res = px[i] - yr[r_ps + 2 * f + i];
                cost += 0.5f * w * res * res;
#pragma unroll
                for (int c = 0; c < 9; ++c) fb[68 + 10 * i + c] = sw * J[i][c];
                fb[68 + 10 * i + 9] = sw * res;
            }
            put_cj(CJ_FOOT * f + 68, 20, fb + 68);
        }
        // swing row: peak z_foot - ref
        {
            const float w = Wv[r_sw + f], sw = sqrtf(w);
            const float res = peak * pz - yr[r_sw + f];
            cost += 0.5f * w * res * res;
#pragma unroll
            for (int c = 0; c < 9; ++c) fb[57 + c] = sw * peak * J[2][c];
            fb[66] = sw * res;
        }
        // contact rows: c (J v + p_gain e_z (z - plane_z)) - ref
        {
            float sres[3], swc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float vel = 0.0f;
#pragma unroll
                for (int c = 0; c < 9; ++c) vel += J[i][c] * x[WV + xi_col(f, c)];
                const float w = Wv[r_ct + 3 * f + i], sw = sqrtf(w);
                const float res = cf * (vel + (i == 2 ? mp.p_gain * (pz - ppz) : 0.0f)) - yr[r_ct + 3 * f + i];
                cost += 0.5f * w * res * res;
                sres[i] = sw * res; swc[i] = sw * cf;
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                fb[6 * c + 0] = swc[0] * Jd[0][c]; fb[6 * c + 1] = swc[1] * Jd[1][c]; fb[6 * c + 2] = swc[2] * (Jd[2][c] + mp.p_gain * J[2][c]);
                fb[6 * c + 3] = swc[0] * J[0][c];  fb[6 * c + 4] = swc[1] * J[1][c];  fb[6 * c + 5] = swc[2] * J[2][c];
            }
            fb[54] = sres[0]; fb[55] = sres[1]; fb[56] = sres[2];
        }
        put_cj(CJ_FOOT * f, 68, fb);
        if (!term) {   // momentum rows of the dynamics
            const float ff[3] = {u[WF + 3 * f], u[WF + 3 * f + 1], u[WF + 3 * f + 2]};
            float tq[3];
#if WB_ART
            const float arm[3] = {Rb[0] - com[0], Rb[1] - com[1], Rb[2] - com[2]};      // p_f - com
            cross(arm, ff, tq);
#else
            cross(Rb, ff, tq);
#endif
#pragma unroll
            for (int i = 0; i < 3; ++i) { F[i] += cf * ff[i]; tau_acc[i] += cf * tq[i]; }
            // d(arm x f)/d xi_c, c = 3..8 (arm = R b does not depend on r)
#pragma unroll
            for (int c = 3; c < 9; ++c) {
                const float da[3] = {J[0][c], J[1][c], J[2][c]};
                float tc[3];
                cross(da, ff, tc);
#pragma unroll
                for (int i = 0; i < 3; ++i) hq[i][xi_col(f, c) - 3] += dt * cf * tc[i];
            }
#if WB_ART
            const float ax[9] = {0.f, -arm[2], arm[1], arm[2], 0.f, -arm[0], -arm[1], arm[0], 0.f};
#else
            const float ax[9] = {0.f, -Rb[2], Rb[1], Rb[2], 0.f, -Rb[0], -Rb[1], Rb[0], 0.f};
#endif
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) hfr[i * 12 + 3 * f + j] = dt * cf * ax[3 * i + j];
            cdt[f] = dt * cf;
        }
    }
#if WB_ART
    {
        // ---- consistency rows  h - A_g(q) v  of the tree: dense over q_3..q_17 (-dh_dq) and v (-A_g), into the node's dense record
        float* dc = static_cast<float*>(__builtin_assume_aligned(m.dcons + (size_t)t * DC_FLOATS, 16));
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float w = Wv[r_cs + i], sw = sqrtf(w);
            const float res = x[WH + i] - mr[MR_AGV + i] - yr[r_cs + i];
            cost += 0.5f * w * res * res;
            float row[DC_ROW];
#pragma unroll
            for (int j = 0; j < 15; ++j) row[j] = -sw * mr[MR_DH + 18 * i + 3 + j];
#pragma unroll
            for (int j = 0; j < 18; ++j) row[DC_V + j] = -sw * mr[MR_AG + 18 * i + j];
            row[DC_H] = sw; row[DC_RES] = sw * res; row[35] = 0.0f;
#pragma unroll
            for (int j = 0; j < DC_ROW; j += 4) *reinterpret_cast<f32x4*>(dc + DC_ROW * i + j) = f32x4{row[j], row[j + 1], row[j + 2], row[j + 3]};
        }
        // d h_ang+ / d q_j gains  -dt (d com / d q_j) x sum c_f f_f,  d com / d q_j = A_g[lin][j] / m
        if (!term) {
#pragma unroll
            for (int j = 0; j < 15; ++j) {
                const float dcq[3] = {mr[MR_AG + 3 + j] / m.m_tree, mr[MR_AG + 18 + 3 + j] / m.m_tree, mr[MR_AG + 36 + 3 + j] / m.m_tree};
                float tc[3];
                cross(dcq, F, tc);
#pragma unroll
                for (int i = 0; i < 3; ++i) hq[i][j] -= dt * tc[i];
            }
        }
    }
#else
    // ---- consistency rows  h - A_g(q) v,  A_g v = [m rdot ; R I_b E(theta) thetadot]
    {
        float cb[36];      // the consistency part of the compact Jacobian record
        cb[33] = cb[34] = cb[35] = 0.0f;
        const float thd[3] = {x[WV + 3], x[WV + 4], x[WV + 5]};
        const float Ib[3] = {mp.ixx, mp.iyy, mp.izz};
        float sy, cy, sx, cx;
        sincosf(x[WQ + 4], &sy, &cy);
        sincosf(x[WQ + 5], &sx, &cx);
        const M3 E = {{-sy, 0.f, 1.f, cy * sx, cx, 0.f, cx * cy, -sx, 0.f}};
        const M3 Ea[3] = {{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}},
                          {{-cy, 0.f, 0.f, -sy * sx, 0.f, 0.f, -cx * sy, 0.f, 0.f}},
                          {{0.f, 0.f, 0.f, cy * cx, -sx, 0.f, -sx * cy, -cx, 0.f}}};
        float wbv[3], Iw[3], L[3];
        mv(E, thd, wbv);
#pragma unroll
        for (int i = 0; i < 3; ++i) Iw[i] = Ib[i] * wbv[i];
        mv(br.R, Iw, L);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            {   // linear momentum
                const float w = Wv[r_cs + i], sw = sqrtf(w);
                const float res = x[WH + i] - mp.mass * x[WV + i] - yr[r_cs + i];
                cost += 0.5f * w * res * res;
                cb[3 * i] = sw; cb[3 * i + 1] = -sw * mp.mass; cb[3 * i + 2] = sw * res;
            }
            {   // angular momentum
                const float w = Wv[r_cs + 3 + i], sw = sqrtf(w);
                const float res = x[WH + 3 + i] - L[i] - yr[r_cs + 3 + i];
                cost += 0.5f * w * res * res;
                cb[9 + 2 * i] = sw; cb[10 + 2 * i] = sw * res;
            }
        }
#pragma unroll
        for (int aa = 0; aa < 3; ++aa) {
            float t0[3], t1[3], t2[3], ew[3], iew[3], iec[3];
            mv(br.Ra[aa], Iw, t0);
            mv(Ea[aa], thd, ew);
#pragma unroll
            for (int i = 0; i < 3; ++i) { iew[i] = Ib[i] * ew[i]; iec[i] = Ib[i] * E.m[3 * i + aa]; }
            mv(br.R, iew, t1);
            mv(br.R, iec, t2);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float sw = sqrtf(Wv[r_cs + 3 + i]);
                cb[15 + 3 * aa + i] = -sw * (t0[i] + t1[i]);
                cb[24 + 3 * aa + i] = -sw * t2[i];
            }
        }
        put_cj(CJ_CONS, 36, cb);
    }
#endif
    // ---- diagonal residuals (base, joint) on x[0..35]: gradient and cost
    {
        float gq[36];
#pragma unroll
        for (int s = 0; s < 36; ++s) {
            const float w = wdiag(a, s, term);
            const float e = x[s] - yr[yref_of_state(s)];
            gq[s] = w * e;
            cost += 0.5f * w * e * e;
        }
        put_rec(R_GQ, gq);
    }
    if (!term) {
        // input residuals: acc on a[6..17], f_reg on f
        float rr[32];
        rr[30] = rr[31] = 0.0f;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            float g = 0.0f;
            if (i >= 6 && i < 18) {
                const float w = a.W[RY_ACC + i - 6], e = u[i] - yr[RY_ACC + i - 6];
                g = w * e; cost += 0.5f * w * e * e;
            } else if (i >= WF) {
                const float w = a.W[RY_FREG + i - WF], e = u[i] - yr[RY_FREG + i - WF];
                g = w * e; cost += 0.5f * w * e * e;
            }
            rr[i] = g;
        }
        put_rec(R_R, rr);
        // dynamics defect
        const float* xn_g = static_cast<const float*>(__builtin_assume_aligned(Xg + (size_t)shifted_node(k + 1, a.shift, N) * NX, 8));
        float xn[NX], dd[48];
#pragma unroll
        for (int i = 36; i < 48; ++i) dd[i] = 0.0f;
#pragma unroll
        for (int i = 0; i < NX; i += 2) { const f32x2 v = *reinterpret_cast<const f32x2*>(xn_g + i); xn[i] = v[0]; xn[i + 1] = v[1]; }
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const float vn = x[WV + i] + dt * u[WA + i];
            dd[WV + i] = vn - xn[WV + i];
            dd[WQ + i] = x[WQ + i] + dt * vn - xn[WQ + i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#if WB_ART
            dd[pos_of(WH + i)] = x[WH + i] + dt * (F[i] + (i == 2 ? m.m_tree * mp.gz : 0.0f)) - xn[WH + i];
#else
            dd[pos_of(WH + i)] = x[WH + i] + dt * (F[i] + (i == 2 ? mp.mass * mp.gz : 0.0f)) - xn[WH + i];
#endif
            dd[pos_of(WH + 3 + i)] = x[WH + 3 + i] + dt * tau_acc[i] - xn[WH + 3 + i];
        }
        put_rec(R_D, dd);
        {
            float hq16[48];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 16; ++j) hq16[i * 16 + j] = j < 15 ? hq[i][j < 15 ? j : 0] : 0.0f;
            put_rec(R_HQ, hq16);
        }
        put_rec(R_HF, hfr);
        put_rec(R_CDT, cdt);
        // friction pyramid
        float fv[12], g[NG];
#pragma unroll
        for (int i = 0; i < 12; ++i) fv[i] = u[WF + i];
        gdot(mp, fv, g);
        put_rec(R_C, g);       // h = 0
        static_assert(R_ACT % 4 == 0 && R_COST == R_ACT + 1 && R_ZERO == R_ACT + 2 && R_DT == R_ACT + 3 && R_DT2 % 4 == 0, "tail of the record");
        const unsigned act = (a.n_ipm > 0) ? active_mask(p) : 0u;
        *reinterpret_cast<f32x4*>(rec + R_ACT) = f32x4{__uint_as_float(act), cost, 0.0f, dt};
        rec[R_DT2] = dt * dt;
    } else {
        rec[R_COST] = cost;
    }
}

}  // namespace wb
}  // namespace nmpc
