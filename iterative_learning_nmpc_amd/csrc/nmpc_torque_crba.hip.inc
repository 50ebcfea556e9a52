// nmpc_torque_crba.hip.inc -- the tree's inertia (nmpc_mass_matrix_batch, nmpc_centroidal_batch of include/nmpc_torque.h);
// included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_fd.hip.inc, whose conventions it keeps: body
// coordinates, x_parent = R x_child + p, force vectors (moment about the body origin; force), a symmetric 6x6 as A 6, B 9, C 6.
//
// The composite-rigid-body algorithm (Featherstone, RBDA table 6.2) for 1-DoF joints.  I^c_i is the inertia of the subtree of
// body i, frozen at q, about the origin of frame i; column i of M is the force F = I^c_i S_i that accelerates that subtree along
// joint i, read at every joint j on the path to the root: M[i][j] = M[j][i] = S_j^T F, F carried into frame j.  The same F in
// world axes about the tree's centre of mass is column i of the centroidal momentum map A_g(q), h = A_g v (Orin & Goswami).
// Nothing is inverted: massless bodies add nothing, a non-finite q stays in its robot's row.
// One thread per robot, CR_W robots per block, per-body state in an LDS slice [joint][CR_SLOTS][CR_W].  Joint transforms are
// recomputed where a pass needs them, as in the forward dynamics.
#pragma once

constexpr int CR_Q = 0;      // q_i
constexpr int CR_RW = 1;     // Rw 9: world rotation of frame i
constexpr int CR_PW = 10;    // pw 3: world position of the origin of frame i
constexpr int CR_I = 13;     // I^c 21: A 6, B 9, C 6
constexpr int CR_SLOTS = 34;

constexpr size_t crba_lds_bytes(int n, int width) { return (size_t)n * CR_SLOTS * width * sizeof(float); }
// robots per block by the rule of fd_block_width: the slice of the largest tree fits the CU at 32 (139 264 B), so there is one width
constexpr int CR_W = crba_lds_bytes(MAXJ, 32) <= FD_LDS_MAX ? 32 : 16;
static_assert(CR_W == 32, "the composite-inertia slice of the largest tree no longer fits a CU at 32 robots per block");

struct CrbaArgs {
    int B;
    const float *q, *v;                                   // v: only for h
    float *M, *com, *h, *Ag;                              // each may be nullptr
};

__global__ __launch_bounds__(CR_W) void crba_kernel(const Model* __restrict__ mp, const CrbaArgs p) {
    const Model& m = *mp;
    const int b = blockIdx.x * CR_W + threadIdx.x;
    if (b >= p.B) return;
    const int n = m.n;
    const Slice<CR_SLOTS, CR_W> at;
    const float* qb = p.q + (size_t)b * n;

    // outward: world pose of every frame, the body's own inertia about its origin, the first moment of the tree
    V3 first{0, 0, 0};
    float total = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float qi = qb[i];
        at(i, CR_Q) = qi;
        M3 R; V3 pl;
        joint_transform(m, i, qi, R, pl);
        const int par = m.parent[i];
        M3 Rw = R;
        V3 pw = pl;
        if (par >= 0) {
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, CR_RW + k);
            Rw = mul(Rp, R);
            pw = at.get3(par, CR_PW) + mul(Rp, pl);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, CR_RW + k) = Rw.m[k];
        at.put3(i, CR_PW, pw);
        // spatial inertia about the body origin: A = Ic - m [c]x [c]x, B = m [c]x, C = m 1
        const float mass = m.mass[i];
        const V3 c = v3(m.com[i]);
        const float* I = m.inertia[i];
        const float cc = dot(c, c);
        at(i, CR_I + 0) = I[0] + mass * (cc - c.x * c.x); at(i, CR_I + 1) = I[1] - mass * c.x * c.y; at(i, CR_I + 2) = I[2] - mass * c.x * c.z;
        at(i, CR_I + 3) = I[3] + mass * (cc - c.y * c.y); at(i, CR_I + 4) = I[4] - mass * c.y * c.z; at(i, CR_I + 5) = I[5] + mass * (cc - c.z * c.z);
        const M3 Bm = skew(mass * c);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, CR_I + 6 + k) = Bm.m[k];
        at(i, CR_I + 15) = mass; at(i, CR_I + 16) = 0.0f; at(i, CR_I + 17) = 0.0f; at(i, CR_I + 18) = mass; at(i, CR_I + 19) = 0.0f; at(i, CR_I + 20) = mass;
        first = first + mass * (pw + mul(Rw, c));
        total += mass;
    }
    const V3 com{first.x / total, first.y / total, first.z / total};      // the host refuses a centroidal call on a massless tree
    if (p.com) { float* cb = p.com + (size_t)b * 3; cb[0] = com.x; cb[1] = com.y; cb[2] = com.z; }
    if (!p.M && !p.h && !p.Ag) return;

    // inward: I^c of a body goes to its parent, to the parent's frame: R (.) R^T, then shifted by p:
    //   C' = C, B' = B + P C, A' = A - B P + P B'^T    (P = [p]x)
    for (int i = n - 1; i >= 0; --i) {
        const int par = m.parent[i];
        if (par < 0) continue;
        S6 A, C; M3 Bm;
#pragma unroll
        for (int k = 0; k < 6; ++k) A.m[k] = at(i, CR_I + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bm.m[k] = at(i, CR_I + 6 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) C.m[k] = at(i, CR_I + 15 + k);
        M3 R; V3 pl;
        joint_transform(m, i, at(i, CR_Q), R, pl);
        const M3 Ar = rotated(R, full(A)), Br = rotated(R, Bm), Cr = rotated(R, full(C)), P = skew(pl);
        M3 Bp = mul(P, Cr);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bp.m[k] += Br.m[k];
        const M3 BP = mul(Br, P), PBt = mul(P, transposed(Bp));
        M3 Ap;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ap.m[k] = Ar.m[k] - BP.m[k] + PBt.m[k];
        const S6 Au = upper(Ap), Cu = upper(Cr);
#pragma unroll
        for (int k = 0; k < 6; ++k) at(par, CR_I + k) += Au.m[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) at(par, CR_I + 6 + k) += Bp.m[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) at(par, CR_I + 15 + k) += Cu.m[k];
    }

    // columns: F = I^c_i S_i, in world axes about the centre of mass for A_g and h, up the path to the root for M
    const float* vb = p.h ? p.v + (size_t)b * n : nullptr;
    float* Mb = p.M ? p.M + (size_t)b * n * n : nullptr;
    float* Ab = p.Ag ? p.Ag + (size_t)b * 6 * n : nullptr;
    V3 h_l{0, 0, 0}, h_n{0, 0, 0};
    for (int i = 0; i < n; ++i) {
        S6 A, C; M3 Bm;
#pragma unroll
        for (int k = 0; k < 6; ++k) A.m[k] = at(i, CR_I + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bm.m[k] = at(i, CR_I + 6 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) C.m[k] = at(i, CR_I + 15 + k);
        const V3 ax = v3(m.axis[i]);
        const bool rev = m.type[i] == 0;
        V3 F_n = rev ? mul(A, ax) : mul(Bm, ax), F_l = rev ? mul_t(Bm, ax) : mul(C, ax);
        if (Ab || vb) {
            M3 Rw;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rw.m[k] = at(i, CR_RW + k);
            const V3 l_w = mul(Rw, F_l), n_w = mul(Rw, F_n) + cross(at.get3(i, CR_PW) - com, l_w);
            if (Ab) {
                Ab[i] = l_w.x; Ab[n + i] = l_w.y; Ab[2 * n + i] = l_w.z;
                Ab[3 * n + i] = n_w.x; Ab[4 * n + i] = n_w.y; Ab[5 * n + i] = n_w.z;
            }
            if (vb) {
                const float vi = vb[i];
                h_l = h_l + vi * l_w; h_n = h_n + vi * n_w;
            }
        }
        if (!Mb) continue;
        Mb[(size_t)i * n + i] = dot(ax, rev ? F_n : F_l);
        // row i below the diagonal and column i above it, each entry once: parents come before their children, so the ancestors
        // of i are met in falling order; F is in the frame of `frame`, the last of them it has reached
        int frame = i, anc = m.parent[i];
        for (int j = i - 1; j >= 0; --j) {
            float e = 0.0f;
            if (j == anc) {
                M3 R; V3 pl;
                joint_transform(m, frame, at(frame, CR_Q), R, pl);
                F_l = mul(R, F_l);
                F_n = mul(R, F_n) + cross(pl, F_l);
                e = dot(v3(m.axis[j]), m.type[j] == 0 ? F_n : F_l);
                frame = j; anc = m.parent[j];
            }
            Mb[(size_t)i * n + j] = e;
            Mb[(size_t)j * n + i] = e;
        }
    }
    if (p.h) {
        float* hb = p.h + (size_t)b * 6;
        hb[0] = h_l.x; hb[1] = h_l.y; hb[2] = h_l.z; hb[3] = h_n.x; hb[4] = h_n.y; hb[5] = h_n.z;
    }
}
