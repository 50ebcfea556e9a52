// nmpc_torque_momentum.hip.inc -- the momentum pass on the nodes of a whole-body solve (nmpc_wb_set_momentum_model of
// include/nmpc.h, articulated mode); included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_cmd.hip.inc, whose
// passes it runs: one thread per (problem, node), MM_W of them per block, per-body state in an LDS slice [joint][CD_SLOTS][MM_W].
//
// For node k of problem b the kernel reads q and v from the solver's iterate X[b][.][42] -- through the warm-start index map of
// the linearisation (nmpc::wb::shifted_node), so that both see the same node -- and writes the node's momentum record
// (nmpc_wb_momentum.hpp): A_g, dh_dq = d(A_g v)/dq, A_g v and the centre of mass from the origin of the base frame.
// The recursion is cmd_kernel's: world-axes spatial vectors about the origin O of the first frame that carries mass, frame
// origins accumulated from there, so that the base position does not enter the arithmetic; the columns of A_g come out of the
// same inward pass as the derivatives, column j = I^c_j S_j about O moved to the centre of mass:
//     lin = m_j s_v - k_j x s_w,    ang_G = A_j s_w + k_j x s_v - com x lin,
// and A_g v = (sum of the bodies' momenta) about the centre of mass.  Nothing is inverted but the total mass, which the host
// has checked.
#pragma once

constexpr int MM_W = CD_W;
static_assert(MM_W == 32, "the momentum pass runs 32 nodes per block on cmd_kernel's slice");

struct MomentumArgs {
    int B, N, shift, anchor;                              // anchor, chain: as CmdArgs
    unsigned chain;
    const float* X;                                       // [B][N+1][42]: q at 0, v at 18
    float* rec;                                           // [B][N+1][MR_FLOATS]
    const int* skip;                                      // nullptr, or [B] flag words: a problem with skip[b] & skip_mask != 0 is left out
    int skip_mask;
    const int* done;                                      // nullptr, or the finished flag of problem 0: a problem whose flag is set is left out
    size_t done_stride;                                   // words from one problem's flag to the next
};

__global__ __launch_bounds__(MM_W) void wb_momentum_kernel(const Model* __restrict__ mp, const MomentumArgs p) {
    using namespace nmpc::wb;
    const Model& m = *mp;
    const long long t = (long long)blockIdx.x * MM_W + threadIdx.x;
    if (t >= (long long)p.B * (p.N + 1)) return;
    const int b = (int)(t / (p.N + 1)), node = (int)(t - (long long)b * (p.N + 1));
    if (p.skip && (p.skip[b] & p.skip_mask) != 0) return;
    if (p.done && p.done[(size_t)b * p.done_stride]) return;
    const int n = m.n;                                    // 18: the host has checked
    const Slice<CD_SLOTS, MM_W> at;
    const float* qb = p.X + ((size_t)b * (p.N + 1) + shifted_node(node, p.shift, p.N)) * NX + WQ;
    const float* vb = qb + (WV - WQ);
    float* rec = p.rec + (size_t)t * MR_FLOATS;
    auto rotation = [&](int i) {
        M3 R;
#pragma unroll
        for (int k = 0; k < 9; ++k) R.m[k] = at(i, CD_RW + k);
        return R;
    };

    // world rotation of every frame; its offset in the parent frame waits in the slots of d
    for (int i = 0; i < n; ++i) {
        M3 R; V3 pl;
        joint_transform(m, i, qb[i], R, pl);
        const int par = m.parent[i];
        const M3 Rw = par >= 0 ? mul(rotation(par), R) : R;
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, CD_RW + k) = Rw.m[k];
        at.put3(i, CD_D, pl);
    }
    // O is the origin of the anchor's frame: d = 0 there, and back along its path to the root
    V3 O;
    {
        V3 d{0, 0, 0};
        for (int k = p.anchor;;) {
            const V3 pl = at.get3(k, CD_D);
            at.put3(k, CD_D, d);
            const int par = m.parent[k];
            if (par < 0) { O = pl - d; break; }
            d = d - mul(rotation(par), pl);
            k = par;
        }
    }

    // outward: the other frame origins, velocities, every body's own inertia and momentum about O, the totals of the tree
    V3 first{0, 0, 0}, l_all{0, 0, 0}, n_all{0, 0, 0};
    float total = 0.0f;
    for (int i = 0; i < n; ++i) {
        const int par = m.parent[i];
        const M3 Rw = rotation(i);
        V3 d = at.get3(i, CD_D), w{0, 0, 0}, u{0, 0, 0};
        if (!((p.chain >> i) & 1u)) {
            d = par >= 0 ? at.get3(par, CD_D) + mul(rotation(par), d) : d - O;
            at.put3(i, CD_D, d);
        }
        if (par >= 0) { w = at.get3(par, CD_V); u = at.get3(par, CD_V + 3); }
        const V3 z = mul(Rw, v3(m.axis[i]));
        const float vi = vb[i];
        if (m.type[i] == 0) {          // S = (z; d x z)
            w = w + vi * z;
            u = u + vi * cross(d, z);
        } else {                       // S = (0; z)
            u = u + vi * z;
        }
        at.put3(i, CD_V, w); at.put3(i, CD_V + 3, u);
        // about O: A = R Ic R^T + m (c.c 1 - c c^T), k = m c; momentum l = m (u + w x c), moment = R Ic R^T w + c x l
        const float mass = m.mass[i];
        const V3 c = d + mul(Rw, v3(m.com[i]));
        const float* I = m.inertia[i];
        const S6 Ib = upper(rotated(Rw, full(S6{{I[0], I[1], I[2], I[3], I[4], I[5]}})));
        const float cc = dot(c, c);
        at(i, CD_A + 0) = Ib.m[0] + mass * (cc - c.x * c.x); at(i, CD_A + 1) = Ib.m[1] - mass * c.x * c.y; at(i, CD_A + 2) = Ib.m[2] - mass * c.x * c.z;
        at(i, CD_A + 3) = Ib.m[3] + mass * (cc - c.y * c.y); at(i, CD_A + 4) = Ib.m[4] - mass * c.y * c.z; at(i, CD_A + 5) = Ib.m[5] + mass * (cc - c.z * c.z);
        const V3 k = mass * c, l = mass * (u + cross(w, c));
        const V3 mom = mul(Ib, w) + cross(c, l);
        at.put3(i, CD_K, k);
        at(i, CD_M) = mass;
        at.put3(i, CD_H, mom);
        at.put3(i, CD_H + 3, l);
        first = first + k; l_all = l_all + l; n_all = n_all + mom; total += mass;
    }
    const V3 com{first.x / total, first.y / total, first.z / total};      // from O; the host refuses a massless tree
    {
        const V3 k_g = n_all - cross(com, l_all);
        rec[MR_AGV + 0] = l_all.x; rec[MR_AGV + 1] = l_all.y; rec[MR_AGV + 2] = l_all.z;
        rec[MR_AGV + 3] = k_g.x; rec[MR_AGV + 4] = k_g.y; rec[MR_AGV + 5] = k_g.z;
        rec[MR_COM + 0] = com.x; rec[MR_COM + 1] = com.y; rec[MR_COM + 2] = com.z;
    }

    // inward: about one point in one set of axes, I^c and h^c of a subtree are sums
    for (int i = n - 1; i >= 0; --i) {
        const int par = m.parent[i];
        if (par < 0) continue;
#pragma unroll
        for (int k = CD_A; k < CD_SLOTS; ++k) at(par, k) += at(i, k);
    }

    // columns of A_g and of dh_dq
    float* Ab = rec + MR_AG;
    float* Db = rec + MR_DH;
    for (int j = 0; j < n; ++j) {
        const int par = m.parent[j];
        const V3 z = mul(rotation(j), v3(m.axis[j]));
        const bool rev = m.type[j] == 0;
        const V3 zero{0, 0, 0};
        const V3 sw = rev ? z : zero, sv = rev ? cross(at.get3(j, CD_D), z) : z;
        V3 wp = zero, up = zero;
        if (par >= 0) { wp = at.get3(par, CD_V); up = at.get3(par, CD_V + 3); }
        const V3 al = cross(sw, wp), be = cross(sw, up) + cross(sv, wp);      // S_j x v_p
        S6 A;
#pragma unroll
        for (int k = 0; k < 6; ++k) A.m[k] = at(j, CD_A + k);
        const V3 k = at.get3(j, CD_K), hn = at.get3(j, CD_H), hl = at.get3(j, CD_H + 3);
        const float mj = at(j, CD_M);
        const V3 dn = cross(sw, hn) + cross(sv, hl) - (mul(A, al) + cross(k, be));
        const V3 dl = cross(sw, hl) - (mj * be - cross(k, al));
        const V3 lin = mj * sv - cross(k, sw);                                // I^c_j S_j: the linear part ...
        const V3 ang = mul(A, sw) + cross(k, sv) - cross(com, lin);           // ... and the moment, about the centre of mass
        const V3 dc{lin.x / total, lin.y / total, lin.z / total};
        const V3 dk = dn - cross(dc, l_all) - cross(com, dl);
        Ab[j] = lin.x; Ab[n + j] = lin.y; Ab[2 * n + j] = lin.z;
        Ab[3 * n + j] = ang.x; Ab[4 * n + j] = ang.y; Ab[5 * n + j] = ang.z;
        Db[j] = dl.x; Db[n + j] = dl.y; Db[2 * n + j] = dl.z;
        Db[3 * n + j] = dk.x; Db[4 * n + j] = dk.y; Db[5 * n + j] = dk.z;
    }
}
