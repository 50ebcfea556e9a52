// nmpc_torque_cmd.hip.inc -- the derivatives of the tree's centroidal momentum (nmpc_centroidal_derivatives_batch of
// include/nmpc_torque.h); included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_crba.hip.inc, whose family it
// belongs to: one thread per robot, CD_W robots per block, per-body state in an LDS slice [joint][CD_SLOTS][CD_W].
//
// h = A_g(q) v is the momentum of all bodies; at fixed v, for a tree of 1-DoF joints and a fixed reference point O,
//     d h_O / d q_j = S_j x* h^c_j  -  I^c_j (S_j x v_p(j))
// with S_j the motion axis of joint j, h^c_j and I^c_j the momentum and the inertia of the subtree of body j, v_p(j) the velocity of
// the parent body (zero for a root), x the motion and x* the force cross product: a displacement along joint j carries the
// subtree's momentum with it, except for the part of its velocity that comes from the ancestors, which does not turn.
// Everything here is a world-axes spatial vector about one point O: motion vectors (w; u), u the velocity of the body-fixed point
// at O, force vectors (moment about O; force).  About one point in one set of axes the inertia of a subtree is a plain sum and
// keeps the form of a rigid body's -- A 6 (rotational, about O), k 3 (the first moment: B = [k]x), m 1 (C = m 1) -- so the inward
// pass is sixteen additions per body and needs no transform.  O is the origin of the first frame that carries mass (`anchor`; the
// trunk of the quadruped), and the frame origins are accumulated from there -- back along the anchor's path to the root (`chain`),
// outward everywhere else -- never from the world origin: d, u, k, A and both momenta stay at the size of the robot whatever the
// base position, and the base coordinates of a floating base do not enter at all.
// The centroidal quantities follow from the columns about O:
//     d com / d q_j = lin(I^c_j S_j) / m,     d k_G / d q_j = d k_O / d q_j - d com / d q_j x l - (com - O) x d l / d q_j,
//     hdot_bias = sum_j dh_dq[:, j] v_j   in joint order  (q_dot = v for this state).
// Nothing is inverted: massless bodies add nothing, a q or v that is not finite stays in its robot's row.  All outputs are always
// computed and only the stores depend on what was asked for, so an output's bits do not depend on its neighbours.
#pragma once

constexpr int CD_RW = 0;     // Rw 9: world rotation of frame i
constexpr int CD_D = 9;      // d 3: origin of frame i from O, world axes (until the outward pass: its offset in the parent frame)
constexpr int CD_V = 12;     // w 3, u 3: velocity of body i
constexpr int CD_A = 18;     // I^c: A 6, k 3, m 1
constexpr int CD_K = 24;
constexpr int CD_M = 27;
constexpr int CD_H = 28;     // h^c: moment about O 3, linear 3
constexpr int CD_SLOTS = 34;

constexpr size_t cmd_lds_bytes(int n, int width) { return (size_t)n * CD_SLOTS * width * sizeof(float); }
// robots per block by the rule of fd_block_width: the slice of the largest tree fits the CU at 32 (139 264 B), so there is one width
constexpr int CD_W = cmd_lds_bytes(MAXJ, 32) <= FD_LDS_MAX ? 32 : 16;
static_assert(CD_W == 32, "the momentum-derivative slice of the largest tree no longer fits a CU at 32 robots per block");
static_assert(MAXJ <= 32, "CmdArgs::chain has one bit per joint");

struct CmdArgs {
    int B, anchor;                                        // anchor: the first joint whose body has mass
    unsigned chain;                                       // bit i: joint i is the anchor or one of its ancestors
    const float *q, *v;
    float *dh, *dcom, *bias;                              // each may be nullptr
};

__global__ __launch_bounds__(CD_W) void cmd_kernel(const Model* __restrict__ mp, const CmdArgs p) {
    const Model& m = *mp;
    const int b = blockIdx.x * CD_W + threadIdx.x;
    if (b >= p.B) return;
    const int n = m.n;
    const Slice<CD_SLOTS, CD_W> at;
    const float* qb = p.q + (size_t)b * n;
    const float* vb = p.v + (size_t)b * n;
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
    // O is the origin of the anchor's frame: d = 0 there, and back along its path to the root, where the world position of O falls out
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
    V3 first{0, 0, 0}, l_all{0, 0, 0};
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
        at.put3(i, CD_K, k);
        at(i, CD_M) = mass;
        at.put3(i, CD_H, mul(Ib, w) + cross(c, l));
        at.put3(i, CD_H + 3, l);
        first = first + k; l_all = l_all + l; total += mass;
    }
    const V3 com{first.x / total, first.y / total, first.z / total};      // from O; the host refuses a massless tree

    // inward: about one point in one set of axes, I^c and h^c of a subtree are sums
    for (int i = n - 1; i >= 0; --i) {
        const int par = m.parent[i];
        if (par < 0) continue;
#pragma unroll
        for (int k = CD_A; k < CD_SLOTS; ++k) at(par, k) += at(i, k);
    }

    // columns
    float* Db = p.dh ? p.dh + (size_t)b * 6 * n : nullptr;
    float* Cb = p.dcom ? p.dcom + (size_t)b * 3 * n : nullptr;
    V3 b_l{0, 0, 0}, b_n{0, 0, 0};
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
        const V3 lin = mj * sv - cross(k, sw);                                // the linear part of I^c_j S_j
        const V3 dc{lin.x / total, lin.y / total, lin.z / total};
        const V3 dk = dn - cross(dc, l_all) - cross(com, dl);
        if (Db) {
            Db[j] = dl.x; Db[n + j] = dl.y; Db[2 * n + j] = dl.z;
            Db[3 * n + j] = dk.x; Db[4 * n + j] = dk.y; Db[5 * n + j] = dk.z;
        }
        if (Cb) { Cb[j] = dc.x; Cb[n + j] = dc.y; Cb[2 * n + j] = dc.z; }
        const float vj = vb[j];
        b_l = b_l + vj * dl; b_n = b_n + vj * dk;
    }
    if (p.bias) {
        float* bb = p.bias + (size_t)b * 6;
        bb[0] = b_l.x; bb[1] = b_l.y; bb[2] = b_l.z; bb[3] = b_n.x; bb[4] = b_n.y; bb[5] = b_n.z;
    }
}
