// nmpc_torque_centroidal.hip.inc -- the centroidal momentum of the articulated tree about an anchor point at the robot: one kernel
// text, centroidal_kernel<Io>, with three entry points that differ only in the policy Io (at the end of this file):
//     CmdIo            nmpc_centroidal_derivatives_batch of include/nmpc_torque.h: dh_dq = d(A_g v)/dq, d com/dq, hdot_bias;
//     NodeRecordIo     nmpc_torque::momentum_records, the momentum pass on the nodes of a whole-body solve in the articulated mode
//                      (nmpc_wb_set_momentum_model of include/nmpc.h): A_g, dh_dq, A_g v and the centre of mass of every node;
//     StateMomentumIo  nmpc_state_momentum_batch: A_g(q) v of a plant state alone, which the device rollouts put into x0.
// Included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_crba.hip.inc, whose family it belongs to: one thread
// per row (robot, node or state), CD_W rows per block, per-body state in an LDS slice [joint][cd_slots<Io>][CD_W].
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
// The centroidal quantities follow from the totals and from the columns about O, column j of A_g being I^c_j S_j moved to the
// centre of mass:
//     A_g v = [l; n_O - com x l],     lin = m_j s_v - k_j x s_w,     ang_G = A_j s_w + k_j x s_v - com x lin,
//     d com / d q_j = lin / m,        d k_G / d q_j = d k_O / d q_j - d com / d q_j x l - (com - O) x d l / d q_j,
//     hdot_bias = sum_j dh_dq[:, j] v_j   in joint order  (q_dot = v for this state).
// Nothing is inverted but the total mass, which the host has checked: massless bodies add nothing, a q or v that is not finite stays
// in its own row, a row that is left out touches no memory.  Whatever a policy has is always computed and only the stores depend
// on what was asked for, so an output's bits do not depend on its neighbours.
//
// A policy says whether a thread is left out (left_out) and where its q and v are (state), what becomes of the totals (totals),
// and what of each column (columns before the first: where they go; column; bias after the last).  left_out only tests and state
// only computes addresses: a test that also located the row, or a column store that computed its own address, was compiled to other
// code than the kernels this text replaced (DESIGN.md 8d).  Its traits say what is compiled for it: COLUMNS -- the composite quantities in the
// slice (34 slots against the 18 that a child reads of its parent: rotation, origin, velocity), the inward pass and the columns --,
// MOMENT -- the moment of the tree about O --, MAP -- the angular rows of A_g --, BIAS -- the sum over the columns.  The body is one
// text on purpose and not three kernels around shared inline passes: a pass behind a call is laid out differently by the compiler
// than the same loop in the kernel, and the fused products change with it.
#pragma once

constexpr int CD_RW = 0;     // Rw 9: world rotation of frame i
constexpr int CD_D = 9;      // d 3: origin of frame i from O, world axes (until the outward pass: its offset in the parent frame)
constexpr int CD_V = 12;     // w 3, u 3: velocity of body i
constexpr int CD_KIN = 18;   // so far: what a child reads of its parent, the whole slice of a policy without columns
constexpr int CD_A = 18;     // I^c: A 6, k 3, m 1
constexpr int CD_K = 24;
constexpr int CD_M = 27;
constexpr int CD_H = 28;     // h^c: moment about O 3, linear 3
constexpr int CD_SLOTS = 34;

constexpr size_t cd_lds_bytes(int slots, int n, int width) { return (size_t)n * slots * width * sizeof(float); }
// rows per block by the rule of fd_block_width: the widest slice of the largest tree fits the CU at 32 (139 264 B), so there is one width
constexpr int CD_W = cd_lds_bytes(CD_SLOTS, MAXJ, 32) <= FD_LDS_MAX ? 32 : 16;
static_assert(CD_W == 32, "the centroidal slice of the largest tree no longer fits a CU at 32 rows per block");
static_assert(MAXJ <= 32, "the chain mask has one bit per joint");

struct CmdArgs {
    int B, anchor;                                        // anchor: the first joint whose body has mass
    unsigned chain;                                       // bit i: joint i is the anchor or one of its ancestors
    const float *q, *v;
    float *dh, *dcom, *bias;                              // each may be nullptr
};

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

struct StateMomentumArgs {
    int B, anchor;                                        // anchor, chain: as CmdArgs
    unsigned chain;
    int qv_stride, h_stride, h2_stride, skip_mask;        // floats from one state's q, v / h / h2 to the next
    const float *q, *v;
    float *h, *h2;                                        // h2 may be nullptr
    const int* skip;                                      // nullptr, or [B] flag words: a state with skip[b] & skip_mask != 0 is left out
};

// the slots of a policy's slice, and the bytes of it for a tree of n joints
template <class Io> constexpr int cd_slots = Io::COLUMNS ? CD_SLOTS : CD_KIN;
template <class Io> constexpr size_t centroidal_lds_bytes(int n) { return cd_lds_bytes(cd_slots<Io>, n, CD_W); }

template <class Io>
__global__ __launch_bounds__(CD_W) void centroidal_kernel(const Model* __restrict__ mp, const typename Io::Args p) {
    const Model& m = *mp;
    Io io;
    if (io.left_out(p)) return;
    const int n = m.n;
    const float *qb, *vb;
    io.state(p, n, qb, vb);
    const Slice<cd_slots<Io>, CD_W> at;
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
        if constexpr (Io::COLUMNS) {   // a policy without columns keeps a body's inertia and momentum in registers for its own iteration
            const float cc = dot(c, c);
            at(i, CD_A + 0) = Ib.m[0] + mass * (cc - c.x * c.x); at(i, CD_A + 1) = Ib.m[1] - mass * c.x * c.y; at(i, CD_A + 2) = Ib.m[2] - mass * c.x * c.z;
            at(i, CD_A + 3) = Ib.m[3] + mass * (cc - c.y * c.y); at(i, CD_A + 4) = Ib.m[4] - mass * c.y * c.z; at(i, CD_A + 5) = Ib.m[5] + mass * (cc - c.z * c.z);
        }
        const V3 k = mass * c, l = mass * (u + cross(w, c));
        const V3 mom = mul(Ib, w) + cross(c, l);
        if constexpr (Io::COLUMNS) {
            at.put3(i, CD_K, k);
            at(i, CD_M) = mass;
            at.put3(i, CD_H, mom);
            at.put3(i, CD_H + 3, l);
        }
        first = first + k; l_all = l_all + l; total += mass;
        if constexpr (Io::MOMENT) n_all = n_all + mom;
    }
    const V3 com{first.x / total, first.y / total, first.z / total};      // from O; the host refuses a massless tree
    if constexpr (Io::MOMENT) io.totals(p, l_all, n_all - cross(com, l_all), com);

    if constexpr (Io::COLUMNS) {
        // inward: about one point in one set of axes, I^c and h^c of a subtree are sums
        for (int i = n - 1; i >= 0; --i) {
            const int par = m.parent[i];
            if (par < 0) continue;
#pragma unroll
            for (int k = CD_A; k < CD_SLOTS; ++k) at(par, k) += at(i, k);
        }

        // columns of A_g and of dh_dq
        io.columns(p, n);
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
            const V3 lin = mj * sv - cross(k, sw);                                // I^c_j S_j: the linear part ...
            V3 ang = zero;
            if constexpr (Io::MAP) ang = mul(A, sw) + cross(k, sv) - cross(com, lin);      // ... and the moment, about the centre of mass
            const V3 dc{lin.x / total, lin.y / total, lin.z / total};
            const V3 dk = dn - cross(dc, l_all) - cross(com, dl);
            io.column(n, j, lin, ang, dl, dk, dc);
            if constexpr (Io::BIAS) {
                const float vj = vb[j];
                b_l = b_l + vj * dl; b_n = b_n + vj * dk;
            }
        }
        if constexpr (Io::BIAS) io.bias(p, b_l, b_n);
    }
}

// six floats in the slot order of h: linear, then angular
__device__ __forceinline__ void put6(float* o, V3 l, V3 a) { o[0] = l.x; o[1] = l.y; o[2] = l.z; o[3] = a.x; o[4] = a.y; o[5] = a.z; }
// column j of a [6][n] map: three linear rows, then three angular ones
__device__ __forceinline__ void put_column(float* o, int n, int j, V3 l, V3 a) {
    o[j] = l.x; o[n + j] = l.y; o[2 * n + j] = l.z;
    o[3 * n + j] = a.x; o[4 * n + j] = a.y; o[5 * n + j] = a.z;
}

// the derivatives of a batch of robots: dense q, v; each output may be missing
struct CmdIo {
    using Args = CmdArgs;
    static constexpr bool COLUMNS = true, MOMENT = false, MAP = false, BIAS = true;
    int b;
    float *Db, *Cb;
    __device__ __forceinline__ bool left_out(const Args& p) {
        b = blockIdx.x * CD_W + threadIdx.x;
        return b >= p.B;
    }
    __device__ __forceinline__ void state(const Args& p, int n, const float*& q, const float*& v) const {
        q = p.q + (size_t)b * n;
        v = p.v + (size_t)b * n;
    }
    __device__ __forceinline__ void columns(const Args& p, int n) {
        Db = p.dh ? p.dh + (size_t)b * 6 * n : nullptr;
        Cb = p.dcom ? p.dcom + (size_t)b * 3 * n : nullptr;
    }
    __device__ __forceinline__ void column(int n, int j, V3, V3, V3 dl, V3 dk, V3 dc) const {
        if (Db) put_column(Db, n, j, dl, dk);
        if (Cb) { Cb[j] = dc.x; Cb[n + j] = dc.y; Cb[2 * n + j] = dc.z; }
    }
    __device__ __forceinline__ void bias(const Args& p, V3 b_l, V3 b_n) const {
        if (p.bias) put6(p.bias + (size_t)b * 6, b_l, b_n);
    }
};

// node k of problem b of a whole-body solve: q and v from the solver's iterate X[b][.][42] -- through the warm-start index map of the
// linearisation (nmpc::wb::shifted_node), so that both see the same node --, the node's momentum record (nmpc_wb_momentum.hpp) out;
// n is 18: the host has checked
struct NodeRecordIo {
    using Args = MomentumArgs;
    static constexpr bool COLUMNS = true, MOMENT = true, MAP = true, BIAS = false;
    long long t;
    int b;
    float *rec, *Ab, *Db;
    __device__ __forceinline__ bool left_out(const Args& p) {
        t = (long long)blockIdx.x * CD_W + threadIdx.x;
        if (t >= (long long)p.B * (p.N + 1)) return true;
        b = (int)(t / (p.N + 1));
        if (p.skip && (p.skip[b] & p.skip_mask) != 0) return true;
        if (p.done && p.done[(size_t)b * p.done_stride]) return true;
        return false;
    }
    __device__ __forceinline__ void state(const Args& p, int, const float*& q, const float*& v) {
        using namespace nmpc::wb;
        const int node = (int)(t - (long long)b * (p.N + 1));
        q = p.X + ((size_t)b * (p.N + 1) + shifted_node(node, p.shift, p.N)) * NX + WQ;
        v = q + (WV - WQ);
        rec = p.rec + (size_t)t * MR_FLOATS;
    }
    __device__ __forceinline__ void totals(const Args&, V3 l, V3 k_g, V3 com) const {
        using namespace nmpc::wb;
        put6(rec + MR_AGV, l, k_g);
        rec[MR_COM + 0] = com.x; rec[MR_COM + 1] = com.y; rec[MR_COM + 2] = com.z;
    }
    __device__ __forceinline__ void columns(const Args&, int) {
        using namespace nmpc::wb;
        Ab = rec + MR_AG;
        Db = rec + MR_DH;
    }
    __device__ __forceinline__ void column(int n, int j, V3 lin, V3 ang, V3 dl, V3 dk, V3) const {
        put_column(Ab, n, j, lin, ang);
        put_column(Db, n, j, dl, dk);
    }
};

// a plant state in strided rows: h = A_g(q) v, and a second copy where one is asked for
struct StateMomentumIo {
    using Args = StateMomentumArgs;
    static constexpr bool COLUMNS = false, MOMENT = true, MAP = false, BIAS = false;
    int b;
    __device__ __forceinline__ bool left_out(const Args& p) {
        b = blockIdx.x * CD_W + threadIdx.x;
        if (b >= p.B) return true;
        if (p.skip && (p.skip[b] & p.skip_mask) != 0) return true;
        return false;
    }
    __device__ __forceinline__ void state(const Args& p, int, const float*& q, const float*& v) const {
        q = p.q + (size_t)b * p.qv_stride;
        v = p.v + (size_t)b * p.qv_stride;
    }
    __device__ __forceinline__ void totals(const Args& p, V3 l, V3 k_g, V3) const {
        put6(p.h + (size_t)b * p.h_stride, l, k_g);
        if (p.h2) put6(p.h2 + (size_t)b * p.h2_stride, l, k_g);
    }
};
