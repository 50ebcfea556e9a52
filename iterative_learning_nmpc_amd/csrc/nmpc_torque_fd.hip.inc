// nmpc_torque_fd.hip.inc -- forward dynamics of the torque layer (nmpc_fd_accel_batch, nmpc_fd_step_batch of
// include/nmpc_torque.h); included by nmpc_torque.hip inside namespace nmpc_torque, after Model, V3, M3, joint_transform.
//
// a = M(q)^-1 (S^T tau - h(q, v) + sum J_foot^T f) by the articulated-body algorithm (Featherstone, RBDA table 7.1) in the
// conventions of id_torques_kernel -- body coordinates, x_parent = R x_child + p, motion vectors (w; vo), force vectors (moment
// about the body origin; force), spatial inertia about the body origin, a world-frame foot force rotated by the accumulated
// Rw, gravity as the acceleration of the world -- so that the two are inverse up to rounding.  Every joint has one degree of
// freedom: the pivot d = S^T I^A S is a scalar and nothing is inverted.  A symmetric 6x6 (I^A) is kept as
//     [ A  B ]   moment = A dw + B dvo       A, C symmetric (6 entries each: xx xy xz yy yz zz), B general (9, row-major)
//     [ B' C ]   force  = B' dw + C dvo
// One thread per robot, as the inverse dynamics: serial along the tree, robots independent.  Per-body state in an LDS slice
// [joint][FD_SLOTS][W] (W robots per block): the parent look-up is a run-time index, register arrays would go to scratch.
// Joint transforms are recomputed in every pass instead of stored (27 -> 0 slots for three sincos and 27 FMAs).
#pragma once

constexpr int FD_V = 0;      // w 3, vo 3 on the way out; the body's acceleration (dw; dvo) in the last pass
constexpr int FD_C = 6;      // c = v x (S qd): the velocity-product term
constexpr int FD_RW = 12;    // Rw 9 on the way out; from the inward pass on U 6 (moment; force), then d, u
constexpr int FD_P = 21;     // p^A 6 (moment; force)
constexpr int FD_I = 27;     // I^A 21: A 6, B 9, C 6
constexpr int FD_Q = 48;     // q_i, qd_i of the robot (the state of nmpc_fd_step_batch between substeps), the joint's force
constexpr int FD_SLOTS = 51;
constexpr size_t FD_LDS_MAX = 160 * 1024;   // of a gfx950 CU, and the most one block can be given

constexpr size_t fd_lds_bytes(int n, int width) { return (size_t)n * FD_SLOTS * width * sizeof(float); }
// robots per block: 32 where the slice of n joints fits the CU (n <= 25), 16 otherwise (32 joints: 104 448 B)
constexpr int fd_block_width(int n) { return fd_lds_bytes(n, 32) <= FD_LDS_MAX ? 32 : 16; }

struct S6 {
    float m[6];                                           // xx xy xz yy yz zz
};
__device__ __forceinline__ V3 mul(const S6& A, V3 x) {
    return {A.m[0] * x.x + A.m[1] * x.y + A.m[2] * x.z, A.m[1] * x.x + A.m[3] * x.y + A.m[4] * x.z, A.m[2] * x.x + A.m[4] * x.y + A.m[5] * x.z};
}
__device__ __forceinline__ M3 full(const S6& A) { return {{A.m[0], A.m[1], A.m[2], A.m[1], A.m[3], A.m[4], A.m[2], A.m[4], A.m[5]}}; }
__device__ __forceinline__ S6 upper(const M3& A) { return {{A.m[0], A.m[1], A.m[2], A.m[4], A.m[5], A.m[8]}}; }
__device__ __forceinline__ M3 transposed(const M3& A) { return {{A.m[0], A.m[3], A.m[6], A.m[1], A.m[4], A.m[7], A.m[2], A.m[5], A.m[8]}}; }
__device__ __forceinline__ M3 skew(V3 a) { return {{0.0f, -a.z, a.y, a.z, 0.0f, -a.x, -a.y, a.x, 0.0f}}; }
// x y^T scaled: the rank-one terms of I^a = I^A - U U^T / d
__device__ __forceinline__ void sub_outer(M3& A, V3 x, V3 y, float s) {
    const float xs[3] = {s * x.x, s * x.y, s * x.z}, ys[3] = {y.x, y.y, y.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A.m[3 * i + j] -= xs[i] * ys[j];
}
__device__ __forceinline__ void sub_outer(S6& A, V3 x, float s) {
    const V3 xs = s * x;
    A.m[0] -= xs.x * x.x; A.m[1] -= xs.x * x.y; A.m[2] -= xs.x * x.z; A.m[3] -= xs.y * x.y; A.m[4] -= xs.y * x.z; A.m[5] -= xs.z * x.z;
}
// R A R^T
__device__ __forceinline__ M3 rotated(const M3& R, const M3& A) { return mul(mul(R, A), transposed(R)); }

// Where the foot forces of the recursion come from.  `force.any()`: are there any; `force(k, p, pd)`: the world-frame force on
// foot k, whose point is at p and moves with pd in the world.  A source that reads p, pd says so with `kinematic`: the outward
// pass then also carries the world position of every body origin, in three slots past FD_SLOTS (FD_PW) that its slice must have.
constexpr int FD_PW = FD_SLOTS;
// A source may also push a body: with a member `static constexpr bool pushes = true` it has `pushed(i)`, is body i pushed in this
// evaluation, and `body()`, the world-frame force at the origin of that body's frame (no moment: a foot force with zero offset).
// The hook is read under `if constexpr`, so a source without the member compiles to what it compiled to before there was one.
template <class Force, class = void>
struct force_pushes : std::false_type {};
template <class Force>
struct force_pushes<Force, std::void_t<decltype(Force::pushes)>> : std::bool_constant<Force::pushes> {};
// A source may also load a body with a point-mass payload (nmpc_contact_set_payloads, DESIGN.md 8d): with a member
// `static constexpr bool loads = true` it has `loaded(i)`, does body i carry the payload, `load_mass()`, m_p, and `load_at()`, its
// position r in that body's frame.  Read under `if constexpr` as the push is: a source without the member compiles to what it did.
template <class Force, class = void>
struct force_loads : std::false_type {};
template <class Force>
struct force_loads<Force, std::void_t<decltype(Force::loads)>> : std::bool_constant<Force::loads> {};
// A source may also arm the joints with a reflected rotor inertia (nmpc_contact_set_actuators, DESIGN.md 8d): with a member
// `static constexpr bool arms = true` it has `armature(i)`, what the pivot of joint i gains (0 on a joint without an actuator):
// the tree whose joint-space inertia is M(q) + diag(armature).  Read under `if constexpr` as the other two.
template <class Force, class = void>
struct force_arms : std::false_type {};
template <class Force>
struct force_arms<Force, std::void_t<decltype(Force::arms)>> : std::bool_constant<Force::arms> {};

// the spatial inertia of a point mass mp at r, added to the FD_I slots of body i: A += mp (|r|^2 1 - r r^T), B += mp [r]x, C += mp 1
template <class At>
__device__ __forceinline__ void add_point_inertia(const At& at, int i, float mp, V3 r) {
    const float rr = dot(r, r);
    at(i, FD_I + 0) += mp * (rr - r.x * r.x); at(i, FD_I + 1) -= mp * r.x * r.y; at(i, FD_I + 2) -= mp * r.x * r.z;
    at(i, FD_I + 3) += mp * (rr - r.y * r.y); at(i, FD_I + 4) -= mp * r.y * r.z; at(i, FD_I + 5) += mp * (rr - r.z * r.z);
    const M3 Bm = skew(mp * r);
#pragma unroll
    for (int k = 0; k < 9; ++k) at(i, FD_I + 6 + k) += Bm.m[k];
    at(i, FD_I + 15) += mp; at(i, FD_I + 18) += mp; at(i, FD_I + 20) += mp;
}

// given forces: f (world-frame foot forces of this robot, or nullptr) is read from memory
struct GivenForces {
    const float* __restrict__ f;
    static constexpr bool kinematic = false;
    __device__ __forceinline__ bool any() const { return f; }
    __device__ __forceinline__ V3 operator()(int k, V3, V3) const { return v3(f + 3 * k); }
};

// The accelerations of the robot whose q_i, qd_i and joint forces lie in slots FD_Q .. FD_Q + 2 of its LDS slice, under the foot
// forces of `force`.  qdd_i is left in slot FD_Q + 2 of joint i.  Returns false if a pivot is not a positive finite number (a
// massless leaf body): the caller writes NaN.  W: robots per block (the slice's stride), NS: slots per joint of the slice.
template <int W, int NS, class Force>
__device__ __forceinline__ bool fd_accel_body(const Model& m, const Force& force) {
    static_assert(NS >= FD_SLOTS + (Force::kinematic ? 3 : 0), "the slice is too narrow for this force source");
    const int n = m.n;
    const Slice<NS, W> at;

    // outward: velocities, c = v x (S qd), world rotation, I^A = I, p^A = v x* (I v) - foot forces
    for (int i = 0; i < n; ++i) {
        M3 R; V3 p;
        joint_transform(m, i, at(i, FD_Q), R, p);
        const int par = m.parent[i];
        V3 w_p{0, 0, 0}, vo_p{0, 0, 0};
        M3 Rw = R;
        V3 pw = p;                     // world position of the body origin (kinematic force sources only)
        if (par >= 0) {
            w_p = at.get3(par, FD_V); vo_p = at.get3(par, FD_V + 3);
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, FD_RW + k);
            Rw = mul(Rp, R);
            if constexpr (Force::kinematic) pw = at.get3(par, FD_PW) + mul(Rp, p);
        }
        if constexpr (Force::kinematic) at.put3(i, FD_PW, pw);
        V3 w = mul_t(R, w_p), vo = mul_t(R, vo_p + cross(w_p, p));
        const V3 ax = v3(m.axis[i]);
        const float qd = at(i, FD_Q + 1);
        V3 c_w{0, 0, 0}, c_v;
        if (m.type[i] == 0) {          // S = (axis; 0)
            c_w = cross(w, qd * ax); c_v = cross(vo, qd * ax);
            w = w + qd * ax;
        } else {                       // S = (0; axis)
            c_v = cross(w, qd * ax);
            vo = vo + qd * ax;
        }
        at.put3(i, FD_V, w); at.put3(i, FD_V + 3, vo); at.put3(i, FD_C, c_w); at.put3(i, FD_C + 3, c_v);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, FD_RW + k) = Rw.m[k];
        // spatial inertia about the body origin: A = Ic - m [c]x [c]x, B = m [c]x, C = m 1
        const float mass = m.mass[i];
        const V3 c = v3(m.com[i]);
        const float* I = m.inertia[i];
        const float cc = dot(c, c);
        at(i, FD_I + 0) = I[0] + mass * (cc - c.x * c.x); at(i, FD_I + 1) = I[1] - mass * c.x * c.y; at(i, FD_I + 2) = I[2] - mass * c.x * c.z;
        at(i, FD_I + 3) = I[3] + mass * (cc - c.y * c.y); at(i, FD_I + 4) = I[4] - mass * c.y * c.z; at(i, FD_I + 5) = I[5] + mass * (cc - c.z * c.z);
        const M3 Bm = skew(mass * c);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, FD_I + 6 + k) = Bm.m[k];
        at(i, FD_I + 15) = mass; at(i, FD_I + 16) = 0.0f; at(i, FD_I + 17) = 0.0f; at(i, FD_I + 18) = mass; at(i, FD_I + 19) = 0.0f; at(i, FD_I + 20) = mass;
        // v x* (I v), as id_torques_kernel has it
        auto inertia = [&](V3 x) { return V3{I[0] * x.x + I[1] * x.y + I[2] * x.z, I[1] * x.x + I[3] * x.y + I[4] * x.z, I[2] * x.x + I[4] * x.y + I[5] * x.z}; };
        const V3 h_l = mass * (vo + cross(w, c)), h_n = inertia(w) + cross(c, h_l);
        V3 p_n = cross(w, h_n) + cross(vo, h_l), p_l = cross(w, h_l);
        // contact forces: world-frame force at the foot point of this body
        if (force.any()) {
            for (int k = 0; k < m.nf; ++k) {
                if (m.foot_joint[k] != i) continue;
                V3 fp{0, 0, 0}, fv{0, 0, 0};       // the foot point's world position and velocity, for a source that reads them
                if constexpr (Force::kinematic) {
                    const V3 r = v3(m.foot_offset[k]);
                    fp = pw + mul(Rw, r); fv = mul(Rw, vo + cross(w, r));
                }
                const V3 l = mul_t(Rw, force(k, fp, fv));
                p_l = p_l - l;
                p_n = p_n - cross(v3(m.foot_offset[k]), l);
            }
        }
        at.put3(i, FD_P, p_n); at.put3(i, FD_P + 3, p_l);
        // the push: p^A -= (0; Rw^T F) on the pushed body, and no term at all (not a zero force) on any other evaluation.
        // It is applied to the slice, from the slice, behind a compiler barrier: the branch then uses no value of the pass
        // above, whose arithmetic stays the one of a source without the hook (as a term on p_l in registers the pass is
        // vectorised and fused differently).
        if constexpr (force_pushes<Force>::value) {
            if (force.pushed(i)) {
                __asm__ volatile("" ::: "memory");
                M3 Rs;
#pragma unroll
                for (int k = 0; k < 9; ++k) Rs.m[k] = at(i, FD_RW + k);
                at.put3(i, FD_P + 3, at.get3(i, FD_P + 3) - mul_t(Rs, force.body()));
            }
        }
        // the payload: I += I_p and p^A += v x* (I_p v) on the loaded body, to the slice and from the slice behind the same
        // barrier, for the same reason
        if constexpr (force_loads<Force>::value) {
            if (force.loaded(i)) {
                __asm__ volatile("" ::: "memory");
                const float mp = force.load_mass();
                const V3 r = force.load_at();
                add_point_inertia(at, i, mp, r);
                const V3 ws = at.get3(i, FD_V), vs = at.get3(i, FD_V + 3);
                const V3 g_l = mp * (vs + cross(ws, r)), g_n = cross(r, g_l);
                at.put3(i, FD_P, at.get3(i, FD_P) + cross(ws, g_n) + cross(vs, g_l));
                at.put3(i, FD_P + 3, at.get3(i, FD_P + 3) + cross(ws, g_l));
            }
        }
    }

    // inward: U = I^A S, d = S^T U, u = tau - S^T p^A; I^a = I^A - U U^T / d and p^a = p^A + I^a c + U u / d go to the parent
    bool sound = true;
    for (int i = n - 1; i >= 0; --i) {
        S6 A, C; M3 Bm;
#pragma unroll
        for (int k = 0; k < 6; ++k) A.m[k] = at(i, FD_I + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bm.m[k] = at(i, FD_I + 6 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) C.m[k] = at(i, FD_I + 15 + k);
        const V3 ax = v3(m.axis[i]);
        const bool rev = m.type[i] == 0;
        const V3 U_n = rev ? mul(A, ax) : mul(Bm, ax), U_l = rev ? mul_t(Bm, ax) : mul(C, ax);
        const V3 p_n = at.get3(i, FD_P), p_l = at.get3(i, FD_P + 3);
        float d = dot(ax, rev ? U_n : U_l);
        if constexpr (force_arms<Force>::value) d += force.armature(i);      // the rotor turns with the joint alone: S^T I^A S + armature
        const float u = at(i, FD_Q + 2) - dot(ax, rev ? p_n : p_l);
        sound = sound && d > 0.0f && d < INFINITY;
        at.put3(i, FD_RW, U_n); at.put3(i, FD_RW + 3, U_l);
        at(i, FD_RW + 6) = d; at(i, FD_RW + 7) = u;
        const int par = m.parent[i];
        if (par < 0) continue;
        const float inv_d = 1.0f / d;
        sub_outer(A, U_n, inv_d); sub_outer(Bm, U_n, U_l, inv_d); sub_outer(C, U_l, inv_d);
        const V3 c_w = at.get3(i, FD_C), c_v = at.get3(i, FD_C + 3);
        const float s = u * inv_d;
        const V3 a_n = p_n + mul(A, c_w) + mul(Bm, c_v) + s * U_n, a_l = p_l + mul_t(Bm, c_w) + mul(C, c_v) + s * U_l;
        // to the parent's frame: forces l' = R l, n' = R n + p x l'; the inertia R (.) R^T, then shifted by p:
        //   C' = C, B' = B + P C, A' = A - B P + P B'^T    (P = [p]x)
        M3 R; V3 p;
        joint_transform(m, i, at(i, FD_Q), R, p);
        const V3 l_p = mul(R, a_l);
        at.put3(par, FD_P + 3, at.get3(par, FD_P + 3) + l_p);
        at.put3(par, FD_P, at.get3(par, FD_P) + mul(R, a_n) + cross(p, l_p));
        const M3 Ar = rotated(R, full(A)), Br = rotated(R, Bm), Cr = rotated(R, full(C)), P = skew(p);
        M3 Bp = mul(P, Cr);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bp.m[k] += Br.m[k];
        const M3 BP = mul(Br, P), PBt = mul(P, transposed(Bp));
        M3 Ap;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ap.m[k] = Ar.m[k] - BP.m[k] + PBt.m[k];
        const S6 Au = upper(Ap), Cu = upper(Cr);
#pragma unroll
        for (int k = 0; k < 6; ++k) at(par, FD_I + k) += Au.m[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) at(par, FD_I + 6 + k) += Bp.m[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) at(par, FD_I + 15 + k) += Cu.m[k];
    }

    // outward: a' = X a_parent + c, qdd = (u - U^T a') / d, a = a' + S qdd; the world accelerates with -gravity
    for (int i = 0; i < n; ++i) {
        M3 R; V3 p;
        joint_transform(m, i, at(i, FD_Q), R, p);
        const int par = m.parent[i];
        V3 dw_p{0, 0, 0}, dvo_p{-m.gravity[0], -m.gravity[1], -m.gravity[2]};
        if (par >= 0) { dw_p = at.get3(par, FD_V); dvo_p = at.get3(par, FD_V + 3); }
        V3 dw = mul_t(R, dw_p) + at.get3(i, FD_C), dvo = mul_t(R, dvo_p + cross(dw_p, p)) + at.get3(i, FD_C + 3);
        const float qdd = (at(i, FD_RW + 7) - dot(at.get3(i, FD_RW), dw) - dot(at.get3(i, FD_RW + 3), dvo)) / at(i, FD_RW + 6);
        const V3 ax = v3(m.axis[i]);
        if (m.type[i] == 0) dw = dw + qdd * ax;
        else dvo = dvo + qdd * ax;
        at.put3(i, FD_V, dw); at.put3(i, FD_V + 3, dvo);
        at(i, FD_Q + 2) = qdd;
    }
    return sound;
}

struct FdArgs {
    int B, n_sub;                                         // n_sub = 0: nmpc_fd_accel_batch (tau is the joint force, nothing is integrated)
    float dt, kp, kd;
    const float *q, *v, *tau, *q_des, *f;                 // tau: tau of accel, tau_ff of step
    float *q_out, *v_out, *a_out;
};

// One launch for either entry point: load q, v into the slice, per substep the PD law (as pd_torques_kernel, v_plan = 0), the
// recursion and the semi-implicit Euler update, then the state and the last acceleration out.  The outputs are written after
// the last read of the inputs, so q_out, v_out may alias q, v.  The copy loops are kept as written: unrolled and vectorised
// with their run-time overlap checks they cost 26 SGPR spills around the recursion and save nothing.
template <int W>
__global__ __launch_bounds__(W) void fd_kernel(const Model* __restrict__ mp, const FdArgs p) {
    const Model& m = *mp;
    const int b = blockIdx.x * W + threadIdx.x;
    if (b >= p.B) return;
    const int n = m.n, nu = m.nu, base = n - nu;
    const Slice<FD_SLOTS, W> at;
    const float* qb = p.q + (size_t)b * n;
    const float* vb = p.v + (size_t)b * n;
    const float* tb = p.tau ? p.tau + (size_t)b * nu : nullptr;
    const float* db = p.q_des ? p.q_des + (size_t)b * nu : nullptr;
    const float* fb = p.f ? p.f + (size_t)b * m.nf * 3 : nullptr;
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = 0; i < n; ++i) { at(i, FD_Q) = qb[i]; at(i, FD_Q + 1) = vb[i]; }
    bool sound = true;
    const int steps = p.n_sub > 0 ? p.n_sub : 1;
    for (int s = 0; s < steps; ++s) {
#pragma clang loop unroll(disable) vectorize(disable)
        for (int i = 0; i < n; ++i) {
            float t = 0.0f;
            if (i >= base) {
                t = tb ? tb[i - base] : 0.0f;
                if (db) t = t + p.kp * (db[i - base] - at(i, FD_Q)) + p.kd * (0.0f - at(i, FD_Q + 1));
            }
            at(i, FD_Q + 2) = t;
        }
        sound = fd_accel_body<W, FD_SLOTS>(m, GivenForces{fb}) && sound;
        if (p.n_sub > 0)
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < n; ++i) {
                const float v = at(i, FD_Q + 1) + p.dt * at(i, FD_Q + 2);
                at(i, FD_Q + 1) = v;
                at(i, FD_Q) = at(i, FD_Q) + p.dt * v;
            }
    }
    const float nan = __builtin_nanf("");
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = 0; i < n; ++i) {
        const size_t e = (size_t)b * n + i;
        if (p.a_out) p.a_out[e] = sound ? at(i, FD_Q + 2) : nan;
        if (p.q_out) p.q_out[e] = sound ? at(i, FD_Q) : nan;
        if (p.v_out) p.v_out[e] = sound ? at(i, FD_Q + 1) : nan;
    }
}
