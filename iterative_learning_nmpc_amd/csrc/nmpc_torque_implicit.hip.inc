// nmpc_torque_implicit.hip.inc -- the linearly implicit integrator of the ground-contact plant (nmpc_contact_set_integrator of
// include/nmpc_torque.h, which states the scheme); included by nmpc_torque.hip inside namespace nmpc_torque, after
// nmpc_torque_contact.hip.inc and nmpc_torque_crba.hip.inc and before nmpc_torque_track.hip.inc, whose chain calls it.
//
// One substep: the PD law, the clamp and the explicit acceleration a_exp are the explicit step's own (fd_accel_body under the
// ground law, the push as one more force); then the stiff terms are taken at the end of the substep, linearised at its start:
//     A a = rhs,   A = M(q) + sum_feet (dt J^T C J + dt^2 kz Jz^T Jz) + (dt kd + dt^2 kp) on the unclamped actuated joints,
//     rhs = M a_exp - dt sum_feet kz pd_z Jz^T - dt kp v on those joints;   v += dt a;  q += dt v.
// M comes from the composite-rigid-body passes of crba_kernel, restated here on the slots of the forward dynamics' slice that the
// recursion has left free (that kernel keeps its text: its outputs are held bit for bit).  J_k is nonzero only on the joints
// between foot k and the root, so J_k^T C J_k couples only joints on one path to the root: A has exactly the sparsity of M, and
// the L^T D L factorisation that eliminates the leaves first (Featherstone, RBDA table 6.3) fills nothing in.  M and A are a
// packed lower triangle [entry][W] behind the slice; only the entries (i, j) of joints on one path are ever written or read.
// This file is the correction alone.  The control steps around it are contact_chain_kernel's (nmpc_torque_track.hip.inc), whose
// ImplicitArgs instantiation serves nmpc_contact_step_batch and nmpc_contact_track_batch (and through them the policy and expert
// rollouts): the integrator has one copy of its substep and a chain of steps is its track bit for bit.
#pragma once

constexpr int IM_W = 16;                                  // robots per block: the slice and the triangle of the largest tree fit the CU
constexpr int IM_J = FD_P;                                // column i of the foot Jacobian in world axes 3 (p^A is spent after the recursion)
constexpr int IM_R = FD_P + 3;                            // rhs_i, then the solution a_i
constexpr size_t im_triangle(int n) { return (size_t)n * (n + 1) / 2; }
// the slice, the triangle, and behind it the block's law (the chains with a slot per lane: chain_lds_bytes, nmpc_torque_track.hip.inc)
constexpr size_t im_lds_bytes(int n) { return ((size_t)n * CT_SLOTS + im_triangle(n)) * IM_W * sizeof(float) + sizeof(ContactCfg); }

// no payload: what implicit_accel_body is given by a chain without one
struct NoLoad {
    static constexpr bool loads = false, drives = false;
};
// the lane's payload on body `on`
struct LaneLoaded {
    const Payload* load;
    int on;
    static constexpr bool loads = true, drives = false;
};
// the lane's payload and its actuator (nmpc_contact_set_actuators): the rotor inertia on the diagonal of the mass matrix, the
// passive damping taken implicitly on every actuated joint; kp, kd of the call below are then the lane's own
struct LaneDriven : LaneLoaded {
    const Actuator* drive;
    static constexpr bool drives = true;
};

// the law and a push that acts only in the substeps of its window
struct WindowedPushForces : PushedGroundForces {
    bool on;
    __device__ __forceinline__ bool pushed(int i) const { return on && i == joint; }
};

// This thread's packed lower triangle, [entry][W] behind the block's slice.
template <int W>
struct Triangle {
    float* base;
    __device__ __forceinline__ float& operator()(int i, int j) const { return base[(i * (i + 1) / 2 + j) * W + threadIdx.x]; }      // i >= j
};

// The implicit correction of one substep: from q, v, a_exp in slots FD_Q .. FD_Q + 2 of the slice (as fd_accel_body leaves them)
// to a in slot FD_Q + 2.  unclamped: bit i set for an actuated joint i whose PD torque the clamp did not cut (0 without a PD
// target).  Returns false if a pivot of the factorisation is not a positive finite number.
// load: the payload whose inertia the mass matrix carries (NoLoad: none, and the text below compiles to what it was without it);
// with Load::drives also the lane's actuator: M becomes M + armature on the actuated diagonal, in A and in rhs = (M + D) a_exp, and
// every actuated joint gains dt damping on the diagonal whether the clamp cut its torque or not.
template <int W, class Load = NoLoad>
__device__ __forceinline__ bool implicit_accel_body(const Model& m, const ContactCfg& c, const Triangle<W> A, float dt, float kp, float kd,
                                                    unsigned unclamped, [[maybe_unused]] const Load load = {}) {
    const int n = m.n;
    const Slice<CT_SLOTS, W> at;

    // outward (crba_kernel's): world pose of every frame, the body's own inertia about its origin
    for (int i = 0; i < n; ++i) {
        M3 R; V3 pl;
        joint_transform(m, i, at(i, FD_Q), R, pl);
        const int par = m.parent[i];
        M3 Rw = R;
        V3 pw = pl;
        if (par >= 0) {
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, FD_RW + k);
            Rw = mul(Rp, R);
            pw = at.get3(par, FD_PW) + mul(Rp, pl);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, FD_RW + k) = Rw.m[k];
        at.put3(i, FD_PW, pw);
        const float mass = m.mass[i];
        const V3 cm = v3(m.com[i]);
        const float* I = m.inertia[i];
        const float cc = dot(cm, cm);
        at(i, FD_I + 0) = I[0] + mass * (cc - cm.x * cm.x); at(i, FD_I + 1) = I[1] - mass * cm.x * cm.y; at(i, FD_I + 2) = I[2] - mass * cm.x * cm.z;
        at(i, FD_I + 3) = I[3] + mass * (cc - cm.y * cm.y); at(i, FD_I + 4) = I[4] - mass * cm.y * cm.z; at(i, FD_I + 5) = I[5] + mass * (cc - cm.z * cm.z);
        const M3 Bm = skew(mass * cm);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, FD_I + 6 + k) = Bm.m[k];
        at(i, FD_I + 15) = mass; at(i, FD_I + 16) = 0.0f; at(i, FD_I + 17) = 0.0f; at(i, FD_I + 18) = mass; at(i, FD_I + 19) = 0.0f; at(i, FD_I + 20) = mass;
        // the payload, as fd_accel_body adds it: to the slice, from the slice, behind the barrier
        if constexpr (Load::loads) {
            if (i == load.on) {
                __asm__ volatile("" ::: "memory");
                add_point_inertia(at, i, load.load->mass, V3{load.load->x, load.load->y, load.load->z});
            }
        }
    }

    // inward (crba_kernel's): I^c of a body goes to its parent's frame, C' = C, B' = B + P C, A' = A - B P + P B'^T  (P = [p]x)
    for (int i = n - 1; i >= 0; --i) {
        const int par = m.parent[i];
        if (par < 0) continue;
        S6 Ai, Ci; M3 Bm;
#pragma unroll
        for (int k = 0; k < 6; ++k) Ai.m[k] = at(i, FD_I + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bm.m[k] = at(i, FD_I + 6 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) Ci.m[k] = at(i, FD_I + 15 + k);
        M3 R; V3 pl;
        joint_transform(m, i, at(i, FD_Q), R, pl);
        const M3 Ar = rotated(R, full(Ai)), Br = rotated(R, Bm), Cr = rotated(R, full(Ci)), P = skew(pl);
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

    // columns: F = I^c_i S_i carried up the path to the root gives row i of M below the diagonal; rhs = M a_exp on the way
    // (row i is complete when its last descendant has been through: parents come before their children)
    for (int i = 0; i < n; ++i) {
        S6 Ai, Ci; M3 Bm;
#pragma unroll
        for (int k = 0; k < 6; ++k) Ai.m[k] = at(i, FD_I + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) Bm.m[k] = at(i, FD_I + 6 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) Ci.m[k] = at(i, FD_I + 15 + k);
        const V3 ax = v3(m.axis[i]);
        const bool rev = m.type[i] == 0;
        V3 F_n = rev ? mul(Ai, ax) : mul(Bm, ax), F_l = rev ? mul_t(Bm, ax) : mul(Ci, ax);
        const float a_i = at(i, FD_Q + 2);
        float d = dot(ax, rev ? F_n : F_l);
        if constexpr (Load::drives)
            if (i >= n - m.nu) d += load.drive->armature;
        A(i, i) = d;
        float acc = d * a_i;
        for (int frame = i, j = m.parent[i]; j >= 0; frame = j, j = m.parent[j]) {
            M3 R; V3 pl;
            joint_transform(m, frame, at(frame, FD_Q), R, pl);
            F_l = mul(R, F_l);
            F_n = mul(R, F_n) + cross(pl, F_l);
            const float e = dot(v3(m.axis[j]), m.type[j] == 0 ? F_n : F_l);
            A(i, j) = e;
            acc += e * at(j, FD_Q + 2);
            at(j, IM_R) += e * a_i;
        }
        at(i, IM_R) = acc;
    }

    // the feet in the ground: J_k on the path of foot k, pd_k = J_k v, and the symmetric positive semidefinite parts of
    // -df/dpd (C_k) and -df/dp (kz_k) of the law
    for (int k = 0; k < m.nf; ++k) {
        const int fj = m.foot_joint[k];
        M3 Rw;
#pragma unroll
        for (int e = 0; e < 9; ++e) Rw.m[e] = at(fj, FD_RW + e);
        const V3 pf = at.get3(fj, FD_PW) + mul(Rw, v3(m.foot_offset[k]));
        const float delta = c.ground_z - pf.z;
        if (!(delta > 0.0f)) continue;
        V3 pd{0, 0, 0};
        for (int i = fj; i >= 0; i = m.parent[i]) {
            M3 Ri;
#pragma unroll
            for (int e = 0; e < 9; ++e) Ri.m[e] = at(i, FD_RW + e);
            const V3 z = mul(Ri, v3(m.axis[i]));
            const V3 col = m.type[i] == 0 ? cross(z, pf - at.get3(i, FD_PW)) : z;
            at.put3(i, IM_J, col);
            pd = pd + at(i, FD_Q + 1) * col;
        }
        const float fz = contact_law(c, pf, pd).z;
        const float g = fmaxf(0.0f, 1.0f - c.damping * pd.z);
        const float r2 = pd.x * pd.x + pd.y * pd.y + c.slip2, r = sqrtf(r2);
        const float s1 = c.mu * fz / r, s3 = c.mu * fz / (r2 * r);
        const float Cxx = s1 - s3 * pd.x * pd.x, Cxy = -s3 * pd.x * pd.y, Cyy = s1 - s3 * pd.y * pd.y;
        const float Czz = g > 0.0f ? c.stiffness * delta * c.damping : 0.0f, kz = c.stiffness * g;
        const float wz = dt * Czz + dt * dt * kz, rz = dt * kz * pd.z;
        for (int i = fj; i >= 0; i = m.parent[i]) {
            const V3 Ji = at.get3(i, IM_J);
            const V3 t{dt * (Cxx * Ji.x + Cxy * Ji.y), dt * (Cxy * Ji.x + Cyy * Ji.y), wz * Ji.z};
            at(i, IM_R) -= rz * Ji.z;
            for (int j = i; j >= 0; j = m.parent[j]) A(i, j) += dot(t, at.get3(j, IM_J));
        }
    }

    // the PD law on the joints the clamp did not cut
    for (int i = n - m.nu; i < n; ++i) {
        if constexpr (Load::drives) {
            if (!((unclamped >> i) & 1u)) { A(i, i) += dt * load.drive->damping; continue; }
            A(i, i) += dt * (kd + load.drive->damping) + dt * dt * kp;
        } else {
            if (!((unclamped >> i) & 1u)) continue;
            A(i, i) += dt * kd + dt * dt * kp;
        }
        at(i, IM_R) -= dt * kp * at(i, FD_Q + 1);
    }

    // A = L^T D L, leaves first: L (unit lower triangular) below the diagonal, D on it, no entry off the paths is touched
    bool sound = true;
    for (int k = n - 1; k >= 0; --k) {
        const float d = A(k, k);
        sound = sound && d > 0.0f && d < INFINITY;
        const float inv_d = 1.0f / d;
        for (int i = m.parent[k]; i >= 0; i = m.parent[i]) {
            const float l = A(k, i) * inv_d;
            for (int j = i; j >= 0; j = m.parent[j]) A(i, j) -= l * A(k, j);
            A(k, i) = l;
        }
    }
    // a = L^-1 D^-1 L^-T rhs
    for (int i = n - 1; i >= 0; --i) {
        const float y = at(i, IM_R);
        for (int j = m.parent[i]; j >= 0; j = m.parent[j]) at(j, IM_R) -= A(i, j) * y;
    }
    for (int i = 0; i < n; ++i) {
        float x = at(i, IM_R) / A(i, i);
        for (int j = m.parent[i]; j >= 0; j = m.parent[j]) x -= A(i, j) * at(j, IM_R);
        at(i, IM_R) = x;
        at(i, FD_Q + 2) = x;
    }
    return sound;
}
