// nmpc_torque_state_momentum.hip.inc -- the centroidal momentum of a plant state (nmpc_state_momentum_batch of
// include/nmpc_torque.h); included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_momentum.hip.inc, whose outward
// pass it runs and nothing else: one thread per state, SM_W of them per block, per-body state in an LDS slice [joint][SM_SLOTS][SM_W].
//
// h = A_g(q) v is the sum of the bodies' momenta, so it needs neither the composite inertias nor the columns of A_g: frame
// rotations, the frame origins from the anchor point O (the origin of the first frame that carries mass; back along its path to the
// root, outward everywhere else, never from the world origin -- the base position does not enter the arithmetic), body velocities
// as world-axes spatial vectors about O, every body's momentum about O, the totals, the centre of mass from O, and then
//     h = [l; n_O - com x l].
// The slice holds only what a child reads of its parent -- rotation, origin, velocity -- 18 slots per joint against the 34 of
// cmd_kernel; a body's inertia and momentum live in registers for the length of its own iteration.  Nothing is inverted but the
// total mass, which the host has checked; a q or v that is not finite stays in its own row.  A skipped row touches no memory.
#pragma once

constexpr int SM_RW = 0;     // Rw 9: world rotation of frame i
constexpr int SM_D = 9;      // d 3: origin of frame i from O, world axes (until the outward pass: its offset in the parent frame)
constexpr int SM_V = 12;     // w 3, u 3: velocity of body i
constexpr int SM_SLOTS = 18;

constexpr size_t sm_lds_bytes(int n, int width) { return (size_t)n * SM_SLOTS * width * sizeof(float); }
// states per block by the rule of fd_block_width: the slice of the largest tree fits the CU at 32 (73 728 B), so there is one width
constexpr int SM_W = sm_lds_bytes(MAXJ, 32) <= FD_LDS_MAX ? 32 : 16;
static_assert(SM_W == 32, "the state-momentum slice of the largest tree no longer fits a CU at 32 states per block");

struct StateMomentumArgs {
    int B, anchor;                                        // anchor, chain: as CmdArgs
    unsigned chain;
    int qv_stride, h_stride, h2_stride, skip_mask;        // floats from one state's q, v / h / h2 to the next
    const float *q, *v;
    float *h, *h2;                                        // h2 may be nullptr
    const int* skip;                                      // nullptr, or [B] flag words: a state with skip[b] & skip_mask != 0 is left out
};

__global__ __launch_bounds__(SM_W) void state_momentum_kernel(const Model* __restrict__ mp, const StateMomentumArgs p) {
    const Model& m = *mp;
    const int b = blockIdx.x * SM_W + threadIdx.x;
    if (b >= p.B) return;
    if (p.skip && (p.skip[b] & p.skip_mask) != 0) return;
    const int n = m.n;
    const Slice<SM_SLOTS, SM_W> at;
    const float* qb = p.q + (size_t)b * p.qv_stride;
    const float* vb = p.v + (size_t)b * p.qv_stride;
    auto rotation = [&](int i) {
        M3 R;
#pragma unroll
        for (int k = 0; k < 9; ++k) R.m[k] = at(i, SM_RW + k);
        return R;
    };

    // world rotation of every frame; its offset in the parent frame waits in the slots of d
    for (int i = 0; i < n; ++i) {
        M3 R; V3 pl;
        joint_transform(m, i, qb[i], R, pl);
        const int par = m.parent[i];
        const M3 Rw = par >= 0 ? mul(rotation(par), R) : R;
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, SM_RW + k) = Rw.m[k];
        at.put3(i, SM_D, pl);
    }
    // O is the origin of the anchor's frame: d = 0 there, and back along its path to the root
    V3 O;
    {
        V3 d{0, 0, 0};
        for (int k = p.anchor;;) {
            const V3 pl = at.get3(k, SM_D);
            at.put3(k, SM_D, d);
            const int par = m.parent[k];
            if (par < 0) { O = pl - d; break; }
            d = d - mul(rotation(par), pl);
            k = par;
        }
    }

    // outward: the other frame origins, velocities, every body's momentum about O, the totals of the tree
    V3 first{0, 0, 0}, l_all{0, 0, 0}, n_all{0, 0, 0};
    float total = 0.0f;
    for (int i = 0; i < n; ++i) {
        const int par = m.parent[i];
        const M3 Rw = rotation(i);
        V3 d = at.get3(i, SM_D), w{0, 0, 0}, u{0, 0, 0};
        if (!((p.chain >> i) & 1u)) {
            d = par >= 0 ? at.get3(par, SM_D) + mul(rotation(par), d) : d - O;
            at.put3(i, SM_D, d);
        }
        if (par >= 0) { w = at.get3(par, SM_V); u = at.get3(par, SM_V + 3); }
        const V3 z = mul(Rw, v3(m.axis[i]));
        const float vi = vb[i];
        if (m.type[i] == 0) {          // S = (z; d x z)
            w = w + vi * z;
            u = u + vi * cross(d, z);
        } else {                       // S = (0; z)
            u = u + vi * z;
        }
        at.put3(i, SM_V, w); at.put3(i, SM_V + 3, u);
        // about O: k = m c; momentum l = m (u + w x c), moment = R Ic R^T w + c x l
        const float mass = m.mass[i];
        const V3 c = d + mul(Rw, v3(m.com[i]));
        const float* I = m.inertia[i];
        const S6 Ib = upper(rotated(Rw, full(S6{{I[0], I[1], I[2], I[3], I[4], I[5]}})));
        const V3 k = mass * c, l = mass * (u + cross(w, c));
        const V3 mom = mul(Ib, w) + cross(c, l);
        first = first + k; l_all = l_all + l; n_all = n_all + mom; total += mass;
    }
    const V3 com{first.x / total, first.y / total, first.z / total};      // from O; the host refuses a massless tree
    const V3 k_g = n_all - cross(com, l_all);
    const float out[6] = {l_all.x, l_all.y, l_all.z, k_g.x, k_g.y, k_g.z};
    float* hb = p.h + (size_t)b * p.h_stride;
#pragma unroll
    for (int k = 0; k < 6; ++k) hb[k] = out[k];
    if (p.h2) {
        float* h2b = p.h2 + (size_t)b * p.h2_stride;
#pragma unroll
        for (int k = 0; k < 6; ++k) h2b[k] = out[k];
    }
}
