// nmpc_torque_contact.hip.inc -- the ground-contact plant of the torque layer (nmpc_foot_kinematics_batch,
// nmpc_contact_forces_batch, nmpc_contact_step_batch of include/nmpc_torque.h); included by nmpc_torque.hip inside namespace
// nmpc_torque, after nmpc_torque_fd.hip.inc.
//
// The declared law (DESIGN.md 8d): the ground is the plane z = ground_z with normal e_z; a foot point at p moving with pd,
// penetration delta = ground_z - p_z, gets
//     f_z  = k delta max(0, 1 - c pd_z)                   for delta > 0, else no force      (Hunt-Crossley: continuous, never pulls)
//     f_xy = -mu f_z pd_xy / sqrt(|pd_xy|^2 + v_eps^2)                                       (regularised Coulomb)
// One device function states it; the forces kernel evaluates it on the foot kinematics, the step evaluates it inside the
// articulated-body recursion (fd_accel_body with GroundForces as its force source) where the first outward pass visits the
// body that carries the foot, so the forces never go through memory between substeps.
#pragma once

struct ContactCfg {                                       // nmpc_contact_cfg as the kernels read it
    float ground_z, stiffness, damping, mu, slip2, tau_max;   // slip2 = slip_velocity^2
};

__device__ __forceinline__ V3 contact_law(const ContactCfg& c, V3 p, V3 pd) {
    const float delta = c.ground_z - p.z;
    if (!(delta > 0.0f)) return {0.0f, 0.0f, 0.0f};
    const float fz = c.stiffness * delta * fmaxf(0.0f, 1.0f - c.damping * pd.z);
    const float s = -c.mu * fz / sqrtf(pd.x * pd.x + pd.y * pd.y + c.slip2);
    return {s * pd.x, s * pd.y, fz};
}

// A ground per robot (nmpc_contact_set_grounds, DESIGN.md 8d): row b of the attached table [n_rows][6] in the field order of
// nmpc_contact_cfg, as the kernels read a law.  slip2 is the fp32 product device_cfg forms on the host, so a row equal to a
// uniform struct is that struct's ContactCfg bit for bit.  Nothing of a row is validated here (include/nmpc_torque.h).
__device__ __forceinline__ ContactCfg ground_row(const float* __restrict__ rows, int b) {
    const float* r = rows + (size_t)b * 6;
    return {r[0], r[1], r[2], r[3], r[4] * r[4], r[5]};
}

// ---- foot kinematics, and the law on them ---------------------------------------------------------------------------------
constexpr int FK_RW = 0;     // Rw 9
constexpr int FK_PW = 9;     // world position of the body origin 3
constexpr int FK_V = 12;     // w 3, vo 3 (body coordinates)
constexpr int FK_SLOTS = 18;
constexpr size_t fk_lds_bytes(int n) { return (size_t)n * FK_SLOTS * TPB * sizeof(float); }

struct FootArgs {
    static constexpr bool grounds = false;
    int B;
    const float *q, *v;                                   // v nullptr: at rest
    float *pos, *vel, *f;                                 // each may be nullptr; f: the law of c on (pos, vel)
    ContactCfg c;
};

struct FootRowsArgs : FootArgs {                          // the law of robot b's row on (pos, vel); c is not read
    static constexpr bool grounds = true;
    const float* rows;
};

// One outward pass: Rw, the world position of the body origin and the body-coordinate velocity (w, vo); the foot point of a
// body is then p = p_w + Rw r, pd = Rw (vo + w x r).  One thread per robot, LDS slice [joint][FK_SLOTS][TPB].
// The pass keeps its text here and in observe_kernel: as one function template called from both, this kernel rounded differently.
// Two instantiations, switched at compile time by Args::grounds: foot_kernel<FootArgs> compiles to the instructions foot_kernel
// had before it was a template (DESIGN.md 8d) -- as a function template called from two kernels of its own it did not.
template <class Args>
__global__ __launch_bounds__(TPB) void foot_kernel(const Model* __restrict__ mp, const Args a) {
    const Model& m = *mp;
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= a.B) return;
    const int n = m.n;
    const Slice<FK_SLOTS, TPB> at;
    const float* qb = a.q + (size_t)b * n;
    const float* vb = a.v ? a.v + (size_t)b * n : nullptr;
    for (int i = 0; i < n; ++i) {
        M3 R; V3 p;
        joint_transform(m, i, qb[i], R, p);
        const int par = m.parent[i];
        V3 w_p{0, 0, 0}, vo_p{0, 0, 0}, pw = p;
        M3 Rw = R;
        if (par >= 0) {
            w_p = at.get3(par, FK_V); vo_p = at.get3(par, FK_V + 3);
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, FK_RW + k);
            Rw = mul(Rp, R);
            pw = at.get3(par, FK_PW) + mul(Rp, p);
        }
        V3 w = mul_t(R, w_p), vo = mul_t(R, vo_p + cross(w_p, p));
        const float qd = vb ? vb[i] : 0.0f;
        const V3 ax = v3(m.axis[i]);
        if (m.type[i] == 0) w = w + qd * ax;
        else vo = vo + qd * ax;
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, FK_RW + k) = Rw.m[k];
        at.put3(i, FK_PW, pw); at.put3(i, FK_V, w); at.put3(i, FK_V + 3, vo);
    }
    [[maybe_unused]] ContactCfg own;                      // Args::grounds: this robot's row
    if constexpr (Args::grounds)
        if (a.f) own = ground_row(a.rows, b);
    for (int k = 0; k < m.nf; ++k) {
        const int j = m.foot_joint[k];
        M3 Rw;
#pragma unroll
        for (int e = 0; e < 9; ++e) Rw.m[e] = at(j, FK_RW + e);
        const V3 r = v3(m.foot_offset[k]);
        const V3 p = at.get3(j, FK_PW) + mul(Rw, r), pd = mul(Rw, at.get3(j, FK_V + 3) + cross(at.get3(j, FK_V), r));
        const size_t e = ((size_t)b * m.nf + k) * 3;
        if (a.pos) { a.pos[e] = p.x; a.pos[e + 1] = p.y; a.pos[e + 2] = p.z; }
        if (a.vel) { a.vel[e] = pd.x; a.vel[e + 1] = pd.y; a.vel[e + 2] = pd.z; }
        if (a.f) {
            V3 f;
            if constexpr (Args::grounds) f = contact_law(own, p, pd);
            else f = contact_law(a.c, p, pd);
            a.f[e] = f.x; a.f[e + 1] = f.y; a.f[e + 2] = f.z;
        }
    }
}

// ---- the contact step -----------------------------------------------------------------------------------------------------
constexpr int CT_SLOTS = FD_SLOTS + 3;                    // the slice of fd_accel_body and FD_PW, the world position of the body origin
// the slice, and behind it the parameters of the law: six uniform values that would otherwise live in scalar registers across
// the whole recursion, which fills the scalar file on its own (they cost 13 SGPR spills there)
constexpr size_t ct_lds_bytes(int n, int width) { return (size_t)n * CT_SLOTS * width * sizeof(float) + sizeof(ContactCfg); }
// robots per block: 32 where the slice of n joints fits the CU (n <= 23), 16 otherwise (32 joints: 110 616 B)
constexpr int ct_block_width(int n) { return ct_lds_bytes(n, 32) <= FD_LDS_MAX ? 32 : 16; }
static_assert(ct_lds_bytes(MAXJ, 16) == 110616, "the contact step of the largest tree at 16 robots per block");
// the largest tree that runs at 32 robots per block: its slice is the most contact_step_kernel<32> can be asked for
constexpr int ct_wide_joints() {
    int n = MAXJ;
    while (n > 1 && ct_block_width(n) != 32) --n;
    return n;
}

// the law as the force source of fd_accel_body; `out` (this robot's row of f_out, or nullptr) takes the forces as they are used
struct GroundForces {
    const ContactCfg* c;                                  // in LDS, behind the block's slice: the block's, or under a table the lane's
    float* out;
    static constexpr bool kinematic = true;
    __device__ __forceinline__ bool any() const { return true; }
    __device__ __forceinline__ V3 operator()(int k, V3 p, V3 pd) const {
        const V3 f = contact_law(*c, p, pd);
        if (out) { out[3 * k] = f.x; out[3 * k + 1] = f.y; out[3 * k + 2] = f.z; }
        return f;
    }
};

// the law and a push (DESIGN.md 8d): the world-frame force F at the origin of the body frame of `joint`, in every evaluation --
// a substep that is not pushed is not run with this source at all (nmpc_torque.hip cuts a call into pushed and un-pushed launches)
struct PushedGroundForces : GroundForces {
    V3 F;
    int joint;
    static constexpr bool pushes = true;
    __device__ __forceinline__ bool pushed(int i) const { return i == joint; }
    __device__ __forceinline__ V3 body() const { return F; }
};

// A payload per robot (nmpc_contact_set_payloads, DESIGN.md 8d): a point mass at r in the frame of one body of the tree, row b of
// the attached table [n_rows][4] as it is.  Nothing of a row is validated here (include/nmpc_torque.h).
struct Payload {
    float mass, x, y, z;
};
// what a lane of the payload chains keeps behind the slice (nmpc_torque_track.hip.inc has the footprint): its law and, beside it,
// its payload (ten words: the 32 lanes of a block at that stride fall on 32 different banks of 64)
struct LaneLoad {
    ContactCfg c;
    Payload load;
};
// a force source of the plant under the lane's payload on body `on`: the hook of fd_accel_body reads the four words where they lie
template <class Source>
struct Loaded : Source {
    const Payload* load;                                  // in LDS, beside the lane's law
    int on;
    static constexpr bool loads = true;
    __device__ __forceinline__ bool loaded(int i) const { return i == on; }
    __device__ __forceinline__ float load_mass() const { return load->mass; }
    __device__ __forceinline__ V3 load_at() const { return {load->x, load->y, load->z}; }
};

// An actuator per robot (nmpc_contact_set_actuators, DESIGN.md 8d): the gains of the PD law, a passive joint damping and a reflected
// rotor inertia on every actuated joint, row b of the attached table [n_rows][4] as it is.  Nothing of a row is validated here
// (include/nmpc_torque.h).
struct Actuator {
    float kp, kd, damping, armature;
};
// what a lane of the actuator chains keeps behind the slice: its law, its payload (the zero row where no table of payloads is
// attached) and its actuator.  Fourteen words: on the 64 banks of a wide read the 32 lanes of a block at that stride fall on 32
// different banks (14 l mod 64 is one-to-one on l < 32); a one-word read or a write is banked on 32 (ds_read_b32 and
// every ds_write on CDNA), where 14 l mod 32 takes 16 values and a slot word costs one more LDS cycle -- as the six words of a law and the ten
// of a LaneLoad do (6 l, 10 l mod 32 take 16 values too).  The slot is read a few times per joint and substep beside the
// hundreds of slice accesses of the recursion.
struct LaneDrive {
    ContactCfg c;
    Payload load;
    Actuator drive;
};
// a force source of the plant under the lane's actuator: the hook of fd_accel_body adds the rotor inertia to the pivot of the
// actuated joints, i >= base
template <class Source>
struct Driven : Source {
    const Actuator* drive;                                // in LDS, beside the lane's law and payload
    int base;
    static constexpr bool arms = true;
    __device__ __forceinline__ float armature(int i) const { return i >= base ? drive->armature : 0.0f; }
};

struct ContactArgs {
    int B, n_sub;
    float dt, kp, kd;
    ContactCfg c;
    const float *q, *v, *tau, *q_des;                     // tau: tau_ff
    float *q_out, *v_out, *a_out, *f_out, *tau_out;
};

// fd_kernel's step with the law in place of given forces and the torque limit after the PD law.  f_out and tau_out are
// written by the last substep as its force and torque are formed (nothing reads them), a_out, q_out, v_out after the last read
// of the inputs, so q_out, v_out may alias q, v.  The copy loops are kept as written, as fd_kernel's.
// Both keep their text: as wrappers of one step driver with two plants the bits held, but fd_kernel<32> was 0.7-1.2 % slower.
// Nor is this kernel an instantiation of contact_chain_kernel (nmpc_torque_track.hip.inc), which states the same substep for
// every chain of control steps: its arguments are another struct (inputs apart from the outputs, one target row, no table, no
// skip flags) and it writes NaN on the way out where the chain fills the slice, so joining would take a switch at every one of
// those places.  As the instantiation of the chain for StepArgs : PushArgs with Forces::ground (the step's start state and
// outputs on the un-pushed recursion) it gave this kernel's bits, but it is another 194 instructions (the control-step loop,
// the table and the skip flags stay in) and cost the policy rollout 1.6 us of the 150 us of a two-substep step, eight times the
// parent's own spread (DESIGN.md 8d): a fix to the PD law, the clamp, the Euler update or the NaN rule goes here and into the
// chain.
template <int W>
__global__ __launch_bounds__(W) void contact_step_kernel(const Model* __restrict__ mp, const ContactArgs p) {
    extern __shared__ float body[];                       // [joint][CT_SLOTS][W]
    const Model& m = *mp;
    const int n = m.n, nu = m.nu, base = n - nu, nf3 = 3 * m.nf;
    ContactCfg* cfg = reinterpret_cast<ContactCfg*>(body + n * CT_SLOTS * W);
    if (threadIdx.x == 0) *cfg = p.c;
    __syncthreads();
    const int b = blockIdx.x * W + threadIdx.x;
    if (b >= p.B) return;
    const Slice<CT_SLOTS, W> at;
    const float* qb = p.q + (size_t)b * n;
    const float* vb = p.v + (size_t)b * n;
    const float* tb = p.tau ? p.tau + (size_t)b * nu : nullptr;
    const float* db = p.q_des ? p.q_des + (size_t)b * nu : nullptr;
    float* fo = p.f_out ? p.f_out + (size_t)b * nf3 : nullptr;
    float* to = p.tau_out ? p.tau_out + (size_t)b * nu : nullptr;
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = 0; i < n; ++i) { at(i, FD_Q) = qb[i]; at(i, FD_Q + 1) = vb[i]; }
    bool sound = true;
    for (int s = 0; s < p.n_sub; ++s) {
        const bool last = s == p.n_sub - 1;
#pragma clang loop unroll(disable) vectorize(disable)
        for (int i = 0; i < n; ++i) {
            float t = 0.0f;
            if (i >= base) {
                t = tb ? tb[i - base] : 0.0f;
                if (db) t = t + p.kp * (db[i - base] - at(i, FD_Q)) + p.kd * (0.0f - at(i, FD_Q + 1));
                { const float lim = cfg->tau_max; if (lim > 0.0f) t = t > lim ? lim : (t < -lim ? -lim : t); }   // a NaN stays NaN
                if (last && to) to[i - base] = t;
            }
            at(i, FD_Q + 2) = t;
        }
        sound = fd_accel_body<W, CT_SLOTS>(m, GroundForces{cfg, last ? fo : nullptr}) && sound;
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
        p.q_out[e] = sound ? at(i, FD_Q) : nan;
        p.v_out[e] = sound ? at(i, FD_Q + 1) : nan;
    }
    if (!sound) {
#pragma clang loop unroll(disable) vectorize(disable)
        for (int i = 0; fo && i < nf3; ++i) fo[i] = nan;
#pragma clang loop unroll(disable) vectorize(disable)
        for (int i = 0; to && i < nu; ++i) to[i] = nan;
    }
}
