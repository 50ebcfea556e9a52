// nmpc_torque_track.hip.inc -- the chain of control steps on the ground-contact plant: a table of PD targets tracked in one launch,
// pushed, under a window per robot, under the implicit integrator, under a ground or under a payload per robot (nmpc_contact_track_batch of
// include/nmpc_torque.h, and every launch of nmpc_contact_step_batch but the un-pushed explicit one); included by nmpc_torque.hip inside namespace nmpc_torque,
// after nmpc_torque_implicit.hip.inc.
//
// The whole-body expert on the declared plant (DESIGN.md 8h): the label row of a plan, A = (tau_id + kd v_plan) / kp + q_plan,
// handed to the contact step as q_des gives tau = tau_id + kp (q_plan - q) + kd (v_plan - v), the reference's
// _compute_pd_torques on the plan's inverse-dynamics torque (mpc.py:583-599).  So a replanning interval is a chain of contact
// steps, one per row of the label table; contact_chain_kernel runs that chain in one launch with the robot's state resident in
// the LDS, and observe_kernel<ObserveRowsArgs> (nmpc_torque_policy.hip.inc) turns the states it went through into the 44-slot
// rows and the fall predicates.  Both are held bit for bit to the chain of public calls they replace
// (tests/test_gpu_contact_track.py).
#pragma once

// ---- the arguments of the chain, one struct per instantiation of contact_chain_kernel ---------------------------------------------
// What a struct's constants switch in the kernel is stated there; the kernel reads nothing of a struct that its constants rule out.
// Slot and lane_slots name what lies behind the slice (under the implicit integrator behind the triangle): one Slot for the block,
// or one per lane; the footprint, the block width and the launch follow from them (chain_lds_bytes below).
enum class Forces {
    ground,                                               // GroundForces in every substep
    pushed,                                               // PushedGroundForces in every substep
    either,                                               // per substep and robot one of the two, by the robot's own window
    windowed                                              // WindowedPushForces: one source, the push switched by the window
};

// The un-pushed track: the state in q, v goes through n_steps control steps, in place.
struct TrackArgs {
    static constexpr bool step_io = false, implicit = false, grounds = false, payloads = false, actuators = false, lane_slots = false;
    static constexpr Forces forces = Forces::ground;
    using Slot = ContactCfg;                              // the block's law
    int B, n_steps, n_sub, a_rows, qv_rows, skip_mask;
    float dt, kp, kd;
    ContactCfg c;
    const float *tau, *A;                                 // tau: tau_ff [B][nu] or nullptr; A: robot b's targets from A + b * a_rows * nu
    const int* skip;                                      // nullptr: nobody is left out
    float *q, *v;                                         // in/out
    float *Q, *V;                                         // both or neither: the state before control step k at + (b * qv_rows + k) * n
};

// The pushed substeps (DESIGN.md 8d), every substep of the launch pushed.  nmpc_torque.hip cuts a plant call into runs of un-pushed
// substeps, which stay launches of contact_step_kernel / the TrackArgs chain as they are, and runs of pushed ones, which are
// launches of this chain for the step and for the track alike: an un-pushed substep is the un-pushed kernel's arithmetic because
// it is that kernel, and a pushed chain of steps is its track because both run this instantiation.  (A window flag inside one
// kernel does not give that: the compiler fuses the recursion of such a kernel differently, and its un-pushed substeps are not the
// un-pushed kernel's bits.)  So it serves both callers (step_io): a start state apart from q, v and the outputs of the last
// substep for the step; a table of targets, rows Q, V and skip flags for the track.
struct PushArgs : TrackArgs {                             // A == nullptr: no PD target (the step's q_des == NULL)
    static constexpr bool step_io = true;
    static constexpr Forces forces = Forces::pushed;
    const float* force;                                   // robot b's world-frame force at force + 3 b
    int joint;
    const float *q_in, *v_in;                             // the start state; nullptr: q, v
    float *a_out, *f_out, *tau_out;                       // of the last substep of the last control step (each may be nullptr)
};

// A window of its own per robot, nmpc_contact_set_push_windows (DESIGN.md 8d): robot b is pushed in the substeps
// first[b] <= s0 + k n_sub + i < first[b] + count[b], so the cut of a call into pushed and un-pushed launches, which is uniform over
// the batch, cannot be made on the host.  One launch per call instead, and in every substep the robot takes one of two calls of
// the recursion -- the un-pushed one under GroundForces, which is the call of contact_step_kernel / the TrackArgs chain, or the
// pushed one under PushedGroundForces, which is the PushArgs chain's.  The two are separate inlined copies on the two sides of a
// branch, not one copy under a flag: each is compiled in blocks of its own, as in the kernel it comes from, and an un-pushed robot
// runs no instruction of the push.  Robots of one block share its width and its slice layout and nothing else, so lanes whose
// windows differ in a substep run the two sides one after the other under their execution masks (a substep then costs two
// recursions for that wave); a wave whose lanes agree skips the other side.  Held bit for bit, robot by robot, to the cut path
// under that robot's window (tests/test_gpu_push_windows_plant.py).
struct WindowArgs : PushArgs {
    static constexpr Forces forces = Forces::either;
    const int *first, *count;                             // robot b's window, in the count the call's substep 0 is substep s0 of
    long long s0;
};

// The linearly implicit integrator (nmpc_torque_implicit.hip.inc): every substep solves twice, and the window of a push is tested
// per substep inside the one source -- there are no un-pushed bits of another kernel to keep.  With windows per robot attached the
// same test reads the robot's own window: the launch is the same.  The triangle of implicit_accel_body lies between the slice and
// the law.
struct ImplicitArgs : PushArgs {                          // force == nullptr: no push
    static constexpr bool implicit = true;
    static constexpr Forces forces = Forces::windowed;
    long long push_lo, push_hi;                           // the pushed substeps k * n_sub + s of the launch: [push_lo, push_hi)
    const int *win_first, *win_count;                     // nmpc_contact_set_push_windows (nullptr: the window above for every robot):
    long long win_s0;                                     // robot b's window [win_first[b], + win_count[b]) less win_s0 instead
};

// A ground per robot, nmpc_contact_set_grounds (DESIGN.md 8d): c is not read; every lane has a ContactCfg of its own behind the
// block's slice (under the implicit integrator behind the triangle), filled from row b of the table, and the law and the clamp
// read it through the pointer they read the block's one law through.  One instantiation per integrator, one launch per call.
// The explicit one has no cut into launches to lean on either (the table is attached whether or not a push is), so it takes a
// push as the implicit chain states it -- none, one window for the batch, or the robot's own -- and in every substep one of the
// two inlined recursions of WindowArgs, for the reason stated there: robot b is then the bits of the uniform launches under its
// own row (tests/test_gpu_grounds.py).
struct ImplicitGroundsArgs : ImplicitArgs {
    static constexpr bool grounds = true, lane_slots = true;      // the lane's law
    const float* rows;                                    // [>= B][6] in the field order of nmpc_contact_cfg
};
struct GroundsArgs : ImplicitGroundsArgs {
    static constexpr bool implicit = false;
    static constexpr Forces forces = Forces::either;
};

// A payload per robot, nmpc_contact_set_payloads (DESIGN.md 8d): of the family above, so every lane has a slot of its own behind
// the slice (behind the triangle when implicit), now its law and beside it the four words of row b of the payload table.  The law
// is row b of the table of grounds if one is attached (rows), else c: both are the ContactCfg the uniform call reads, bit for bit.
// The recursion runs under Loaded<> sources, whose hook adds the point mass to the inertia and the velocity-product force of body
// `payload_joint`; the implicit correction forms its mass matrix with the same addition.  One instantiation per integrator, one
// launch per call, the push stated and taken as under a table of grounds.
struct ImplicitPayloadsArgs : ImplicitGroundsArgs {
    static constexpr bool payloads = true;
    using Slot = LaneLoad;                                // the lane's law and its payload
    const float* payload_rows;                            // [>= B][4]: m_p, r_x, r_y, r_z
    int payload_joint;
};
struct PayloadsArgs : ImplicitPayloadsArgs {
    static constexpr bool implicit = false;
    static constexpr Forces forces = Forces::either;
};

// An actuator per robot, nmpc_contact_set_actuators (DESIGN.md 8d): of the same family, the lane's slot now its law, its payload
// and the four words of row b of the actuator table.  The law is taken as under PayloadsArgs (row b of the table of grounds, else
// c); the payload is row b of the table of payloads, or the zero row where none is attached (payload_rows == nullptr: the hook adds
// zeros).  The PD law reads the lane's kp, kd in place of the call's, the joint force loses damping v after the clamp, the
// recursion runs under Driven<Loaded<>> sources, whose hook adds the rotor inertia to the pivots of the actuated joints, and the
// implicit correction is handed the same four words.  One instantiation per integrator, one launch per call, the push stated and
// taken as under a table of grounds.
struct ImplicitActuatorsArgs : ImplicitPayloadsArgs {
    static constexpr bool actuators = true;
    using Slot = LaneDrive;                               // the lane's law, its payload and its actuator
    const float* actuator_rows;                           // [>= B][4]: kp, kd, damping, armature
};
struct ActuatorsArgs : ImplicitActuatorsArgs {
    static constexpr bool implicit = false;
    static constexpr Forces forces = Forces::either;
};

// ---- the footprint of an instantiation ------------------------------------------------------------------------------------------
template <class... Args>
struct ArgsList {};
using ChainArgs = ArgsList<TrackArgs, PushArgs, WindowArgs, ImplicitArgs, GroundsArgs, ImplicitGroundsArgs, PayloadsArgs, ImplicitPayloadsArgs,
                           ActuatorsArgs, ImplicitActuatorsArgs>;

// the LDS of a block of w robots of n joints: the slice, the triangle if implicit, then one slot or a slot per lane (six words
// per lane fall on 32 different banks, as the ten of a LaneLoad and the fourteen of a LaneDrive do)
template <class Args>
constexpr size_t chain_lds_bytes(int n, int w) {
    return ((size_t)n * CT_SLOTS + (Args::implicit ? im_triangle(n) : 0)) * w * sizeof(float) + (Args::lane_slots ? w : 1) * sizeof(typename Args::Slot);
}
// robots per block: the implicit chain's one width, else 32 where that footprint fits the CU and 16 otherwise
template <class Args>
constexpr int chain_block_width(int n) { return Args::implicit ? IM_W : (chain_lds_bytes<Args>(n, 32) <= FD_LDS_MAX ? 32 : 16); }
// the largest tree that runs at 32 robots per block: its footprint is the most the 32-wide instantiation can be asked for
template <class Args>
constexpr int chain_wide_joints() {
    int n = MAXJ;
    while (n > 1 && chain_block_width<Args>(n) != 32) --n;
    return n;
}
// the chains that the cut path alternates with contact_step_kernel run at its width
template <class Args>
constexpr bool chain_steps_width() {
    for (int n = 1; n <= MAXJ; ++n)
        if (chain_block_width<Args>(n) != ct_block_width(n)) return false;
    return true;
}
static_assert(chain_steps_width<TrackArgs>() && chain_steps_width<PushArgs>() && chain_steps_width<WindowArgs>(),
              "a chain of the cut path no longer runs at the width of contact_step_kernel");
static_assert(chain_lds_bytes<GroundsArgs>(23, 32) == 159744 && chain_wide_joints<GroundsArgs>() == 23, "a law per lane: 23 joints x 32 robots");
static_assert(chain_lds_bytes<PayloadsArgs>(23, 32) == 160256 && chain_wide_joints<PayloadsArgs>() == 23, "a law and a payload per lane: 23 joints x 32 robots");
static_assert(sizeof(LaneDrive) == 56, "a law, a payload and an actuator per lane: 14 words");
static_assert(chain_lds_bytes<ActuatorsArgs>(23, 32) == 160768 && chain_wide_joints<ActuatorsArgs>() == 23, "a law, a payload and an actuator per lane: 23 joints x 32 robots");
static_assert(chain_lds_bytes<ImplicitActuatorsArgs>(MAXJ, IM_W) == 145280 && MAXJ == 32, "the implicit actuator chain of the largest tree at 16 robots per block");

// ---- the chain ------------------------------------------------------------------------------------------------------------------
// contact_step_kernel's substep, n_steps * n_sub times on the state in the slice: per control step the state goes out to row k
// of Q, V (if given), the PD target becomes row k of the robot's table, and n_sub substeps follow.  A control step whose
// recursion met an unsound pivot leaves NaN in the whole state, as the contact step writes it and the next call of a chain
// reads it back, so the NaN appears in the row of Q, V the chain would first have it in.
// The one text of the PD law, the clamp, the Euler update and the NaN rule for every chain: what the instantiations differ in is
// switched at compile time by the constants of Args, and each instantiation compiles to the instructions of the kernel that was
// written out for it before (DESIGN.md 8d has the comparison).  The text stands in the kernel, not in a function the kernels
// call, and no switch is a run-time one: either reshapes the recursion.  contact_step_kernel and fd_kernel keep their own text,
// as their comments say.
template <int W, class Args>
__global__ __launch_bounds__(W) void contact_chain_kernel(const Model* __restrict__ mp, const Args p) {
    extern __shared__ float body[];                       // [joint][CT_SLOTS][W], under the implicit integrator the triangle [entry][W], then the law
    const Model& m = *mp;
    const int n = m.n, nu = m.nu, base = n - nu;
    [[maybe_unused]] const int nf3 = 3 * m.nf;
    float* const behind = body + n * CT_SLOTS * W;
    ContactCfg* cfg = reinterpret_cast<ContactCfg*>(Args::implicit ? behind + (n * (n + 1) / 2) * W : behind);
    [[maybe_unused]] Payload* load = nullptr;             // Args::payloads: the lane's payload, beside its law
    [[maybe_unused]] Actuator* drive = nullptr;           // Args::actuators: the lane's actuator, beside the two
    if constexpr (Args::actuators) {
        LaneDrive* const lane = reinterpret_cast<LaneDrive*>(cfg) + threadIdx.x;
        cfg = &lane->c; load = &lane->load; drive = &lane->drive;
    } else if constexpr (Args::payloads) {
        LaneLoad* const lane = reinterpret_cast<LaneLoad*>(cfg) + threadIdx.x;
        cfg = &lane->c; load = &lane->load;
    } else if constexpr (Args::grounds) {
        cfg += threadIdx.x;                               // the lane's own slot, which nobody else reads: no barrier
    } else {
        if (threadIdx.x == 0) *cfg = p.c;
        __syncthreads();
    }
    const int b = blockIdx.x * W + threadIdx.x;
    if (b >= p.B) return;
    if (p.skip && (p.skip[b] & p.skip_mask)) return;
    if constexpr (Args::actuators) {
        *cfg = p.rows ? ground_row(p.rows, b) : p.c;
        *load = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.payload_rows) {
            const float* r = p.payload_rows + (size_t)b * 4;
            *load = {r[0], r[1], r[2], r[3]};
        }
        const float* r = p.actuator_rows + (size_t)b * 4;
        *drive = {r[0], r[1], r[2], r[3]};
    } else if constexpr (Args::payloads) {
        *cfg = p.rows ? ground_row(p.rows, b) : p.c;
        const float* r = p.payload_rows + (size_t)b * 4;
        *load = {r[0], r[1], r[2], r[3]};
    } else if constexpr (Args::grounds) {
        *cfg = ground_row(p.rows, b);
    }
    const Slice<CT_SLOTS, W> at;
    float* qb = p.q + (size_t)b * n;
    float* vb = p.v + (size_t)b * n;
    const float *qi = qb, *vi = vb;
    const float* tb = p.tau ? p.tau + (size_t)b * nu : nullptr;
    [[maybe_unused]] float *fo = nullptr, *to = nullptr;
    [[maybe_unused]] V3 F;                                // set where Args has a push
    [[maybe_unused]] long long push_lo = 0, push_hi = 0;
    if constexpr (Args::step_io) {
        if (p.q_in) qi = p.q_in + (size_t)b * n;
        if (p.v_in) vi = p.v_in + (size_t)b * n;
        fo = p.f_out ? p.f_out + (size_t)b * nf3 : nullptr;
        to = p.tau_out ? p.tau_out + (size_t)b * nu : nullptr;
    }
    constexpr bool stated = Args::forces == Forces::windowed || Args::grounds;      // the window as ImplicitArgs states it
    if constexpr (!stated && (Args::forces == Forces::pushed || Args::forces == Forces::either)) F = v3(p.force + (size_t)b * 3);
    if constexpr (!stated && Args::forces == Forces::either) { push_lo = (long long)p.first[b] - p.s0; push_hi = push_lo + p.count[b]; }      // count <= 0: never pushed
    if constexpr (stated) {
        F = p.force ? v3(p.force + (size_t)b * 3) : V3{0, 0, 0};
        push_lo = p.push_lo; push_hi = p.push_hi;
        if (p.win_first) { push_lo = (long long)p.win_first[b] - p.win_s0; push_hi = push_lo + p.win_count[b]; }
    }
    // the gains of the PD law: the call's, under Args::actuators the lane's (read where they lie, as the law is)
    const auto kp = [&]() -> float { if constexpr (Args::actuators) return drive->kp; else return p.kp; };
    const auto kd = [&]() -> float { if constexpr (Args::actuators) return drive->kd; else return p.kd; };
    const float nan = __builtin_nanf("");
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = 0; i < n; ++i) { at(i, FD_Q) = qi[i]; at(i, FD_Q + 1) = vi[i]; }
    bool sound = true;                                    // of the last control step
    for (int k = 0; k < p.n_steps; ++k) {
        if (p.Q) {
            float* Qk = p.Q + ((size_t)b * p.qv_rows + k) * n;
            float* Vk = p.V + ((size_t)b * p.qv_rows + k) * n;
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < n; ++i) { Qk[i] = at(i, FD_Q); Vk[i] = at(i, FD_Q + 1); }
        }
        const float* db = !Args::step_io || p.A ? p.A + ((size_t)b * p.a_rows + k) * nu : nullptr;
        sound = true;
        for (int s = 0; s < p.n_sub; ++s) {
            [[maybe_unused]] const bool last = k == p.n_steps - 1 && s == p.n_sub - 1;
            [[maybe_unused]] const long long sub = (long long)k * p.n_sub + s;
            [[maybe_unused]] bool on = false;             // Forces::windowed: is this substep pushed
            if constexpr (Args::forces == Forces::windowed) on = p.force && sub >= push_lo && sub < push_hi;
            [[maybe_unused]] unsigned unclamped = 0;     // bit i: the clamp did not cut the PD torque of joint i
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < n; ++i) {
                float t = 0.0f;
                if (i >= base) {
                    t = tb ? tb[i - base] : 0.0f;
                    if (!Args::step_io || db) t = t + kp() * (db[i - base] - at(i, FD_Q)) + kd() * (0.0f - at(i, FD_Q + 1));
                    const float lim = cfg->tau_max;
                    if constexpr (Args::implicit)
                        if (db && (!(lim > 0.0f) || fabsf(t) < lim)) unclamped |= 1u << i;
                    if (lim > 0.0f) t = t > lim ? lim : (t < -lim ? -lim : t);      // a NaN stays NaN
                    if constexpr (Args::step_io)
                        if (last && to) to[i - base] = t;
                    if constexpr (Args::actuators) t = t - drive->damping * at(i, FD_Q + 1);      // passive: after the clamp, never cut by it
                }
                at(i, FD_Q + 2) = t;
            }
            if constexpr (Args::actuators && Args::forces == Forces::either) {
                if (sub >= push_lo && sub < push_hi)
                    sound = fd_accel_body<W, CT_SLOTS>(m, Driven<Loaded<PushedGroundForces>>{{{{cfg, last ? fo : nullptr}, F, p.joint}, load, p.payload_joint}, drive, base}) && sound;
                else
                    sound = fd_accel_body<W, CT_SLOTS>(m, Driven<Loaded<GroundForces>>{{{cfg, last ? fo : nullptr}, load, p.payload_joint}, drive, base}) && sound;
            } else if constexpr (Args::actuators) {
                sound = fd_accel_body<W, CT_SLOTS>(m, Driven<Loaded<WindowedPushForces>>{{{{{cfg, last ? fo : nullptr}, F, p.joint}, on}, load, p.payload_joint}, drive, base}) && sound;
            } else if constexpr (Args::payloads && Args::forces == Forces::either) {
                if (sub >= push_lo && sub < push_hi)
                    sound = fd_accel_body<W, CT_SLOTS>(m, Loaded<PushedGroundForces>{{{cfg, last ? fo : nullptr}, F, p.joint}, load, p.payload_joint}) && sound;
                else
                    sound = fd_accel_body<W, CT_SLOTS>(m, Loaded<GroundForces>{{cfg, last ? fo : nullptr}, load, p.payload_joint}) && sound;
            } else if constexpr (Args::payloads) {
                sound = fd_accel_body<W, CT_SLOTS>(m, Loaded<WindowedPushForces>{{{{cfg, last ? fo : nullptr}, F, p.joint}, on}, load, p.payload_joint}) && sound;
            } else if constexpr (Args::forces == Forces::ground) {
                sound = fd_accel_body<W, CT_SLOTS>(m, GroundForces{cfg, nullptr}) && sound;
            } else if constexpr (Args::forces == Forces::pushed) {
                sound = fd_accel_body<W, CT_SLOTS>(m, PushedGroundForces{{cfg, last ? fo : nullptr}, F, p.joint}) && sound;
            } else if constexpr (Args::forces == Forces::either) {
                if (sub >= push_lo && sub < push_hi)
                    sound = fd_accel_body<W, CT_SLOTS>(m, PushedGroundForces{{cfg, last ? fo : nullptr}, F, p.joint}) && sound;
                else
                    sound = fd_accel_body<W, CT_SLOTS>(m, GroundForces{cfg, last ? fo : nullptr}) && sound;
            } else {
                sound = fd_accel_body<W, CT_SLOTS>(m, WindowedPushForces{{{cfg, last ? fo : nullptr}, F, p.joint}, on}) && sound;
            }
            if constexpr (Args::implicit && Args::actuators)
                sound = implicit_accel_body<W>(m, *cfg, Triangle<W>{behind}, p.dt, kp(), kd(), unclamped, LaneDriven{{load, p.payload_joint}, drive}) && sound;
            else if constexpr (Args::implicit && Args::payloads)
                sound = implicit_accel_body<W>(m, *cfg, Triangle<W>{behind}, p.dt, kp(), kd(), unclamped, LaneLoaded{load, p.payload_joint}) && sound;
            else if constexpr (Args::implicit)
                sound = implicit_accel_body<W>(m, *cfg, Triangle<W>{behind}, p.dt, kp(), kd(), unclamped) && sound;
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < n; ++i) {
                const float v = at(i, FD_Q + 1) + p.dt * at(i, FD_Q + 2);
                at(i, FD_Q + 1) = v;
                at(i, FD_Q) = at(i, FD_Q) + p.dt * v;
            }
        }
        if (!sound) {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < n; ++i) { at(i, FD_Q) = nan; at(i, FD_Q + 1) = nan; }
        }
    }
    // the state, and for the step the outputs of the last substep: NaN rows where the last control step was unsound
#pragma clang loop unroll(disable) vectorize(disable)
    for (int i = 0; i < n; ++i) {
        if constexpr (Args::step_io)
            if (p.a_out) p.a_out[(size_t)b * n + i] = sound ? at(i, FD_Q + 2) : nan;
        qb[i] = at(i, FD_Q); vb[i] = at(i, FD_Q + 1);
    }
    if constexpr (Args::step_io) {
        if (!sound) {
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; fo && i < nf3; ++i) fo[i] = nan;
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; to && i < nu; ++i) to[i] = nan;
        }
    }
}

