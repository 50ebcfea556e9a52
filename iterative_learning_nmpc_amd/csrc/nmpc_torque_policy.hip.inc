// nmpc_torque_policy.hip.inc -- the observation of a plant state on the ground-contact plant: of one state per robot for the
// policy-driven rollout (nmpc_observe_batch, and through it nmpc_policy_rollout_batch, of include/nmpc_torque.h) and of the rows
// of a table of states (nmpc_observe_rows_batch); included by nmpc_torque.hip inside namespace nmpc_torque, after
// nmpc_torque_contact.hip.inc.
//
// The plant state (q, v [18] in the solver's Euler layout [x y z yaw pitch roll joints]) becomes the reference's 44-slot state
// row (RolloutMPC.py:221; the layout of `record` in nmpc_wb_rollout.hip.inc), the policy input made of it, and the fall
// predicates.  The feet of base_wrt_feet are the tree's own -- the points the contact law pushes --, so the kernel runs the
// outward pass of foot_kernel (a copy without the velocities, DESIGN.md 8d: Rw and the world position of the body origins, 12 slots), not
// the closed-form geometry of the whole-body model.  One thread per robot, LDS slice [joint][OB_SLOTS][TPB].
#pragma once

constexpr int OB_RW = 0;     // Rw 9
constexpr int OB_PW = 9;     // world position of the body origin 3
constexpr int OB_SLOTS = 12;
constexpr int OB_STATE = 44; // slots of a state row
constexpr size_t ob_lds_bytes(int n) { return (size_t)n * OB_SLOTS * TPB * sizeof(float); }

// ---- the arguments of the observation, one struct per instantiation of observe_kernel -------------------------------------
// nmpc_observe_batch: one state per robot, its row and the policy input made of it
struct ObserveArgs {
    static constexpr bool rows = false;
    int B, n_goal, s_first, s_stride, step_index, term_mask;
    double t, period;
    float collision_height;
    const float *q, *v, *goal;
    const double *s_mean, *s_std;                         // both or neither
    float *S, *X;                                         // each may be nullptr
    int* failed;                                          // may be nullptr
};

// nmpc_observe_rows_batch: the rows of a table of states per robot (the states a chain of control steps ran through,
// nmpc_torque_track.hip.inc), no policy input, robots left out by skip flags
struct ObserveRowsArgs {
    static constexpr bool rows = true;
    int B, n_rows, qv_rows, s_rows, step_index, term_mask, skip_mask;
    double t0, dt_row, period;
    float collision_height;
    const float *Q, *V;                                   // row k of robot b at + (b * qv_rows + k) * 18
    float* S;                                             // row k of robot b at + (b * s_rows + k) * 44; may be nullptr
    int* failed;                                          // may be nullptr
    const int* skip;
};

// the time of row k, in the two roundings of the host expression t0 + k * dt_row
__device__ inline double row_time(double t0, int k, double dt_row) {
#pragma clang fp contract(off)
    const double d = (double)k * dt_row;
    return t0 + d;
}

// The one text of the outward pass, the 44-slot row, the fall predicates and the joint limits.  What the two instantiations differ
// in is switched at compile time by Args::rows: a table of rows per robot with skip flags, or a single state with the policy
// input X (normalised from s_first on, the goal behind it).  The flags of all rows are gathered in a register and the stamp is
// set once after them, which is what n_rows calls with one step index leave (the first call that sees a terminating bit stamps,
// the later ones find the stamp); with the single state that is read, stamp and write.  The text stands in the kernel, as
// contact_chain_kernel's (nmpc_torque_track.hip.inc); DESIGN.md 8d has the comparison with the two kernels written out before.
template <class Args>
__global__ __launch_bounds__(TPB) void observe_kernel(const Model* __restrict__ mp, const Args a) {
    const Model& m = *mp;
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= a.B) return;
    if constexpr (Args::rows)
        if (a.skip && (a.skip[b] & a.skip_mask)) return;
    const int n = m.n;
    const Slice<OB_SLOTS, TPB> at;
    int flags = a.failed ? a.failed[b] : 0;
    int n_rows = 1;
    if constexpr (Args::rows) n_rows = a.n_rows;
    for (int r = 0; r < n_rows; ++r) {
        const float *qb, *vb;
        bool wanted;                                      // is a row, or a policy input, made of this state
        if constexpr (Args::rows) {
            qb = a.Q + ((size_t)b * a.qv_rows + r) * n;
            vb = a.V + ((size_t)b * a.qv_rows + r) * n;
            wanted = a.S;
        } else {
            qb = a.q + (size_t)b * n;
            vb = a.v + (size_t)b * n;
            wanted = a.S || a.X;
        }
        if (wanted) {
            float* Sb;
            [[maybe_unused]] float* Xb = nullptr;
            if constexpr (Args::rows) {
                Sb = a.S + ((size_t)b * a.s_rows + r) * OB_STATE;
            } else {
                Sb = a.S ? a.S + (size_t)b * a.s_stride : nullptr;
                Xb = a.X ? a.X + (size_t)b * (OB_STATE + a.n_goal) : nullptr;
            }
            // slot j of the row, and of the policy input: nmpc_batch::write_element's expression on the fp32 value the row holds
            auto put = [&](int j, float s) {
                if constexpr (Args::rows) {
                    Sb[j] = s;
                } else {
                    if (Sb) Sb[j] = s;
                    if (Xb) Xb[j] = (a.s_mean && j >= a.s_first) ? (float)(((double)s - a.s_mean[j]) / a.s_std[j]) : s;
                }
            };
            // the outward pass of foot_kernel, positions only
            for (int i = 0; i < n; ++i) {
                M3 R; V3 p;
                joint_transform(m, i, qb[i], R, p);
                const int par = m.parent[i];
                V3 pw = p;
                M3 Rw = R;
                if (par >= 0) {
                    M3 Rp;
#pragma unroll
                    for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, OB_RW + k);
                    Rw = mul(Rp, R);
                    pw = at.get3(par, OB_PW) + mul(Rp, p);
                }
#pragma unroll
                for (int k = 0; k < 9; ++k) at(i, OB_RW + k) = Rw.m[k];
                at.put3(i, OB_PW, pw);
            }
            // the row: [phase, v_lin 3, body rates 3, joint rates 12, z, quaternion wxyz (w >= 0) 4, joints 12, base_wrt_feet 8]
            if constexpr (Args::rows) put(0, (float)nmpc::recorded_phase(row_time(a.t0, r, a.dt_row), a.period));
            else put(0, (float)nmpc::recorded_phase(a.t, a.period));
            {   // E(theta) thetadot (wb_body_rates) and the quaternion of `record`, in fp64 from the fp32 state
                const double yaw = qb[3], pitch = qb[4], roll = qb[5], dyaw = vb[3], dpitch = vb[4], droll = vb[5];
                const double sy = sin(pitch), cy = cos(pitch), sx = sin(roll), cx = cos(roll);
                put(4, (float)(-sy * dyaw + droll));
                put(5, (float)(cy * sx * dyaw + cx * dpitch));
                put(6, (float)(cx * cy * dyaw - sx * dpitch));
                const double hy = cos(0.5 * yaw), ky = sin(0.5 * yaw), hp = cos(0.5 * pitch), kp = sin(0.5 * pitch), hr = cos(0.5 * roll), kr = sin(0.5 * roll);
                double qw = hy * hp * hr + ky * kp * kr, qx = hy * hp * kr - ky * kp * hr, qy = hy * kp * hr + ky * hp * kr, qz = ky * hp * hr - hy * kp * kr;
                if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
                put(20, (float)qw); put(21, (float)qx); put(22, (float)qy); put(23, (float)qz);
            }
            put(19, qb[2]);
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < 3; ++i) put(1 + i, vb[i]);
#pragma clang loop unroll(disable) vectorize(disable)
            for (int i = 0; i < 12; ++i) { put(7 + i, vb[6 + i]); put(24 + i, qb[6 + i]); }
#pragma clang loop unroll(disable) vectorize(disable)
            for (int k = 0; k < 4; ++k) {
                const int j = m.foot_joint[k];
                M3 Rw;
#pragma unroll
                for (int e = 0; e < 9; ++e) Rw.m[e] = at(j, OB_RW + e);
                const V3 p = at.get3(j, OB_PW) + mul(Rw, v3(m.foot_offset[k]));
                put(36 + 2 * k, qb[0] - p.x); put(37 + 2 * k, qb[1] - p.y);
            }
            if constexpr (!Args::rows) {
#pragma clang loop unroll(disable) vectorize(disable)
                for (int k = 0; Xb && k < a.n_goal; ++k) Xb[OB_STATE + k] = a.goal[(size_t)b * a.n_goal + k];
            }
        }
        if (a.failed) {
            // the command handed to the predicates is the state's own velocity: the velocity-tracking bit is never raised here
            const double own[2] = {(double)vb[0], (double)vb[1]};
            flags |= nmpc::unsafe_state_flags(qb[5], qb[4], qb[2], vb[0], vb[1], own, a.collision_height);
#pragma clang loop unroll(disable) vectorize(disable)
            for (int f = 0; f < 4; ++f) {       // joint limits in degrees: hip +-70, thigh [25, 115], knee [-155, -60] (the whole-body advance kernel's block)
                const float dg = 57.29577951308232f;
                const float hip = qb[6 + 3 * f] * dg, th = qb[7 + 3 * f] * dg, kn = qb[8 + 3 * f] * dg;
                if (!(hip >= -70.0f && hip <= 70.0f) || !(th >= 25.0f && th <= 115.0f) || !(kn >= -155.0f && kn <= -60.0f))
                    flags |= NMPC_ROLLOUT_FLAG_JOINT_LIMIT;
            }
        }
    }
    if (a.failed) {
        if ((flags & a.term_mask) && !(flags >> NMPC_ROLLOUT_TERM_SHIFT)) flags |= (a.step_index + 1) << NMPC_ROLLOUT_TERM_SHIFT;   // commit_flags' stamp
        a.failed[b] = flags;
    }
}

// row k of the [B][rows][n] tables Q, V from the dense [B][n] plant state (nmpc_policy_rollout_set_states): Q, V point at row k
// of robot 0
__global__ __launch_bounds__(256) void state_rows_kernel(int B, int n, const float* __restrict__ q, const float* __restrict__ v,
                                                         float* __restrict__ Q, float* __restrict__ V, size_t stride) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * n) return;
    const size_t b = e / n, j = b * stride + (e - b * n);
    Q[j] = q[e];
    V[j] = v[e];
}

// row k of a [B][rows][nu] table from the dense [B][nu] actions of one control step: dst points at row k of robot 0
__global__ __launch_bounds__(256) void action_rows_kernel(int B, int nu, const float* __restrict__ src, float* __restrict__ dst, int stride) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * nu) return;
    const size_t b = e / nu;
    dst[b * stride + (e - b * nu)] = src[e];
}
