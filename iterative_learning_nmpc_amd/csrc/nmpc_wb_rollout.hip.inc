// nmpc_wb_rollout.hip.inc -- device-resident receding-horizon rollouts of the whole-body model (the reference's own problem).
//
// LocomotionMPC.open_loop (mpc_controller/mpc.py:416-462) for B rollouts from ONE host call, every replanning step
//   nmpc_wb_rollout_prepare_kernel   what `optimize` hands to `solver.init` (mpc.py:325-366, solver.py:153-252,355-394):
//                                    contact and peak windows of the gait table (contact_planner.py:121-149) with the
//                                    node-0 rule of setup_initial_feet_pos (solver.py:194-210), base references with the
//                                    reference's quantisation (mpc.py:210-272), joint / swing / force references, x0 with the
//                                    momentum slots of the current state (pin_data.hg, solver.py:187), plane points with the
//                                    stance feet anchored where forward kinematics puts them; first solve: X = [x0, 0 ...], U = 0
//   nmpc_wb_linearize_kernel / nmpc_wb_qp_kernel       the solve, warm-start shift folded in (15 SQP iterations first)
//   nmpc_wb_rollout_advance_kernel   the plan up-sampled to the simulation rate by cubic Hermite segments through
//                                    (q_k, v_k) and (v_k, a_{k-1}) (interpolate_trajectory_with_derivatives, mpc.py:388-414),
//                                    followed as if it were the plant for `replanning_steps` steps; recorded rows in the
//                                    reference's 44-slot layout [phase, v_mj(18), q_mj[2:](17), base_wrt_feet(8)]
//                                    (DAgger/utils/RolloutMPC.py:221; MuJoCo layout: dynamics.py:75-98), unsafe-state flags
//                                    incl. joint limits (Rollout_combined_controller.py:367-431), early termination, base push,
//                                    reference integration (mpc.py:204-208); with a contact plant attached
//                                    (nmpc_wb_rollout_set_plant) the torque layer has moved the plant and written the rows, and
//                                    the kernel only keeps the flags, applies the push and integrates the reference
// What the two plants share -- the arguments of a rollout step, the fp64 base references, the contact window, the unsafe-state
// predicates, the bookkeeping of failed[b], the push and the reference integration -- is in nmpc_rollout_common.hpp; here are
// forward kinematics, momentum, the 44-slot row, the joint limits and the label hold kernel, and what the prepare kernel shares
// with the labeller's (nmpc_wb_label.hip.inc): the measured state and the write-out of a gathered problem.  Included by nmpc_api.hip.

#include "nmpc_rollout_common.hpp"
#include "nmpc_wb_plan.hpp"

#pragma clang fp contract(off)

namespace nmpc {
namespace wb {

struct WbRolloutArgs : RolloutCommon {
    int force_gravity;
    float step_height;
    ModelParams mp;
    const signed char* peaks;             // dev [4][npc] swing-peak table
    float *q, *v;                         // dev [B][18] plant state, Euler layout (q = r, yaw, pitch, roll, joints; v = qdot)
    const float* joint_ref;               // dev [12]
    float* x0;                            // dev initial states of the solve (momentum slots included)
    int plant;                            // 0: plant = plan; 1: the contact plant has moved q, v and written this replan's rows and
                                          // flags (nmpc_wb_rollout_set_plant), the kernel keeps the books only
};

// foot positions in the world, [4][3], and the centroidal momentum of (q, v), in fp64 like the host helpers
// (wholebody.feet_position_w / centroidal_momentum: the declared model of DESIGN.md 3.2)
__device__ inline void wb_feet_world(const ModelParams& mp, const double* q, double (&p)[12]) {
    double R[9];
    rpy_matrix(q[5], q[4], q[3], R);
    for (int f = 0; f < 4; ++f) {
        const double sgx = (f < 2) ? 1.0 : -1.0, sgy = (f & 1) ? -1.0 : 1.0;
        const double q1 = q[6 + 3 * f], q2 = q[7 + 3 * f], q3 = q[8 + 3 * f];
        const double vx = -(double)mp.l1 * sin(q2) - (double)mp.l2 * sin(q2 + q3);
        const double vz = -(double)mp.l1 * cos(q2) - (double)mp.l2 * cos(q2 + q3);
        const double d = sgy * (double)mp.lhip;
        const double bb[3] = {sgx * (double)mp.hipx + vx, sgy * (double)mp.hipy + d * cos(q1) - vz * sin(q1), d * sin(q1) + vz * cos(q1)};
        for (int i = 0; i < 3; ++i) p[3 * f + i] = q[i] + (R[3 * i] * bb[0] + R[3 * i + 1] * bb[1] + R[3 * i + 2] * bb[2]);
    }
}
__device__ inline void wb_body_rates(const double* q, const double* v, double (&w)[3]) {      // E(theta) thetadot (transform.py:80-86)
    const double sy = sin(q[4]), cy = cos(q[4]), sx = sin(q[5]), cx = cos(q[5]);
    w[0] = -sy * v[3] + v[5];
    w[1] = cy * sx * v[3] + cx * v[4];
    w[2] = cx * cy * v[3] - sx * v[4];
}
__device__ inline void wb_momentum(const ModelParams& mp, const double* q, const double* v, double (&h)[6]) {
    double R[9], w[3];
    rpy_matrix(q[5], q[4], q[3], R);
    wb_body_rates(q, v, w);
    const double Iw[3] = {(double)mp.ixx * w[0], (double)mp.iyy * w[1], (double)mp.izz * w[2]};
    for (int i = 0; i < 3; ++i) {
        h[i] = (double)mp.mass * v[i];
        h[3 + i] = R[3 * i] * Iw[0] + R[3 * i + 1] * Iw[1] + R[3 * i + 2] * Iw[2];
    }
}

// What a block gathers of one problem before it writes it out -- the rollout's prepare kernel below and the labeller's
// (nmpc_wb_label.hip.inc) fill it from different places and write it with one text.
struct WbProblem {
    float ref[12], ref_e[12], cflag[4 * 65], pflag[4 * 65], fshare[65], x0s[NX], feet[12];
    int first_swing[4];
};
struct WbProblemOut {                     // the problem's own slices of the tensors of the solve
    float *yref, *yref_e, *params, *x0, *X, *U;
};

// x0 = [q, v, h_g(q, v)] and the feet of the plant state (qf, vf), by one thread
__device__ inline void wb_measured_state(const ModelParams& mp, const float* qf, const float* vf, WbProblem& P) {
    double q[18], v[18], p[12], h[6];
    for (int i = 0; i < 18; ++i) { q[i] = qf[i]; v[i] = vf[i]; }
    wb_feet_world(mp, q, p);
    wb_momentum(mp, q, v, h);
    for (int i = 0; i < 12; ++i) P.feet[i] = (float)p[i];
    for (int i = 0; i < 18; ++i) { P.x0s[WQ + i] = qf[i]; P.x0s[WV + i] = vf[i]; }
    for (int i = 0; i < 6; ++i) P.x0s[WH + i] = (float)h[i];
}

// references, parameters, x0 and node 0 of the guess from a gathered problem, by the 64 threads of its block; cold: the rest of the
// guess is zero.  Synchronises first: the caller has filled ref, ref_e, the windows, x0s and feet.
__device__ inline void wb_write_problem(WbProblem& P, int tid, int N, const float* joint_ref, float step_height, int force_gravity,
                                        float height_offset, bool cold, const WbProblemOut& o) {
    __syncthreads();
    if (tid < 4) {      // a foot in contact at node 0 keeps its position up to its next swing node; np.argmin: never swings -> 0 nodes
        int fs = 0;
        if (P.cflag[tid * 65] > 0.5f) {
            for (int k = 0; k <= N; ++k)
                if (P.cflag[tid * 65 + k] < 0.5f) { fs = k; break; }
        }
        P.first_swing[tid] = fs;
    }
    __syncthreads();
    for (int e = tid; e < N * NY; e += 64) {
        const int k = e / NY, i = e - k * NY;
        float val = 0.0f;
        if (i < RY_JOINT) val = P.ref[i];                                                   // base (12)
        else if (i < RY_JOINT + 12) val = joint_ref[i - RY_JOINT];                          // joint positions; rates 0 (solver.py:175-177)
        else if (i >= RY_SWING && i < RY_FREG) val = step_height;                           // swing height (solver.py:170)
        else if (i >= RY_FREG && i < RY_CNT && force_gravity && (i - RY_FREG) % 3 == 2)     // [decl] option: weight share instead of the reference's zero
            val = P.cflag[((i - RY_FREG) / 3) * 65 + k] * P.fshare[k];
        o.yref[e] = val;
    }
    for (int i = tid; i < NYE; i += 64) {
        float val = 0.0f;
        if (i < RE_JOINT) val = P.ref_e[i];
        else if (i < RE_JOINT + 12) val = joint_ref[i - RE_JOINT];
        else if (i >= RE_SWING && i < RE_CNT) val = step_height;
        o.yref_e[i] = val;
    }
    for (int e = tid; e < (N + 1) * NP; e += 64) {
        const int k = e / NP, i = e - k * NP;
        float val;
        if (i < 4) val = P.cflag[i * 65 + k];
        else if (i < 8) val = P.pflag[(i - 4) * 65 + k];
        else {
            const int f = (i - 8) / 3, c = (i - 8) % 3;
            val = (k < P.first_swing[f]) ? P.feet[3 * f + c] : (c == 2 ? height_offset : 0.0f);     // solver.py:212-225,194-210
        }
        o.params[e] = val;
    }
    if (tid < NX) {
        o.x0[tid] = P.x0s[tid];
        // set_initial_state: node 0 of the guess is the measured state (a fixed point of the warm-start shift map)
        o.X[tid] = P.x0s[tid];
    }
    if (cold) {         // first solve: the views are zero but for node 0 (solver.py:386-388: no warm start)
        for (int e = NX + tid; e < (N + 1) * NX; e += 64) o.X[e] = 0.0f;
        for (int e = tid; e < N * NU; e += 64) o.U[e] = 0.0f;
    }
}

// one block (64 threads) per rollout
__global__ __launch_bounds__(64) void nmpc_wb_rollout_prepare_kernel(const WbRolloutArgs a) {
    __shared__ WbProblem P;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    if (a.failed[b] & a.term_mask) return;
    const float* qf = a.q + (size_t)b * 18;
    const float* vf = a.v + (size_t)b * 18;
    if (tid == 0) {
        base_ref_vel_tracking_dev((double)qf[0], (double)qf[1], (double)qf[3], a.ref_state + (size_t)b * 12, a.v_des + (size_t)b * 3,
                                  a.w_des + (size_t)b * 3, a.t_horizon, a.nom_height + a.height_offset, P.ref, P.ref_e);
    } else if (tid == 1) {
        wb_measured_state(a.mp, qf, vf, P);
    }
    contact_window<65>(a, tid, a.peaks, true, -a.mp.gz * a.mp.mass, P.cflag, P.pflag, P.fshare);
    wb_write_problem(P, tid, N, a.joint_ref, a.step_height, a.force_gravity, (float)a.height_offset, a.first != 0,
                     {a.yref + (size_t)b * N * NY, a.yref_e + (size_t)b * NYE, a.params + (size_t)b * (N + 1) * NP,
                      a.x0 + (size_t)b * NX, a.X + (size_t)b * (N + 1) * NX, a.U + (size_t)b * N * NU});
}

// one thread per rollout
__global__ void nmpc_wb_rollout_advance_kernel(const WbRolloutArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int N = a.N;
    float* qf = a.q + (size_t)b * 18;
    float* vf = a.v + (size_t)b * 18;
    const float* Xb = a.X + (size_t)b * (N + 1) * NX;
    const float* Ub = a.U + (size_t)b * N * NU;
    int flags = a.failed[b];
    const int rows_per_replan = a.record_sim_steps ? a.replanning_steps : 1;
    float* rows = a.S + ((size_t)b * a.n_rows + a.row0) * 44;
    const double period = (double)a.nominal_period;
    // the 44-slot row of a state (q, v in the Euler layout): MuJoCo velocities (body rates), z, quaternion (w, x, y, z), joints,
    // base_wrt_feet from forward kinematics; and the unsafe-state predicates on it
    auto record = [&](float* row, double phase, const double* q, const double* v) {
        double w[3], p[12];
        wb_body_rates(q, v, w);
        wb_feet_world(a.mp, q, p);
        const double cy = cos(0.5 * q[3]), sy = sin(0.5 * q[3]), cp = cos(0.5 * q[4]), sp = sin(0.5 * q[4]), cr = cos(0.5 * q[5]), sr = sin(0.5 * q[5]);
        double qw = cy * cp * cr + sy * sp * sr, qx = cy * cp * sr - sy * sp * cr, qy = cy * sp * cr + sy * cp * sr, qz = sy * cp * cr - cy * sp * sr;
        if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }          // Eigen's matrix -> quaternion conversion returns w >= 0
        row[0] = (float)phase;
        for (int i = 0; i < 3; ++i) { row[1 + i] = (float)v[i]; row[4 + i] = (float)w[i]; }
        for (int i = 0; i < 12; ++i) row[7 + i] = (float)v[6 + i];
        row[19] = (float)q[2];
        row[20] = (float)qw; row[21] = (float)qx; row[22] = (float)qy; row[23] = (float)qz;
        for (int i = 0; i < 12; ++i) row[24 + i] = (float)q[6 + i];
        for (int f = 0; f < 4; ++f) { row[36 + 2 * f] = (float)(q[0] - p[3 * f]); row[37 + 2 * f] = (float)(q[1] - p[3 * f + 1]); }
        flags |= unsafe_state_flags((float)q[5], (float)q[4], (float)q[2], (float)v[0], (float)v[1], a.v_des + b * 3, a.collision_height);
        for (int f = 0; f < 4; ++f) {       // joint limits in degrees: hip +-70, thigh [25, 115], knee [-155, -60]
            const float dg = 57.29577951308232f;
            const float hip = (float)q[6 + 3 * f] * dg, th = (float)q[7 + 3 * f] * dg, kn = (float)q[8 + 3 * f] * dg;
            if (!(hip >= -70.0f && hip <= 70.0f) || !(th >= 25.0f && th <= 115.0f) || !(kn >= -155.0f && kn <= -60.0f))
                flags |= NMPC_ROLLOUT_FLAG_JOINT_LIMIT;
        }
    };
    // terminated in an earlier replan; in plant mode this replan's observation has already raised its flags, so there only a
    // stamp tells an earlier termination from one of this replan
    const bool earlier = a.plant ? (flags & a.term_mask) && (flags >> NMPC_ROLLOUT_TERM_SHIFT) : (flags & a.term_mask) != 0;
    if (earlier) {                         // frozen (hold_last_row)
        if (a.row0 > 0) {
            hold_last_row(rows, 44, rows_per_replan);
        } else {                           // a call that continues an already terminated rollout: its frozen state
            double q[18], v[18];
            for (int i = 0; i < 18; ++i) { q[i] = qf[i]; v[i] = vf[i]; }
            const int keep = flags;
            for (int j = 0; j < rows_per_replan; ++j) record(rows + j * 44, 0.0, q, v);
            flags = keep;
        }
        return;
    }
    flags |= solver_status_flag(a.status[b]);
    if (a.plant) {                         // the rows are written and the plant has moved: the books, the push and the reference
        if (commit_flags(a, b, flags)) return;
        apply_push(vf, a, b, a.mp.mass);
        integrate_base_reference(a, b);
        return;
    }
    // the plan at time t of the horizon (nmpc_wb_plan.hpp: the Hermite segments of mpc.py:388-414, shared with the label kernel)
    auto plan_at = [&](double t, double (&q)[18], double (&v)[18]) { wb_plan_at(Xb, Ub, N, a.dt_nodes, t, q, v); };
    double q[18], v[18];
    if (!a.record_sim_steps) {
        for (int i = 0; i < 18; ++i) { q[i] = qf[i]; v[i] = vf[i]; }
        const double tw = (long long)a.replan_index * a.replanning_steps * a.sim_dt;      // (a continued rollout's index: no int product)
        record(rows, recorded_phase(tw, period), q, v);       // the state this replan started from
    } else {
        for (int j = 0; j < a.replanning_steps; ++j) {                              // the states the plant runs through
            plan_at((j + 1) * a.sim_dt, q, v);
            const double tw = ((long long)a.replan_index * a.replanning_steps + j + 1) * a.sim_dt;
            record(rows + j * 44, recorded_phase(tw, period), q, v);
        }
    }
    if (commit_flags(a, b, flags)) return;       // terminated by this replan's rows: frozen from here on
    // plant = plan, `replanning_steps` simulation steps on
    plan_at(a.replanning_steps * a.sim_dt, q, v);
    for (int i = 0; i < 18; ++i) { qf[i] = (float)q[i]; vf[i] = (float)v[i]; }
    apply_push(vf, a, b, a.mp.mass);
    integrate_base_reference(a, b);
}

// Labels (nmpc_wb_rollout_set_actions) of the rollouts that terminated before this replan: their last written label row,
// repeated (zeros if they have none) -- what the advance kernel does with their rows of S.  One thread per element.
__global__ void nmpc_wb_rollout_hold_actions_kernel(int B, int n_rows, int row0, int rows, int term_mask, const int* __restrict__ failed,
                                                    float* __restrict__ A) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = (size_t)rows * 12;
    if (e >= (size_t)B * per) return;
    const size_t b = e / per, r = e - b * per;
    if (!(failed[b] & term_mask)) return;
    float* Ab = A + (b * n_rows + row0) * 12;
    Ab[r] = row0 > 0 ? Ab[(ptrdiff_t)(r % 12) - 12] : 0.0f;
}

// The push windows of the rollouts (nmpc_wb_rollout_set_push_windows, seconds) in substeps of the plant, for a push as a force:
// the expressions the host has for the cfg's one window (nmpc_wb_rollout_batch), per rollout, once at the entry of a rollout.
__global__ void nmpc_wb_push_substeps_kernel(int B, const float* __restrict__ start, const float* __restrict__ duration, int n_sub,
                                             double sim_dt, int* __restrict__ first, int* __restrict__ count) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    first[b] = (int)lround((double)start[b] * n_sub / sim_dt);
    const int n = (int)lround((double)duration[b] * n_sub / sim_dt);
    count[b] = n < 0 ? 0 : n;
}

}  // namespace wb
}  // namespace nmpc
