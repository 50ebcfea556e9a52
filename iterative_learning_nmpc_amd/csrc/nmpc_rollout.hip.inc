// nmpc_rollout.hip.inc -- device-resident receding-horizon rollouts (centroidal model).
//
// The simulator-free rollout of the reference, LocomotionMPC.open_loop (mpc_controller/mpc.py:416-462):
// every replanning step  references -> init -> solve -> follow the plan,  restated so that a whole
// rollout (T/0.04 solves) of B problems runs from ONE host call with no host round trip:
//   nmpc_rollout_prepare_kernel   contact window (contact_planner.py:121-134), base references with the
//                                 reference's quantisation and crossed clips (mpc.py:210-272, in fp64),
//                                 per-stage output references and parameters, first-solve warm start
//   nmpc_shift_kernel / nmpc_linearize_kernel / nmpc_qp_kernel        (the solve path)
//   nmpc_rollout_advance_kernel   record the state row(s) (DAgger/utils/RolloutMPC.py:221 slot order) -- one per
//                                 replan, or one per simulation step with the plan up-sampled by cubic Hermite
//                                 segments (mpc.py:371-414) --, unsafe-state flags
//                                 (Rollout_combined_controller.py:367-446), plant = plan, base push, touch-downs,
//                                 integrate the reference (mpc.py:204-208)
// Footsteps (cfg.footsteps): a foot in contact at the first node keeps its position up to its next swing node
// (setup_initial_feet_pos, solver.py:194-210); every touch-down inside the window gets the Raibert target of
// RaiberContactPlanner.get_locations (contact_planner.py:265-322) from the current base state and command.
// What the two plants share -- the arguments of a rollout step, the fp64 base references, the contact window, the unsafe-state
// predicates, the bookkeeping of failed[b], the push and the reference integration -- is in nmpc_rollout_common.hpp; here are the
// Raibert footstep planner, the fp32 Hermite rows and the 19-slot row of the centroidal plant.  Included by nmpc_api.hip.

#include "nmpc_rollout_common.hpp"

#pragma clang fp contract(off)      // explicit: these kernels are compared bit for bit with their fp32 / fp64 restatements

namespace nmpc {

struct RolloutArgs : RolloutCommon {
    int nodes_per_replan;
    float mass, gz;
    float phase;                          // gait phase recorded with the state row (one row per replan)
    float* x;                             // dev [B][12] plant state
    float* foot_pos;                      // dev [B][4][3] in/out: where each foot last stood / stands
    int footsteps;                        // Raibert footsteps (nmpc_rollout_cfg)
    float hip_offset[8], stance_ratio[4], foot_size;
};

// one block (64 threads) per problem
__global__ __launch_bounds__(64) void nmpc_rollout_prepare_kernel(const RolloutArgs a) {
    __shared__ float ref[12], ref_e[12], cflag[4 * 129], fshare[129];
    __shared__ float floc[4 * 129 * 3];   // per-node foot locations of the plan (footsteps)
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    if (a.failed[b] & a.term_mask) return;       // terminated in an earlier replan: nothing to prepare, the solve skips it
    const float* x = a.x + (size_t)b * 12;
    if (tid == 0)
        base_ref_vel_tracking_dev((double)x[0], (double)x[1], (double)x[3], a.ref_state + (size_t)b * 12, a.v_des + (size_t)b * 3,
                                  a.w_des + (size_t)b * 3, a.t_horizon, a.nom_height + a.height_offset, ref, ref_e);
    contact_window<129>(a, tid, nullptr, false, -a.gz * a.mass, cflag, nullptr, fshare);
    __syncthreads();
    const float* fp = a.foot_pos + (size_t)b * 12;
    if (a.footsteps && tid < 4) {
        // contact_planner.py:265-322 for foot `tid`, in fp64 as the host computes it; then the stance anchoring
        const int f = tid;
        const double com_x = x[0], com_y = x[1], com_z = (double)x[2] - a.height_offset;
        const double vc_x = a.v_des[b * 3], vc_y = a.v_des[b * 3 + 1], w_yaw = a.w_des[b * 3 + 2];
        const double cyw = cos((double)x[3]), syw = sin((double)x[3]);
        const double hx = cyw * a.hip_offset[2 * f] - syw * a.hip_offset[2 * f + 1];
        const double hy = syw * a.hip_offset[2 * f] + cyw * a.hip_offset[2 * f + 1];
        const double ratio = a.stance_ratio[f], t_stance = (double)a.nominal_period * ratio;
        const double lev = 0.5 * sqrt(fmax(com_z, 0.0) / 9.81);   // (the reference's sqrt(com_z / g) is NaN for a base below the ground)
        const double lx = lev * vc_x, ly = lev * vc_y;
        float cur[3] = {0.0f, 0.0f, 0.0f};
        bool anchored = cflag[f * 129] > 0.5f;        // in contact at node 0: keep the position up to the next swing
        // numpy argmin quirk (solver.py:207): a foot in contact over the whole window is not anchored at all
        bool any_swing = false;
        for (int k = 0; k <= N; ++k) any_swing = any_swing || cflag[f * 129 + k] < 0.5f;
        anchored = anchored && any_swing;
        float prev = (float)a.gait[f * a.npc + (a.node + a.npc - 1) % a.npc];
        for (int k = 0; k <= N; ++k) {
            const float c = cflag[f * 129 + k];
            if (c > 0.5f && prev < 0.5f) {            // touch-down node (switch_cnt == 1)
                const double t_touch = rint(k * a.dt_nodes * 1000.0) / 1000.0;
                cur[0] = (float)(com_x + hx + vc_x * t_touch * (1.0 + ratio) + 0.1 * (vc_x - (double)x[6]) + 0.5 * vc_x * t_stance + ly * w_yaw);
                cur[1] = (float)(com_y + hy + vc_y * t_touch * (1.0 + ratio) + 0.1 * (vc_y - (double)x[7]) + 0.5 * vc_y * t_stance - lx * w_yaw);
                cur[2] = a.foot_size;
            }
            if (anchored && c < 0.5f) anchored = false;
            for (int i = 0; i < 3; ++i) floc[(f * 129 + k) * 3 + i] = anchored ? fp[3 * f + i] : cur[i];
            prev = c;
        }
    }
    __syncthreads();
    float* yr = a.yref + (size_t)b * N * 24;
    float* pr = a.params + (size_t)b * (N + 1) * 16;
    for (int e = tid; e < N * 24; e += 64) {
        const int k = e / 24, i = e - k * 24;
        float v = 0.0f;
        if (i < 12) v = ref[i];
        else if ((i - 12) % 3 == 2) v = cflag[((i - 12) / 3) * 129 + k] * fshare[k];
        yr[e] = v;
    }
    for (int e = tid; e < (N + 1) * 16; e += 64) {
        const int k = e / 16, i = e - k * 16;
        pr[e] = (i < 4) ? cflag[i * 129 + k] : a.footsteps ? floc[(((i - 4) / 3) * 129 + k) * 3 + (i - 4) % 3] : fp[i - 4];
    }
    if (tid < 12) a.yref_e[(size_t)b * 12 + tid] = ref_e[tid];
    if (a.first) {   // first solve: X held at the current state, U = force references (solver.py:388: no warm start)
        float* Xb = a.X + (size_t)b * (N + 1) * 12;
        float* Ub = a.U + (size_t)b * N * 12;
        for (int e = tid; e < (N + 1) * 12; e += 64) Xb[e] = x[e % 12];
        for (int e = tid; e < N * 12; e += 64) {
            const int k = e / 12, i = e - k * 12;
            Ub[e] = (i % 3 == 2) ? cflag[(i / 3) * 129 + k] * fshare[k] : 0.0f;
        }
    }
}

// cubic Hermite basis at s in [0, 1] for a segment of length h: value = h00 y0 + h10 h m0 + h01 y1 + h11 h m1
__device__ inline float hermite(float y0, float m0, float y1, float m1, float h, float s) {
    const float s2 = s * s, om = 1.0f - s;
    return (1.0f + 2.0f * s) * om * om * y0 + s * om * om * h * m0 + s2 * (3.0f - 2.0f * s) * y1 + s2 * (s - 1.0f) * h * m1;
}
// Euler-angle rates T(theta) w of a centroidal state (transform.py:72-78); w stored (wz, wy, wx)
__device__ inline void euler_rates(const float* xk, float (&thd)[3]) {
    float sy, cy, sx, cx;
    sincosf(xk[4], &sy, &cy);
    sincosf(xk[5], &sx, &cx);
    const float wx = xk[11], wy = xk[10], wz = xk[9];
    thd[0] = (sx * wy + cx * wz) / cy;
    thd[1] = cx * wy - sx * wz;
    thd[2] = wx + (sx * wy + cx * wz) * sy / cy;
}

// one thread per problem
__global__ void nmpc_rollout_advance_kernel(const RolloutArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    float* x = a.x + (size_t)b * 12;
    float* fp = a.foot_pos + (size_t)b * 12;
    const float* Xb = a.X + (size_t)b * (a.N + 1) * 12;
    const float* pb = a.params + (size_t)b * (a.N + 1) * 16;
    int flags = a.failed[b];
    const int rows_per_replan = a.record_sim_steps ? a.replanning_steps : 1;
    if (flags & a.term_mask) {                     // terminated in an earlier replan: frozen (hold_last_row)
        float* rows = a.S + ((size_t)b * a.n_rows + a.row0) * 19;
        if (a.row0 > 0) {
            hold_last_row(rows, 19, rows_per_replan);
        } else {                                   // a call that continues an already terminated rollout: its frozen state
            float last[19];
            last[0] = a.phase;
            for (int i = 0; i < 3; ++i) { last[1 + i] = x[6 + i]; last[4 + i] = x[9 + i]; }
            for (int i = 0; i < 4; ++i) last[7 + i] = x[2 + i];
            for (int f = 0; f < 4; ++f) { last[11 + 2 * f] = x[0] - fp[3 * f]; last[12 + 2 * f] = x[1] - fp[3 * f + 1]; }
            for (int j = 0; j < rows_per_replan; ++j)
                for (int i = 0; i < 19; ++i) rows[j * 19 + i] = last[i];
        }
        return;
    }
    flags |= solver_status_flag(a.status[b]);
    auto check_state = [&](const float* s12) {
        flags |= unsafe_state_flags(s12[5], s12[4], s12[2], s12[6], s12[7], a.v_des + b * 3, a.collision_height);
    };
    auto write_row = [&](float* row, float phase, const float* s12, int node) {
        row[0] = phase;
        for (int i = 0; i < 3; ++i) { row[1 + i] = s12[6 + i]; row[4 + i] = s12[9 + i]; }
        for (int i = 0; i < 4; ++i) row[7 + i] = s12[2 + i];
        for (int f = 0; f < 4; ++f) {
            // a foot that stands at this node of the plan is where the plan puts it, a swinging one where it last stood
            const bool stands = a.footsteps && pb[node * 16 + f] > 0.5f;
            const float fx = stands ? pb[node * 16 + 4 + 3 * f] : fp[3 * f], fy = stands ? pb[node * 16 + 5 + 3 * f] : fp[3 * f + 1];
            row[11 + 2 * f] = s12[0] - fx;
            row[12 + 2 * f] = s12[1] - fy;
        }
    };
    if (!a.record_sim_steps) {
        write_row(a.S + ((size_t)b * a.n_rows + a.row0) * 19, a.phase, x, 0);
        check_state(x);
    } else {
        // one row per simulation step: the plan up-sampled as the reference does (mpc.py:371-414) -- positions on
        // cubic Hermite segments through (q_k, qdot_k), velocities through (v_k, a_{k-1}) with a_k = (v_{k+1} - v_k)/dt
        // (the reference shifts the accelerations by one node, mpc.py:409-410); sample j is at t = (j + 1) sim_dt
        const float dtn = (float)a.dt_nodes;
        const double period = (double)a.nominal_period;
        for (int j = 0; j < a.replanning_steps; ++j) {
            const double t = (j + 1) * a.sim_dt;
            int k = (int)floor(t / a.dt_nodes + 1e-9);
            if (k > a.N - 1) k = a.N - 1;
            const float s = (float)((t - k * a.dt_nodes) / a.dt_nodes);
            const float* x0 = Xb + (size_t)k * 12;
            const float* x1 = x0 + 12;
            float d0[3], d1[3], s12[12];
            euler_rates(x0, d0);
            euler_rates(x1, d1);
            for (int i = 0; i < 3; ++i) {
                s12[i] = hermite(x0[i], x0[6 + i], x1[i], x1[6 + i], dtn, s);
                s12[3 + i] = hermite(x0[3 + i], d0[i], x1[3 + i], d1[i], dtn, s);
            }
            const int ka = k > 0 ? k - 1 : 0, kb = k;             // acceleration rows used as slopes at nodes k, k+1
            for (int i = 6; i < 12; ++i) {
                const float m0 = (Xb[(size_t)(ka + 1) * 12 + i] - Xb[(size_t)ka * 12 + i]) / dtn;
                const float m1 = (Xb[(size_t)(kb + 1) * 12 + i] - Xb[(size_t)kb * 12 + i]) / dtn;
                s12[i] = hermite(x0[i], m0, x1[i], m1, dtn, s);
            }
            const double tw = (a.replan_index * a.replanning_steps + j + 1) * a.sim_dt;      // time of the recorded step
            write_row(a.S + ((size_t)b * a.n_rows + a.row0 + j) * 19, (float)recorded_phase(tw, period), s12, k);
            check_state(s12);
        }
    }
    if (commit_flags(a, b, flags)) return;       // terminated by this replan's rows: frozen from here on
    // plant = plan
    const float* Xn = Xb + (size_t)a.nodes_per_replan * 12;
    for (int i = 0; i < 12; ++i) x[i] = Xn[i];
    apply_push(x + 6, a, b, a.mass);
    // feet that stand at the node the plant has reached are where the plan put them (touch-downs in between)
    if (a.footsteps)
        for (int f = 0; f < 4; ++f)
            if (pb[a.nodes_per_replan * 16 + f] > 0.5f)
                for (int i = 0; i < 3; ++i) fp[3 * f + i] = pb[a.nodes_per_replan * 16 + 4 + 3 * f + i];
    integrate_base_reference(a, b);
}

}  // namespace nmpc
