// nmpc_rollout_common.hpp -- the plant-independent part of a device rollout step.
//
// The two device-resident rollout harnesses -- nmpc_rollout.hip.inc (centroidal plant, 19-slot rows) and nmpc_wb_rollout.hip.inc
// (whole-body plant, 44-slot rows) -- run the same loop of LocomotionMPC.open_loop (mpc_controller/mpc.py:416-462) around
// different plants.  One copy of what does not depend on the plant: the kernel arguments both have (RolloutCommon, which the
// host loop of nmpc_api.hip works on), the fp64 base references with the reference's quantisation, the contact window of the
// gait table, the unsafe-state predicates, the recorded gait phase, the bookkeeping of failed[b], the rows of a rollout that
// terminated earlier, the base push and the integration of the base reference.
// Contraction is off inside the functions (a pragma at file scope would reach into the including file): both plants round alike.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nmpc.h"

namespace nmpc {

// What RolloutArgs and WbRolloutArgs have in common; both derive from it, so a.B is a.B in every kernel.
struct RolloutCommon {
    int B, N, npc, node, first;           // nodes per gait cycle, current optimisation node, first replan (cold start)
    int replanning_steps, replan_index, n_replans, record_sim_steps;
    int row0;                             // first row of S this replan writes
    int n_rows;                           // rows of S per rollout
    int term_mask;                        // flag bits that terminate a rollout (terminate_mask of the configuration)
    double sim_dt, t_horizon, nom_height, height_offset, dt_nodes;
    float push_dt;                        // 0: no push during this interval
    float collision_height;               // base height below which NMPC_ROLLOUT_FLAG_COLLISION is raised
    float nominal_period;                 // gait period (recorded phase; Raibert footsteps)
    const signed char* gait;              // dev [4][npc] contact table
    const double *v_des, *w_des;          // dev [B][3]
    double* ref_state;                    // dev [B][12] integrated base reference (fp64, as the host keeps it)
    const float* push_force;              // dev [B][3] or nullptr
    float *yref, *yref_e, *params;        // dev problem tensors of the solve
    float *X, *U;                         // dev trajectories
    float* S;                             // dev [B][n_rows][row width of the plant] recorded states
    const int* status;                    // dev [B] status of the last solve
    int* failed;                          // dev [B] sticky flag bits NMPC_ROLLOUT_FLAG_*, replan of termination above them
    // a push window per rollout (nmpc_rollout_set_push_windows, nmpc_wb_rollout_set_push_windows); win_start == nullptr: push_dt
    // above holds for every rollout.  t_now: the time of this replan; win_slack: half a simulation step; dt_replan: the interval.
    const float *win_start, *win_duration;    // dev [B] seconds
    double t_now, win_slack, dt_replan;
};

__device__ inline void rpy_matrix(double roll, double pitch, double yaw, double (&R)[9]) {
#pragma clang fp contract(off)
    const double cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}
// numpy.round(x, d): rint(x * 10^d) / 10^d
__device__ inline double np_round(double x, double p10) {
#pragma clang fp contract(off)
    return rint(x * p10) / p10;
}
// Python's builtin round(x, 1): the decimal nearest to the exact binary value (ties to even)
__device__ inline double py_round1(double x) {
#pragma clang fp contract(off)
    const double t = x * 10.0;
    const double e = fma(x, 10.0, -t);          // exact residual of the product
    double r = rint(t);
    const double fl = floor(t);
    if (t - fl == 0.5) r = (e > 0.0) ? fl + 1.0 : (e < 0.0) ? fl : r;
    return r / 10.0;
}
__device__ inline double clipd(double v, double lo, double hi) {   // np.clip
#pragma clang fp contract(off)
    return fmin(fmax(v, lo), hi);
}

// LocomotionMPC.compute_base_ref_vel_tracking (mpc.py:210-272) for one rollout, in fp64 with the reference's quantisation
// (np.round to 2 / 1 decimals, the builtin round for the yaw) and crossed-bounds clips; (px, py, yaw) = q[0], q[1], q[3] of the
// plant, rs = the controller's integrated reference.
__device__ inline void base_ref_vel_tracking_dev(double px, double py, double yaw, const double* rs, const double* v_des_p,
                                                 const double* w_des_p, double t_horizon, double height, float (&ref)[12],
                                                 float (&ref_e)[12]) {
#pragma clang fp contract(off)
    const double v_des[3] = {v_des_p[0], v_des_p[1], v_des_p[2]};
    const double w_des[3] = {w_des_p[0], w_des_p[1], w_des_p[2]};
    double r[12] = {0}, re[12], R[9];
    r[0] = np_round(px, 100.0);
    r[1] = np_round(py, 100.0);
    r[2] = height;
    r[3] = py_round1(yaw);
    rpy_matrix(rs[5], rs[4], rs[3], R);                   // rpyToMatrix(ref_state[3:6][::-1])
    double vg[3];
    for (int i = 0; i < 3; ++i) vg[i] = np_round(R[3 * i] * v_des[0] + R[3 * i + 1] * v_des[1] + R[3 * i + 2] * v_des[2], 10.0);
    r[6] = vg[0]; r[7] = vg[1]; r[8] = vg[2];
    r[9] = w_des[2]; r[10] = w_des[1]; r[11] = w_des[0];
    for (int i = 0; i < 12; ++i) re[i] = r[i];
    rpy_matrix(w_des[0] * t_horizon, w_des[1] * t_horizon, w_des[2] * t_horizon, R);
    for (int i = 0; i < 3; ++i) re[6 + i] = R[3 * i] * r[6] + R[3 * i + 1] * r[7] + R[3 * i + 2] * r[8];
    for (int i = 0; i < 2; ++i) {
        const double reach = vg[i] * t_horizon;
        re[i] = clipd(rs[i] + reach, -r[i] + 1.2 * reach, r[i] + 1.2 * reach);
    }
    const double yaw_reach = w_des[2] * t_horizon;
    re[3] = clipd(rs[3] + yaw_reach, -rs[3] + 1.5 * yaw_reach, rs[3] + 1.5 * yaw_reach);
    for (int i = 0; i < 2; ++i) r[i] += 0.75 * (re[i] - r[i]);
    r[3] += 0.75 * (re[3] - r[3]);
    re[8] = 0.0; re[4] = re[5] = 0.0; r[4] = r[5] = 0.0; re[10] = re[11] = 0.0;
    for (int i = 0; i < 12; ++i) { ref[i] = (float)r[i]; ref_e[i] = (float)re[i]; }
}

// The window of the gait table that starts at the current node (contact_planner.py:121-149), by the 64 threads of a block: per
// node k <= N the contact flags of the four feet at cflag[f * STRIDE + k] (and the swing-peak flags at pflag, where peaks is
// given), and the share of `weight` that each standing foot carries.  stand_first: every foot stands at the very first node of
// a rollout (setup_initial_feet_pos, solver.py:199-200).  The caller synchronises.  The node is an argument: a rollout step has
// one per launch (below), the labeller one per problem (nmpc_wb_label.hip.inc).
template <int STRIDE>
__device__ inline void contact_window(const signed char* gait, int npc, int N, int node, int tid, const signed char* peaks,
                                      bool stand_first, float weight, float* cflag, float* pflag, float* fshare) {
#pragma clang fp contract(off)
    for (int k = tid; k <= N; k += 64) {
        float n = 0.0f;
        for (int f = 0; f < 4; ++f) {
            float c = (float)gait[f * npc + (node + k) % npc];
            if (stand_first && node == 0 && k == 0) c = 1.0f;
            cflag[f * STRIDE + k] = c;
            if (peaks) pflag[f * STRIDE + k] = (float)peaks[f * npc + (node + k) % npc];
            n += c;
        }
        fshare[k] = weight / fmaxf(n, 1.0f);
    }
}
template <int STRIDE>
__device__ inline void contact_window(const RolloutCommon& a, int tid, const signed char* peaks, bool stand_first, float weight,
                                      float* cflag, float* pflag, float* fshare) {
    contact_window<STRIDE>(a.gait, a.npc, a.N, a.node, tid, peaks, stand_first, weight, cflag, pflag, fshare);
}

// check_unsafe_state_v2 (Rollout_combined_controller.py:367-431) on a recorded state, in fp32: the flag bits it raises.
// (Joint limits have no centroidal counterpart and stay with the whole-body plant.)
__device__ inline int unsafe_state_flags(float roll, float pitch, float z, float vx, float vy, const double* v_des_b,
                                         float collision_height) {
#pragma clang fp contract(off)
    const float lim = 25.0f * 0.017453292519943295f;
    int flags = 0;
    if (fabsf(roll) > lim) flags |= NMPC_ROLLOUT_FLAG_ROLL;
    if (fabsf(pitch) > lim) flags |= NMPC_ROLLOUT_FLAG_PITCH;
    if (z < 0.18f || z > 0.45f) flags |= NMPC_ROLLOUT_FLAG_HEIGHT;
    if (fabsf(vx - (float)v_des_b[0]) > 0.10f || fabsf(vy - (float)v_des_b[1]) > 0.10f) flags |= NMPC_ROLLOUT_FLAG_VEL_TRACKING;
    if (z < collision_height) flags |= NMPC_ROLLOUT_FLAG_COLLISION;
    if (!(fabsf(z) <= 1e30f)) flags |= NMPC_ROLLOUT_FLAG_SOLVER;
    return flags;
}

// gait phase recorded with the state at time t of the rollout: np.round(phase, 4)
__device__ inline double recorded_phase(double t, double period) {
#pragma clang fp contract(off)
    return rint(fmod(t, period) / period * 1.0e4) / 1.0e4;
}

// The bookkeeping of failed[b] around the rows of a replan.  Before the rows are checked: a solve that failed raises the
// solver flag.  After them: a rollout that one of the terminating bits now ends, and that carries no stamp yet, is stamped
// with 1 + the index of this replan; the flags are stored; true: frozen from here on.
__device__ inline int solver_status_flag(int status) {
#pragma clang fp contract(off)
    return (status == NMPC_STATUS_NAN || status == NMPC_STATUS_QP) ? NMPC_ROLLOUT_FLAG_SOLVER : 0;
}
__device__ inline bool commit_flags(const RolloutCommon& a, int b, int flags) {
#pragma clang fp contract(off)
    if ((flags & a.term_mask) && !(flags >> NMPC_ROLLOUT_TERM_SHIFT)) flags |= (a.replan_index + 1) << NMPC_ROLLOUT_TERM_SHIFT;
    a.failed[b] = flags;
    return (flags & a.term_mask) != 0;
}

// A rollout terminated in an earlier replan of this call (the reference's simulator stops such a rollout, RolloutMPC.py:424-437):
// its plant and its controller are frozen, and the rows of this replan repeat the row before them -- the one that terminated it,
// or a copy of it -- so that S stays finite.  The rollout is invalid as a whole and is to be discarded or redone by the caller.
__device__ inline void hold_last_row(float* rows, int width, int rows_per_replan) {
#pragma clang fp contract(off)
    for (int j = 0; j < rows_per_replan; ++j)
        for (int i = 0; i < width; ++i) rows[j * width + i] = rows[i - width];
}

// base push over a replanning interval: v += F * push_dt / m.  With a window per rollout, push_dt is decided here as the host
// loop decides it for the whole batch (run_rollout, nmpc_api.hip): the same comparison in doubles on the rollout's own window.
__device__ inline void apply_push(float* v3, const RolloutCommon& a, int b, float mass) {
#pragma clang fp contract(off)
    float push_dt = a.push_dt;
    if (a.win_start) {
        const float start = a.win_start[b], duration = a.win_duration[b];
        push_dt = (a.push_force && duration > 0.0f && a.t_now >= (double)start - a.win_slack &&
                   a.t_now < (double)start + (double)duration - a.win_slack) ? (float)a.dt_replan : 0.0f;
    }
    if (push_dt > 0.0f && a.push_force)
        for (int i = 0; i < 3; ++i) v3[i] += a.push_force[b * 3 + i] * push_dt / mass;
}

// one simulation step of the integrated base reference rs[12] (increment_base_ref_position, mpc.py:204-208)
__device__ inline void base_reference_step(double* rs, const double (&v_des)[3], double wz, double sim_dt) {
#pragma clang fp contract(off)
    double R[9];
    rpy_matrix(rs[5], rs[4], rs[3], R);
    const double vx = np_round(R[0] * v_des[0] + R[1] * v_des[1] + R[2] * v_des[2], 10.0);
    const double vy = np_round(R[3] * v_des[0] + R[4] * v_des[1] + R[5] * v_des[2], 10.0);
    rs[0] += vx * sim_dt;
    rs[1] += vy * sim_dt;
    rs[3] += wz * sim_dt;
}

// integrate the base reference of rollout b over the replanning interval, one simulation step at a time
__device__ inline void integrate_base_reference(const RolloutCommon& a, int b) {
#pragma clang fp contract(off)
    double* rs = a.ref_state + (size_t)b * 12;
    const double v_des[3] = {a.v_des[b * 3], a.v_des[b * 3 + 1], a.v_des[b * 3 + 2]};
    const double wz = a.w_des[b * 3 + 2];
    for (int s = 0; s < a.replanning_steps; ++s) base_reference_step(rs, v_des, wz, a.sim_dt);
}

}  // namespace nmpc
