// nmpc_wb_label.hip.inc -- DAgger relabelling (nmpc_wb_label_states_batch of include/nmpc.h): the problems of the whole-body
// expert's FIRST solve from plant states that somebody else's rollout visited.
//
// nmpc_wb_rollout_prepare_kernel prepares one problem per rollout, and the rollouts of a call share the gait clock: the node
// and the integrated base reference belong to the replan.  Visited states come from different control steps, so here both
// belong to the problem: problem m = b * K + k (robot b, row k) reads node[k] and advances a private copy of ref_state[b] by
// ref_steps[k] simulation steps.  Everything else -- the windows with the node-0 rule, the base references with the reference's
// quantisation, x0 with its momentum slots, the anchored plane points, the cold guess -- is the text of nmpc_wb_rollout.hip.inc
// and nmpc_rollout_common.hpp, so a problem prepared here is bit for bit the one a rollout that stands at that node with that
// reference prepares.  Included by nmpc_api.hip after nmpc_wb_rollout.hip.inc.

#pragma clang fp contract(off)

namespace nmpc {
namespace wb {

struct WbLabelArgs {
    int m0, K, N, npc;                    // first problem of this chunk (the launch has one block per problem of it), rows per robot
    int qv_rows, force_gravity;
    float step_height;
    double sim_dt, t_horizon, nom_height, height_offset;
    ModelParams mp;
    const signed char *gait, *peaks;      // dev [4][npc]
    const int *node, *ref_steps;          // dev [K]
    const int* failed;                    // dev [B] or nullptr
    const float *Q, *V;                   // dev, row k of robot b at (b * qv_rows + k) * 18
    const float* joint_ref;               // dev [12]
    const double *v_des, *w_des, *ref_state;   // dev [B][3], [B][3], [B][12]; read only
    float *yref, *yref_e, *params, *x0, *X, *U;   // the chunk's tensors of the solve: problem m at index m - m0
    int* skip;                            // dev [chunk]: 1 where the state lies behind its robot's termination
};

// one block (64 threads) per problem of the chunk; always a cold start
__global__ __launch_bounds__(64) void nmpc_wb_label_prepare_kernel(const WbLabelArgs a) {
    __shared__ WbProblem P;
    const int i = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int m = a.m0 + i, b = m / a.K, k = m - b * a.K;
    // the cut of a policy rollout: stamp s = 1 + the control step whose observation terminated the robot, rows k >= s - 1 are
    // those of a fallen robot
    const int stamp = a.failed ? a.failed[b] >> NMPC_ROLLOUT_TERM_SHIFT : 0;
    const bool behind = stamp != 0 && k >= stamp - 1;
    if (tid == 0) a.skip[i] = behind ? 1 : 0;
    if (behind) return;
    const float* qf = a.Q + ((size_t)b * a.qv_rows + k) * 18;
    const float* vf = a.V + ((size_t)b * a.qv_rows + k) * 18;
    const int node = a.node[k];
    if (tid == 0) {
        double rs[12];
        for (int j = 0; j < 12; ++j) rs[j] = a.ref_state[(size_t)b * 12 + j];
        const double v_des[3] = {a.v_des[b * 3], a.v_des[b * 3 + 1], a.v_des[b * 3 + 2]};
        const double wz = a.w_des[b * 3 + 2];
        for (int s = 0, n = a.ref_steps[k]; s < n; ++s) base_reference_step(rs, v_des, wz, a.sim_dt);
        base_ref_vel_tracking_dev((double)qf[0], (double)qf[1], (double)qf[3], rs, a.v_des + (size_t)b * 3, a.w_des + (size_t)b * 3,
                                  a.t_horizon, a.nom_height + a.height_offset, P.ref, P.ref_e);
    } else if (tid == 1) {
        wb_measured_state(a.mp, qf, vf, P);
    }
    contact_window<65>(a.gait, a.npc, N, node, tid, a.peaks, true, -a.mp.gz * a.mp.mass, P.cflag, P.pflag, P.fshare);
    wb_write_problem(P, tid, N, a.joint_ref, a.step_height, a.force_gravity, (float)a.height_offset, true,
                     {a.yref + (size_t)i * N * NY, a.yref_e + (size_t)i * NYE, a.params + (size_t)i * (N + 1) * NP,
                      a.x0 + (size_t)i * NX, a.X + (size_t)i * (N + 1) * NX, a.U + (size_t)i * N * NU});
}

}  // namespace wb
}  // namespace nmpc
