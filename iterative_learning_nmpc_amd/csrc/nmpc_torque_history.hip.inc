// nmpc_torque_history.hip.inc -- observation and action history on the policy input of the contact plant (nmpc_history_push_batch,
// nmpc_history_push_actions_batch, nmpc_policy_rollout_set_history of include/nmpc_torque.h); included by nmpc_torque.hip inside
// namespace nmpc_torque, after nmpc_torque_noise.hip.inc.
//
// What a robot's ground, payload, actuator, delay and sensor bias are does not stand in one 44-slot row: it shows in how successive
// rows and the issued PD targets relate.  So the policy may be shown the wide row
//   W_k = [ O_k | O_{k-1} | ... | O_{k-n_obs+1} | A_{k-1} | ... | A_{k-n_act} ]
// which two shift registers per robot keep: `hist` [rows][n_obs][44], slot 0 the incoming slot and slot h the observed row of h
// control steps ago, and `act` [rows][n_act][12], slot i the target issued i + 1 control steps before the next one (the delay
// register's convention, nmpc_torque_delay.hip.inc).  Both passes stand behind the observation and behind the contact step, which
// stay as they are.  Every word of W and of the registers is a copy of an input word; X is nmpc_batch::write_element's expression on it.
#pragma once

constexpr int HIST_NU = 12;                               // actuated joints of the whole-body tree, the width of an action slot
constexpr int HIST_COLS = OB_STATE + HIST_NU;             // threads of a robot in front of its goal threads

struct HistoryPushArgs {
    int n_obs, n_act, n_goal, s_first, w_stride;
    float* hist;                                          // [B][n_obs][44], aged in place
    const float* act;                                     // [B][n_act][12]; nullptr with n_act == 0
    const float* goal;                                    // [B][n_goal]; read only with an X
    const double *s_mean, *s_std;                         // [n_wide], both or neither
    float *W, *X;                                         // robot b's raw wide row at W + b * w_stride, its input at X + b * (n_wide + n_goal)
};

// One thread per (robot, column of 44 + 12 + n_goal).  Thread (b, j < 44) owns column j of robot b's n_obs slots: from the oldest
// slot down it reads the slot, writes the entry of W and X that is made of it and hands the word to the slot above, which it has
// read already; slot 0 keeps its content.  Thread (b, 44 + i) writes joint i's n_act entries and moves nothing; the goal threads
// copy the goal behind the wide row of X.  No thread reads a word another thread writes.
__global__ __launch_bounds__(256) void history_push_kernel(int B, const HistoryPushArgs p) {
    const int cols = HIST_COLS + p.n_goal;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * cols) return;
    const size_t b = e / cols;
    const int j = (int)(e - b * cols);
    const int n_wide = OB_STATE * p.n_obs + HIST_NU * p.n_act;
    float* const Wb = p.W ? p.W + b * p.w_stride : nullptr;
    float* const Xb = p.X ? p.X + b * (n_wide + p.n_goal) : nullptr;
    // column c of the wide row: the raw word, and nmpc_batch::write_element's expression on it
    auto put = [&](int c, float w) {
        if (Wb) Wb[c] = w;
        if (Xb) Xb[c] = (p.s_mean && c >= p.s_first) ? (float)(((double)w - p.s_mean[c]) / p.s_std[c]) : w;
    };
    if (j < OB_STATE) {
        float* const col = p.hist + b * p.n_obs * OB_STATE + j;
        for (int h = p.n_obs - 1; h >= 0; --h) {
            const float w = col[h * OB_STATE];
            put(h * OB_STATE + j, w);
            if (h + 1 < p.n_obs) col[(h + 1) * OB_STATE] = w;
        }
    } else if (j < HIST_COLS) {
        const int i = j - OB_STATE;
        const float* const reg = p.act + b * p.n_act * HIST_NU + i;
        for (int s = 0; s < p.n_act; ++s) put(OB_STATE * p.n_obs + s * HIST_NU + i, reg[s * HIST_NU]);
    } else if (Xb) {
        const int k = j - HIST_COLS;
        Xb[n_wide + k] = p.goal[b * p.n_goal + k];
    }
}

// One thread per (robot, joint): its column of the action register moves up by one slot, the oldest first, and slot 0 takes the
// target just issued, A + b * a_stride.
__global__ __launch_bounds__(256) void history_push_actions_kernel(int B, int n_act, float* __restrict__ act, const float* __restrict__ A, int a_stride) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * HIST_NU) return;
    const size_t b = e / HIST_NU;
    const int i = (int)(e - b * HIST_NU);
    float* const reg = act + b * n_act * HIST_NU + i;
    for (int s = n_act - 1; s > 0; --s) reg[s * HIST_NU] = reg[(s - 1) * HIST_NU];
    reg[0] = A[b * a_stride + i];
}
