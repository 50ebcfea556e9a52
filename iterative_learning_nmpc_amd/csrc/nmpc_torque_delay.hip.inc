// nmpc_torque_delay.hip.inc -- the delay line in front of the control-step chain of the contact plant (nmpc_delay_line_batch,
// nmpc_contact_set_delays of include/nmpc_torque.h); included by nmpc_torque.hip inside namespace nmpc_torque, after
// nmpc_torque_track.hip.inc.
//
// A transport delay of d control steps between a PD target being issued and the joint answering it is a re-indexing of target
// rows: the row applied in control step k is the row issued in control step k - d, and for k < d a row issued before the call,
// which a shift register per robot keeps.  So it is a pass of its own over the table, in front of the chain, and the chain kernels
// stay as they are (a run-time switch of the target row inside contact_chain_kernel would reshape its recursion,
// nmpc_torque_track.hip.inc).  Nothing here computes: every output word is a copy of an input word.
#pragma once

// issued:  robot b's row k at issued  + (b * issued_rows  + k) * nu, k < n_steps
// applied: robot b's row k at applied + (b * applied_rows + k) * nu, k < n_steps; does not overlap issued
// history: robot b's slot j at history + (b * depth + j) * nu, j < depth: the target issued j + 1 control steps before the next one
struct DelayArgs {
    int n_steps, nu, depth, issued_rows, applied_rows, skip_mask;
    const int *delay, *skip;                              // delay [B]; skip [B] or nullptr
    const float* issued;
    float *applied, *history;
};

// One thread per (robot, actuated joint): a thread touches its own column of the three tables alone, and the threads of a robot
// read and write runs of nu consecutive floats.  With d = min(max(delay[b], 0), depth):
//   applied[k] = k >= d ? issued[k - d] : history[d - 1 - k]                            0 <= d - 1 - k < depth, 0 <= k - d < n_steps
//   history'[j] = n_steps - 1 - j >= 0 ? issued[n_steps - 1 - j] : history[j - n_steps]  0 <= j - n_steps < j
// The register is updated in place after the applied rows are out, j descending: every slot read lies below every slot written.
__global__ __launch_bounds__(256) void delay_line_kernel(int B, const DelayArgs p) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * p.nu) return;
    const size_t b = e / p.nu, nu = p.nu;
    const size_t i = e - b * nu;
    if (p.skip && (p.skip[b] & p.skip_mask)) return;
    int d = p.delay[b];
    d = d < 0 ? 0 : (d > p.depth ? p.depth : d);
    const float* in = p.issued + b * p.issued_rows * nu + i;
    float* out = p.applied + b * p.applied_rows * nu + i;
    float* reg = p.history + b * p.depth * nu + i;
    for (int k = 0; k < p.n_steps; ++k) out[k * nu] = k >= d ? in[(k - d) * nu] : reg[(d - 1 - k) * nu];
    for (int j = p.depth - 1; j >= 0; --j) {
        const int src = p.n_steps - 1 - j;
        reg[j * nu] = src >= 0 ? in[src * nu] : reg[(j - p.n_steps) * nu];
    }
}
