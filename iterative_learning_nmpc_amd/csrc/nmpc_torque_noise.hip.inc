// nmpc_torque_noise.hip.inc -- sensor noise and bias on the policy input of the contact plant (nmpc_observe_noise_batch,
// nmpc_contact_set_noise of include/nmpc_torque.h) and the rows the sensors showed (nmpc_observed_rows_batch,
// nmpc_policy_rollout_set_observed); included by nmpc_torque.hip inside namespace nmpc_torque, after nmpc_torque_delay.hip.inc.
// The variate is nmpc_noise::variate of nmpc_noise.hpp, which nmpc_torque.hip includes in front of the namespace.
//
// What a policy is shown is not the plant state: encoders, an IMU and a state estimator stand between the two.  The perturbation
// is a pass of its own over the policy input X, behind observe_kernel, which stays as it is: the state rows S, the fall flags and
// the plant keep the true state, and only the columns of X that carry the 44-slot row move.  The draw is counter-based -- a pure
// function of (seed, robot, step, slot) -- so a launch needs no state, a robot's stream does not depend on the batch it is in,
// and a numpy restatement gives the same bits: the variate is an exact integer and one fp32 product, no transcendental.
#pragma once

constexpr int NOISE_ROW = 2 * OB_STATE;                   // a row of the table: sigma[44], then bias[44]

struct NoiseArgs {
    int x_stride, s_first;
    unsigned first_robot, step, key0, key1;
    const float* noise;                                   // [B][NOISE_ROW]
    const double* s_std;                                  // [44] or nullptr: X is raw
    float* X;                                             // robot b's input at X + b * x_stride, its first 44 slots are touched
};

// slot j of robot r at step s: g = the centred sum of the four 16-bit halves of two Philox words, scaled to unit variance
// (nmpc_noise::variate at the fourth counter word 0, |g| < 3.4641); the perturbation of the raw slot is bias + sigma g in fp64, each operation rounded once
__device__ inline double noise_draw(unsigned r, unsigned s, unsigned j, unsigned key0, unsigned key1, float sigma, float bias) {
#pragma clang fp contract(off)
    const float g = nmpc_noise::variate(r, s, j, 0u, key0, key1);
    const double scaled = (double)sigma * (double)g;
    return (double)bias + scaled;
}

// One thread per (robot, slot): the 44 threads of a robot read a run of its table row twice and read and write a run of its row
// of X; a slot whose sigma and bias are both zero is not written, and the goal columns behind slot 43 are never addressed.
__global__ __launch_bounds__(256) void observe_noise_kernel(int B, const NoiseArgs p) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * OB_STATE) return;
    const size_t b = e / OB_STATE;
    const int j = (int)(e - b * OB_STATE);
    const float sigma = p.noise[b * NOISE_ROW + j], bias = p.noise[b * NOISE_ROW + OB_STATE + j];
    if (sigma == 0.0f && bias == 0.0f) return;
    const double n = noise_draw(p.first_robot + (unsigned)b, p.step, (unsigned)j, p.key0, p.key1, sigma, bias);
    float* x = p.X + b * p.x_stride + j;
    *x = (float)((double)*x + ((p.s_std && j >= p.s_first) ? n / p.s_std[j] : n));
}

struct ObservedArgs {
    int s_stride, o_stride;
    unsigned first_robot, step, key0, key1;
    const float* noise;                                   // [B][NOISE_ROW] or nullptr: no table, O is S
    const float* S;                                       // robot b's true row at S + b * s_stride
    float* O;                                             // robot b's observed row at O + b * o_stride; may be S itself
};

// The raw 44-slot row as the sensors show it, one thread per (robot, slot): O = (float)(S + n) with the n that observe_noise_kernel
// puts on X at this step where the slot has noise, the bits of S elsewhere and without a table.  Each thread reads and writes its
// own element alone, so O may be S (the perturbation in place).
__global__ __launch_bounds__(256) void observed_rows_kernel(int B, const ObservedArgs p) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * OB_STATE) return;
    const size_t b = e / OB_STATE;
    const int j = (int)(e - b * OB_STATE);
    const float s = p.S[b * p.s_stride + j];
    float o = s;
    if (p.noise) {
        const float sigma = p.noise[b * NOISE_ROW + j], bias = p.noise[b * NOISE_ROW + OB_STATE + j];
        if (sigma != 0.0f || bias != 0.0f)
            o = (float)((double)s + noise_draw(p.first_robot + (unsigned)b, p.step, (unsigned)j, p.key0, p.key1, sigma, bias));
    }
    p.O[b * p.o_stride + j] = o;
}
