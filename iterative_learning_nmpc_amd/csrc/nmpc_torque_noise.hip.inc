// nmpc_torque_noise.hip.inc -- sensor noise and bias on the policy input of the contact plant (nmpc_observe_noise_batch,
// nmpc_contact_set_noise of include/nmpc_torque.h); included by nmpc_torque.hip inside namespace nmpc_torque, after
// nmpc_torque_delay.hip.inc.  The generator is nmpc_batch::philox4x32_10 of nmpc_batch_row.hpp, which nmpc_torque.hip includes
// in front of the namespace.
//
// What a policy is shown is not the plant state: encoders, an IMU and a state estimator stand between the two.  The perturbation
// is a pass of its own over the policy input X, behind observe_kernel, which stays as it is: the state rows S, the fall flags and
// the plant keep the true state, and only the columns of X that carry the 44-slot row move.  The draw is counter-based -- a pure
// function of (seed, robot, step, slot) -- so a launch needs no state, a robot's stream does not depend on the batch it is in,
// and a numpy restatement gives the same bits: the variate is an exact integer and one fp32 product, no transcendental.
#pragma once

constexpr int NOISE_ROW = 2 * OB_STATE;                   // a row of the table: sigma[44], then bias[44]
constexpr float NOISE_UNIT = 0x1.bb67aep-16f;             // (float)(1 / sqrt((2^32 - 1) / 3)): four uniforms on 0 .. 65535 have variance (2^32 - 1) / 3

struct NoiseArgs {
    int x_stride, s_first;
    unsigned first_robot, step, key0, key1;
    const float* noise;                                   // [B][NOISE_ROW]
    const double* s_std;                                  // [44] or nullptr: X is raw
    float* X;                                             // robot b's input at X + b * x_stride, its first 44 slots are touched
};

// slot j of robot r at step s: g = the centred sum of the four 16-bit halves of two Philox words, scaled to unit variance
// (|g| <= 131070 NOISE_UNIT < 3.4641); the perturbation of the raw slot is bias + sigma g in fp64, each operation rounded once
__device__ inline double noise_draw(unsigned r, unsigned s, unsigned j, unsigned key0, unsigned key1, float sigma, float bias) {
#pragma clang fp contract(off)
    unsigned w0, w1;
    nmpc_batch::philox4x32_10(r, s, j, 0u, key0, key1, w0, w1);
    const int t = (int)((w0 & 0xffffu) + (w0 >> 16) + (w1 & 0xffffu) + (w1 >> 16)) - 131070;
    const float g = (float)t * NOISE_UNIT;
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
