// nmpc_noise.hpp -- the one text of the counter-based variate that every noise rule of the library draws: the sensor noise on the
// policy input and the observed rows beside a rollout (nmpc_torque_noise.hip.inc, fourth counter word 0) and the input noise of a
// training batch (nmpc_policy.hip, fourth counter word 1).  The generator is nmpc_batch::philox4x32_10 of nmpc_batch_row.hpp.
#pragma once
#include "nmpc_batch_row.hpp"

namespace nmpc_noise {

constexpr float UNIT = 0x1.bb67aep-16f;                   // (float)(1 / sqrt((2^32 - 1) / 3)): four uniforms on 0 .. 65535 have variance (2^32 - 1) / 3

// g at counter (c0, c1, c2, c3) under the key (key0, key1): the centred sum of the four 16-bit halves of the first two Philox
// words, an exact integer t with |t| <= 131070, scaled to unit variance by one fp32 product (|g| < 3.4641); no transcendental,
// so a restatement on the host gives the same bits
__device__ __forceinline__ float variate(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned key0, unsigned key1) {
#pragma clang fp contract(off)
    unsigned w0, w1;
    nmpc_batch::philox4x32_10(c0, c1, c2, c3, key0, key1, w0, w1);
    const int t = (int)((w0 & 0xffffu) + (w0 >> 16) + (w1 & 0xffffu) + (w1 >> 16)) - 131070;
    return (float)t * UNIT;
}

}  // namespace nmpc_noise
