// nmpc_batch_row.hpp -- the two device functions a training batch is made of, one copy each for the translation units
// that make batches: nmpc_dataset.hip (nmpc_assemble_batch: rows by index) and nmpc_policy.hip (nmpc_weighted_sample:
// indices; nmpc_policy_train_epoch: index and row in one kernel).  The epoch call is bit-identical to the chain of the
// other two because all three run this code.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nmpc_policy.h"

namespace nmpc_batch {

// Element j of output row i, taken from table row `row` (in range: the caller checked):  x[i] = [state_norm, goal_norm],
// y[i] = action.  (s - mean) / std in fp64, then fp32; states are normalised from column s_first on; a NULL mean leaves
// the field raw.
__device__ __forceinline__ void write_element(const nmpc_batch_source& t, size_t row, int i, int j, float* __restrict__ x,
                                              float* __restrict__ y) {
    const int n_x = t.n_state + t.n_goal;
    if (j < t.n_state) {
        const float s = t.states[row * t.n_state + j];
        x[(size_t)i * n_x + j] = (t.s_mean && j >= t.s_first) ? (float)(((double)s - t.s_mean[j]) / t.s_std[j]) : s;
    } else if (j < n_x) {
        const int k = j - t.n_state;
        const float g = t.goals[row * t.n_goal + k];
        x[(size_t)i * n_x + j] = t.g_mean ? (float)(((double)g - t.g_mean[k]) / t.g_std[k]) : g;
    } else {
        const int k = j - n_x;
        y[(size_t)i * t.n_action + k] = t.actions[row * t.n_action + k];
    }
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned& o0, unsigned& o1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

// Sample i of a seed: a Philox-4x32-10 uniform number from (seed, i), then the inverse-CDF lookup -- the first index
// with cdf > u * total, in [0, n).  A row of weight zero repeats its predecessor's cdf and is never that first index.
__device__ __forceinline__ long long sample_row(const double* __restrict__ cdf, long long n, double total,
                                                unsigned long long seed, int i) {
    unsigned a, b;
    philox4x32_10((unsigned)i, 0u, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), a, b);
    const double u = ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);   // 53 bits in [0, 1)
    const double target = u * total;
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace nmpc_batch
