// nmpc_wb_plan.hpp -- a whole-body plan (X [N+1][42], U [N][30] of one problem) sampled at a time of its horizon.
//
// The up-sampling of interpolate_trajectory_with_derivatives (mpc_controller/mpc.py:388-414): positions on cubic Hermite
// segments through (q_k, v_k), velocities through (v_k, a'_k) with a'_k = a_{max(k-1, 0)} (the reference prepends the first
// acceleration row, mpc.py:409-410), in fp64 from the fp32 plan.  One copy for the two kernels that sample a plan -- the
// advance kernel of the device rollouts (nmpc_wb_rollout.hip.inc: the recorded state rows) and the label kernel of the torque
// layer (nmpc_torque.hip: the action that goes with each row) -- so that the state under a label is the state of its row.
// Contraction is off inside the functions (a pragma at file scope would reach into the including file): every caller rounds alike.
#pragma once
#include "nmpc_wb_model.hpp"

namespace nmpc {
namespace wb {

struct PlanSample {      // segment k and the Hermite basis at t
    int k;
    double h, h00, h10, h01, h11;
};

__device__ inline PlanSample wb_plan_sample(double t, double dt_nodes, int N) {
#pragma clang fp contract(off)
    PlanSample c;
    int k = (int)floor(t / dt_nodes + 1e-9);
    if (k > N - 1) k = N - 1;
    const double h = dt_nodes, s = (t - k * h) / h;
    const double om = 1.0 - s;
    c.k = k; c.h = h;
    c.h00 = (1.0 + 2.0 * s) * om * om; c.h10 = s * om * om; c.h01 = s * s * (3.0 - 2.0 * s); c.h11 = s * s * (s - 1.0);
    return c;
}

// coordinate i of the sample: q_i and v_i
__device__ inline void wb_plan_component(const PlanSample& c, const float* Xb, const float* Ub, int i, double& q, double& v) {
#pragma clang fp contract(off)
    const double h = c.h, h00 = c.h00, h10 = c.h10, h01 = c.h01, h11 = c.h11;
    const float* x0 = Xb + (size_t)c.k * NX;
    const float* x1 = x0 + NX;
    const float* a0 = Ub + (size_t)(c.k > 0 ? c.k - 1 : 0) * NU;
    const float* a1 = Ub + (size_t)c.k * NU;
    q = h00 * (double)x0[WQ + i] + h10 * h * (double)x0[WV + i] + h01 * (double)x1[WQ + i] + h11 * h * (double)x1[WV + i];
    v = h00 * (double)x0[WV + i] + h10 * h * (double)a0[WA + i] + h01 * (double)x1[WV + i] + h11 * h * (double)a1[WA + i];
}

__device__ inline void wb_plan_at(const float* Xb, const float* Ub, int N, double dt_nodes, double t, double (&q)[18], double (&v)[18]) {
    const PlanSample c = wb_plan_sample(t, dt_nodes, N);
    for (int i = 0; i < 18; ++i) wb_plan_component(c, Xb, Ub, i, q[i], v[i]);
}

}  // namespace wb
}  // namespace nmpc
