// nmpc_torque.hip -- the torque layer on gfx950 (C-ABI: include/nmpc_torque.h).
//
// Batched recursive Newton-Euler inverse dynamics with external foot forces (dynamics.py:136-163), the PD
// law around it (mpc.py:592-599), the recorded PD-target action (RolloutMPC.py:228-250) and the action labels of a whole
// plan (plan_actions_kernel: one thread per (rollout, simulation step), the same recursion on the sampled plan).  One thread
// per robot: the recursion over the tree is serial (a body needs its parent), robots are independent, and
// a batch of rollouts brings thousands of them.  The model is read through wave-uniform (scalar) loads;
// the per-body quantities the recursion has to keep (velocity, acceleration, world rotation on the way
// out; force and moment on the way back) live in a 3.5 KB LDS slice per thread laid out [slot][thread], so
// that the parent look-ups -- a run-time index, which would push register arrays into scratch memory --
// are conflict-free LDS reads.  ~5 kFLOP per robot: the layer is latency-, not throughput-relevant.
// The other direction -- accelerations from torques and given contact forces, and a PD-driven integration step around them --
// is nmpc_torque_fd.hip.inc, included below; the declared ground-contact law, the foot kinematics it needs and the plant step
// that evaluates it inside that recursion are nmpc_torque_contact.hip.inc; the observation of a plant state for a policy in the
// loop and of the rows of a table of states -- one kernel text, two instantiations -- is nmpc_torque_policy.hip.inc, and the loop
// itself (nmpc_policy_rollout_batch) is host code at the end of this file;
// what the tree's inertia is -- the mass matrix, the centre of mass and the centroidal momentum map of one composite-rigid-body
// pass -- is nmpc_torque_crba.hip.inc; the correction of the plant's second integrator, which takes the stiff contact and PD terms
// implicitly and spends that mass matrix on it, is nmpc_torque_implicit.hip.inc; the chain of control steps on the plant -- one
// kernel text, instantiated for a table of PD targets tracked in one launch, for pushed substeps, for a push window per robot,
// for the implicit integrator and for either integrator under a ground, a payload or an actuator per robot -- is nmpc_torque_track.hip.inc, with
// the one rule of what lies behind an instantiation's slice, its LDS footprint and its block width; the centroidal momentum about an anchor
// point at the robot is nmpc_torque_centroidal.hip.inc, one kernel text with three entry points: how the momentum moves with q --
// d(A_g v)/dq, d com/dq and the bias of its time derivative --, the momentum pass on the nodes of a whole-body solve, and the
// momentum A_g(q) v of a plant state alone, which the device rollouts put into x0; the delay line in front of the chain -- a
// shift register of issued PD targets per robot, a pass of copies -- is nmpc_torque_delay.hip.inc; sensor noise and bias on the
// policy input behind the observation -- a counter-based draw per robot, step and slot -- is nmpc_torque_noise.hip.inc, and so are
// the rows the sensors showed beside a policy rollout.
#include <hip/hip_runtime.h>

#include "nmpc_host.hpp"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nmpc.h"
#include "../../include/nmpc_policy.h"
#include "../../include/nmpc_torque.h"
#include "nmpc_batch_row.hpp"
#include "nmpc_noise.hpp"
#include "nmpc_rollout_common.hpp"
#include "nmpc_torque_plan.hpp"
#include "nmpc_wb_plan.hpp"
#include "nmpc_wb_momentum.hpp"

namespace nmpc_torque {

constexpr int MAXJ = NMPC_TREE_MAX_JOINTS, MAXF = NMPC_TREE_MAX_FEET;
constexpr int TPB = 32;                    // robots per block: 27 floats x 32 joints x 32 threads = 108 KB of LDS at most
constexpr int SLOTS = 27;                  // w 3, vo 3, dw 3, dvo 3 (reused as moment 3, force 3 ...), Rw 9, n 3, l 3
constexpr size_t id_lds_bytes(int n) { return (size_t)n * SLOTS * TPB * sizeof(float); }

struct Model {                             // device copy, fixed-size arrays
    int n, nu, nf;
    int parent[MAXJ], type[MAXJ];
    float axis[MAXJ][3], R[MAXJ][9], p[MAXJ][3], mass[MAXJ], com[MAXJ][3], inertia[MAXJ][6];
    int foot_joint[MAXF];
    float foot_offset[MAXF][3];
    float gravity[3];
};

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 v3(const float* p) { return {p[0], p[1], p[2]}; }

struct M3 {
    float m[9];
};
__device__ __forceinline__ V3 mul(const M3& R, V3 a) {
    return {R.m[0] * a.x + R.m[1] * a.y + R.m[2] * a.z, R.m[3] * a.x + R.m[4] * a.y + R.m[5] * a.z, R.m[6] * a.x + R.m[7] * a.y + R.m[8] * a.z};
}
__device__ __forceinline__ V3 mul_t(const M3& R, V3 a) {
    return {R.m[0] * a.x + R.m[3] * a.y + R.m[6] * a.z, R.m[1] * a.x + R.m[4] * a.y + R.m[7] * a.z, R.m[2] * a.x + R.m[5] * a.y + R.m[8] * a.z};
}
__device__ __forceinline__ M3 mul(const M3& A, const M3& B) {
    M3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[3 * i + j] = A.m[3 * i] * B.m[j] + A.m[3 * i + 1] * B.m[3 + j] + A.m[3 * i + 2] * B.m[6 + j];
    return C;
}

// This thread's robot in the block's LDS slice [joint][NS slots][W threads]: the per-body state of every recursion of the family.
template <int NS, int W>
struct Slice {
    __device__ __forceinline__ float& operator()(int joint, int slot) const {
        extern __shared__ float body[];
        return body[(joint * NS + slot) * W + threadIdx.x];
    }
    __device__ __forceinline__ V3 get3(int joint, int slot) const { return {(*this)(joint, slot), (*this)(joint, slot + 1), (*this)(joint, slot + 2)}; }
    __device__ __forceinline__ void put3(int joint, int slot, V3 x) const { (*this)(joint, slot) = x.x; (*this)(joint, slot + 1) = x.y; (*this)(joint, slot + 2) = x.z; }
};

// x_parent = R x_child + p for joint i at coordinate qi: R = R_fix Rot(axis, qi) (revolute) or R_fix, p moved
// along the axis (prismatic).  Rodrigues: Rot = I + sin K + (1 - cos) K^2.
__device__ __forceinline__ void joint_transform(const Model& m, int i, float qi, M3& R, V3& p) {
    M3 Rf;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rf.m[k] = m.R[i][k];
    const V3 ax = v3(m.axis[i]);
    p = v3(m.p[i]);
    if (m.type[i] == 0) {
        float s, c;
        sincosf(qi, &s, &c);
        const float t = 1.0f - c;
        M3 J;
        J.m[0] = 1.0f - t * (ax.y * ax.y + ax.z * ax.z); J.m[1] = -s * ax.z + t * ax.x * ax.y;           J.m[2] = s * ax.y + t * ax.x * ax.z;
        J.m[3] = s * ax.z + t * ax.x * ax.y;             J.m[4] = 1.0f - t * (ax.x * ax.x + ax.z * ax.z); J.m[5] = -s * ax.x + t * ax.y * ax.z;
        J.m[6] = -s * ax.y + t * ax.x * ax.z;            J.m[7] = s * ax.x + t * ax.y * ax.z;             J.m[8] = 1.0f - t * (ax.x * ax.x + ax.y * ax.y);
        R = mul(Rf, J);
    } else {
        R = Rf;
        p = p + mul(Rf, qi * ax);
    }
}

__global__ __launch_bounds__(TPB) void id_torques_kernel(const Model* __restrict__ mp, int B, const float* __restrict__ q,
                                                         const float* __restrict__ v, const float* __restrict__ a,
                                                         const float* __restrict__ f, float* __restrict__ tau) {
    const Model& m = *mp;
    const int b = blockIdx.x * TPB + threadIdx.x;
    if (b >= B) return;
    const int n = m.n;
    const Slice<SLOTS, TPB> at;
    const float* qb = q + (size_t)b * n;
    const float* vb = v + (size_t)b * n;
    const float* ab = a + (size_t)b * n;

    // outward: velocities, accelerations (gravity enters as an acceleration of the world), net force and moment
    for (int i = 0; i < n; ++i) {
        M3 R; V3 p;
        joint_transform(m, i, qb[i], R, p);
        const int par = m.parent[i];
        V3 w_p{0, 0, 0}, vo_p{0, 0, 0}, dw_p{0, 0, 0}, dvo_p{-m.gravity[0], -m.gravity[1], -m.gravity[2]};
        M3 Rw = R;
        if (par >= 0) {
            w_p = at.get3(par, 0); vo_p = at.get3(par, 3); dw_p = at.get3(par, 6); dvo_p = at.get3(par, 9);
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, 12 + k);
            Rw = mul(Rp, R);
        }
        V3 w = mul_t(R, w_p), vo = mul_t(R, vo_p + cross(w_p, p));
        V3 dw = mul_t(R, dw_p), dvo = mul_t(R, dvo_p + cross(dw_p, p));
        const V3 ax = v3(m.axis[i]);
        const float qd = vb[i], qdd = ab[i];
        if (m.type[i] == 0) {          // S = (axis; 0):  a += S qdd + v x (S qd)
            dw = dw + qdd * ax + cross(w, qd * ax);
            dvo = dvo + cross(vo, qd * ax);
            w = w + qd * ax;
        } else {                       // S = (0; axis)
            dvo = dvo + qdd * ax + cross(w, qd * ax);
            vo = vo + qd * ax;
        }
        at.put3(i, 0, w); at.put3(i, 3, vo); at.put3(i, 6, dw); at.put3(i, 9, dvo);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, 12 + k) = Rw.m[k];
        // f = I a + v x* (I v) with the spatial inertia about the body origin
        const float mass = m.mass[i];
        const V3 c = v3(m.com[i]);
        const float* I = m.inertia[i];
        auto inertia = [&](V3 x) { return V3{I[0] * x.x + I[1] * x.y + I[2] * x.z, I[1] * x.x + I[3] * x.y + I[4] * x.z, I[2] * x.x + I[4] * x.y + I[5] * x.z}; };
        const V3 h_l = mass * (vo + cross(w, c)), h_n = inertia(w) + cross(c, h_l);
        const V3 g_l = mass * (dvo + cross(dw, c)), g_n = inertia(dw) + cross(c, g_l);
        at.put3(i, 21, g_n + cross(w, h_n) + cross(vo, h_l));      // moment about the body origin
        at.put3(i, 24, g_l + cross(w, h_l));                       // force
    }
    // contact forces: world-frame force at the foot point of its body (= - J^T f, dynamics.py:158-161)
    if (f) {
        for (int k = 0; k < m.nf; ++k) {
            const int j = m.foot_joint[k];
            M3 Rw;
#pragma unroll
            for (int e = 0; e < 9; ++e) Rw.m[e] = at(j, 12 + e);
            const V3 l = mul_t(Rw, v3(f + ((size_t)b * m.nf + k) * 3));
            at.put3(j, 24, at.get3(j, 24) - l);
            at.put3(j, 21, at.get3(j, 21) - cross(v3(m.foot_offset[k]), l));
        }
    }
    // inward: joint torques, forces handed to the parents
    for (int i = n - 1; i >= 0; --i) {
        const V3 fn = at.get3(i, 21), fl = at.get3(i, 24);
        const int act = i - (n - m.nu);
        if (act >= 0) tau[(size_t)b * m.nu + act] = dot(v3(m.axis[i]), m.type[i] == 0 ? fn : fl);
        const int par = m.parent[i];
        if (par >= 0) {
            M3 R; V3 p;
            joint_transform(m, i, qb[i], R, p);
            const V3 l_p = mul(R, fl);
            at.put3(par, 24, at.get3(par, 24) + l_p);
            at.put3(par, 21, at.get3(par, 21) + mul(R, fn) + cross(p, l_p));
        }
    }
}

// The same recursion for the label kernel below, its inputs behind an accessor: `in` gives the robot's coordinates q(i), v(i),
// a(i) of joint i, has_f() and f_at(k), the world-frame force at foot k; out(i, act, tau) takes the torque of actuated joint
// i = n - nu + act on the way back.  Per-body state in the block's LDS slice [joint][SLOTS][TPB], as above.
// id_torques_kernel above keeps its own text: routed through this function it compiles to other packed / fused products and
// rounds differently on tilted trees, and its outputs are held bit for bit.  Nor did one __global__ template over a job type
// (prologue, accessors, sink and epilogue of either kernel, switched at compile time) keep both: its id instantiation gave
// nmpc_id_torques_batch's bits, but its plan instantiation fused other products than plan_actions_kernel does through this
// function and changed the labels on tilted trees.  A change to the recursion goes into both.
template <class In, class Out>
__device__ __forceinline__ void id_torques_body(const Model& m, const In& in, const Out& out) {
    const int n = m.n;
    const Slice<SLOTS, TPB> at;

    // outward: velocities, accelerations (gravity enters as an acceleration of the world), net force and moment
    for (int i = 0; i < n; ++i) {
        M3 R; V3 p;
        joint_transform(m, i, in.q(i), R, p);
        const int par = m.parent[i];
        V3 w_p{0, 0, 0}, vo_p{0, 0, 0}, dw_p{0, 0, 0}, dvo_p{-m.gravity[0], -m.gravity[1], -m.gravity[2]};
        M3 Rw = R;
        if (par >= 0) {
            w_p = at.get3(par, 0); vo_p = at.get3(par, 3); dw_p = at.get3(par, 6); dvo_p = at.get3(par, 9);
            M3 Rp;
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp.m[k] = at(par, 12 + k);
            Rw = mul(Rp, R);
        }
        V3 w = mul_t(R, w_p), vo = mul_t(R, vo_p + cross(w_p, p));
        V3 dw = mul_t(R, dw_p), dvo = mul_t(R, dvo_p + cross(dw_p, p));
        const V3 ax = v3(m.axis[i]);
        const float qd = in.v(i), qdd = in.a(i);
        if (m.type[i] == 0) {          // S = (axis; 0):  a += S qdd + v x (S qd)
            dw = dw + qdd * ax + cross(w, qd * ax);
            dvo = dvo + cross(vo, qd * ax);
            w = w + qd * ax;
        } else {                       // S = (0; axis)
            dvo = dvo + qdd * ax + cross(w, qd * ax);
            vo = vo + qd * ax;
        }
        at.put3(i, 0, w); at.put3(i, 3, vo); at.put3(i, 6, dw); at.put3(i, 9, dvo);
#pragma unroll
        for (int k = 0; k < 9; ++k) at(i, 12 + k) = Rw.m[k];
        // f = I a + v x* (I v) with the spatial inertia about the body origin
        const float mass = m.mass[i];
        const V3 c = v3(m.com[i]);
        const float* I = m.inertia[i];
        auto inertia = [&](V3 x) { return V3{I[0] * x.x + I[1] * x.y + I[2] * x.z, I[1] * x.x + I[3] * x.y + I[4] * x.z, I[2] * x.x + I[4] * x.y + I[5] * x.z}; };
        const V3 h_l = mass * (vo + cross(w, c)), h_n = inertia(w) + cross(c, h_l);
        const V3 g_l = mass * (dvo + cross(dw, c)), g_n = inertia(dw) + cross(c, g_l);
        at.put3(i, 21, g_n + cross(w, h_n) + cross(vo, h_l));      // moment about the body origin
        at.put3(i, 24, g_l + cross(w, h_l));                       // force
    }
    // contact forces: world-frame force at the foot point of its body (= - J^T f, dynamics.py:158-161)
    if (in.has_f()) {
        for (int k = 0; k < m.nf; ++k) {
            const int j = m.foot_joint[k];
            M3 Rw;
#pragma unroll
            for (int e = 0; e < 9; ++e) Rw.m[e] = at(j, 12 + e);
            const V3 l = mul_t(Rw, in.f_at(k));
            at.put3(j, 24, at.get3(j, 24) - l);
            at.put3(j, 21, at.get3(j, 21) - cross(v3(m.foot_offset[k]), l));
        }
    }
    // inward: joint torques, forces handed to the parents
    for (int i = n - 1; i >= 0; --i) {
        const V3 fn = at.get3(i, 21), fl = at.get3(i, 24);
        const int act = i - (n - m.nu);
        if (act >= 0) out(i, act, dot(v3(m.axis[i]), m.type[i] == 0 ? fn : fl));
        const int par = m.parent[i];
        if (par >= 0) {
            M3 R; V3 p;
            joint_transform(m, i, in.q(i), R, p);
            const V3 l_p = mul(R, fl);
            at.put3(par, 24, at.get3(par, 24) + l_p);
            at.put3(par, 21, at.get3(par, 21) + mul(R, fn) + cross(p, l_p));
        }
    }
}

// The labels of one plan: thread (b, j) samples rollout b's plan at t = (j + 1) sim_dt (nmpc_wb_plan.hpp, the advance kernel's
// own sampling), holds a, f of node zoh[j], runs the recursion above on them and writes the PD target that reproduces the
// torque.  The coordinates are evaluated where the recursion asks for them (a Hermite sample is per coordinate), so nothing
// of q, v, a, f goes through memory or through run-time indexed registers.  tau, q_j, v_j wait in slots 0..2 of their joint
// (free on the way back) for the actuator permutation.
struct PlanArgs {
    int B, n_steps, N, a_rows, skip_mask;
    double dt_nodes, sim_dt;
    float kp, kd;
    const float *X, *U;
    const int *zoh, *perm, *skip;
    float* A;
};

struct PlanIn {
    nmpc::wb::PlanSample c;
    const float *Xb, *Ub, *ub;                             // the rollout's plan; ub = U[zoh[j]]
    __device__ __forceinline__ void qv(int i, float& q, float& v) const {
        double qd, vd;
        nmpc::wb::wb_plan_component(c, Xb, Ub, i, qd, vd);
        q = (float)qd; v = (float)vd;
    }
    __device__ __forceinline__ float q(int i) const { float q, v; qv(i, q, v); return q; }
    __device__ __forceinline__ float v(int i) const { float q, v; qv(i, q, v); return v; }
    __device__ __forceinline__ float a(int i) const { return ub[nmpc::wb::WA + i]; }
    __device__ __forceinline__ bool has_f() const { return true; }
    __device__ __forceinline__ V3 f_at(int k) const { return v3(ub + nmpc::wb::WF + 3 * k); }
};

__global__ __launch_bounds__(TPB) void plan_actions_kernel(const Model* __restrict__ mp, const PlanArgs p) {
    const Model& m = *mp;
    const size_t e = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= (size_t)p.B * p.n_steps) return;
    const size_t b = e / p.n_steps;
    const int j = (int)(e - b * p.n_steps);
    if (p.skip && (p.skip[b] & p.skip_mask)) return;
    int hold = p.zoh[j];
    hold = hold < 0 ? 0 : (hold > p.N - 1 ? p.N - 1 : hold);
    PlanIn in;
    in.c = nmpc::wb::wb_plan_sample((j + 1) * p.sim_dt, p.dt_nodes, p.N);
    in.Xb = p.X + b * (p.N + 1) * nmpc::wb::NX;
    in.Ub = p.U + b * p.N * nmpc::wb::NU;
    in.ub = in.Ub + (size_t)hold * nmpc::wb::NU;
    const Slice<SLOTS, TPB> at;
    id_torques_body(m, in, [&](int i, int, float t) {
        at(i, 0) = t;
        in.qv(i, at(i, 1), at(i, 2));
    });
    const int n = m.n, nu = m.nu;
    float* Ab = p.A + (b * p.a_rows + j) * nu;
    for (int i = 0; i < nu; ++i) {
        int src = p.perm ? p.perm[i] : i;
        src = src < 0 ? 0 : (src >= nu ? nu - 1 : src);
        Ab[i] = (at(n - nu + src, 0) + p.kd * at(n - nu + i, 2)) / p.kp + at(n - nu + i, 1);
    }
}

__global__ void pd_torques_kernel(int B, int n, int nu, const float* __restrict__ tau_ff, const float* __restrict__ q,
                                  const float* __restrict__ v, const float* __restrict__ q_plan, const float* __restrict__ v_plan,
                                  float kp, float kd, float* __restrict__ tau) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * nu) return;
    const size_t b = e / nu, j = b * n + (n - nu) + (e - b * nu);
    tau[e] = (tau_ff ? tau_ff[e] : 0.0f) + kp * (q_plan[j] - q[j]) + kd * (v_plan[j] - v[j]);
}

__global__ void pd_target_action_kernel(int B, int n, int nu, const float* __restrict__ tau, const int* __restrict__ perm,
                                        const float* __restrict__ q, const float* __restrict__ v, float kp, float kd,
                                        float* __restrict__ action) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * nu) return;
    const size_t b = e / nu;
    const int i = (int)(e - b * nu);
    int src = perm ? perm[i] : i;
    src = src < 0 ? 0 : (src >= nu ? nu - 1 : src);
    const size_t j = b * n + (n - nu) + i;
    action[e] = (tau[b * nu + src] + kd * v[j]) / kp + q[j];
}

#include "nmpc_torque_fd.hip.inc"
#include "nmpc_torque_contact.hip.inc"
#include "nmpc_torque_policy.hip.inc"
#include "nmpc_torque_crba.hip.inc"
#include "nmpc_torque_implicit.hip.inc"
#include "nmpc_torque_track.hip.inc"
#include "nmpc_torque_delay.hip.inc"
#include "nmpc_torque_noise.hip.inc"
#include "nmpc_torque_history.hip.inc"
#include "nmpc_torque_centroidal.hip.inc"

}  // namespace nmpc_torque

// ================================================================================================
namespace {

using namespace nmpc_torque;
using nmpc::fail;
using nmpc::launched;

struct Torque {
    Model host{};
    Model* dev = nullptr;
    int device = 0;
    int fd_width = 32;                  // robots per block of fd_kernel: fd_block_width(n), or 16 if NMPC_FD_WIDTH=16 asks for it (tools/fd_cost.py)
    int ct_width = 32;                  // robots per block of contact_step_kernel: ct_block_width(n)
    int anchor = -1;                    // the centroidal kernels' reference frame: the first joint whose body has mass (-1: the tree has none)
    unsigned chain = 0;                 // bit i: joint i is the anchor or one of its ancestors
    float* act = nullptr;               // [act_rows][nu]: the actions of nmpc_policy_rollout_batch when its caller keeps none
    int act_rows = 0;
    struct {                            // nmpc_policy_rollout_set_states: the plant states beside a policy rollout (Q == nullptr: none)
        float *Q = nullptr, *V = nullptr;
        int rows = 0;
    } states;
    struct {                            // nmpc_policy_rollout_set_observed: the rows the sensors showed beside a policy rollout (O == nullptr: none)
        float* O = nullptr;
        int rows = 0;
    } observed;
    nmpc_push_cfg push{};               // nmpc_contact_set_push: the push of the plant calls (force == nullptr: none)
    nmpc_torque::PushWindows windows{}; // nmpc_contact_set_push_windows: a window per robot in place of the push's own (first == nullptr: none)
    struct Table {                      // a row per robot (rows == nullptr: none)
        const float* rows = nullptr;
        int n_rows = 0;
    };
    Table grounds;                      // nmpc_contact_set_grounds: a law per robot in place of the plant calls' cfg
    Table payloads;                     // nmpc_contact_set_payloads: a point mass per robot on body `payload_joint` in the plant calls
    int payload_joint = 0;
    Table actuators;                    // nmpc_contact_set_actuators: gains, joint damping and rotor inertia per robot in the plant calls
    struct {                            // nmpc_contact_set_delays: a transport delay per robot in front of the plant calls (delay == nullptr: none)
        const int* delay = nullptr;     // [rows]: control steps robot b lags by
        float* history = nullptr;       // [rows][depth][nu]: the shift register of issued targets
        int depth = 0;
        float* work = nullptr;          // [rows][work_rows][nu]: where the applied rows of a call go
        int work_rows = 0, rows = 0;
    } delays;
    struct {                            // nmpc_contact_set_noise: sensor noise and bias per robot on the policy input (table == nullptr: none)
        const float* table = nullptr;   // [rows][88]: sigma[44], bias[44] of robot b, in the units of the raw row
        int rows = 0;
        unsigned long long seed = 0;    // the Philox key
        long long first_robot = 0;      // robot b of a call draws as robot first_robot + b of the population
        long long step = 0;             // the noise step of the next observation with an X; host state
    } noise;
    struct {                            // nmpc_policy_rollout_set_history: observation and action history on the policy input (hist == nullptr: none)
        float* hist = nullptr;          // [rows][n_obs][44]: slot 0 the incoming slot, slot h the observed row of h control steps ago
        int n_obs = 0;
        float* act = nullptr;           // [rows][n_act][12]: slot i the target issued i + 1 control steps before the next one
        int n_act = 0;
        float* W = nullptr;             // [rows][w_rows][n_wide]: the raw wide rows beside a policy rollout, or nullptr
        int w_rows = 0, rows = 0;
        int n_wide() const { return OB_STATE * n_obs + HIST_NU * n_act; }
    } history;
    int integrator = NMPC_INTEGRATOR_EXPLICIT;      // nmpc_contact_set_integrator: how the plant calls take their substeps
    std::string err;
};

Torque* const no_handle = nullptr;      // for nmpc_torque_create and calls without a handle: errors go to the family's slot

// the instantiation of a `template <int W>` kernel at a run-time block width of 32 or 16, for its attributes and its launches
#define KERNEL_AT_WIDTH(kernel, w) ((w) == 32 ? kernel<32> : kernel<16>)

// one of the plant steps, `width` robots per block
template <class Args>
int launch_step(Torque* t, void (*kernel)(const Model*, Args), int width, size_t lds, const Args& p, void* stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((p.B + width - 1) / width)), dim3(width), lds, static_cast<hipStream_t>(stream), t->dev, p);
    return launched(t);
}

// the instantiation of contact_chain_kernel for Args at a run-time block width; the implicit chain has the one width IM_W
template <class Args>
auto chain_kernel(int w) {
    static_assert(chain_lds_bytes<Args>(MAXJ, chain_block_width<Args>(MAXJ)) <= FD_LDS_MAX, "the largest tree no longer fits a CU at the narrow width of this chain");
    if constexpr (Args::implicit) return contact_chain_kernel<IM_W, Args>;
    else return w == 32 ? contact_chain_kernel<32, Args> : contact_chain_kernel<16, Args>;
}

// one launch of the chain, at the width and with the footprint its Args state for the handle's tree
template <class Args>
int launch_chain(Torque* t, const Args& p, void* stream) {
    const int n = t->host.n, w = chain_block_width<Args>(n);
    return launch_step(t, chain_kernel<Args>(w), w, chain_lds_bytes<Args>(n, w), p, stream);
}

// one of the element-wise kernels: a thread per entry of a [B][nu] table
template <class... KArgs, class... Args>
int launch_elementwise(Torque* t, void (*kernel)(int, KArgs...), int B, void* stream, Args... args) {
    const size_t n = (size_t)B * t->host.nu;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, args...);
    return launched(t);
}

// why a step cannot be taken (nullptr: it can)
const char* step_refusal(int n_sub, float dt) {
    if (n_sub < 1) return "n_sub must be at least 1";
    if (!(dt > 0.0f)) return "dt must be positive";
    return nullptr;
}

// the tree of the whole-body model, whose state layout the observation and the plan labels read
bool whole_body_tree(const Model& m) { return m.n == 18 && m.nu == 12 && m.nf == 4; }

// more than the default 64 KB of LDS per block for a kernel: up to `bytes`
#define LDS_LIMIT(kernel, bytes) \
    NMPC_TRY(no_handle, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)))

// the most an instantiation of the chain can be asked for at the width the handle's tree runs it at: chain_wide_joints() joints x 32
// robots, the largest tree x 16 (the implicit chains: x IM_W)
template <class Args>
int chain_lds_limit(Torque* t) {
    const int w = chain_block_width<Args>(t->host.n);
    LDS_LIMIT(chain_kernel<Args>(w), w == 32 ? chain_lds_bytes<Args>(chain_wide_joints<Args>(), 32) : chain_lds_bytes<Args>(MAXJ, w));
    return NMPC_OK;
}
template <class... Args>
int chain_lds_limits(Torque* t, ArgsList<Args...>) {
    int rc = NMPC_OK;
    ((rc = rc ? rc : chain_lds_limit<Args>(t)), ...);
    return rc;
}

// the device side of nmpc_torque_create, on the handle's device; what was allocated before an error is nmpc_torque_destroy's to free
int allocate(Torque* t) {
    NMPC_TRY(no_handle, hipMalloc(reinterpret_cast<void**>(&t->dev), sizeof(Model)));
    NMPC_TRY(no_handle, hipMemcpy(t->dev, &t->host, sizeof(Model), hipMemcpyHostToDevice));
    // inverse dynamics: the slice of the largest tree; forward dynamics: the most its instantiation can be asked for (25 joints x 32
    // robots, 32 joints x 16)
    LDS_LIMIT(id_torques_kernel, id_lds_bytes(MAXJ));
    LDS_LIMIT(KERNEL_AT_WIDTH(fd_kernel, t->fd_width), t->fd_width == 32 ? fd_lds_bytes(25, 32) : fd_lds_bytes(MAXJ, 16));
    // the contact plant: the kinematics slice of the largest tree, for the step the most its instantiation can be asked for by its
    // width rule (ct_block_width: ct_wide_joints() joints x 32 robots, the largest tree x 16), and for the chains the same by theirs
    LDS_LIMIT(foot_kernel<FootArgs>, fk_lds_bytes(MAXJ));
    LDS_LIMIT(foot_kernel<FootRowsArgs>, fk_lds_bytes(MAXJ));
    LDS_LIMIT(KERNEL_AT_WIDTH(contact_step_kernel, t->ct_width), t->ct_width == 32 ? ct_lds_bytes(ct_wide_joints(), 32) : ct_lds_bytes(MAXJ, 16));
    if (const int rc = chain_lds_limits(t, ChainArgs{})) return rc;
    // the composite-inertia pass and the three entry points of the centroidal kernel: the slice of the largest tree at the one
    // width each has
    LDS_LIMIT(crba_kernel, crba_lds_bytes(MAXJ, CR_W));
    LDS_LIMIT(centroidal_kernel<CmdIo>, centroidal_lds_bytes<CmdIo>(MAXJ));
    LDS_LIMIT(centroidal_kernel<NodeRecordIo>, centroidal_lds_bytes<NodeRecordIo>(MAXJ));
    LDS_LIMIT(centroidal_kernel<StateMomentumIo>, centroidal_lds_bytes<StateMomentumIo>(MAXJ));
    return NMPC_OK;
}

// the total mass of the handle's tree
float total_mass(const Model& m) {
    float total = 0.0f;
    for (int i = 0; i < m.n; ++i) total += m.mass[i];
    return total;
}

// why the centroidal quantities of the handle's tree cannot be had (nullptr: they can)
const char* centroidal_refusal(const Torque* t) {
    return t->anchor < 0 ? "the tree has no mass: its centre of mass is undefined" : nullptr;
}

// one entry point of the centroidal kernel on `rows` rows, about the handle's anchor
template <class Io>
int launch_centroidal(Torque* t, typename Io::Args p, long long rows, void* stream) {
    p.anchor = t->anchor; p.chain = t->chain;
    hipLaunchKernelGGL(centroidal_kernel<Io>, dim3((unsigned)((rows + CD_W - 1) / CD_W)), dim3(CD_W), centroidal_lds_bytes<Io>(t->host.n),
                       static_cast<hipStream_t>(stream), t->dev, p);
    return launched(t);
}

// both composite-inertia entry points: one launch of crba_kernel
int launch_crba(Torque* t, const CrbaArgs& p, void* stream) {
    return launch_step(t, crba_kernel, CR_W, crba_lds_bytes(t->host.n, CR_W), p, stream);
}

// both forward-dynamics entry points: one launch of fd_kernel at the handle's block width
int launch_fd(Torque* t, const FdArgs& p, void* stream) {
    const int w = t->fd_width;
    return launch_step(t, KERNEL_AT_WIDTH(fd_kernel, w), w, fd_lds_bytes(t->host.n, w), p, stream);
}

// why a contact configuration cannot be used (nullptr: it can), and the form the kernels read
const char* contact_cfg_refusal(const nmpc_contact_cfg* c) {
    if (!c) return "cfg is NULL";
    for (const float x : {c->ground_z, c->stiffness, c->damping, c->mu, c->slip_velocity, c->tau_max})
        if (!std::isfinite(x)) return "the contact parameters must be finite";
    if (c->stiffness < 0.0f || c->damping < 0.0f || c->mu < 0.0f) return "stiffness, damping and mu must not be negative";
    if (!(c->slip_velocity > 0.0f)) return "slip_velocity must be positive";
    return nullptr;
}

ContactCfg device_cfg(const nmpc_contact_cfg& c) {
    return {c.ground_z, c.stiffness, c.damping, c.mu, c.slip_velocity * c.slip_velocity, c.tau_max};
}

// why a state cannot be observed (nullptr: it can): the arguments nmpc_observe_batch and nmpc_policy_rollout_batch share
const char* observe_refusal(const Torque* t, int B, const float* q, const float* v, double period, const float* goal, int n_goal,
                            const double* s_mean, const double* s_std, int s_first, const float* S, int s_stride, const float* X) {
    if (!whole_body_tree(t->host))
        return "the observation needs the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4";
    if (B < 0 || !q || !v) return "need B >= 0 and q, v";
    if (!(period > 0.0)) return "period must be positive";
    if (n_goal < 0) return "n_goal must not be negative";
    if (X && n_goal > 0 && !goal) return "X needs goal";
    if (!s_mean != !s_std) return "s_mean and s_std come together or not at all";
    if (s_first < 0 || s_first > OB_STATE) return "s_first must be in [0, 44]";
    if (S && s_stride < OB_STATE) return "s_stride must be at least 44";
    if (X && t->noise.table && B > t->noise.rows) return "noise: B exceeds rows";
    return nullptr;
}

// why the attached noise cannot be put on the B rows of X (nullptr: it can)
const char* observe_noise_refusal(const Torque* t, int B, const float* X, int x_stride, int s_first) {
    if (!t->noise.table) return "noise: no table is attached (nmpc_contact_set_noise)";
    if (B > t->noise.rows) return "noise: B exceeds rows";
    if (!X) return "noise: X is needed";
    if (x_stride < OB_STATE) return "noise: x_stride must be at least 44";
    if (s_first < 0 || s_first > OB_STATE) return "noise: s_first must be in [0, 44]";
    return nullptr;
}

// the one launch of the noise: what observe_noise_refusal accepted, at noise step `step`
int launch_observe_noise(Torque* t, int B, float* X, int x_stride, const double* s_std, int s_first, long long step, void* stream) {
    NoiseArgs p{};
    p.x_stride = x_stride; p.s_first = s_first;
    p.first_robot = (unsigned)t->noise.first_robot; p.step = (unsigned)step;
    p.key0 = (unsigned)t->noise.seed; p.key1 = (unsigned)(t->noise.seed >> 32);
    p.noise = t->noise.table; p.s_std = s_std; p.X = X;
    const size_t n = (size_t)B * OB_STATE;
    hipLaunchKernelGGL(observe_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, p);
    return launched(t);
}

// why the observed rows of S cannot be written to O (nullptr: they can); with no table attached O is S
const char* observed_rows_refusal(const Torque* t, int B, const float* S, int s_stride, const float* O, int o_stride) {
    if (!S || !O) return "observed: S and O are needed";
    if (s_stride < OB_STATE || o_stride < OB_STATE) return "observed: s_stride and o_stride must be at least 44";
    if (t->noise.table && B > t->noise.rows) return "observed: B exceeds the rows of the noise table";
    return nullptr;
}

// the one launch of the observed rows: what observed_rows_refusal accepted, at noise step `step`
int launch_observed_rows(Torque* t, int B, const float* S, int s_stride, float* O, int o_stride, long long step, void* stream) {
    ObservedArgs p{};
    p.s_stride = s_stride; p.o_stride = o_stride;
    p.first_robot = (unsigned)t->noise.first_robot; p.step = (unsigned)step;
    p.key0 = (unsigned)t->noise.seed; p.key1 = (unsigned)(t->noise.seed >> 32);
    p.noise = t->noise.table; p.S = S; p.O = O;
    const size_t n = (size_t)B * OB_STATE;
    hipLaunchKernelGGL(observed_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, p);
    return launched(t);
}

// why registers of these depths cannot be a history (nullptr: they can): what the attach call and the two pushes share
const char* history_depth_refusal(const float* hist, int n_obs, const float* act, int n_act) {
    if (n_obs < 1 || n_obs > NMPC_HISTORY_MAX) return "history: n_obs must be in [1, NMPC_HISTORY_MAX]";
    if (n_act < 0 || n_act > NMPC_HISTORY_MAX) return "history: n_act must be in [0, NMPC_HISTORY_MAX]";
    if (!hist) return "history: hist is needed";
    if (n_act > 0 && !act) return "history: act is needed with n_act > 0";
    return nullptr;
}

// why the wide row of B robots cannot be pushed out of these registers (nullptr: it can)
const char* history_push_refusal(const Torque* t, int B, const float* hist, int n_obs, const float* act, int n_act, const float* goal, int n_goal,
                                 const double* s_mean, const double* s_std, int s_first, const float* W, int w_stride, const float* X) {
    if (!whole_body_tree(t->host)) return "history: the wide row needs the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4";
    if (B < 1) return "history: need B >= 1";
    if (const char* why = history_depth_refusal(hist, n_obs, act, n_act)) return why;
    const int n_wide = OB_STATE * n_obs + HIST_NU * n_act;
    if (!W && !X) return "history: W or X is needed";
    if (W && w_stride < n_wide) return "history: w_stride must be at least n_wide";
    if (n_goal < 0) return "history: n_goal must not be negative";
    if (!s_mean != !s_std) return "history: s_mean and s_std come together or not at all";
    if (s_first < 0 || s_first > n_wide) return "history: s_first must be in [0, n_wide]";
    if (X && n_goal > 0 && !goal) return "history: X needs goal";
    return nullptr;
}

// the one launch of the wide row: what history_push_refusal accepted
int launch_history_push(Torque* t, int B, float* hist, int n_obs, const float* act, int n_act, const float* goal, int n_goal, const double* s_mean,
                        const double* s_std, int s_first, float* W, int w_stride, float* X, void* stream) {
    HistoryPushArgs p{};
    p.n_obs = n_obs; p.n_act = n_act; p.n_goal = n_goal; p.s_first = s_first; p.w_stride = w_stride;
    p.hist = hist; p.act = act; p.goal = goal; p.s_mean = s_mean; p.s_std = s_std; p.W = W; p.X = X;
    const size_t n = (size_t)B * (HIST_COLS + n_goal);
    hipLaunchKernelGGL(history_push_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, p);
    return launched(t);
}

// the one launch of the action register: slot 0 <- the dense or strided rows A
int launch_history_push_actions(Torque* t, int B, float* act, int n_act, const float* A, int a_stride, void* stream) {
    return launch_elementwise(t, history_push_actions_kernel, B, stream, n_act, act, A, a_stride);
}

// the kinematics pass, with or without the law; with the law of the attached table of grounds if there is one
int launch_feet(Torque* t, const FootArgs& a, void* stream) {
    const size_t lds = fk_lds_bytes(t->host.n);
    if (!a.f || !t->grounds.rows) return launch_step(t, foot_kernel<FootArgs>, TPB, lds, a, stream);
    FootRowsArgs r{};
    static_cast<FootArgs&>(r) = a;
    r.rows = t->grounds.rows;
    return launch_step(t, foot_kernel<FootRowsArgs>, TPB, lds, r, stream);
}

// why a push cannot be attached to a tree of n_joints joints (nullptr: it can)
const char* push_refusal(const nmpc_push_cfg& p, int n_joints) {
    if (!p.force) return "push: force is NULL";
    if (p.force_rows < 1) return "push: force_rows must be at least 1";
    if (p.joint < 0 || p.joint >= n_joints) return "push: joint must be in [0, n_joints)";
    if (p.n_substeps < 0) return "push: n_substeps must not be negative";
    return nullptr;
}

// The window of `push` (force == nullptr: none) in a call of `total` substeps whose substep 0 is substep s0 of the count the
// window is stated in: the intersection [lo, hi) in the call's own count; lo == hi: nothing of the call is pushed.
struct Window { long long lo = 0, hi = 0; };
Window push_window(const nmpc_push_cfg& push, long long s0, long long total) {
    Window w;
    if (!push.force) return w;
    const long long first = (long long)push.first_substep - s0, end = first + push.n_substeps;
    w.lo = first > 0 ? first : 0; w.hi = end < total ? end : total;
    if (w.hi <= w.lo) w = Window{};
    return w;
}

// why the attached table of grounds cannot serve a call of B robots (nullptr: it can, or there is none)
const char* grounds_batch_refusal(const Torque* t, int B) {
    return t->grounds.rows && B > t->grounds.n_rows ? "grounds: B exceeds n_rows" : nullptr;
}

// why `push`, the windows per robot and the attached tables cannot serve a plant call of B robots (nullptr: they can, or there are none)
const char* plant_batch_refusal(const Torque* t, const nmpc_push_cfg& push, const nmpc_torque::PushWindows& wins, int B) {
    if (push.force && B > push.force_rows) return "push: B exceeds force_rows";
    if (wins.first && !push.force) return "push windows: no push is attached (nmpc_contact_set_push)";
    if (wins.first && B > wins.rows) return "push windows: B exceeds rows";
    if (const char* why = grounds_batch_refusal(t, B)) return why;
    if (t->payloads.rows && B > t->payloads.n_rows) return "payloads: B exceeds n_rows";
    if (t->delays.delay && B > t->delays.rows) return "delays: B exceeds rows";
    return t->actuators.rows && B > t->actuators.n_rows ? "actuators: B exceeds n_rows" : nullptr;
}

// why the attached delay line cannot take n_steps issued rows of B robots to `applied` (nullptr: it can)
const char* delay_line_refusal(const Torque* t, int B, int n_steps, const float* issued, int issued_rows, const float* applied, int applied_rows) {
    if (!t->delays.delay) return "delays: no table is attached (nmpc_contact_set_delays)";
    if (B > t->delays.rows) return "delays: B exceeds rows";
    if (n_steps < 1) return "delays: n_steps must be at least 1";
    if (issued_rows < n_steps || applied_rows < n_steps) return "delays: issued_rows and applied_rows must be at least n_steps";
    if (!issued || !applied) return "delays: issued and applied are needed";
    const size_t nu = (size_t)t->host.nu;
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(issued), a0 = reinterpret_cast<uintptr_t>(applied);
    const uintptr_t i1 = i0 + (((size_t)B - 1) * issued_rows + n_steps) * nu * sizeof(float);
    const uintptr_t a1 = a0 + (((size_t)B - 1) * applied_rows + n_steps) * nu * sizeof(float);
    if (i0 < a1 && a0 < i1) return "delays: applied overlaps issued";
    return nullptr;
}

// the one launch of the delay line: what delay_line_refusal accepted, through the attached register
int launch_delay_line(Torque* t, int B, int n_steps, const float* issued, int issued_rows, float* applied, int applied_rows, const int* skip,
                      int skip_mask, void* stream) {
    DelayArgs p{};
    p.n_steps = n_steps; p.nu = t->host.nu; p.depth = t->delays.depth; p.issued_rows = issued_rows; p.applied_rows = applied_rows;
    p.skip_mask = skip ? skip_mask : 0; p.skip = p.skip_mask ? skip : nullptr;
    p.delay = t->delays.delay; p.issued = issued; p.applied = applied; p.history = t->delays.history;
    return launch_elementwise(t, delay_line_kernel, B, stream, p);
}

// A plant call that launch_whole below does not take is cut into runs of substeps that are all un-pushed -- launches of the
// un-pushed kernels, as a call without a push makes them -- and runs that are all pushed, launches of the PushArgs chain
// (nmpc_torque_track.hip.inc says why).

// why the implicit integrator cannot run a tree of n joints (nullptr: it can)
const char* implicit_refusal(int n) {
    if (im_lds_bytes(n) > FD_LDS_MAX) return "integrator: the implicit slice of this tree does not fit the LDS";
    return nullptr;
}

// The arguments every launch of the chain shares; a caller adds what is its own -- the step its start state and the outputs of
// the last substep, the track its rows and skip flags -- and a launch the push, the windows and the piece of the call it runs.
PushArgs chain_args(int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg& cfg, const float* tau_ff, const float* A, int a_rows, float kp,
                    float kd, float* q, float* v) {
    PushArgs p{};
    p.B = B; p.n_steps = n_steps; p.n_sub = n_sub; p.a_rows = a_rows; p.dt = dt; p.kp = kp; p.kd = kd; p.c = device_cfg(cfg);
    p.tau = tau_ff; p.A = A; p.q = q; p.v = v;
    return p;
}

// one launch of a chain that is told its push -- the window `win` of the push's own, or with `wins` the robot's, in a call whose
// substep 0 is substep s0 of their count -- and tests it per substep: the implicit chain, and either integrator under a table of
// grounds, of payloads or of actuators; under payloads the table of grounds may be absent (rows == nullptr: the call's own law),
// under actuators the table of payloads too (payload_rows == nullptr: the zero row).
template <class Args>
int launch_stated(Torque* t, const PushArgs& call, const nmpc_push_cfg& push, const Window& win, const nmpc_torque::PushWindows& wins,
                  long long s0, void* stream) {
    Args p{};
    static_cast<PushArgs&>(p) = call;
    if constexpr (Args::grounds) p.rows = t->grounds.rows;
    if constexpr (Args::payloads) { p.payload_rows = t->payloads.rows; p.payload_joint = t->payload_joint; }
    if constexpr (Args::actuators) p.actuator_rows = t->actuators.rows;
    if (win.hi > win.lo) { p.force = push.force; p.joint = push.joint; p.push_lo = win.lo; p.push_hi = win.hi; }
    if (wins.first) { p.force = push.force; p.joint = push.joint; p.win_first = wins.first; p.win_count = wins.count; p.win_s0 = s0; }
    return launch_chain(t, p, stream);
}

// a plant call of the explicit integrator under windows per robot: one launch of the WindowArgs chain
int launch_windowed(Torque* t, const PushArgs& call, const nmpc_push_cfg& push, const nmpc_torque::PushWindows& wins, long long s0, void* stream) {
    WindowArgs p{call};
    p.force = push.force; p.joint = push.joint; p.first = wins.first; p.count = wins.count; p.s0 = s0;
    return launch_chain(t, p, stream);
}

// Does a plant call run as one launch, and of which instantiation?  It does under a table of actuators (whatever the push, the
// grounds and the payloads), under a table of payloads (whatever the push and the grounds), under a table of grounds (whatever the push), under the implicit integrator and under windows per robot: then that
// launch is made, rc is its result and the answer is true.  Otherwise nothing is launched: the caller cuts the call at the window.
bool launch_whole(Torque* t, const PushArgs& call, const nmpc_push_cfg& push, const Window& win, const nmpc_torque::PushWindows& wins,
                  long long s0, void* stream, int& rc) {
    const bool implicit = t->integrator == NMPC_INTEGRATOR_LINEARLY_IMPLICIT;
    if (t->actuators.rows)
        rc = implicit ? launch_stated<ImplicitActuatorsArgs>(t, call, push, win, wins, s0, stream) : launch_stated<ActuatorsArgs>(t, call, push, win, wins, s0, stream);
    else if (t->payloads.rows)
        rc = implicit ? launch_stated<ImplicitPayloadsArgs>(t, call, push, win, wins, s0, stream) : launch_stated<PayloadsArgs>(t, call, push, win, wins, s0, stream);
    else if (t->grounds.rows)
        rc = implicit ? launch_stated<ImplicitGroundsArgs>(t, call, push, win, wins, s0, stream) : launch_stated<GroundsArgs>(t, call, push, win, wins, s0, stream);
    else if (implicit)
        rc = launch_stated<ImplicitArgs>(t, call, push, win, wins, s0, stream);
    else if (wins.first)
        rc = launch_windowed(t, call, push, wins, s0, stream);
    else
        return false;
    return true;
}

// nmpc_contact_step_batch: the call's substep i is substep s0 + i of the count `push` and `wins` are stated in.  One launch where
// launch_whole makes it; else, under an explicit push, at most three: before, inside and after the window; the first reads q, v,
// the later ones go on in place on q_out, v_out, and the last one writes a_out, f_out, tau_out.
int contact_step(Torque* t, int B, int n_sub, float dt, const nmpc_contact_cfg* cfg, const float* q, const float* v, const float* tau_ff,
                 const float* q_des, float kp, float kd, float* q_out, float* v_out, float* a_out, float* f_out, float* tau_out,
                 const nmpc_push_cfg& push, const nmpc_torque::PushWindows& wins, long long s0, void* stream) {
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !q_out || !v_out) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, q_out, v_out");
    if (const char* why = step_refusal(n_sub, dt)) return fail(t, NMPC_E_ARG, why);
    if (const char* why = contact_cfg_refusal(cfg)) return fail(t, NMPC_E_ARG, why);
    if (const char* why = plant_batch_refusal(t, push, wins, B)) return fail(t, NMPC_E_ARG, why);
    const bool delayed = t->delays.delay && q_des;      // without a q_des nothing was issued: the register does not move
    if (delayed)
        if (const char* why = delay_line_refusal(t, B, 1, q_des, 1, t->delays.work, 1)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    if (delayed) {                                      // one control step is fed, once per call: the pieces of the cut path share it
        if (const int rc = launch_delay_line(t, B, 1, q_des, 1, t->delays.work, 1, nullptr, 0, stream)) return rc;
        q_des = t->delays.work;                         // dense [B][nu]
    }
    const Window win = wins.first ? Window{} : push_window(push, s0, n_sub);
    PushArgs call = chain_args(B, 1, n_sub, dt, *cfg, tau_ff, q_des, 1, kp, kd, q_out, v_out);
    call.q_in = q; call.v_in = v; call.a_out = a_out; call.f_out = f_out; call.tau_out = tau_out;
    if (int rc; launch_whole(t, call, push, win, wins, s0, stream, rc)) return rc;
    const int cuts[4] = {0, (int)win.lo, (int)win.hi, n_sub};
    bool first = true;
    for (int r = 0; r < 3; ++r) {
        const int count = cuts[r + 1] - cuts[r];
        if (count <= 0) continue;
        const bool last = cuts[r + 1] == n_sub;
        const float *qi = first ? q : q_out, *vi = first ? v : v_out;
        if (r == 1) {
            PushArgs p = call;
            p.n_sub = count; p.q_in = qi; p.v_in = vi; p.force = push.force; p.joint = push.joint;
            if (!last) p.a_out = p.f_out = p.tau_out = nullptr;
            if (const int rc = launch_chain(t, p, stream)) return rc;
        } else {
            const int w = t->ct_width;
            ContactArgs p{};
            p.B = B; p.n_sub = count; p.dt = dt; p.kp = kp; p.kd = kd; p.c = device_cfg(*cfg);
            p.q = qi; p.v = vi; p.tau = tau_ff; p.q_des = q_des; p.q_out = q_out; p.v_out = v_out;
            if (last) { p.a_out = a_out; p.f_out = f_out; p.tau_out = tau_out; }
            if (const int rc = launch_step(t, KERNEL_AT_WIDTH(contact_step_kernel, w), w, ct_lds_bytes(t->host.n, w), p, stream)) return rc;
        }
        first = false;
    }
    return NMPC_OK;
}

// nmpc_contact_track_batch, in substeps s = k * n_sub + i of the call, substep 0 being substep s0 of the count `wins` are stated in.
// One launch where launch_whole makes it; else, under an explicit push, whole control steps of one kind go into one launch, a
// control step the window starts or ends in is cut at that substep, and only its first piece writes its row of Q, V.
int contact_track(Torque* t, int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg* cfg, float* q, float* v, const float* tau_ff,
                  const float* A, int a_rows, float kp, float kd, float* Q, float* V, int qv_rows, const int* skip, int skip_mask,
                  const nmpc_push_cfg& push, const nmpc_torque::PushWindows& wins, long long s0, void* stream) {
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v");
    if (n_steps < 1) return fail(t, NMPC_E_ARG, "n_steps must be at least 1");
    if (const char* why = step_refusal(n_sub, dt)) return fail(t, NMPC_E_ARG, why);
    if (const char* why = contact_cfg_refusal(cfg)) return fail(t, NMPC_E_ARG, why);
    if (!A) return fail(t, NMPC_E_ARG, "A is NULL");
    if (a_rows < n_steps) return fail(t, NMPC_E_ARG, "a_rows must be at least n_steps");
    if (!Q != !V) return fail(t, NMPC_E_ARG, "Q and V come together or not at all");
    if (Q && qv_rows < n_steps) return fail(t, NMPC_E_ARG, "qv_rows must be at least n_steps");
    if (Q && !whole_body_tree(t->host))
        return fail(t, NMPC_E_ARG, "the rows Q, V need the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4");
    if (const char* why = plant_batch_refusal(t, push, wins, B)) return fail(t, NMPC_E_ARG, why);
    if (t->delays.delay) {
        if (n_steps > t->delays.work_rows) return fail(t, NMPC_E_ARG, "delays: n_steps exceeds work_rows");
        if (const char* why = delay_line_refusal(t, B, n_steps, A, a_rows, t->delays.work, t->delays.work_rows)) return fail(t, NMPC_E_ARG, why);
    }
    NMPC_ENTER(t, t->device);
    if (t->delays.delay) {                              // the issued rows through the register, once per call; the call then runs on the applied ones
        if (const int rc = launch_delay_line(t, B, n_steps, A, a_rows, t->delays.work, t->delays.work_rows, skip, skip_mask, stream)) return rc;
        A = t->delays.work; a_rows = t->delays.work_rows;
    }
    const int n = t->host.n, nu = t->host.nu;
    const long long total = (long long)n_steps * n_sub;
    const Window win = wins.first ? Window{} : push_window(push, 0, total);
    PushArgs call = chain_args(B, n_steps, n_sub, dt, *cfg, tau_ff, A, a_rows, kp, kd, q, v);
    call.qv_rows = qv_rows; call.skip_mask = skip ? skip_mask : 0; call.skip = call.skip_mask ? skip : nullptr;
    call.Q = Q; call.V = V;                      // one launch takes the whole table; the cut path below moves A, Q, V piece by piece
    if (int rc; launch_whole(t, call, push, win, wins, s0, stream, rc)) return rc;
    for (long long s = 0; s < total;) {
        const bool pushed = s >= win.lo && s < win.hi;
        const long long change = s < win.lo ? win.lo : (s < win.hi ? win.hi : total);      // where the kind of substep changes next
        const long long k = s / n_sub, i0 = s % n_sub, step_end = (k + 1) * n_sub;
        PushArgs p = call;
        p.A = A + (size_t)k * nu;
        p.Q = Q && i0 == 0 ? Q + (size_t)k * n : nullptr;
        p.V = Q && i0 == 0 ? V + (size_t)k * n : nullptr;
        if (i0 != 0 || change < step_end) {      // a piece of control step k
            const long long end = change < step_end ? change : step_end;
            p.n_steps = 1; p.n_sub = (int)(end - s);
            s = end;
        } else {                                 // whole control steps up to the next change
            p.n_steps = (int)(change / n_sub - k);
            s = (k + p.n_steps) * n_sub;
        }
        int rc;
        if (pushed) {
            p.force = push.force; p.joint = push.joint;
            rc = launch_chain(t, p, stream);
        } else {
            rc = launch_chain(t, static_cast<const TrackArgs&>(p), stream);
        }
        if (rc) return rc;
    }
    return NMPC_OK;
}

}  // namespace

bool nmpc_torque::push_attached(void* handle) { return handle && static_cast<const Torque*>(handle)->push.force; }

int nmpc_torque::contact_track_pushed(void* handle, int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg* cfg, float* q, float* v,
                                      const float* tau_ff, const float* A, int a_rows, float kp, float kd, float* Q, float* V, int qv_rows,
                                      const int* skip, int skip_mask, const nmpc_push_cfg& push, const PushWindows& windows, long long s0,
                                      void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (const char* why = push_refusal(push, t->host.n)) return fail(t, NMPC_E_ARG, why);
    return contact_track(t, B, n_steps, n_sub, dt, cfg, q, v, tau_ff, A, a_rows, kp, kd, Q, V, qv_rows, skip, skip_mask, push, windows, s0, stream);
}

const char* nmpc_torque::plan_actions_refusal(void* handle, int n_steps, const int* zoh, float kp, int device) {
    const Torque* t = static_cast<const Torque*>(handle);
    if (!t) return "null torque handle";
    if (!whole_body_tree(t->host))
        return "plan labels need the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4";
    if (n_steps < 1) return "n_steps must be at least 1";
    if (!zoh) return "zoh is NULL";
    if (!(kp != 0.0f)) return "kp must not be zero";
    if (device >= 0 && t->device != device) return "the torque handle lives on another device";
    return nullptr;
}

const char* nmpc_torque::label_states_refusal(void* handle, int n_rows, int qv_rows, int a_rows, const int* zoh, float kp, int device) {
    if (n_rows < 1) return "n_rows must be at least 1";
    if (qv_rows < n_rows) return "qv_rows must be at least n_rows";
    if (a_rows < n_rows) return "a_rows must be at least n_rows";
    return plan_actions_refusal(handle, 1, zoh, kp, device);
}

const char* nmpc_torque::momentum_refusal(void* handle, int device) {
    const Torque* t = static_cast<const Torque*>(handle);
    if (!t) return "null torque handle";
    if (t->host.n != 18) return "the articulated momentum model needs a tree in the coordinates of the whole-body model: n_joints = 18";
    if (const char* why = centroidal_refusal(t)) return why;
    if (device >= 0 && t->device != device) return "the torque handle lives on another device";
    return nullptr;
}

float nmpc_torque::tree_mass(void* handle) { return total_mass(static_cast<const Torque*>(handle)->host); }

int nmpc_torque::momentum_records(void* handle, int B, int N, int shift, const float* X, const int* skip, int skip_mask, const int* done,
                                  size_t done_stride, float* rec, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (const char* why = momentum_refusal(handle, -1)) return fail(t, NMPC_E_ARG, why);
    MomentumArgs p{};
    p.B = B; p.N = N; p.shift = shift; p.X = X; p.rec = rec; p.skip = skip_mask ? skip : nullptr; p.skip_mask = skip_mask;
    p.done = done; p.done_stride = done_stride;
    return launch_centroidal<NodeRecordIo>(t, p, (long long)B * (N + 1), stream);
}

const char* nmpc_torque::contact_track_refusal(void* handle, const nmpc_contact_cfg* ground, int n_sub, float dt, int device) {
    const Torque* t = static_cast<const Torque*>(handle);
    if (!t) return "null torque handle";
    if (!whole_body_tree(t->host))
        return "the rows of a tracked plan need the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4";
    if (const char* why = step_refusal(n_sub, dt)) return why;
    if (const char* why = contact_cfg_refusal(ground)) return why;
    if (device >= 0 && t->device != device) return "the torque handle lives on another device";
    return nullptr;
}

extern "C" {

int nmpc_torque_create(const nmpc_tree_model* mdl, int device_id, void** handle) {
    if (handle) *handle = nullptr;
    if (!mdl || !handle) return fail(no_handle, NMPC_E_ARG, "null argument");
    if (mdl->n_joints < 1 || mdl->n_joints > MAXJ || mdl->n_actuated < 1 || mdl->n_actuated > mdl->n_joints ||
        mdl->n_feet < 0 || mdl->n_feet > MAXF)
        return fail(no_handle, NMPC_E_ARG, "need 1 <= n_actuated <= n_joints <= 32, 0 <= n_feet <= 8");
    if (!mdl->parent || !mdl->type || !mdl->axis || !mdl->placement || !mdl->mass || !mdl->com || !mdl->inertia ||
        (mdl->n_feet > 0 && (!mdl->foot_joint || !mdl->foot_offset)))
        return fail(no_handle, NMPC_E_ARG, "null model array");
    Model m{};
    m.n = mdl->n_joints; m.nu = mdl->n_actuated; m.nf = mdl->n_feet;
    for (int i = 0; i < m.n; ++i) {
        if (mdl->parent[i] < -1 || mdl->parent[i] >= i) return fail(no_handle, NMPC_E_ARG, "parents must come before their children");
        if (mdl->type[i] != 0 && mdl->type[i] != 1) return fail(no_handle, NMPC_E_ARG, "joint type is 0 (revolute) or 1 (prismatic)");
        const float* ax = mdl->axis + 3 * i;
        const float len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        if (!(std::fabs(len - 1.0f) < 1e-4f)) return fail(no_handle, NMPC_E_ARG, "joint axes must be unit vectors");
        if (!(mdl->mass[i] >= 0.0f)) return fail(no_handle, NMPC_E_ARG, "negative mass");
        m.parent[i] = mdl->parent[i]; m.type[i] = mdl->type[i]; m.mass[i] = mdl->mass[i];
        std::memcpy(m.axis[i], ax, 12); std::memcpy(m.R[i], mdl->placement + 12 * i, 36);
        std::memcpy(m.p[i], mdl->placement + 12 * i + 9, 12); std::memcpy(m.com[i], mdl->com + 3 * i, 12);
        std::memcpy(m.inertia[i], mdl->inertia + 6 * i, 24);
    }
    for (int k = 0; k < m.nf; ++k) {
        if (mdl->foot_joint[k] < 0 || mdl->foot_joint[k] >= m.n) return fail(no_handle, NMPC_E_ARG, "foot_joint out of range");
        m.foot_joint[k] = mdl->foot_joint[k];
        std::memcpy(m.foot_offset[k], mdl->foot_offset + 3 * k, 12);
    }
    std::memcpy(m.gravity, mdl->gravity, 12);
    NMPC_ENTER(no_handle, device_id);
    Torque* t = new Torque();
    t->host = m; t->device = device_id;
    t->fd_width = fd_block_width(m.n);
    t->ct_width = ct_block_width(m.n);
    for (int i = m.n - 1; i >= 0; --i)
        if (m.mass[i] > 0.0f) t->anchor = i;
    for (int k = t->anchor; k >= 0; k = m.parent[k]) t->chain |= 1u << k;
    if (const char* w = std::getenv("NMPC_FD_WIDTH"))
        if (!std::strcmp(w, "16")) t->fd_width = 16;
    if (const int rc = allocate(t)) { nmpc_torque_destroy(t); return rc; }
    *handle = t;
    return NMPC_OK;
}

void nmpc_torque_destroy(void* handle) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return;
    nmpc::DeviceGuard guard(t->device);      // nothing to return: a failed switch goes to the family's slot, the buffers are freed all the same
    if (guard.err != hipSuccess) fail(no_handle, NMPC_E_HIP, std::string("nmpc_torque_destroy: ") + hipGetErrorString(guard.err));
    if (t->dev) (void)hipFree(t->dev);
    if (t->act) (void)hipFree(t->act);
    delete t;
}

const char* nmpc_torque_last_error(void* handle) { return nmpc::last_error(static_cast<Torque*>(handle)); }

int nmpc_id_torques_batch(void* handle, int B, const float* q, const float* v, const float* a, const float* f, float* tau,
                          void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !a || !tau) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, a, tau");
    NMPC_ENTER(t, t->device);
    hipLaunchKernelGGL(id_torques_kernel, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), id_lds_bytes(t->host.n),
                       static_cast<hipStream_t>(stream), t->dev, B, q, v, a, f, tau);
    return launched(t);
}

int nmpc_fd_accel_batch(void* handle, int B, const float* q, const float* v, const float* tau, const float* f, float* a, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !a) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, a");
    NMPC_ENTER(t, t->device);
    FdArgs p{};
    p.B = B; p.q = q; p.v = v; p.tau = tau; p.f = f; p.a_out = a;
    return launch_fd(t, p, stream);
}

int nmpc_fd_step_batch(void* handle, int B, int n_sub, float dt, const float* q, const float* v, const float* tau_ff, const float* q_des,
                       float kp, float kd, const float* f, float* q_out, float* v_out, float* a_out, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !q_out || !v_out) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, q_out, v_out");
    if (const char* why = step_refusal(n_sub, dt)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    FdArgs p{};
    p.B = B; p.n_sub = n_sub; p.dt = dt; p.kp = kp; p.kd = kd;
    p.q = q; p.v = v; p.tau = tau_ff; p.q_des = q_des; p.f = f; p.q_out = q_out; p.v_out = v_out; p.a_out = a_out;
    return launch_fd(t, p, stream);
}

int nmpc_mass_matrix_batch(void* handle, int B, const float* q, float* M, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !M) return fail(t, NMPC_E_ARG, "need B >= 0 and q, M");
    NMPC_ENTER(t, t->device);
    CrbaArgs p{};
    p.B = B; p.q = q; p.M = M;
    return launch_crba(t, p, stream);
}

int nmpc_centroidal_batch(void* handle, int B, const float* q, const float* v, float* com, float* h, float* Ag, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || (!com && !h && !Ag)) return fail(t, NMPC_E_ARG, "need B >= 0, q and com, h or Ag");
    if (h && !v) return fail(t, NMPC_E_ARG, "h needs v");
    if (const char* why = centroidal_refusal(t)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    CrbaArgs p{};
    p.B = B; p.q = q; p.v = h ? v : nullptr; p.com = com; p.h = h; p.Ag = Ag;
    return launch_crba(t, p, stream);
}

int nmpc_centroidal_derivatives_batch(void* handle, int B, const float* q, const float* v, float* dh_dq, float* dcom_dq, float* hdot_bias,
                                      void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || (!dh_dq && !dcom_dq && !hdot_bias))
        return fail(t, NMPC_E_ARG, "need B >= 0, q, v and dh_dq, dcom_dq or hdot_bias");
    if (const char* why = centroidal_refusal(t)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    CmdArgs p{};
    p.B = B; p.q = q; p.v = v; p.dh = dh_dq; p.dcom = dcom_dq; p.bias = hdot_bias;
    return launch_centroidal<CmdIo>(t, p, B, stream);
}

int nmpc_state_momentum_batch(void* handle, int B, const float* q, const float* v, int qv_stride, float* h, int h_stride, float* h2,
                              int h2_stride, const int* skip, int skip_mask, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !h) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, h");
    if (qv_stride < t->host.n) return fail(t, NMPC_E_ARG, "qv_stride must be at least n_joints");
    if (h_stride < 6 || (h2 && h2_stride < 6)) return fail(t, NMPC_E_ARG, "h_stride and h2_stride must be at least 6");
    if (const char* why = centroidal_refusal(t)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    StateMomentumArgs p{};
    p.B = B; p.qv_stride = qv_stride; p.h_stride = h_stride; p.h2_stride = h2_stride; p.skip_mask = skip ? skip_mask : 0;
    p.q = q; p.v = v; p.h = h; p.h2 = h2; p.skip = p.skip_mask ? skip : nullptr;
    return launch_centroidal<StateMomentumIo>(t, p, B, stream);
}

int nmpc_foot_kinematics_batch(void* handle, int B, const float* q, const float* v, float* pos, float* vel, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || (!pos && !vel)) return fail(t, NMPC_E_ARG, "need B >= 0, q and pos or vel");
    NMPC_ENTER(t, t->device);
    FootArgs a{};
    a.B = B; a.q = q; a.v = v; a.pos = pos; a.vel = vel;
    return launch_feet(t, a, stream);
}

int nmpc_contact_forces_batch(void* handle, int B, const nmpc_contact_cfg* cfg, const float* q, const float* v, float* f, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !f) return fail(t, NMPC_E_ARG, "need B >= 0 and q, f");
    if (const char* why = contact_cfg_refusal(cfg)) return fail(t, NMPC_E_ARG, why);
    if (const char* why = grounds_batch_refusal(t, B)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    FootArgs a{};
    a.B = B; a.q = q; a.v = v; a.f = f; a.c = device_cfg(*cfg);
    return launch_feet(t, a, stream);
}

int nmpc_contact_step_batch(void* handle, int B, int n_sub, float dt, const nmpc_contact_cfg* cfg, const float* q, const float* v,
                            const float* tau_ff, const float* q_des, float kp, float kd, float* q_out, float* v_out, float* a_out,
                            float* f_out, float* tau_out, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    return contact_step(t, B, n_sub, dt, cfg, q, v, tau_ff, q_des, kp, kd, q_out, v_out, a_out, f_out, tau_out, t->push, t->windows, 0, stream);
}

int nmpc_contact_set_push(void* torque, const nmpc_push_cfg* push) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (push)
        if (const char* why = push_refusal(*push, t->host.n)) return fail(t, NMPC_E_ARG, why);      // what was attached stays
    t->push = push ? *push : nmpc_push_cfg{};
    return NMPC_OK;
}

int nmpc_contact_set_push_windows(void* torque, const int* first_substep, const int* n_substeps, int rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (!first_substep && !n_substeps) { t->windows = {}; return NMPC_OK; }
    if (!first_substep || !n_substeps)      // what was attached stays
        return fail(t, NMPC_E_ARG, "push windows: first_substep and n_substeps come together or not at all");
    if (rows < 1) return fail(t, NMPC_E_ARG, "push windows: rows must be at least 1");
    t->windows = {first_substep, n_substeps, rows};
    return NMPC_OK;
}

int nmpc_contact_set_grounds(void* torque, const float* rows, int n_rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (rows && n_rows < 1) return fail(t, NMPC_E_ARG, "grounds: n_rows must be at least 1");      // what was attached stays
    t->grounds = {};
    if (rows) t->grounds = {rows, n_rows};
    return NMPC_OK;
}

int nmpc_contact_set_payloads(void* torque, const float* rows, int n_rows, int joint) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (rows) {                                           // what was attached stays
        if (n_rows < 1) return fail(t, NMPC_E_ARG, "payloads: n_rows must be at least 1");
        if (joint < 0 || joint >= t->host.n) return fail(t, NMPC_E_ARG, "payloads: joint must be in [0, n_joints)");
    }
    t->payloads = {};
    if (rows) { t->payloads = {rows, n_rows}; t->payload_joint = joint; }
    return NMPC_OK;
}

int nmpc_contact_set_actuators(void* torque, const float* rows, int n_rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (rows && n_rows < 1) return fail(t, NMPC_E_ARG, "actuators: n_rows must be at least 1");      // what was attached stays
    t->actuators = {};
    if (rows) t->actuators = {rows, n_rows};
    return NMPC_OK;
}

int nmpc_contact_set_delays(void* torque, const int* delay, float* history, int depth, float* work, int work_rows, int rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (delay) {                                          // what was attached stays
        if (depth < 1 || depth > NMPC_DELAY_MAX_DEPTH) return fail(t, NMPC_E_ARG, "delays: depth must be in [1, NMPC_DELAY_MAX_DEPTH]");
        if (rows < 1) return fail(t, NMPC_E_ARG, "delays: rows must be at least 1");
        if (work_rows < 1) return fail(t, NMPC_E_ARG, "delays: work_rows must be at least 1");
        if (!history || !work) return fail(t, NMPC_E_ARG, "delays: history and work are needed");
    }
    t->delays = {};
    if (delay) { t->delays.delay = delay; t->delays.history = history; t->delays.depth = depth; t->delays.work = work; t->delays.work_rows = work_rows; t->delays.rows = rows; }
    return NMPC_OK;
}

int nmpc_delay_line_batch(void* torque, int B, int n_steps, const float* issued, int issued_rows, float* applied, int applied_rows,
                          const int* skip, int skip_mask, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (B == 0) return NMPC_OK;
    if (B < 0) return fail(t, NMPC_E_ARG, "need B >= 0");
    if (const char* why = delay_line_refusal(t, B, n_steps, issued, issued_rows, applied, applied_rows)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    return launch_delay_line(t, B, n_steps, issued, issued_rows, applied, applied_rows, skip, skip_mask, stream);
}

int nmpc_contact_set_noise(void* torque, const float* noise, int rows, long long seed, long long first_robot, long long step0) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (noise && rows < 1) return fail(t, NMPC_E_ARG, "noise: rows must be at least 1");      // what was attached stays
    t->noise = {};
    if (noise) { t->noise.table = noise; t->noise.rows = rows; t->noise.seed = (unsigned long long)seed; t->noise.first_robot = first_robot; t->noise.step = step0; }
    return NMPC_OK;
}

int nmpc_contact_noise_step(void* torque, long long* step) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (!step) return fail(t, NMPC_E_ARG, "noise: step is NULL");
    if (!t->noise.table) return fail(t, NMPC_E_ARG, "noise: no table is attached (nmpc_contact_set_noise)");
    *step = t->noise.step;
    return NMPC_OK;
}

int nmpc_observe_noise_batch(void* torque, int B, float* X, int x_stride, const double* s_std, int s_first, long long step, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (B == 0) return NMPC_OK;
    if (B < 0) return fail(t, NMPC_E_ARG, "need B >= 0");
    if (const char* why = observe_noise_refusal(t, B, X, x_stride, s_first)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    return launch_observe_noise(t, B, X, x_stride, s_std, s_first, step, stream);
}

int nmpc_observed_rows_batch(void* torque, int B, const float* S, int s_stride, float* O, int o_stride, long long step, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (B == 0) return NMPC_OK;
    if (B < 0) return fail(t, NMPC_E_ARG, "need B >= 0");
    if (const char* why = observed_rows_refusal(t, B, S, s_stride, O, o_stride)) return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    return launch_observed_rows(t, B, S, s_stride, O, o_stride, step, stream);
}

int nmpc_contact_set_integrator(void* torque, int mode) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (mode != NMPC_INTEGRATOR_EXPLICIT && mode != NMPC_INTEGRATOR_LINEARLY_IMPLICIT)      // the mode that was set stays
        return fail(t, NMPC_E_ARG, "integrator: mode must be NMPC_INTEGRATOR_EXPLICIT (0) or NMPC_INTEGRATOR_LINEARLY_IMPLICIT (1)");
    if (mode == NMPC_INTEGRATOR_LINEARLY_IMPLICIT)
        if (const char* why = implicit_refusal(t->host.n)) return fail(t, NMPC_E_ARG, why);
    t->integrator = mode;
    return NMPC_OK;
}

int nmpc_observe_batch(void* handle, int B, const float* q, const float* v, double t, double period, const float* goal, int n_goal,
                       const double* s_mean, const double* s_std, int s_first, float collision_height, float* S, int s_stride, float* X,
                       int* failed, int step_index, int term_mask, void* stream) {
    Torque* h = static_cast<Torque*>(handle);
    if (!h) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (const char* why = observe_refusal(h, B, q, v, period, goal, n_goal, s_mean, s_std, s_first, S, s_stride, X)) return fail(h, NMPC_E_ARG, why);
    NMPC_ENTER(h, h->device);
    ObserveArgs a{};
    a.B = B; a.n_goal = n_goal; a.s_first = s_first; a.s_stride = s_stride; a.step_index = step_index; a.term_mask = term_mask;
    a.t = t; a.period = period; a.collision_height = collision_height;
    a.q = q; a.v = v; a.goal = goal; a.s_mean = s_mean; a.s_std = s_std; a.S = S; a.X = X; a.failed = failed;
    const size_t lds = (S || X) ? ob_lds_bytes(h->host.n) : 0;      // the flags alone run no kinematics and ask for no slice
    hipLaunchKernelGGL(observe_kernel<ObserveArgs>, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), lds, static_cast<hipStream_t>(stream), h->dev, a);
    if (const int rc = launched(h)) return rc;
    if (!X || !h->noise.table) return NMPC_OK;
    // what the policy is shown: the attached noise on the row's columns of X, at the handle's noise step, which then moves on
    if (const int rc = launch_observe_noise(h, B, X, OB_STATE + n_goal, s_std, s_first, h->noise.step, stream)) return rc;
    ++h->noise.step;
    return NMPC_OK;
}

int nmpc_contact_track_batch(void* handle, int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg* cfg, float* q, float* v,
                             const float* tau_ff, const float* A, int a_rows, float kp, float kd, float* Q, float* V, int qv_rows,
                             const int* skip, int skip_mask, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    return contact_track(t, B, n_steps, n_sub, dt, cfg, q, v, tau_ff, A, a_rows, kp, kd, Q, V, qv_rows, skip, skip_mask, t->push, t->windows, 0,
                         stream);
}

int nmpc_observe_rows_batch(void* handle, int B, int n_rows, const float* Q, const float* V, int qv_rows, double t0, double dt_row,
                            double period, float collision_height, float* S, int s_rows, int* failed, int step_index, int term_mask,
                            const int* skip, int skip_mask, void* stream) {
    Torque* h = static_cast<Torque*>(handle);
    if (!h) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (const char* why = observe_refusal(h, B, Q, V, period, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr)) return fail(h, NMPC_E_ARG, why);
    if (n_rows < 1) return fail(h, NMPC_E_ARG, "n_rows must be at least 1");
    if (qv_rows < n_rows) return fail(h, NMPC_E_ARG, "qv_rows must be at least n_rows");
    if (S && s_rows < n_rows) return fail(h, NMPC_E_ARG, "s_rows must be at least n_rows");
    NMPC_ENTER(h, h->device);
    ObserveRowsArgs a{};
    a.B = B; a.n_rows = n_rows; a.qv_rows = qv_rows; a.s_rows = s_rows; a.step_index = step_index; a.term_mask = term_mask;
    a.skip_mask = skip ? skip_mask : 0;
    a.t0 = t0; a.dt_row = dt_row; a.period = period; a.collision_height = collision_height;
    a.Q = Q; a.V = V; a.S = S; a.failed = failed; a.skip = a.skip_mask ? skip : nullptr;
    const size_t lds = S ? ob_lds_bytes(h->host.n) : 0;      // the flags alone run no kinematics and ask for no slice
    hipLaunchKernelGGL(observe_kernel<ObserveRowsArgs>, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), lds, static_cast<hipStream_t>(stream), h->dev, a);
    return launched(h);
}

int nmpc_policy_rollout_set_states(void* torque, float* Q, float* V, int qv_rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    t->states = {};
    if (Q || V) { t->states.Q = Q; t->states.V = V; t->states.rows = qv_rows; }
    return NMPC_OK;
}

int nmpc_policy_rollout_set_observed(void* torque, float* O, int o_rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    t->observed = {};
    if (O) { t->observed.O = O; t->observed.rows = o_rows; }
    return NMPC_OK;
}

int nmpc_policy_rollout_set_history(void* torque, float* hist, int n_obs, float* act, int n_act, float* W, int w_rows, int rows) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (hist) {                                           // what was attached stays
        if (const char* why = history_depth_refusal(hist, n_obs, act, n_act)) return fail(t, NMPC_E_ARG, why);
        if (rows < 1) return fail(t, NMPC_E_ARG, "history: rows must be at least 1");
        if (W && w_rows < 1) return fail(t, NMPC_E_ARG, "history: w_rows must be at least 1");
    }
    t->history = {};
    if (hist) {
        t->history.hist = hist; t->history.n_obs = n_obs; t->history.act = n_act > 0 ? act : nullptr; t->history.n_act = n_act;
        t->history.W = W; t->history.w_rows = W ? w_rows : 0; t->history.rows = rows;
    }
    return NMPC_OK;
}

int nmpc_history_push_batch(void* torque, int B, float* hist, int n_obs, const float* act, int n_act, const float* goal, int n_goal,
                            const double* s_mean, const double* s_std, int s_first, float* W, int w_stride, float* X, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (const char* why = history_push_refusal(t, B, hist, n_obs, act, n_act, goal, n_goal, s_mean, s_std, s_first, W, w_stride, X))
        return fail(t, NMPC_E_ARG, why);
    NMPC_ENTER(t, t->device);
    return launch_history_push(t, B, hist, n_obs, act, n_act, goal, n_goal, s_mean, s_std, s_first, W, w_stride, X, stream);
}

int nmpc_history_push_actions_batch(void* torque, int B, float* act, int n_act, const float* A, int a_stride, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (!whole_body_tree(t->host)) return fail(t, NMPC_E_ARG, "history: the action register needs the whole-body tree: n_joints = 18, n_actuated = 12, n_feet = 4");
    if (B < 1) return fail(t, NMPC_E_ARG, "history: need B >= 1");
    if (n_act < 1 || n_act > NMPC_HISTORY_MAX) return fail(t, NMPC_E_ARG, "history: n_act must be in [1, NMPC_HISTORY_MAX] to push an action");
    if (!act || !A) return fail(t, NMPC_E_ARG, "history: act and A are needed");
    if (a_stride < HIST_NU) return fail(t, NMPC_E_ARG, "history: a_stride must be at least 12");
    NMPC_ENTER(t, t->device);
    return launch_history_push_actions(t, B, act, n_act, A, a_stride, stream);
}

int nmpc_policy_rollout_batch(void* torque, void* policy, int B, const nmpc_policy_rollout_cfg* cfg, const nmpc_contact_cfg* ground,
                              float* q, float* v, const float* tau_ff, const float* goal, const double* s_mean, const double* s_std,
                              float* S, float* A, float* X, int* failed, void* stream) {
    Torque* t = static_cast<Torque*>(torque);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null torque handle");
    if (B == 0) return NMPC_OK;
    if (!policy) return fail(t, NMPC_E_ARG, "policy is NULL");
    if (!cfg) return fail(t, NMPC_E_ARG, "the rollout cfg is NULL");
    if (B < 0 || !q || !v || !goal || !X) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, goal, X");
    if (cfg->n_steps < 1) return fail(t, NMPC_E_ARG, "n_steps must be at least 1");
    if (const char* why = step_refusal(cfg->n_sub, cfg->dt)) return fail(t, NMPC_E_ARG, why);
    if (!std::isfinite(cfg->kp)) return fail(t, NMPC_E_ARG, "kp must be finite");
    if (const char* why = observe_refusal(t, B, q, v, cfg->period, goal, cfg->n_goal, s_mean, s_std, cfg->s_first, nullptr, 0, X))
        return fail(t, NMPC_E_ARG, why);
    if (const char* why = contact_cfg_refusal(ground)) return fail(t, NMPC_E_ARG, std::string("ground: ") + why);
    nmpc_policy_dims d{};
    int policy_device = -1;
    if (nmpc_policy_get_dims(policy, &d, &policy_device) != NMPC_OK) return fail(t, NMPC_E_ARG, "policy is not a policy handle");
    const auto& hs = t->history;
    if (hs.hist && (d.n_in != hs.n_wide() + cfg->n_goal || d.n_out != t->host.nu))
        return fail(t, NMPC_E_ARG, "history: the policy must map n_wide + n_goal inputs to 12 actions");
    if (!hs.hist && (d.n_in != OB_STATE + cfg->n_goal || d.n_out != t->host.nu))
        return fail(t, NMPC_E_ARG, "the policy must map 44 + n_goal inputs to 12 actions");
    if (B > d.batch_max) return fail(t, NMPC_E_ARG, "B exceeds the policy's batch_max");
    if (policy_device != t->device) return fail(t, NMPC_E_ARG, "the policy lives on another device");
    const auto& rec = t->states;
    if (!rec.Q != !rec.V) return fail(t, NMPC_E_ARG, "states: Q and V come together or not at all");
    if (rec.Q && rec.rows < cfg->n_steps) return fail(t, NMPC_E_ARG, "states: qv_rows must be at least n_steps");
    const auto& seen = t->observed;
    if (seen.O && seen.rows < cfg->n_steps) return fail(t, NMPC_E_ARG, "observed: o_rows must be at least n_steps");
    if (hs.hist && B > hs.rows) return fail(t, NMPC_E_ARG, "history: B exceeds rows");
    if (hs.W && hs.w_rows < cfg->n_steps) return fail(t, NMPC_E_ARG, "history: w_rows must be at least n_steps");
    if (const char* why = plant_batch_refusal(t, t->push, t->windows, B)) return fail(t, NMPC_E_ARG, why);
    const int nu = t->host.nu, K = cfg->n_steps;
    if (B > t->act_rows) {              // the dense [B][12] actions of a step (nmpc_policy_forward writes dense rows): grown once per larger batch
        NMPC_ENTER(t, t->device);
        if (t->act) NMPC_TRY(t, hipFree(t->act));
        t->act = nullptr; t->act_rows = 0;
        NMPC_TRY(t, hipMalloc(reinterpret_cast<void**>(&t->act), (size_t)B * nu * sizeof(float)));
        t->act_rows = B;
    }
    // the chain of the public calls; row k of S is written in place through its stride, row k of A is copied from the dense actions
    for (int k = 0; k <= K; ++k) {
        const double at = cfg->t0 + (double)(k * cfg->n_sub) * (double)cfg->dt;
        const bool rows = k < K;
        // with O attached and no S, the observation writes the true row into O's row, which is then perturbed in place
        float* const o_row = rows && seen.O ? seen.O + (size_t)k * OB_STATE : nullptr;
        // with a history attached and neither S nor O, it writes it into slot 0 of the register, which is perturbed in place alike
        float* const h_row = rows ? hs.hist : nullptr;
        float* const s_row = rows && S ? S + (size_t)k * OB_STATE : (o_row ? o_row : h_row);
        const int s_stride = (S || !seen.O) ? (!S && h_row ? hs.n_obs * OB_STATE : K * OB_STATE) : seen.rows * OB_STATE;
        const long long noise_step = t->noise.step;      // the step this observation draws X at, read before it moves on
        if (const int rc = nmpc_observe_batch(t, B, q, v, at, cfg->period, goal, cfg->n_goal, s_mean, s_std, cfg->s_first, cfg->collision_height,
                                              s_row, s_stride, rows ? X : nullptr, failed, k, cfg->term_mask, stream))
            return rc;
        if (!rows) break;
        if (h_row) {                    // the same draw into the incoming slot of the register, in front of O's launch: o_row may hold the true row
            NMPC_ENTER(t, t->device);
            if (const int rc = launch_observed_rows(t, B, s_row, s_stride, h_row, hs.n_obs * OB_STATE, noise_step, stream)) return rc;
        }
        if (o_row) {                    // what the sensors showed in control step k: the draw of this step's X on the true row
            NMPC_ENTER(t, t->device);
            if (const int rc = launch_observed_rows(t, B, s_row, s_stride, o_row, seen.rows * OB_STATE, noise_step, stream)) return rc;
        }
        if (rec.Q) {                    // the state before control step k, beside row k of S and A
            NMPC_ENTER(t, t->device);
            const size_t n = (size_t)B * t->host.n;
            hipLaunchKernelGGL(state_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, t->host.n,
                               q, v, rec.Q + (size_t)k * t->host.n, rec.V + (size_t)k * t->host.n, (size_t)rec.rows * t->host.n);
            if (const int rc = launched(t)) return rc;
        }
        if (h_row) {                    // the wide row of control step k into row k of W and, normalised, over the workspace X; the register ages
            NMPC_ENTER(t, t->device);
            const int n_wide = hs.n_wide();
            if (const int rc = launch_history_push(t, B, hs.hist, hs.n_obs, hs.act, hs.n_act, goal, cfg->n_goal, s_mean, s_std, cfg->s_first,
                                                   hs.W ? hs.W + (size_t)k * n_wide : nullptr, hs.w_rows * n_wide, X, stream))
                return rc;
        }
        if (const int rc = nmpc_policy_forward(policy, B, X, t->act, stream)) {
            const char* why = nmpc_policy_last_error(policy);
            return fail(t, rc, std::string("nmpc_policy_forward: ") + (why ? why : ""));
        }
        if (A) {
            NMPC_ENTER(t, t->device);
            if (const int rc = launch_elementwise(t, action_rows_kernel, B, stream, nu, t->act, A + (size_t)k * nu, K * nu)) return rc;
        }
        // the attached push (if any) with its window, or the robots' windows, moved to this step's substeps: s = k n_sub + i
        if (const int rc = contact_step(t, B, cfg->n_sub, cfg->dt, ground, q, v, tau_ff, t->act, cfg->kp, cfg->kd, q, v, nullptr, nullptr, nullptr,
                                        t->push, t->windows, (long long)k * cfg->n_sub, stream))
            return rc;
        if (h_row && hs.n_act > 0) {    // the target just issued into slot 0 of the action register
            NMPC_ENTER(t, t->device);
            if (const int rc = launch_history_push_actions(t, B, hs.act, hs.n_act, t->act, nu, stream)) return rc;
        }
    }
    return NMPC_OK;
}

int nmpc_pd_torques_batch(void* handle, int B, const float* tau_ff, const float* q, const float* v, const float* q_plan,
                          const float* v_plan, float kp, float kd, float* tau, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !q || !v || !q_plan || !v_plan || !tau) return fail(t, NMPC_E_ARG, "need B >= 0 and q, v, q_plan, v_plan, tau");
    NMPC_ENTER(t, t->device);
    return launch_elementwise(t, pd_torques_kernel, B, stream, t->host.n, t->host.nu, tau_ff, q, v, q_plan, v_plan, kp, kd, tau);
}

int nmpc_pd_target_action_batch(void* handle, int B, const float* tau, const int* perm, const float* q, const float* v, float kp,
                                float kd, float* action, void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (B == 0) return NMPC_OK;
    if (B < 0 || !tau || !q || !v || !action) return fail(t, NMPC_E_ARG, "need B >= 0 and tau, q, v, action");
    if (!(kp != 0.0f)) return fail(t, NMPC_E_ARG, "kp must not be zero");
    NMPC_ENTER(t, t->device);
    return launch_elementwise(t, pd_target_action_kernel, B, stream, t->host.n, t->host.nu, tau, perm, q, v, kp, kd, action);
}

int nmpc_plan_actions_batch(void* handle, int B, int n_steps, int N, const float* X, const float* U, const int* zoh, double dt_nodes,
                            double sim_dt, float kp, float kd, const int* perm, const int* skip, int skip_mask, float* A, int a_rows,
                            void* stream) {
    Torque* t = static_cast<Torque*>(handle);
    if (!t) return fail(no_handle, NMPC_E_ARG, "null handle");
    if (const char* why = plan_actions_refusal(handle, n_steps, zoh, kp, -1)) return fail(t, NMPC_E_ARG, why);   // a handle fit for plans (include/nmpc_torque.h)
    if (B == 0) return NMPC_OK;
    if (B < 0 || N < 1 || !X || !U || !A) return fail(t, NMPC_E_ARG, "need B >= 0, N >= 1 and X, U, A");
    if (a_rows < n_steps) return fail(t, NMPC_E_ARG, "a_rows must be at least n_steps");
    if (!(dt_nodes > 0.0) || !(sim_dt > 0.0) || n_steps * sim_dt > N * dt_nodes * (1.0 + 1e-9))
        return fail(t, NMPC_E_ARG, "need dt_nodes > 0, sim_dt > 0 and n_steps sim_dt within the horizon N dt_nodes");
    NMPC_ENTER(t, t->device);
    PlanArgs p{};
    p.B = B; p.n_steps = n_steps; p.N = N; p.a_rows = a_rows; p.skip_mask = skip ? skip_mask : 0;
    p.dt_nodes = dt_nodes; p.sim_dt = sim_dt; p.kp = kp; p.kd = kd;
    p.X = X; p.U = U; p.zoh = zoh; p.perm = perm; p.skip = p.skip_mask ? skip : nullptr; p.A = A;
    const size_t pairs = (size_t)B * n_steps;
    hipLaunchKernelGGL(plan_actions_kernel, dim3((unsigned)((pairs + TPB - 1) / TPB)), dim3(TPB), id_lds_bytes(t->host.n),
                       static_cast<hipStream_t>(stream), t->dev, p);
    return launched(t);
}

}  // extern "C"
