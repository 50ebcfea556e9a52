// nmpc_api.hip -- host side of the C-ABI declared in include/nmpc.h (libnmpc_hip.so).
// Single translation unit: kernels are included below.  Build: csrc/build.sh (hipcc, gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/nmpc_torque.h"
#include "nmpc_host.hpp"
#include "nmpc_torque_plan.hpp"
#include "nmpc_solve.hip"
#include "nmpc_wb.hip"
#include "nmpc_aux.hip.inc"
#include "nmpc_rollout.hip.inc"
#include "nmpc_wb_rollout.hip.inc"
#include "nmpc_wb_label.hip.inc"

namespace {

using nmpc::fail;
using nmpc::launched;

struct Handle {
    nmpc_dims dims{};
    int device = 0;
    int nx = 0, nu = 0, np = 0, ng = 0;
    int ny = 0, nye = 0;     // cost residuals of a stage / of the terminal node (lengths of W, yref / W_e, yref_e)
    float* ws = nullptr;
    size_t ws_bytes = 0;
    size_t ws_stride = 0;    // floats per problem
    float* dbg = nullptr;    // diagnostic builds only (nmpc_debug_set_buffer)
    float* roll = nullptr;   // rollout problem tensors: x0 alias, yref, yref_e, params (B_max sized)
    bool rolled = false;     // nmpc_rollout_batch has prepared problems in `roll` (nmpc_debug_read_centroidal_rollout_problem)
    int* label_skip = nullptr;   // nmpc_wb_label_states_batch: per-problem skip flags of a chunk (B_max sized)
    int n_cu = 256;          // compute units of the device
    int force_variant = 0;   // NMPC_QP_VARIANT: 0 chosen per call by batch size and horizon (launch_solve), 1 resident, 2 lean (tests, tuning)
    int all_patterns = 0;    // nmpc_set_contact_patterns: 1 = kernel with a static stage body per contact pattern
    const int* skip = nullptr;   // nmpc_set_skip: problems with skip[b] & skip_mask != 0 are left out of the solves
    int skip_mask = 0;
    struct {                     // nmpc_wb_rollout_set_actions: label buffer of the whole-body rollouts (A == nullptr: none)
        void* torque = nullptr;
        const int* zoh = nullptr;
        float kp = 0.0f, kd = 0.0f;
        float* A = nullptr;
    } labels;
    struct {                     // nmpc_wb_rollout_set_plant: the contact plant of the whole-body rollouts (torque == nullptr: plant = plan)
        void* torque = nullptr;
        nmpc_contact_cfg ground{};
        bool ground_set = false; // the caller gave a cfg (a NULL one is refused when the rollout runs)
        int n_sub = 0;
        float kp = 0.0f, kd = 0.0f;
        const int* zoh = nullptr;
        float *Aw = nullptr, *Qw = nullptr, *Vw = nullptr;
    } plant;
    struct {                     // nmpc_wb_set_momentum_model: the articulated momentum model (torque == nullptr: the declared one)
        void* torque = nullptr;  // borrowed: its tree is the model
        float* mrec = nullptr;   // [B_max][N+1] momentum records (nmpc_wb_momentum.hpp), written by the momentum pass of every SQP iteration
        float* dcons = nullptr;  // [B_max][N+1] dense consistency records, linearisation -> QP kernel
        int state_source = NMPC_WB_STATE_MOMENTUM_DECLARED;   // nmpc_wb_set_state_momentum: where the momentum of a measured state comes from
    } momentum;
    bool plant_push_as_force = false;   // nmpc_wb_rollout_set_plant_push: a plant-mode rollout pushes with a force on the plant, not a velocity jump
    int rollout_replan0 = 0;            // nmpc_wb_rollout_set_clock: replan i of a whole-body rollout is replan rollout_replan0 + i of a longer one
    struct {                            // nmpc_rollout_set_push_windows / nmpc_wb_rollout_set_push_windows (start == nullptr: the cfg's window)
        const float *start = nullptr, *duration = nullptr;   // dev [rows] seconds, caller-owned
        int rows = 0;
    } push_windows;
    int* push_substeps = nullptr;       // [2][B_max]: the windows in substeps of the plant, first substeps then counts (push as a force)
    bool ws_dirty = false;   // a dense-LQ call left foreign padding in the tile workspace
    bool mp_set = false, w_set = false;
    nmpc::ModelParams mp{};
    float W[96]{}, We[96]{};
    bool pos_rows = false;   // whole-body: some foot-placement weight is non-zero
    float reg = 1e-6f, reg_e = 1e-5f;
    int max_sqp = 1, n_ipm = 6, line_search = 0;
    float nlp_tol = 0.0f, qp_tol = 1e-2f;
    float mu0 = 10.0f, sigma = 0.2f, s_min = 1.0f, gamma = 0.995f, tau_min = 0.1f, rho = 1e3f;
    std::string err;
};

Handle* const no_handle = nullptr;      // for nmpc_create: errors go to the family's slot

// what several entry points ask of their handle: room for the batch, and a model and weights to solve with
int check_batch(Handle* h, int B) { return (B < 0 || B > h->dims.B_max) ? fail(h, NMPC_E_ARG, "B exceeds B_max") : NMPC_OK; }
int check_configured(Handle* h) { return (!h->mp_set || !h->w_set) ? fail(h, NMPC_E_STATE, "model parameters / weights not set") : NMPC_OK; }

// the handle's configuration as kernel arguments (pointers and batch size left to the caller): what both families take ...
template <class A>
A handle_args(const Handle* h) {
    A a{};
    a.mp = h->mp;
    std::memcpy(a.W, h->W, sizeof(a.W));        // the tile-family models have ny <= 32, ny_e <= 16
    std::memcpy(a.We, h->We, sizeof(a.We));
    a.reg = h->reg; a.reg_e = h->reg_e;
    a.N = h->dims.N;
    a.max_sqp = h->max_sqp; a.n_ipm = h->n_ipm;
    a.nlp_tol = h->nlp_tol; a.mu0 = h->mu0; a.sigma = h->sigma; a.s_min = h->s_min;
    a.gamma = h->gamma; a.tau_min = h->tau_min;
    a.ws = h->ws;
    a.skip = h->skip_mask ? h->skip : nullptr; a.skip_mask = h->skip_mask;
    return a;
}
// ... and what each takes alone: the tile family (SolveArgs, nmpc_solve_layout.hpp)
nmpc::SolveArgs base_args(const Handle* h) {
    nmpc::SolveArgs a = handle_args<nmpc::SolveArgs>(h);
    for (int j = 0; j < 16; ++j)
        a.rs_free[j] = (j < h->nu) ? 1.0f / std::sqrt(h->W[h->nx + j] + h->reg) : 1.0f;
    a.line_search = h->line_search; a.rho = h->rho;
    a.dbg = h->dbg;
    return a;
}

template <class M>
size_t ws_floats_per_problem(int N) { return nmpc::WsLayout<M>(N).stride; }

// the whole-body model (nmpc_wb.hip)
nmpc::wb::WbArgs wb_args(const Handle* h) {
    nmpc::wb::WbArgs a = handle_args<nmpc::wb::WbArgs>(h);
    a.precision = h->dims.precision;
    a.pos_rows = h->pos_rows ? 1 : 0;
    return a;
}

// a dense-LQ call or a change of the weights left foreign values in the tile workspace: back to zeros before the next solve
int clean_workspace(Handle* h, hipStream_t st) {
    if (h->ws_dirty) {
        NMPC_TRY(h, hipMemsetAsync(h->ws, 0, h->ws_bytes, st));
        h->ws_dirty = false;
    }
    return NMPC_OK;
}

// The SQP loop of both families.  One iteration = linearise (thread per stage) + QP/step (wave per problem); linearize is
// absent where the QP kernel linearises itself.  Problems that finish early (converged, NaN, QP failure) set their workspace
// flag and later launches skip them.  `before(a)` runs in front of every iteration's launches with that iteration's arguments and
// returns a code (the momentum pass of the articulated whole-body model); `extra`: what the kernels take beside the argument block.
template <class A, class Before, class... Extra>
int launch_sqp(Handle* h, A a, hipStream_t st, size_t lds_bytes, void (*qp)(const A, const Extra...), void (*linearize)(const A, const Extra...),
               Before before, const Extra&... extra) {
    if (lds_bytes > 64 * 1024)
        NMPC_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(qp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const long long nthreads = (long long)a.B * (a.N + 1);
    const unsigned lin_blocks = (unsigned)((nthreads + 63) / 64);
    const int shift = a.shift;
    for (int it = 0; it < a.max_sqp; ++it) {
        a.it = it;
        a.shift = (it == 0) ? shift : 0;     // later iterations read their own iterate
        if (const int rc = before(a)) return rc;
        if (linearize) hipLaunchKernelGGL(linearize, dim3(lin_blocks), dim3(64), 0, st, a, extra...);
        hipLaunchKernelGGL(qp, dim3(a.B), dim3(64), lds_bytes, st, a, extra...);
    }
    return launched(h);
}
template <class A>
int launch_sqp(Handle* h, A a, hipStream_t st, size_t lds_bytes, void (*qp)(const A), void (*linearize)(const A)) {
    return launch_sqp(h, a, st, lds_bytes, qp, linearize, [](const A&) { return (int)NMPC_OK; });
}

int launch_wb(Handle* h, nmpc::wb::WbArgs a, hipStream_t st) {
    if (h->line_search) return fail(h, NMPC_E_ARG, "the whole-body model takes full steps (line_search = 0)");
    // the linearisation reads rows of 42, 30, 90 / 66 floats in 8 B pieces and parameter rows in 16 B pieces (include/nmpc.h)
    auto misaligned = [](const void* p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1u)) != 0; };
    if (misaligned(a.x0, 8) || misaligned(a.yref, 8) || misaligned(a.yref_e, 8) || misaligned(a.X, 8) || misaligned(a.U, 8) || misaligned(a.params, 16))
        return fail(h, NMPC_E_ARG, "whole-body arrays must be 8 B aligned (params: 16 B)");
    const size_t lds_bytes = (size_t)nmpc::wb::WbLds(a.N).total * sizeof(float);
    if (!h->momentum.torque) return launch_sqp(h, a, st, lds_bytes, nmpc::wb::nmpc_wb_qp_kernel, nmpc::wb::nmpc_wb_linearize_kernel);
    // the articulated momentum model: the momentum pass of the torque family in front of every linearisation (it reads the iterate
    // through the same warm-start shift and leaves out the same finished problems) and the articulated compilation of both kernels
    const auto& mm = h->momentum;
    if (const char* why = nmpc_torque::momentum_refusal(mm.torque, h->device)) return fail(h, NMPC_E_STATE, std::string("momentum model: ") + why);
    const nmpc::wb::WbArtArgs m{mm.mrec, mm.dcons, nmpc_torque::tree_mass(mm.torque)};
    const nmpc::wb::WsLayout wl(a.N);
    auto momentum_pass = [&](const nmpc::wb::WbArgs& w) {
        const int* done = w.it > 0 ? reinterpret_cast<const int*>(w.ws + wl.flag) : nullptr;      // the finished flag of problem 0
        const int rc = nmpc_torque::momentum_records(mm.torque, w.B, w.N, w.shift, w.X, w.skip, w.skip_mask, done, wl.stride, mm.mrec, st);
        return rc ? fail(h, rc, std::string("momentum pass: ") + nmpc_torque_last_error(mm.torque)) : (int)NMPC_OK;
    };
    return launch_sqp(h, a, st, lds_bytes, nmpc::wb::nmpc_wb_qp_art_kernel, nmpc::wb::nmpc_wb_linearize_art_kernel, momentum_pass, m);
}

// the entry points that build x0's momentum from the declared map refuse a handle in the articulated mode, unless the momentum
// of the tree is put into x0 behind them (nmpc_wb_set_state_momentum)
int check_declared_momentum(Handle* h, const char* who) {
    if (!h->momentum.torque || h->momentum.state_source != NMPC_WB_STATE_MOMENTUM_DECLARED) return NMPC_OK;
    return fail(h, NMPC_E_STATE, std::string(who) + " builds the momentum of x0 from the declared map: not available "
                                                    "with the articulated momentum model (nmpc_wb_set_momentum_model)");
}

// a call of the torque layer (include/nmpc_torque.h) made for an entry point of this one: OK, or its code with "<call>: <the layer's message>"
int torque_call(Handle* h, int rc, const char* call, void* torque) {
    return rc ? fail(h, rc, std::string(call) + ": " + nmpc_torque_last_error(torque)) : (int)NMPC_OK;
}

// the whole-body rollouts' and the labeller's carve-up of h->roll: every array starts on a 16 B boundary (launch_wb checks)
struct WbRoll { float *yref, *yref_e, *params, *x0; };
WbRoll wb_roll(const Handle* h) {
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t B_max = (size_t)h->dims.B_max, N = (size_t)h->dims.N;
    WbRoll r{};
    r.yref = h->roll;
    r.yref_e = r.yref + up4(B_max * N * h->ny);
    r.params = r.yref_e + up4(B_max * h->nye);
    r.x0 = r.params + up4(B_max * (N + 1) * h->np);
    return r;
}

// the centroidal rollouts' carve-up of h->roll: the three arrays back to back
struct CentroidalRoll { float *yref, *yref_e, *params; };
CentroidalRoll centroidal_roll(const Handle* h) {
    const size_t B_max = (size_t)h->dims.B_max, N = (size_t)h->dims.N;
    CentroidalRoll r{};
    r.yref = h->roll;
    r.yref_e = r.yref + B_max * N * h->ny;
    r.params = r.yref_e + B_max * h->nye;
    return r;
}

// the momentum model's tree gives x0 its momentum (never without the articulated mode: nmpc_wb_set_momentum_model resets the switch)
bool tree_state_momentum(const Handle* h) { return h->momentum.torque && h->momentum.state_source == NMPC_WB_STATE_MOMENTUM_TREE; }

// h = A_g(q) v of the momentum model's tree for `count` plant states, into the momentum slots of their x0 and of node 0 of their X
int launch_state_momentum(Handle* h, int count, const float* q, const float* v, int qv_stride, float* x0, float* X, const int* skip,
                          int skip_mask, hipStream_t st) {
    void* torque = h->momentum.torque;
    const int rc = nmpc_state_momentum_batch(torque, count, q, v, qv_stride, x0 + nmpc::wb::WH, nmpc::wb::NX, X + nmpc::wb::WH,
                                             (h->dims.N + 1) * nmpc::wb::NX, skip, skip_mask, st);
    return torque_call(h, rc, "nmpc_state_momentum_batch", torque);
}

// what the prepare kernels of the whole-body rollouts and of the labeller take alike (r: WbRolloutArgs or WbLabelArgs): the carve-up of
// h->roll and the model parameters -- where the tree gives x0 its momentum with the mass of the tree, the one the dynamics carry, in the
// force reference's weight share and in a push's velocity jump
template <class R>
int set_wb_problem(Handle* h, R& r) {
    const WbRoll roll = wb_roll(h);
    r.yref = roll.yref; r.yref_e = roll.yref_e; r.params = roll.params; r.x0 = roll.x0;
    r.mp = h->mp;
    if (!tree_state_momentum(h)) return NMPC_OK;
    if (const char* why = nmpc_torque::momentum_refusal(h->momentum.torque, h->device)) return fail(h, NMPC_E_STATE, std::string("momentum model: ") + why);
    r.mp.mass = nmpc_torque::tree_mass(h->momentum.torque);
    return NMPC_OK;
}

// The labeller's problems m0 .. m0 + count, problem m = b K + k, against a table of `rows` rows per robot: where the table has exactly K
// rows per robot they are one dense run of it, otherwise one run per robot.  each(i, run, row) -> code: `run` problems from the chunk's
// problem i on, whose first lies at row `row` of the table; the first code that is not OK ends the walk
template <class Each>
int runs_by_robot(long long m0, int count, int K, int rows, Each each) {
    for (long long m = m0; m < m0 + count;) {
        const long long b = m / K, k = m - b * K;
        const int run = rows == K ? count : (int)((K - k < m0 + count - m) ? K - k : m0 + count - m);
        if (const int rc = each((size_t)(m - m0), run, (size_t)b * rows + k)) return rc;
        m += run;
    }
    return NMPC_OK;
}

// Two variants of the QP kernel (nmpc_qp.hip.inc; Lds, nmpc_solve_layout.hpp).  Resident: stage arrays in the LDS (39.6 KB at N = 50: four waves per CU),
// pinned to one wave per SIMD -- the choice while the batch fits that many waves (B <= 4 x CUs: 2.2 M solves/s at B = 1024).
// Lean: stage arrays in the workspace, 17.7 KB, two waves per SIMD -- the choice for larger batches, where the second wave fills
// the first one's dependency stalls (2.7 M at B = 8192 against 2.3 M resident), for horizons whose resident layout does not
// fit the LDS, and NMPC_QP_VARIANT=lean.  Both run the same arithmetic in the same order (bit-identical results, tested).
template <class M, bool LEAN, bool BF16B, bool ALLV>
int launch_qp(Handle* h, nmpc::SolveArgs a, hipStream_t st) {
    const size_t bytes = (size_t)nmpc::Lds<M, LEAN>(a.N).total * sizeof(float);
    if (bytes > 160 * 1024) return fail(h, NMPC_E_ARG, "horizon too long for the LDS-resident layout");
    // (the code object keeps its kernels in the order they are named in: the QP kernel first)
    void (*const qp)(const nmpc::SolveArgs) = nmpc::nmpc_qp_kernel<M, LEAN, BF16B, ALLV>;
    void (*const linearize)(const nmpc::SolveArgs) = nmpc::nmpc_linearize_kernel<M>;
    return launch_sqp(h, a, st, bytes, qp, nmpc::qp_linearizes_itself(LEAN, a.N) ? nullptr : linearize);
}

template <class M>
int launch_solve(Handle* h, nmpc::SolveArgs a, hipStream_t st) {
    if (a.N > 64 * nmpc::N_LANE_STAGES) return fail(h, NMPC_E_ARG, "horizon too long for the lane = stage phases");
    // problems in flight: a CU holds as many waves as its 160 KB of LDS take, at most one (resident) or two (lean) per SIMD
    auto in_flight = [&](size_t lds_bytes, long long per_simd) -> long long {
        if (lds_bytes > 160 * 1024) return 0;
        const long long by_lds = (long long)((160 * 1024) / lds_bytes);
        return (long long)h->n_cu * (by_lds < 4 * per_simd ? by_lds : 4 * per_simd);
    };
    const long long resident_waves = in_flight((size_t)nmpc::Lds<M, false>(a.N).total * sizeof(float), 1);
    const long long lean_waves = in_flight((size_t)nmpc::Lds<M, true>(a.N).total * sizeof(float), 2);
    const bool lean = h->force_variant ? (h->force_variant > 1)
                                       : (resident_waves == 0 || ((long long)a.B > resident_waves && lean_waves > resident_waves));
    // all static variants only where the model has more than its short list and the caller asked for them
    if constexpr (M::N_STATIC_MASKS > 4) {
        if (h->all_patterns) {
            if (h->dims.precision == 1)
                return lean ? launch_qp<M, true, true, true>(h, a, st) : launch_qp<M, false, true, true>(h, a, st);
            return lean ? launch_qp<M, true, false, true>(h, a, st) : launch_qp<M, false, false, true>(h, a, st);
        }
    }
    if (h->dims.precision == 1)
        return lean ? launch_qp<M, true, true, false>(h, a, st) : launch_qp<M, false, true, false>(h, a, st);
    return lean ? launch_qp<M, true, false, false>(h, a, st) : launch_qp<M, false, false, false>(h, a, st);
}

template <class M>
int read_tile(Handle* h, int b, int k, int which, float* out) {
    using G = nmpc::TileGeom<M>;
    const nmpc::WsLayout<M> wl(h->dims.N);
    const size_t off[4] = {wl.At + (size_t)k * G::A_FLOATS, wl.Bt + (size_t)k * G::B_FLOATS,
                           wl.Kt + (size_t)k * G::K_FLOATS, wl.Ct + (size_t)k * G::C_FLOATS};
    const size_t len[4] = {G::A_FLOATS, G::B_FLOATS, G::K_FLOATS, G::C_FLOATS};
    float img[512];
    NMPC_TRY(h, hipMemcpy(img, h->ws + (size_t)b * wl.stride + off[which], len[which] * sizeof(float),
                         hipMemcpyDeviceToHost));
    std::memset(out, 0, 256 * sizeof(float));
    if (which == 0) {          // A~ : column-major, stride SA, columns 0..nx ; row nx = e_nx
        for (int c = 0; c <= M::NX; ++c)
            for (int i = 0; i < M::NX; ++i) out[i * 16 + c] = img[c * G::SA + i];
        out[M::NX * 16 + M::NX] = 1.0f;
    } else if (which == 1) {   // B~
        for (int c = 0; c < M::NU; ++c)
            for (int i = 0; i < M::NX; ++i) out[i * 16 + c] = img[c * G::SA + i];
    } else {                   // K~ (nu rows) / Acl~ (nx rows): row-major, 16 floats per row, columns by slot
        const int rows = which == 2 ? M::NU : M::NX;
        for (int i = 0; i < rows; ++i) {
            for (int c = 0; c < M::NX; ++c) out[i * 16 + c] = img[i * 16 + nmpc::slot_of(c)];
            out[i * 16 + M::NX] = img[i * 16 + nmpc::HS];
        }
        if (which == 3) out[M::NX * 16 + M::NX] = 1.0f;
    }
    return NMPC_OK;
}
// The replan loop of both device rollouts (LocomotionMPC.open_loop, mpc.py:416-462): per replan  prepare -> solve -> advance,
// all on the caller's stream.  r: the plant's kernel arguments, its own fields, the carve-up of h->roll and the caller's pointers
// filled in; a: the arguments of its solve with x0 and status.  plan(i) sets what the plant alone knows of replan i (its node)
// and returns the warm-start shift of its solve; after_prepare() runs between the prepare kernel and the solve, after_solve(i)
// between the solve and the advance kernel.  replan0: where replan 0 of this call sits in the rollout (nmpc_wb_rollout_set_clock; the
// centroidal harness passes 0) -- replan i has the time, the push window and the stamp of replan replan0 + i and writes the rows
// i * rows_per_replan .. of this call's S.
template <class Cfg, class R, class A, class Plan, class AfterPrepare, class AfterSolve>
int run_rollout(Handle* h, int B, const Cfg* cfg, int replan0, hipStream_t st, R& r, A& a, void (*prepare)(const R),
                int (*solve)(Handle*, A, hipStream_t), void (*advance)(const R), Plan plan, AfterPrepare after_prepare,
                AfterSolve after_solve) {
    NMPC_ENTER(h, h->device);
    if (const int rc = clean_workspace(h, st)) return rc;
    const int N = h->dims.N;
    r.B = B; r.N = N; r.npc = cfg->nodes_per_cycle; r.replanning_steps = cfg->replanning_steps; r.n_replans = cfg->n_replans;
    r.record_sim_steps = cfg->record_sim_steps ? 1 : 0;
    r.sim_dt = cfg->sim_dt; r.t_horizon = cfg->time_horizon; r.nom_height = cfg->nom_height; r.height_offset = cfg->height_offset;
    r.dt_nodes = cfg->time_horizon / N;
    r.nominal_period = cfg->nominal_period; r.collision_height = cfg->collision_height;
    r.term_mask = cfg->terminate_mask & NMPC_ROLLOUT_FLAG_MASK;
    const int rows_per_replan = r.record_sim_steps ? cfg->replanning_steps : 1;
    r.n_rows = cfg->n_replans * rows_per_replan;
    a.B = B; a.yref_per_stage = 1;
    a.yref = r.yref; a.yref_e = r.yref_e; a.params = r.params; a.X = r.X; a.U = r.U; a.stats = nullptr;
    a.skip = r.term_mask ? r.failed : nullptr; a.skip_mask = r.term_mask;     // terminated rollouts cost no solve
    const double dt_replan = cfg->replanning_steps * cfg->sim_dt, slack = 0.5 * cfg->sim_dt;
    for (int i = 0; i < cfg->n_replans; ++i) {
        const bool cold = cfg->first_solve && i == 0;
        r.first = cold ? 1 : 0;
        r.replan_index = replan0 + i;
        r.row0 = i * rows_per_replan;
        // the push window in replanning intervals, half a simulation step of slack on both ends: with plain float compares
        // 5 * 0.04f = 0.19999999 misses a window that starts at 0.2 (the host loop, in doubles, does not)
        const double t_now = (replan0 + i) * dt_replan;
        r.t_now = t_now; r.win_slack = slack; r.dt_replan = dt_replan;      // with a window per rollout the advance kernel decides (apply_push)
        r.push_dt = (r.push_force && cfg->push_duration > 0.0f && t_now >= (double)cfg->push_start - slack &&
                     t_now < (double)cfg->push_start + (double)cfg->push_duration - slack) ? (float)dt_replan : 0.0f;
        const int shift = plan(i);
        hipLaunchKernelGGL(prepare, dim3(B), dim3(64), 0, st, r);
        if (const int rc = after_prepare()) return rc;
        a.shift = cold ? 0 : (shift > N ? N : shift);             // warm start folded into the solve
        a.max_sqp = cold ? cfg->max_sqp_first : h->max_sqp;
        a.nlp_tol = cold ? cfg->nlp_tol_first : cfg->nlp_tol;
        if (const int rc = solve(h, a, st)) return rc;
        if (const int rc = after_solve(i)) return rc;
        hipLaunchKernelGGL(advance, dim3((B + 63) / 64), dim3(64), 0, st, r);
    }
    return launched(h);
}

// why the attached push windows cannot serve a rollout of B rollouts (nullptr: they can, or there are none)
const char* push_windows_refusal(const Handle* h, int B, const float* push_force) {
    if (!h->push_windows.start) return nullptr;
    if (!push_force) return "push windows: the rollout has no push_force";
    if (B > h->push_windows.rows) return "push windows: B exceeds rows";
    return nullptr;
}

// nmpc_rollout_set_push_windows and nmpc_wb_rollout_set_push_windows on a handle of `model_id`
int set_push_windows(Handle* h, int model_id, const char* who, const float* start, const float* duration, int rows) {
    if (!h) return NMPC_E_ARG;
    if (h->dims.model_id != model_id)
        return fail(h, NMPC_E_ARG, std::string(who) + (model_id == NMPC_MODEL_WHOLEBODY ? " needs the whole-body model" : " needs the centroidal model"));
    if (!start && !duration) { h->push_windows = {}; return NMPC_OK; }
    if (!start || !duration) return fail(h, NMPC_E_ARG, "push windows: start and duration come together or not at all");      // what was attached stays
    if (rows < 1) return fail(h, NMPC_E_ARG, "push windows: rows must be at least 1");
    h->push_windows.start = start; h->push_windows.duration = duration; h->push_windows.rows = rows;
    return NMPC_OK;
}

// the device side of nmpc_create, on the handle's device; what was allocated before an error is nmpc_destroy's to free
int allocate(Handle* h) {
    NMPC_TRY(no_handle, hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    NMPC_TRY(no_handle, hipMalloc(reinterpret_cast<void**>(&h->ws), h->ws_bytes));
    NMPC_TRY(no_handle, hipMemset(h->ws, 0, h->ws_bytes));
    const int N = h->dims.N;
    const size_t per = (size_t)N * h->ny + h->nye + (size_t)(N + 1) * (h->np > 0 ? h->np : 1) + h->nx;   // yref, yref_e, params, x0 of the rollouts
    NMPC_TRY(no_handle, hipMalloc(reinterpret_cast<void**>(&h->roll), ((size_t)h->dims.B_max * per + 16) * sizeof(float)));   // (+ the 16 B roundings of the carve-up)
    NMPC_TRY(no_handle, hipMalloc(reinterpret_cast<void**>(&h->label_skip), (size_t)h->dims.B_max * sizeof(int)));
    NMPC_TRY(no_handle, hipMemset(h->label_skip, 0, (size_t)h->dims.B_max * sizeof(int)));
    NMPC_TRY(no_handle, hipMalloc(reinterpret_cast<void**>(&h->push_substeps), 2 * (size_t)h->dims.B_max * sizeof(int)));
    return NMPC_OK;
}
}  // namespace

extern "C" {

int nmpc_model_dims(int model_id, int* nx, int* nu, int* np, int* ng) {
    int d[4];
    if (model_id == NMPC_MODEL_DOUBLE_INTEGRATOR) {
        d[0] = nmpc::DoubleIntegrator::NX; d[1] = nmpc::DoubleIntegrator::NU;
        d[2] = nmpc::DoubleIntegrator::NP; d[3] = nmpc::DoubleIntegrator::NG;
    } else if (model_id == NMPC_MODEL_CENTROIDAL) {
        d[0] = nmpc::Centroidal::NX; d[1] = nmpc::Centroidal::NU;
        d[2] = nmpc::Centroidal::NP; d[3] = nmpc::Centroidal::NG;
    } else if (model_id == NMPC_MODEL_WHOLEBODY) {
        d[0] = nmpc::wb::NX; d[1] = nmpc::wb::NU; d[2] = nmpc::wb::NP; d[3] = nmpc::wb::NG;
    } else {
        return NMPC_E_ARG;
    }
    if (nx) *nx = d[0];
    if (nu) *nu = d[1];
    if (np) *np = d[2];
    if (ng) *ng = d[3];
    return NMPC_OK;
}

int nmpc_model_output_dims(int model_id, int* ny, int* ny_e) {
    int nx, nu;
    if (nmpc_model_dims(model_id, &nx, &nu, nullptr, nullptr)) return NMPC_E_ARG;
    const bool wbm = model_id == NMPC_MODEL_WHOLEBODY;
    if (ny) *ny = wbm ? nmpc::wb::NY : nx + nu;
    if (ny_e) *ny_e = wbm ? nmpc::wb::NYE : nx;
    return NMPC_OK;
}

int nmpc_create(const nmpc_dims* dims, int device_id, void** handle) {
    if (!dims || !handle) return fail(no_handle, NMPC_E_ARG, "null argument");
    *handle = nullptr;
    int nx, nu, np, ng;
    if (nmpc_model_dims(dims->model_id, &nx, &nu, &np, &ng)) return fail(no_handle, NMPC_E_ARG, "unknown model_id");
    if (dims->N < 1 || dims->B_max < 1) return fail(no_handle, NMPC_E_ARG, "N and B_max must be positive");
    if (dims->precision < 0 || dims->precision > 3 || (dims->precision >= 2 && dims->model_id != NMPC_MODEL_WHOLEBODY))
        return fail(no_handle, NMPC_E_ARG, "precision must be 0 (fp32), 1 (bf16 contraction) or, whole-body only, 2 (split bf16) / 3 (three-way split bf16)");
    if (dims->model_id == NMPC_MODEL_WHOLEBODY && dims->N > 64)
        return fail(no_handle, NMPC_E_ARG, "the whole-body model needs N <= 64 (lane = stage phases)");
    NMPC_ENTER(no_handle, device_id);
    Handle* h = new Handle();
    h->dims = *dims;
    h->device = device_id;
    h->nx = nx; h->nu = nu; h->np = np; h->ng = ng;
    nmpc_model_output_dims(dims->model_id, &h->ny, &h->nye);
    if (const char* v = std::getenv("NMPC_QP_VARIANT")) {
        if (!std::strcmp(v, "resident")) h->force_variant = 1;
        else if (!std::strcmp(v, "lean")) h->force_variant = 2;
    }
    h->ws_stride = (dims->model_id == NMPC_MODEL_DOUBLE_INTEGRATOR) ? ws_floats_per_problem<nmpc::DoubleIntegrator>(dims->N)
                 : (dims->model_id == NMPC_MODEL_CENTROIDAL)      ? ws_floats_per_problem<nmpc::Centroidal>(dims->N)
                                                                  : nmpc::wb::WsLayout(dims->N).stride;
    // the kernels place problem b at b * ws_stride (their own WsLayout); nmpc_riccati_kernel places it at b * 2N tiles (K~', Acl~'),
    // more than the double integrator's solve layout from N = 3 on: the allocation holds whichever is larger
    size_t per_problem = h->ws_stride;
    if (dims->model_id != NMPC_MODEL_WHOLEBODY) per_problem = std::max(per_problem, nmpc::riccati_ws_floats(dims->N));
    h->ws_bytes = (size_t)dims->B_max * per_problem * sizeof(float);
    if (const int rc = allocate(h)) { nmpc_destroy(h); return rc; }
    *handle = h;
    return NMPC_OK;
}

void nmpc_destroy(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return;
    nmpc::DeviceGuard guard(h->device);      // nothing to return: a failed switch goes to the family's slot, the buffers are freed all the same
    if (guard.err != hipSuccess) fail(no_handle, NMPC_E_HIP, std::string("nmpc_destroy: ") + hipGetErrorString(guard.err));
    if (h->ws) (void)hipFree(h->ws);
    if (h->roll) (void)hipFree(h->roll);
    if (h->label_skip) (void)hipFree(h->label_skip);
    if (h->push_substeps) (void)hipFree(h->push_substeps);
    if (h->momentum.mrec) (void)hipFree(h->momentum.mrec);
    if (h->momentum.dcons) (void)hipFree(h->momentum.dcons);
    delete h;
}

const char* nmpc_last_error(void* handle) { return nmpc::last_error(static_cast<Handle*>(handle)); }

size_t nmpc_workspace_bytes(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    return h ? h->ws_bytes : 0;
}

int nmpc_set_model_params(void* handle, const float* mp, int count) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !mp) return fail(h, NMPC_E_ARG, "null argument");
    if (count != NMPC_MP_COUNT) return fail(h, NMPC_E_ARG, "model parameter vector must have NMPC_MP_COUNT entries");
    if (!(mp[NMPC_MP_DT] > 0.0f)) return fail(h, NMPC_E_ARG, "dt must be positive");
    if (h->dims.model_id != NMPC_MODEL_DOUBLE_INTEGRATOR &&
        !(mp[NMPC_MP_MASS] > 0 && mp[NMPC_MP_IXX] > 0 && mp[NMPC_MP_IYY] > 0 && mp[NMPC_MP_IZZ] > 0))
        return fail(h, NMPC_E_ARG, "mass and inertia must be positive");
    if (h->dims.model_id == NMPC_MODEL_WHOLEBODY && !(mp[NMPC_MP_L1] > 0 && mp[NMPC_MP_L2] > 0 && mp[NMPC_MP_PGAIN] >= 0))
        return fail(h, NMPC_E_ARG, "link lengths must be positive, p_gain non-negative");
    h->mp = nmpc::ModelParams{mp[0], mp[1], mp[2], mp[3], mp[4], mp[5], mp[6], mp[7],
                              mp[8], mp[9], mp[10], mp[11], mp[12], mp[13], mp[14], mp[15]};
    h->mp_set = true;
    return NMPC_OK;
}

int nmpc_set_weights(void* handle, const float* W, const float* W_e, float reg, float reg_e) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !W || !W_e) return fail(h, NMPC_E_ARG, "null argument");
    for (int i = 0; i < h->ny; ++i) {
        if (!(W[i] >= 0.0f)) return fail(h, NMPC_E_ARG, "weights must be non-negative");
        h->W[i] = W[i];
    }
    for (int i = 0; i < h->nye; ++i) {
        if (!(W_e[i] >= 0.0f)) return fail(h, NMPC_E_ARG, "weights must be non-negative");
        h->We[i] = W_e[i];
    }
    if (!(reg >= 0.0f) || !(reg_e >= 0.0f)) return fail(h, NMPC_E_ARG, "regularisation must be non-negative");
    h->reg = reg; h->reg_e = reg_e;
    h->w_set = true;
    if (h->dims.model_id == NMPC_MODEL_WHOLEBODY) {
        bool pos = false;
        for (int i = 0; i < 8; ++i) pos = pos || W[nmpc::wb::RY_POS + i] > 0.0f || W_e[nmpc::wb::RE_POS + i] > 0.0f;
        if (h->pos_rows && !pos) h->ws_dirty = true;     // the foot-placement rows of the Js images go back to exact zeros
        h->pos_rows = pos;
    }
    return NMPC_OK;
}

int nmpc_set_opts(void* handle, int max_sqp_iter, int max_qp_iter, float nlp_tol, float qp_tol,
                  int line_search) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (max_sqp_iter < 1 || max_qp_iter < 0) return fail(h, NMPC_E_ARG, "iteration counts out of range");
    h->max_sqp = max_sqp_iter; h->n_ipm = max_qp_iter;
    h->nlp_tol = nlp_tol; h->qp_tol = qp_tol; h->line_search = line_search ? 1 : 0;
    return NMPC_OK;
}

int nmpc_set_contact_patterns(void* handle, int all_patterns) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->all_patterns = all_patterns ? 1 : 0;
    return NMPC_OK;
}

int nmpc_set_skip(void* handle, const int* flags, int mask) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->skip = flags;
    h->skip_mask = flags ? mask : 0;
    return NMPC_OK;
}

int nmpc_wb_rollout_set_actions(void* handle, void* torque_handle, const int* zoh, float kp, float kd, float* A) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->labels = {};
    if (A) {
        h->labels.torque = torque_handle; h->labels.zoh = zoh; h->labels.kp = kp; h->labels.kd = kd; h->labels.A = A;
    }
    return NMPC_OK;
}

int nmpc_wb_rollout_set_plant(void* handle, void* torque_handle, const nmpc_contact_cfg* ground, int n_sub, float kp, float kd,
                              const int* zoh, float* Aw, float* Qw, float* Vw) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->plant = {};
    if (torque_handle) {
        auto& p = h->plant;
        p.torque = torque_handle; p.n_sub = n_sub; p.kp = kp; p.kd = kd; p.zoh = zoh; p.Aw = Aw; p.Qw = Qw; p.Vw = Vw;
        if (ground) { p.ground = *ground; p.ground_set = true; }
    }
    return NMPC_OK;
}

int nmpc_wb_set_momentum_model(void* handle, void* torque_handle, int model) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (h->dims.model_id != NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_wb_set_momentum_model needs the whole-body model");
    if (model != NMPC_WB_MOMENTUM_DECLARED && model != NMPC_WB_MOMENTUM_ARTICULATED)
        return fail(h, NMPC_E_ARG, "model is NMPC_WB_MOMENTUM_DECLARED or NMPC_WB_MOMENTUM_ARTICULATED");
    h->momentum.state_source = NMPC_WB_STATE_MOMENTUM_DECLARED;      // never the tree's x0 with the declared dynamics
    if (model == NMPC_WB_MOMENTUM_DECLARED) {      // the buffers of the articulated mode stay with the handle for the next switch
        h->momentum.torque = nullptr;
        return NMPC_OK;
    }
    if (const char* why = nmpc_torque::momentum_refusal(torque_handle, h->device)) return fail(h, NMPC_E_ARG, std::string("momentum model: ") + why);
    NMPC_ENTER(h, h->device);
    const size_t nodes = (size_t)h->dims.B_max * (h->dims.N + 1);
    if (!h->momentum.mrec) NMPC_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->momentum.mrec), nodes * nmpc::wb::MR_FLOATS * sizeof(float)));
    if (!h->momentum.dcons) NMPC_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->momentum.dcons), nodes * nmpc::wb::DC_FLOATS * sizeof(float)));
    h->momentum.torque = torque_handle;
    return NMPC_OK;
}

int nmpc_wb_set_state_momentum(void* handle, int source) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (source != NMPC_WB_STATE_MOMENTUM_DECLARED && source != NMPC_WB_STATE_MOMENTUM_TREE)
        return fail(h, NMPC_E_ARG, "source is NMPC_WB_STATE_MOMENTUM_DECLARED or NMPC_WB_STATE_MOMENTUM_TREE");
    if (source == NMPC_WB_STATE_MOMENTUM_TREE && !h->momentum.torque)
        return fail(h, NMPC_E_STATE, "the momentum of the tree in x0 needs the articulated momentum model (nmpc_wb_set_momentum_model)");
    h->momentum.state_source = source;
    return NMPC_OK;
}

int nmpc_wb_rollout_set_plant_push(void* handle, int as_force) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->plant_push_as_force = as_force != 0;
    return NMPC_OK;
}

int nmpc_rollout_set_push_windows(void* handle, const float* start, const float* duration, int rows) {
    return set_push_windows(static_cast<Handle*>(handle), NMPC_MODEL_CENTROIDAL, "nmpc_rollout_set_push_windows", start, duration, rows);
}

int nmpc_wb_rollout_set_push_windows(void* handle, const float* start, const float* duration, int rows) {
    return set_push_windows(static_cast<Handle*>(handle), NMPC_MODEL_WHOLEBODY, "nmpc_wb_rollout_set_push_windows", start, duration, rows);
}

int nmpc_wb_rollout_set_clock(void* handle, int replan0) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (h->dims.model_id != NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_wb_rollout_set_clock needs the whole-body model");
    if (replan0 < 0) return fail(h, NMPC_E_ARG, "rollout clock: replan0 must not be negative");
    h->rollout_replan0 = replan0;
    return NMPC_OK;
}

int nmpc_set_ipm(void* handle, float mu0, float sigma, float s_min, float gamma, float tau_min,
                 float merit_rho) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (!(mu0 > 0 && sigma > 0 && sigma < 1 && s_min > 0 && gamma > 0 && gamma < 1 && tau_min >= 0 && merit_rho >= 0))
        return fail(h, NMPC_E_ARG, "interior-point constants out of range");
    h->mu0 = mu0; h->sigma = sigma; h->s_min = s_min; h->gamma = gamma; h->tau_min = tau_min; h->rho = merit_rho;
    return NMPC_OK;
}

int nmpc_shift_warm_start(void* handle, int B, int shift, float* X, float* U, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!X || !U) return fail(h, NMPC_E_ARG, "null argument");
    if (const int rc = check_batch(h, B)) return rc;
    if (shift < 0) return fail(h, NMPC_E_ARG, "negative shift");
    if (shift == 0) return NMPC_OK;
    const int N = h->dims.N;
    if (shift > N) shift = N;
    if ((size_t)N * h->nx > 256 * 16 || (size_t)N * h->nu > 256 * 16)
        return fail(h, NMPC_E_ARG, "trajectory too long for the shift kernel");
    NMPC_ENTER(h, h->device);
    hipLaunchKernelGGL(nmpc::nmpc_shift_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       N, h->nx, h->nu, h->dims.model_id == NMPC_MODEL_WHOLEBODY ? nmpc::wb::WF : 0, shift, X, U);
    return launched(h);
}

int nmpc_shift_solve_batch(void* handle, int B, int shift, const float* x0, const float* yref,
                           int yref_per_stage, const float* yref_e, const float* params, float* X, float* U,
                           int* status, float* stats, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;     // an empty batch is a no-op (its tensors have no storage)
    if (!x0 || !yref || !yref_e || !X || !U || (h->np > 0 && !params)) return fail(h, NMPC_E_ARG, "null argument");
    if (const int rc = check_batch(h, B)) return rc;
    if (shift < 0) return fail(h, NMPC_E_ARG, "negative shift");
    if (const int rc = check_configured(h)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    NMPC_ENTER(h, h->device);
    if (const int rc = clean_workspace(h, st)) return rc;
    if (h->dims.model_id == NMPC_MODEL_WHOLEBODY) {
        nmpc::wb::WbArgs w = wb_args(h);
        w.B = B;
        w.shift = shift > h->dims.N ? h->dims.N : shift;
        w.yref_per_stage = yref_per_stage ? 1 : 0;
        w.x0 = x0; w.yref = yref; w.yref_e = yref_e; w.params = params;
        w.X = X; w.U = U; w.status = status; w.stats = stats;
        return launch_wb(h, w, st);
    }
    nmpc::SolveArgs a = base_args(h);
    a.B = B;
    a.shift = shift > h->dims.N ? h->dims.N : shift;
    a.yref_per_stage = yref_per_stage ? 1 : 0;
    a.x0 = x0; a.yref = yref; a.yref_e = yref_e; a.params = params ? params : x0;
    a.X = X; a.U = U; a.status = status; a.stats = stats;
    if (h->dims.model_id == NMPC_MODEL_DOUBLE_INTEGRATOR) return launch_solve<nmpc::DoubleIntegrator>(h, a, st);
    return launch_solve<nmpc::Centroidal>(h, a, st);
}

int nmpc_solve_batch(void* handle, int B, const float* x0, const float* yref, int yref_per_stage,
                     const float* yref_e, const float* params, float* X, float* U, int* status,
                     float* stats, void* stream) {
    return nmpc_shift_solve_batch(handle, B, 0, x0, yref, yref_per_stage, yref_e, params, X, U, status, stats, stream);
}

int nmpc_riccati_batch(void* handle, int Bsz, int nx, int nu, const float* Q, const float* R,
                       const float* q, const float* r, const float* A, const float* B_,
                       const float* d, const float* dx0, float* dX, float* dU, int* status,
                       void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (Bsz == 0) return NMPC_OK;
    if (!Q || !R || !q || !r || !A || !B_ || !d || !dx0 || !dX || !dU) return fail(h, NMPC_E_ARG, "null argument");
    if (nx < 1 || nx > 15 || nu < 1 || nu > 16) return fail(h, NMPC_E_ARG, "need 1 <= nx <= 15, 1 <= nu <= 16");
    if (h->dims.model_id == NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_riccati_batch needs a handle of the tile-family models");
    if (const int rc = check_batch(h, Bsz)) return rc;
    NMPC_ENTER(h, h->device);
    nmpc::RiccatiArgs a{h->dims.N, Bsz, nx, nu, Q, R, q, r, A, B_, d, dx0, dX, dU, status, h->ws};
    h->ws_dirty = true;
    hipLaunchKernelGGL(nmpc::nmpc_riccati_kernel, dim3(Bsz), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return launched(h);
}

int nmpc_tracking_error(void* handle, int B, int T, int ns, const float* S, const float* S_nom,
                        float* err, float* weight, float threshold, float ood_weight, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (B == 0) return NMPC_OK;
    if (!S || !S_nom || !err) return fail(h, NMPC_E_ARG, "null argument");
    if (B < 0 || T < 1 || ns < 2) return fail(h, NMPC_E_ARG, "need B >= 0, T >= 1, ns >= 2");
    const size_t lds = (size_t)nmpc::TRB * (ns | 1) * sizeof(float);
    if (lds > 64 * 1024) return fail(h, NMPC_E_ARG, "state dimension too large for the staging tile");
    const long long rows = (long long)B * T;
    const long long blocks = (rows + nmpc::TRB - 1) / nmpc::TRB;
    if (blocks > 0x7fffffffLL) return fail(h, NMPC_E_ARG, "too many rows");
    NMPC_ENTER(h, nmpc::device_of(S));
    hipLaunchKernelGGL(nmpc::nmpc_tracking_error_kernel, dim3((unsigned)blocks), dim3(nmpc::TRB), lds,
                       static_cast<hipStream_t>(stream), rows, T, ns, S, S_nom, err, weight, threshold,
                       ood_weight);
    return launched(h);
}

int nmpc_rollout_batch(void* handle, int B, const nmpc_rollout_cfg* cfg, const signed char* gait, float* x,
                       const double* v_des, const double* w_des, double* ref_state, float* foot_pos,
                       const float* push_force, const float* phase, float* X, float* U, float* S,
                       int* status, int* failed, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!cfg || !gait || !x || !v_des || !w_des || !ref_state || !foot_pos || !phase || !X || !U || !S || !status || !failed)
        return fail(h, NMPC_E_ARG, "null argument");
    if (h->dims.model_id != NMPC_MODEL_CENTROIDAL) return fail(h, NMPC_E_ARG, "rollouts need the centroidal model");
    if (const int rc = check_batch(h, B)) return rc;
    if (h->dims.N > 128) return fail(h, NMPC_E_ARG, "rollouts need N <= 128");
    if (cfg->n_replans < 1 || cfg->nodes_per_replan < 1 || cfg->nodes_per_replan > h->dims.N ||
        cfg->replanning_steps < 1 || cfg->nodes_per_cycle < 1 || cfg->start_node < 0)
        return fail(h, NMPC_E_ARG, "rollout configuration out of range");
    if (const int rc = check_configured(h)) return rc;
    if (cfg->footsteps && !(cfg->nominal_period > 0.0f)) return fail(h, NMPC_E_ARG, "footsteps need the gait period");
    if (cfg->record_sim_steps &&
        std::fabs(cfg->nodes_per_replan * (cfg->time_horizon / h->dims.N) - cfg->replanning_steps * cfg->sim_dt) > 1e-9)
        return fail(h, NMPC_E_ARG, "per-step recording needs nodes_per_replan * dt_nodes = replanning_steps * sim_dt");
    if (const char* why = push_windows_refusal(h, B, push_force)) return fail(h, NMPC_E_ARG, why);
    nmpc::RolloutArgs r{};
    const CentroidalRoll roll = centroidal_roll(h);
    r.yref = roll.yref; r.yref_e = roll.yref_e; r.params = roll.params;
    r.nodes_per_replan = cfg->nodes_per_replan;
    r.mass = h->mp.mass; r.gz = h->mp.gz;
    r.gait = gait; r.x = x; r.v_des = v_des; r.w_des = w_des; r.ref_state = ref_state; r.foot_pos = foot_pos;
    r.push_force = push_force; r.X = X; r.U = U; r.S = S; r.status = status; r.failed = failed;
    r.win_start = h->push_windows.start; r.win_duration = h->push_windows.duration;
    r.footsteps = cfg->footsteps ? 1 : 0;
    std::memcpy(r.hip_offset, cfg->hip_offset, sizeof(r.hip_offset));
    std::memcpy(r.stance_ratio, cfg->stance_ratio, sizeof(r.stance_ratio));
    r.foot_size = cfg->foot_size;
    nmpc::SolveArgs a = base_args(h);
    a.x0 = x; a.status = status;
    const int rc = run_rollout(h, B, cfg, 0, static_cast<hipStream_t>(stream), r, a, nmpc::nmpc_rollout_prepare_kernel,
                               launch_solve<nmpc::Centroidal>, nmpc::nmpc_rollout_advance_kernel,
                               [&](int i) {
                                   r.node = cfg->start_node + i * cfg->nodes_per_replan;
                                   r.phase = phase[i];
                                   return cfg->nodes_per_replan;
                               },
                               [] { return NMPC_OK; }, [](int) { return NMPC_OK; });
    if (rc == NMPC_OK) h->rolled = true;      // every replan was launched: `roll` holds what the last prepare kernel wrote
    return rc;
}

}  // extern "C"

namespace {

// One nmpc_wb_rollout_batch call as check_wb_rollout accepted it: what the parts of the call share beside the kernel arguments.
struct WbRolloutCall {
    int B = 0, n_replans = 0;
    // the clock (nmpc_wb_rollout_set_clock): replan i of the call is replan replan0 + i of its rollout; a replan is `steps` simulation
    // steps of sim_dt, each n_sub substeps of dt_sub on the plant
    int replan0 = 0, steps = 0, n_sub = 0;
    double sim_dt = 0.0;
    float dt_sub = 0.0f;
    long long sim_step(int i) const { return (long long)(replan0 + i) * steps; }      // where replan i starts: the simulation step,
    long long substep(int i) const { return sim_step(i) * n_sub; }                    // the substep of the plant
    double time(int i) const { return (double)sim_step(i) * sim_dt; }                 // and the time; time(n_replans): where the call ends
    // the labels of a replan's plan, the attached ones (nmpc_wb_rollout_set_actions) or the PD targets of the plant alone: the layer that
    // writes them (nullptr: neither is attached), its hold table and gains, and the attached table A of n_rows rows per rollout (nullptr:
    // the plant's workspace Aw of one replan)
    void* label_torque = nullptr;
    const int* zoh = nullptr;
    float kp = 0.0f, kd = 0.0f, *A = nullptr, *Aw = nullptr;
    template <class R> float* rows(const R& r) const { return A ? A + (size_t)r.row0 * 12 : Aw; }     // where this replan's targets live
    template <class R> int a_rows(const R& r) const { return A ? r.n_rows : steps; }                  // ... at how many rows per rollout
    void* plant = nullptr;                        // nmpc_wb_rollout_set_plant (nullptr: plant = plan)
    bool force_push = false, tree_h = false;      // nmpc_wb_rollout_set_plant_push with a push_force; x0's momentum from the tree
    nmpc_push_cfg plant_push{};                   // the rollout's own push_force, its window in substeps from the rollout's step 0
    nmpc_torque::PushWindows plant_windows{};     // a window per rollout, in substeps: written by the kernel at the entry of the call
    const int* skip = nullptr;                    // terminated rollouts are left out of every launch: failed[b] & term_mask
    int term_mask = 0;
};

// Every check of nmpc_wb_rollout_batch behind its null pointers, and what they decide: c, and in r the problem tensors and the model
// parameters.  After it nothing refuses but a launch.
int check_wb_rollout(Handle* h, int B, const nmpc_wb_rollout_cfg* cfg, const int* nodes, const float* push_force, const int* failed,
                     WbRolloutCall& c, nmpc::wb::WbRolloutArgs& r) {
    if (h->dims.model_id != NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_wb_rollout_batch needs the whole-body model");
    if (const int rc = check_declared_momentum(h, "nmpc_wb_rollout_batch")) return rc;
    if (const int rc = check_batch(h, B)) return rc;
    if (cfg->n_replans < 1 || cfg->replanning_steps < 1 || cfg->nodes_per_cycle < 1 || !(cfg->sim_dt > 0) || !(cfg->time_horizon > 0))
        return fail(h, NMPC_E_ARG, "rollout configuration out of range");
    if (const int rc = check_configured(h)) return rc;
    if (h->line_search) return fail(h, NMPC_E_ARG, "the whole-body model takes full steps (line_search = 0)");
    c.B = B; c.n_replans = cfg->n_replans; c.steps = cfg->replanning_steps; c.sim_dt = cfg->sim_dt;
    // the clock of a continued rollout (nmpc_wb_rollout_set_clock): the stamp of its last replan must fit above the flag bits
    c.replan0 = h->rollout_replan0;
    if ((long long)c.replan0 + cfg->n_replans > (long long)(0x7fffffff >> NMPC_ROLLOUT_TERM_SHIFT))
        return fail(h, NMPC_E_ARG, "rollout clock: replan0 + n_replans exceeds the stamp field of failed[b]");
    if (cfg->replanning_steps * cfg->sim_dt > cfg->time_horizon) return fail(h, NMPC_E_ARG, "replanning interval longer than the horizon");
    for (int i = 0; i < cfg->n_replans; ++i)
        if (nodes[i] < 0 || (i > 0 && nodes[i] < nodes[i - 1])) return fail(h, NMPC_E_ARG, "nodes must be non-negative and non-decreasing");
    const auto& lab = h->labels;
    if (lab.A) {
        if (!cfg->record_sim_steps) return fail(h, NMPC_E_ARG, "action labels go with rows per simulation step: record_sim_steps must be 1");
        if (const char* why = nmpc_torque::plan_actions_refusal(lab.torque, cfg->replanning_steps, lab.zoh, lab.kp, h->device))
            return fail(h, NMPC_E_ARG, std::string("action labels: ") + why);
    }
    const auto& pl = h->plant;
    c.zoh = lab.A ? lab.zoh : pl.zoh; c.A = lab.A; c.Aw = pl.Aw;      // the labels' hold table serves both
    if (pl.torque) {
        c.n_sub = pl.n_sub; c.dt_sub = (float)(cfg->sim_dt / (pl.n_sub > 0 ? pl.n_sub : 1));
        if (!cfg->record_sim_steps) return fail(h, NMPC_E_ARG, "a plant records rows per simulation step: record_sim_steps must be 1");
        if (const char* why = nmpc_torque::plan_actions_refusal(pl.torque, cfg->replanning_steps, c.zoh, pl.kp, h->device))
            return fail(h, NMPC_E_ARG, std::string("plant: ") + why);
        if (const char* why = nmpc_torque::contact_track_refusal(pl.torque, pl.ground_set ? &pl.ground : nullptr, pl.n_sub, c.dt_sub, h->device))
            return fail(h, NMPC_E_ARG, std::string("plant: ") + why);
        if (lab.A && (lab.kp != pl.kp || lab.kd != pl.kd))
            return fail(h, NMPC_E_ARG, "plant: the attached action labels must be recorded with the plant's gains kp, kd");
        if (!(c.A ? c.A : c.Aw) || !pl.Qw || !pl.Vw) return fail(h, NMPC_E_ARG, "plant: the workspaces Qw, Vw and (without attached labels) Aw are needed");
    }
    c.plant = pl.torque; c.label_torque = lab.A ? lab.torque : pl.torque;
    c.kp = lab.A ? lab.kp : pl.kp; c.kd = lab.A ? lab.kd : pl.kd;
    // the push as a force on the plant (nmpc_wb_rollout_set_plant_push): the rollout's own push_force, in substeps of sim_dt / n_sub
    if (h->plant_push_as_force && !pl.torque) return fail(h, NMPC_E_ARG, "plant push: a push as a force needs a plant (nmpc_wb_rollout_set_plant)");
    c.force_push = h->plant_push_as_force && push_force;
    if (c.force_push && nmpc_torque::push_attached(pl.torque))
        return fail(h, NMPC_E_ARG, "plant push: the torque handle has a push of the caller's attached (nmpc_contact_set_push)");
    if (const char* why = push_windows_refusal(h, B, push_force)) return fail(h, NMPC_E_ARG, why);
    if (c.force_push) {
        if (h->push_windows.start) c.plant_windows = {h->push_substeps, h->push_substeps + h->dims.B_max, B};
        auto& push = c.plant_push;
        push.force = push_force; push.force_rows = B; push.joint = 5;
        push.first_substep = (int)std::lround((double)cfg->push_start * pl.n_sub / cfg->sim_dt);
        push.n_substeps = (int)std::lround((double)cfg->push_duration * pl.n_sub / cfg->sim_dt);
        if (push.n_substeps < 0) push.n_substeps = 0;
    }
    c.term_mask = cfg->terminate_mask & NMPC_ROLLOUT_FLAG_MASK; c.skip = c.term_mask ? failed : nullptr;
    c.tree_h = tree_state_momentum(h);
    return set_wb_problem(h, r);
}

// behind the solve of a replan: the labels of its plan, beside the rows the advance kernel or the plant is about to record -- attached
// labels where a rollout has terminated hold its last target
int record_labels(Handle* h, const WbRolloutCall& c, const nmpc::wb::WbRolloutArgs& r, hipStream_t st) {
    if (!c.label_torque) return NMPC_OK;
    const int rc = nmpc_plan_actions_batch(c.label_torque, c.B, c.steps, r.N, r.X, r.U, c.zoh, r.dt_nodes, r.sim_dt, c.kp, c.kd, nullptr, c.skip,
                                           c.term_mask, c.rows(r), c.a_rows(r), st);
    if (rc) return torque_call(h, rc, "nmpc_plan_actions_batch", c.label_torque);
    if (c.A && c.term_mask)
        hipLaunchKernelGGL(nmpc::wb::nmpc_wb_rollout_hold_actions_kernel, dim3((unsigned)(((size_t)c.B * c.steps * 12 + 255) / 256)), dim3(256),
                           0, st, c.B, r.n_rows, r.row0, c.steps, c.term_mask, r.failed, c.A);
    return NMPC_OK;
}

// ... and the expert drives the plant through replan i of the call: the label rows as PD targets of `steps` simulation steps, the states
// before each step into the workspace, and those states as rows row0 .. of S with their flags (no stamp: the advance kernel stamps)
int drive_plant(Handle* h, const WbRolloutCall& c, const nmpc::wb::WbRolloutArgs& r, int i, hipStream_t st) {
    if (!c.plant) return NMPC_OK;
    const auto& pl = h->plant;
    int rc;
    if (c.force_push) {
        nmpc_push_cfg push = c.plant_push;
        // this replan's substeps start at substep(i) of the rollout (a window that lies wholly before them, however far, starts n_substeps
        // before: the int holds it); with a window per rollout the kernel takes the offset off each, they stay as the entry kernel wrote them
        push.first_substep = (int)std::max((long long)push.first_substep - c.substep(i), -(long long)push.n_substeps);
        rc = nmpc_torque::contact_track_pushed(c.plant, c.B, c.steps, c.n_sub, c.dt_sub, &pl.ground, r.q, r.v, nullptr, c.rows(r), c.a_rows(r),
                                               pl.kp, pl.kd, pl.Qw, pl.Vw, c.steps, c.skip, c.term_mask, push, c.plant_windows, c.substep(i), st);
    } else {
        rc = nmpc_contact_track_batch(c.plant, c.B, c.steps, c.n_sub, c.dt_sub, &pl.ground, r.q, r.v, nullptr, c.rows(r), c.a_rows(r), pl.kp, pl.kd,
                                      pl.Qw, pl.Vw, c.steps, c.skip, c.term_mask, st);
    }
    if (rc) return torque_call(h, rc, "nmpc_contact_track_batch", c.plant);
    rc = nmpc_observe_rows_batch(c.plant, c.B, c.steps, pl.Qw, pl.Vw, c.steps, c.time(i), c.sim_dt, (double)r.nominal_period, r.collision_height,
                                 r.S + (size_t)r.row0 * 44, r.n_rows, r.failed, c.replan0 + i, 0, c.skip, c.term_mask, st);
    return torque_call(h, rc, "nmpc_observe_rows_batch", c.plant);
}

}  // namespace

extern "C" {

int nmpc_wb_rollout_batch(void* handle, int B, const nmpc_wb_rollout_cfg* cfg, const signed char* gait, const signed char* peaks,
                          const int* nodes, float* q, float* v, const double* v_des, const double* w_des, double* ref_state,
                          const float* joint_ref, const float* push_force, float* X, float* U, float* S, int* status,
                          int* failed, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!cfg || !gait || !peaks || !nodes || !q || !v || !v_des || !w_des || !ref_state || !joint_ref || !X || !U || !S || !status || !failed)
        return fail(h, NMPC_E_ARG, "null argument");
    WbRolloutCall c;
    nmpc::wb::WbRolloutArgs r{};
    if (const int rc = check_wb_rollout(h, B, cfg, nodes, push_force, failed, c, r)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    r.plant = c.plant ? 1 : 0; r.force_gravity = cfg->force_reference_gravity ? 1 : 0; r.step_height = cfg->step_height;
    r.gait = gait; r.peaks = peaks; r.q = q; r.v = v; r.v_des = v_des; r.w_des = w_des; r.ref_state = ref_state;
    r.joint_ref = joint_ref; r.push_force = push_force;
    r.X = X; r.U = U; r.S = S; r.status = status; r.failed = failed;
    const auto& pw = h->push_windows;
    if (pw.start && !c.force_push) { r.win_start = pw.start; r.win_duration = pw.duration; }      // the velocity jump, decided per rollout
    nmpc::wb::WbArgs w = wb_args(h);
    w.x0 = r.x0; w.status = status;
    if (c.plant_windows.first) {      // a window per rollout, pushed as a force: into substeps of the plant, once for the call
        NMPC_ENTER(h, h->device);
        hipLaunchKernelGGL(nmpc::wb::nmpc_wb_push_substeps_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, pw.start, pw.duration,
                           c.n_sub, cfg->sim_dt, h->push_substeps, h->push_substeps + h->dims.B_max);
        if (const int rc = launched(h)) return rc;
    }
    int last_node = cfg->last_node;
    const int rc = run_rollout(
        h, B, cfg, c.replan0, st, r, w, nmpc::wb::nmpc_wb_rollout_prepare_kernel, launch_wb, nmpc::wb::nmpc_wb_rollout_advance_kernel,
        [&](int i) {          // warm_start_solver(i_node): start_node = i_node - last_node (solver.py:304-309)
            const int shift = nodes[i] - last_node;
            r.node = last_node = nodes[i];
            if (c.force_push) r.push_dt = 0.0f;      // the track launch pushes: no velocity jump in the advance kernel
            return shift;
        },
        [&] {                 // x0's momentum from the tree, for the rollouts the prepare kernel prepared
            return c.tree_h ? launch_state_momentum(h, B, q, v, 18, r.x0, X, c.skip, c.term_mask, st) : (int)NMPC_OK;
        },
        [&](int i) {          // behind the solve: the labels of the plan, then the plant through the interval
            if (const int lrc = record_labels(h, c, r, st)) return lrc;
            return drive_plant(h, c, r, i, st);
        });
    if (rc || !c.plant) return rc;
    // the state the last interval left: a robot that fell in it is flagged and stamped with the last replan
    const int frc = nmpc_observe_batch(c.plant, B, q, v, c.time(c.n_replans), (double)cfg->nominal_period, nullptr, 0, nullptr, nullptr, 0,
                                       cfg->collision_height, nullptr, 0, nullptr, failed, c.replan0 + c.n_replans - 1, c.term_mask, st);
    return torque_call(h, frc, "nmpc_observe_batch", c.plant);
}

int nmpc_wb_label_states_batch(void* handle, void* torque_handle, int B, const nmpc_wb_label_cfg* cfg, const signed char* gait,
                               const signed char* peaks, const int* node, const int* ref_steps, const float* Q, const float* V,
                               int qv_rows, const double* v_des, const double* w_des, const double* ref_state,
                               const float* joint_ref, const int* failed, const int* zoh, float* A, int a_rows, int* status, float* X,
                               float* U, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!cfg || !gait || !peaks || !node || !ref_steps || !Q || !V || !v_des || !w_des || !ref_state || !joint_ref || !zoh || !A || !status ||
        !X || !U)
        return fail(h, NMPC_E_ARG, "null argument");
    if (h->dims.model_id != NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_wb_label_states_batch needs the whole-body model");
    if (const int rc = check_declared_momentum(h, "nmpc_wb_label_states_batch")) return rc;
    if (h->line_search) return fail(h, NMPC_E_ARG, "the whole-body model takes full steps (line_search = 0)");
    if (const int rc = check_configured(h)) return rc;
    if (const char* why = nmpc_torque::label_states_refusal(torque_handle, cfg->n_rows, qv_rows, a_rows, zoh, cfg->kp, h->device))
        return fail(h, NMPC_E_ARG, std::string("labels: ") + why);
    const int N = h->dims.N, K = cfg->n_rows, B_max = h->dims.B_max;
    if (B < 0 || (long long)B * K > 0x7fffffffLL) return fail(h, NMPC_E_ARG, "B out of range");
    if (cfg->nodes_per_cycle < 1 || cfg->max_sqp < 1 || !(cfg->sim_dt > 0) || !(cfg->time_horizon > 0))
        return fail(h, NMPC_E_ARG, "label configuration out of range");
    const double dt_nodes = cfg->time_horizon / N;
    if (cfg->sim_dt > N * dt_nodes * (1.0 + 1e-9)) return fail(h, NMPC_E_ARG, "sim_dt beyond the horizon");
    if (((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(U)) & 7u) != 0)      // launch_wb's rule, in front of the first launch
        return fail(h, NMPC_E_ARG, "whole-body arrays must be 8 B aligned (params: 16 B)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    NMPC_ENTER(h, h->device);
    if (const int rc = clean_workspace(h, st)) return rc;
    nmpc::wb::WbLabelArgs r{};
    r.K = K; r.N = N; r.npc = cfg->nodes_per_cycle; r.qv_rows = qv_rows;
    r.force_gravity = cfg->force_reference_gravity ? 1 : 0;
    r.step_height = cfg->step_height;
    r.sim_dt = cfg->sim_dt; r.t_horizon = cfg->time_horizon; r.nom_height = cfg->nom_height; r.height_offset = cfg->height_offset;
    if (const int rc = set_wb_problem(h, r)) return rc;             // the carve-up and the mass of nmpc_wb_rollout_batch
    const bool tree_h = tree_state_momentum(h);
    r.gait = gait; r.peaks = peaks; r.node = node; r.ref_steps = ref_steps; r.failed = failed; r.Q = Q; r.V = V; r.joint_ref = joint_ref;
    r.v_des = v_des; r.w_des = w_des; r.ref_state = ref_state;
    r.X = X; r.U = U; r.skip = h->label_skip;
    nmpc::wb::WbArgs w = wb_args(h);
    w.yref_per_stage = 1; w.shift = 0;
    w.x0 = r.x0; w.yref = r.yref; w.yref_e = r.yref_e; w.params = r.params; w.X = X; w.U = U; w.stats = nullptr;
    w.max_sqp = cfg->max_sqp; w.nlp_tol = cfg->nlp_tol;
    // the states behind a termination cost no solve: the chunk's own flags for the duration of its solve, whatever nmpc_set_skip
    // holds for the caller's solves (the handle's setting is not written, so there is nothing to put back)
    w.skip = h->label_skip; w.skip_mask = 1;
    const long long total = (long long)B * K;
    for (long long m0 = 0; m0 < total; m0 += B_max) {
        const int count = (int)(total - m0 < B_max ? total - m0 : B_max);
        r.m0 = (int)m0;
        hipLaunchKernelGGL(nmpc::wb::nmpc_wb_label_prepare_kernel, dim3(count), dim3(64), 0, st, r);
        // x0's momentum from the tree: problem m = b K + k reads row k of robot b of Q, V
        if (tree_h)
            if (const int rc = runs_by_robot(m0, count, K, qv_rows, [&](size_t i, int run, size_t row) {
                    return launch_state_momentum(h, run, Q + row * 18, V + row * 18, 18, r.x0 + i * nmpc::wb::NX, X + i * (N + 1) * nmpc::wb::NX,
                                                 h->label_skip + i, 1, st);
                }))
                return rc;
        w.B = count; w.status = status + m0;
        if (const int rc = launch_wb(h, w, st)) return rc;
        // label row 0 of every plan of the chunk: the target applied from the state its solve started from, into A[b][k]
        if (const int rc = runs_by_robot(m0, count, K, a_rows, [&](size_t i, int run, size_t row) {
                const int lrc = nmpc_plan_actions_batch(torque_handle, run, 1, N, X + i * (N + 1) * nmpc::wb::NX, U + i * N * nmpc::wb::NU, zoh, dt_nodes,
                                                        cfg->sim_dt, cfg->kp, cfg->kd, nullptr, h->label_skip + i, 1, A + row * 12, 1, st);
                return torque_call(h, lrc, "nmpc_plan_actions_batch", torque_handle);
            }))
            return rc;
    }
    return launched(h);
}

int nmpc_debug_set_buffer(void* handle, float* dev_buffer) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    h->dbg = dev_buffer;
    return NMPC_OK;
}

int nmpc_debug_read_tile(void* handle, int b, int k, int which, float* out_host) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !out_host) return fail(h, NMPC_E_ARG, "null argument");
    if (b < 0 || b >= h->dims.B_max || k < 0 || k >= h->dims.N || which < 0 || which > 3)
        return fail(h, NMPC_E_ARG, "index out of range");
    NMPC_ENTER(h, h->device);
    NMPC_TRY(h, hipDeviceSynchronize());
    if (h->dims.model_id == NMPC_MODEL_DOUBLE_INTEGRATOR) return read_tile<nmpc::DoubleIntegrator>(h, b, k, which, out_host);
    if (h->dims.model_id == NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "use nmpc_debug_read_workspace for the whole-body model");
    return read_tile<nmpc::Centroidal>(h, b, k, which, out_host);
}

int nmpc_debug_read_workspace(void* handle, int b, size_t offset, size_t count, float* out_host) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !out_host) return fail(h, NMPC_E_ARG, "null argument");
    if (b < 0 || b >= h->dims.B_max || offset + count > h->ws_stride) return fail(h, NMPC_E_ARG, "index out of range");
    NMPC_ENTER(h, h->device);
    NMPC_TRY(h, hipDeviceSynchronize());
    NMPC_TRY(h, hipMemcpy(out_host, h->ws + (size_t)b * h->ws_stride + offset, count * sizeof(float), hipMemcpyDeviceToHost));
    return NMPC_OK;
}

int nmpc_debug_read_momentum(void* handle, int b, int k, float* mrec_host, float* dcons_host) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (!h->momentum.mrec || !h->momentum.dcons) return fail(h, NMPC_E_STATE, "the handle has never been in the articulated momentum mode");
    if (b < 0 || b >= h->dims.B_max || k < 0 || k > h->dims.N) return fail(h, NMPC_E_ARG, "index out of range");
    NMPC_ENTER(h, h->device);
    NMPC_TRY(h, hipDeviceSynchronize());
    const size_t node = (size_t)b * (h->dims.N + 1) + k;
    if (mrec_host)
        NMPC_TRY(h, hipMemcpy(mrec_host, h->momentum.mrec + node * nmpc::wb::MR_FLOATS, nmpc::wb::MR_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    if (dcons_host)
        NMPC_TRY(h, hipMemcpy(dcons_host, h->momentum.dcons + node * nmpc::wb::DC_FLOATS, nmpc::wb::DC_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    return NMPC_OK;
}

int nmpc_debug_read_rollout_problem(void* handle, int b, float* x0_host, float* yref_host) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (h->dims.model_id != NMPC_MODEL_WHOLEBODY) return fail(h, NMPC_E_ARG, "nmpc_debug_read_rollout_problem needs the whole-body model");
    if (b < 0 || b >= h->dims.B_max) return fail(h, NMPC_E_ARG, "index out of range");
    NMPC_ENTER(h, h->device);
    NMPC_TRY(h, hipDeviceSynchronize());
    const WbRoll roll = wb_roll(h);
    if (x0_host) NMPC_TRY(h, hipMemcpy(x0_host, roll.x0 + (size_t)b * h->nx, h->nx * sizeof(float), hipMemcpyDeviceToHost));
    const size_t per = (size_t)h->dims.N * h->ny;
    if (yref_host) NMPC_TRY(h, hipMemcpy(yref_host, roll.yref + (size_t)b * per, per * sizeof(float), hipMemcpyDeviceToHost));
    return NMPC_OK;
}

int nmpc_debug_read_centroidal_rollout_problem(void* handle, int b, float* yref_host, float* yref_e_host, float* params_host) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return NMPC_E_ARG;
    if (h->dims.model_id != NMPC_MODEL_CENTROIDAL) return fail(h, NMPC_E_ARG, "nmpc_debug_read_centroidal_rollout_problem needs the centroidal model");
    if (b < 0 || b >= h->dims.B_max) return fail(h, NMPC_E_ARG, "index out of range");
    if (!h->rolled) return fail(h, NMPC_E_STATE, "the handle has never run a rollout");
    NMPC_ENTER(h, h->device);
    NMPC_TRY(h, hipDeviceSynchronize());
    const CentroidalRoll roll = centroidal_roll(h);
    const size_t N = (size_t)h->dims.N, n_yref = N * h->ny, n_params = (N + 1) * h->np;
    if (yref_host) NMPC_TRY(h, hipMemcpy(yref_host, roll.yref + (size_t)b * n_yref, n_yref * sizeof(float), hipMemcpyDeviceToHost));
    if (yref_e_host) NMPC_TRY(h, hipMemcpy(yref_e_host, roll.yref_e + (size_t)b * h->nye, h->nye * sizeof(float), hipMemcpyDeviceToHost));
    if (params_host) NMPC_TRY(h, hipMemcpy(params_host, roll.params + (size_t)b * n_params, n_params * sizeof(float), hipMemcpyDeviceToHost));
    return NMPC_OK;
}

int nmpc_debug_wb_layout(int N, size_t* out8) {
    if (!out8 || N < 1) return NMPC_E_ARG;
    const nmpc::wb::WsLayout wl(N);
    const nmpc::wb::StageArr sa(N);
    out8[0] = wl.rec; out8[1] = wl.js; out8[2] = wl.qt; out8[3] = wl.kt; out8[4] = wl.arr; out8[5] = wl.stride;
    out8[6] = (size_t)sa.NS; out8[7] = (size_t)nmpc::wb::REC;
    return NMPC_OK;
}

}  // extern "C"
