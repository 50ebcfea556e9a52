// nmpc_aux.hip.inc -- dense-LQ Riccati entry, warm-start shift, tracking error kernels.
// Included by nmpc_api.hip (single translation unit).

#pragma clang fp contract(off)      // explicit: these kernels are compared bit for bit with their fp32 / fp64 restatements

namespace nmpc {

// ------------------------------------------------------------------------------------------------
// Riccati sweep on explicit dense stage data (row-major), one problem per wavefront.
// Tiles are built in registers straight from the dense arrays; only K~ goes through the workspace.
struct RiccatiArgs {
    int N, B, nx, nu;
    const float *Q, *R, *q, *r, *A, *Bm, *d, *dx0;
    float *dX, *dU;
    int* status;
    float* ws;   // per problem 2N tiles (K~', Acl~')
};
// floats of workspace one problem of the Riccati entry takes: what nmpc_create allocates per problem at the least
__host__ __device__ constexpr size_t riccati_ws_floats(int N) { return (size_t)2 * N * TILE; }

__global__ __launch_bounds__(64) void nmpc_riccati_kernel(const RiccatiArgs a) {
    __shared__ __attribute__((aligned(16))) float conv[CONV_FLOATS];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = lane_id(), q4 = lane >> 4, c = lane & 15;
    const int N = a.N, nx = a.nx, nu = a.nu;
    const float* Q = a.Q + (size_t)b * (N + 1) * nx * nx;
    const float* R = a.R + (size_t)b * N * nu * nu;
    const float* qg = a.q + (size_t)b * (N + 1) * nx;
    const float* rg = a.r + (size_t)b * N * nu;
    const float* A = a.A + (size_t)b * N * nx * nx;
    const float* Bm = a.Bm + (size_t)b * N * nx * nu;
    const float* d = a.d + (size_t)b * N * nx;
    float* Kt = a.ws + (size_t)b * riccati_ws_floats(N);
    float* Ct = Kt + (size_t)N * TILE;

    auto tileA = [&](int k, bool transposed) {   // A~ = [A d; 0 1] or its transpose
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = transposed ? c : 4 * q4 + r, j = transposed ? 4 * q4 + r : c;
            float t = 0.0f;
            if (i < nx && j < nx) t = A[((size_t)k * nx + i) * nx + j];
            else if (i < nx && j == nx) t = d[(size_t)k * nx + i];
            else if (i == nx && j == nx) t = 1.0f;
            v[r] = t;
        }
        return v;
    };
    auto tileB = [&](int k, bool transposed) {   // B~ = [B; 0]
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = transposed ? c : 4 * q4 + r, j = transposed ? 4 * q4 + r : c;
            v[r] = (i < nx && j < nu) ? Bm[((size_t)k * nx + i) * nu + j] : 0.0f;
        }
        return v;
    };
    auto tileQ = [&](int k) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * q4 + r, j = c;
            float t = 0.0f;
            if (i < nx && j < nx) t = Q[((size_t)k * nx + i) * nx + j];
            else if (i < nx && j == nx) t = qg[(size_t)k * nx + i];
            else if (i == nx && j < nx) t = qg[(size_t)k * nx + j];
            v[r] = t;
        }
        return v;
    };

    bool ok = true;
    SweepLane sl;
    sl.init(conv, lane, nx, nullptr);   // no uncoupled rows here: every input is coupled
    wave_sync();
#ifdef NMPC_STAMPS
    StageStamps sst = {0, {0, 0, 0, 0, 0, 0, 0, 0}};
#define RIC_SST , sst
#else
#define RIC_SST
#endif
    f32x4 P = tileQ(N);
    for (int k = N - 1; k >= 0; --k) {
        f32x4 St, Rt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * q4 + r;
            St[r] = (c == nx && i < nu) ? rg[(size_t)k * nu + i] : 0.0f;
            Rt[r] = (i < nu && c < nu) ? R[((size_t)k * nu + i) * nu + c] : ((i == c) ? 1.0f : 0.0f);
        }
        f32x4 Kk, Acl;
        NoNextCost none;
        ok = backward_stage<16, 0xFFFFu, false, false>(P, tileA(k, false), tileB(k, false), tileB(k, true), tileQ(k), St, Rt,
                                         conv, sl, lane, 0xFFFFu, Kk, Acl, none RIC_SST) && ok;
        store_tile_t(Kt + (size_t)k * TILE, lane, Kk);
        store_tile_t(Ct + (size_t)k * TILE, lane, Acl);
    }
    __threadfence_block();
    wave_sync();
    float* dX = a.dX + (size_t)b * (N + 1) * nx;
    float* dU = a.dU + (size_t)b * N * nu;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * q4 + r;
        v[r] = (c == 0) ? ((i < nx) ? a.dx0[(size_t)b * nx + i] : (i == nx ? 1.0f : 0.0f)) : 0.0f;
        if (c == 0 && i < nx) dX[i] = v[r];
    }
    for (int k = 0; k < N; ++k) {
        const f32x4 du = xty(load_tile(Kt + (size_t)k * TILE, lane), v);
        v = xty(load_tile(Ct + (size_t)k * TILE, lane), v);
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * q4 + r;
                if (i < nu) dU[(size_t)k * nu + i] = du[r];
                if (i < nx) dX[(size_t)(k + 1) * nx + i] = v[r];
            }
        }
    }
    if (lane == 0 && a.status) a.status[b] = ok ? NMPC_STATUS_OK : NMPC_STATUS_QP;
}

// ------------------------------------------------------------------------------------------------
// Warm-start shift (solver.py:304-322).  One block per problem; the shifted copy goes through
// registers of the same thread so in-place overlap is safe (each element is read before the barrier
// and written after it).
__global__ void nmpc_shift_kernel(int N, int nx, int nu, int nu_keep, int shift, float* X, float* U) {
    const int b = blockIdx.x;
    float* x = X + (size_t)b * (N + 1) * nx;
    float* u = U + (size_t)b * N * nu;
    const int nw = N - shift;
    const int nxe = nw * nx, nue = N * nu;
    constexpr int MAXPT = 16;   // elements per thread held in registers
    float bx[MAXPT], bu[MAXPT];
#pragma unroll
    for (int i = 0; i < MAXPT; ++i) {
        const int e = threadIdx.x + i * blockDim.x;
        bx[i] = (e < nxe) ? x[(size_t)(shift + 1) * nx + e] : 0.0f;
        bu[i] = (e < nw * nu) ? u[(size_t)shift * nu + e] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXPT; ++i) {
        const int e = threadIdx.x + i * blockDim.x;
        if (e < nxe) x[nx + e] = bx[i];
        // tail (e >= nw*nu): zero fill of the contact forces; the first nu_keep inputs of a stage (the whole-body model's
        // accelerations) keep their previous values there (solver.py:316-322)
        if (e < nue && (e < nw * nu || e % nu >= nu_keep)) u[e] = bu[i];
    }
}

// ------------------------------------------------------------------------------------------------
// Tracking error (data_collection_force_perturbation.py:138-156):
//   err[b][t] = || S[b][t][1:] - Snom[t][1:] ||_2 , optional OOD sampling weight.
// HBM-bound streaming kernel: a block stages TRB rows with coalesced loads into LDS (odd row
// stride -> conflict-free), then one thread reduces one row in the oracle's order (no fma
// contraction, so fp32 results equal the fp32 oracle bit for bit).
constexpr int TRB = 128;

__global__ __launch_bounds__(TRB) void nmpc_tracking_error_kernel(
    long long rows, int T, int ns, const float* __restrict__ S, const float* __restrict__ Snom,
    float* __restrict__ err, float* __restrict__ weight, float threshold, float ood_weight) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int stride = ns | 1;
    const long long row0 = (long long)blockIdx.x * TRB;
    const int nrows = (int)((rows - row0 < TRB) ? (rows - row0) : TRB);
    const int nel = nrows * ns;
    const float* src = S + row0 * ns;
    const int t0 = (int)(row0 % T);
    for (int e = threadIdx.x; e < nel; e += TRB) {
        const int rr = e / ns, cc = e - rr * ns;
        int t = t0 + rr;
        t -= (t / T) * T;
        sm[rr * stride + cc] = __fsub_rn(src[e], Snom[(size_t)t * ns + cc]);
    }
    __syncthreads();
    if ((int)threadIdx.x < nrows) {
#pragma clang fp contract(off)
        const float* rowp = sm + threadIdx.x * stride;
        float acc = 0.0f;
        for (int i = 1; i < ns; ++i) {
            const float sq = rowp[i] * rowp[i];   // separate multiply and add (contract off)
            acc = acc + sq;
        }
        const float e = sqrtf(acc);        // correctly rounded (hipcc default)
        err[row0 + threadIdx.x] = e;
        if (weight) weight[row0 + threadIdx.x] = (e > threshold) ? ood_weight : 1.0f;
    }
}

}  // namespace nmpc
