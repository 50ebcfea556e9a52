// nmpc_linearize.hip.inc -- the linearisation of the tile family (included by nmpc_solve.hip): linearize_node and its kernel.
namespace nmpc {

// ------------------------------------------------------------------------------------------------
// Linearisation: thread t <-> (problem b, stage k), k = N is the terminal stage.
// A thread owns a whole 1 KiB tile, so storing it directly would make every wave store touch 64
// different tiles with 16 B each.  Columns therefore go through a 4 KiB LDS stage: the block
// re-distributes one column of 64 stages so that the lanes of a quad group write the contiguous
// bytes of a stage's column (16 tiles per store instruction instead of 64).  The block is ONE wave:
// the LDS hand-over is ordered by issue (wave_sync), not by s_barrier -- __syncthreads would also drain
// the column stores of the previous flush (vmcnt(0)) 25 times per thread (measured: 29.8 -> 24.8 us
// together with requesting the reference row and the next node up front).
// (a device function: the kernel below runs it with thread t <-> (problem, node); the two-wave variant of the QP kernel runs
//  it itself, lane = node, in front of its prologue when the horizon fits one wave -- qp_linearizes_itself)
constexpr int LIN_LDS_FLOATS = 64 * 16 + 2 * 64 * 2;      // column stage + the 2 x 64 tile pointers
template <class M>
__device__ __forceinline__ void linearize_node(const SolveArgs& a, bool in_range, int b_in, int k_in, float* lds) {
#pragma clang fp contract(off)      // as the model functions it calls (nmpc_models.hpp): one rounding behaviour in every caller
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NG = M::NG, NY = NX + NU;
    using G = TileGeom<M>;
    float* stage_col = lds;
    float** tile_of0 = reinterpret_cast<float**>(lds + 64 * 16);
    float** tile_of1 = tile_of0 + 64;
    float** tile_of[2] = {tile_of0, tile_of1};       // A~ / B~ tile of each thread's stage (nullptr: none)
    const int N = a.N;
    const int tid = threadIdx.x;
    const int b = b_in;                   // a valid problem index also where in_range is false (idle lanes only read it)
    const int k = in_range ? k_in : N;
    const WsLayout<M> wl(N);
    float* ws = a.ws + (size_t)b * wl.stride;
    const bool live = in_range && !(a.it > 0 && reinterpret_cast<const int*>(ws + wl.flag)[0]) && !skipped(a, b);
    const bool stage = live && k < N;       // this thread linearises a shooting interval
    const int ks = stage ? k : 0;
    const float* Xg = a.X + (size_t)b * (N + 1) * NX;
    const float* Ug = a.U + (size_t)b * N * NU;
    tile_of[0][tid] = stage ? ws + wl.At + (size_t)k * G::A_FLOATS : nullptr;
    tile_of[1][tid] = stage ? ws + wl.Bt + (size_t)k * G::B_FLOATS : nullptr;
    float x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = Xg[(size_t)shifted_node(live ? k : 0, a.shift, N) * NX + i];
    if (live && k == N) {   // terminal gradient and cost
        const float* yre = a.yref_e + (size_t)b * NX;
        float cst = 0.0f;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const float e = x[i] - yre[i];
            ws[wl.q + (size_t)N * NX + i] = a.We[i] * e;
            cst += 0.5f * a.We[i] * e * e;
        }
        ws[wl.cost + N] = cst;
    }
    float u[NU], xn[NX], p[NP > 0 ? NP : 1];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const float v = Ug[(size_t)(shifted_stage_valid(ks, a.shift, N) ? ks + a.shift : ks) * NU + i];
        u[i] = (a.shift == 0 || shifted_stage_valid(ks, a.shift, N)) ? v : 0.0f;
    }
    const float* pg = a.params + ((size_t)b * (N + 1) + ks) * NP;
#pragma unroll
    for (int i = 0; i < NP; ++i) p[i] = pg[i];
    // everything else the thread will need from memory, requested now: the loads overlap the Jacobians
    // instead of costing a round trip each where they are used
    float x_next[NX], yv[NY];
#pragma unroll
    for (int i = 0; i < NX; ++i) x_next[i] = Xg[(size_t)shifted_node(ks + 1, a.shift, N) * NX + i];
    const float* yk = a.yref + (size_t)b * (a.yref_per_stage ? (size_t)N * NY : (size_t)NY) +
                      (a.yref_per_stage ? (size_t)ks * NY : 0);
#pragma unroll
    for (int i = 0; i < NY; ++i) yv[i] = yk[i];
    wave_sync();
    // every thread of the block takes part in every column flush (idle threads carry a null tile)
    auto flush = [&](int which, int j, const float (&v)[16]) {
#ifdef LIN_T_NOFLUSH   // timing build (tools/lin_timing.sh): no hand-over, the column only stays alive
        float sacc = 0.0f;
        for (int i = 0; i < 16; ++i) sacc += v[i];
        if (sacc == 123.456f) stage_col[tid] = sacc;
        return;
#endif
        f32x4* mine = reinterpret_cast<f32x4*>(stage_col + tid * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) mine[i] = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        wave_sync();
        const int quad = tid & 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int s = (tid >> 2) + 16 * i;
            float* tile = tile_of[which][s];
#ifdef LIN_T_NOSTORE   // timing build: hand-over without the column stores
            if (tile != nullptr && quad < G::RQ && a.B < 0)
#else
            if (tile != nullptr && quad < G::RQ)
#endif
                *reinterpret_cast<f32x4*>(tile + j * G::SA + 4 * quad) =
                    *reinterpret_cast<const f32x4*>(stage_col + s * 16 + 4 * quad);
        }
        wave_sync();
    };
    auto emitA = [&](int j, const float (&colv)[NX]) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = (i < NX) ? colv[i < NX ? i : 0] : 0.0f;
        flush(0, j, v);
    };
    auto emitB = [&](int j, const float (&colv)[NX]) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = (i < NX) ? colv[i < NX ? i : 0] : 0.0f;
        flush(1, j, v);
    };
    M::linearize(a.mp, x, u, p, xn, emitA, emitB);
    {   // defect column  [d; 1]
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            v[i] = (i < NX) ? xn[i < NX ? i : 0] - x_next[i < NX ? i : 0] : 0.0f;
        flush(0, NX, v);
    }
#ifdef LIN_T_NOTAIL    // timing build: no gradients / constraint values / masks
    if (a.B > 0) return;
#endif
    if (!stage) return;
    float cst = 0.0f;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const float e = x[i] - yv[i];
        ws[wl.q + (size_t)k * NX + i] = a.W[i] * e;
        cst += 0.5f * a.W[i] * e * e;
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const float e = u[i] - yv[NX + i];
        ws[wl.r + (size_t)k * NU + i] = a.W[NX + i] * e;
        cst += 0.5f * a.W[NX + i] * e * e;
    }
    ws[wl.cost + k] = cst;
    reinterpret_cast<unsigned*>(ws + wl.umk)[k] = M::input_mask(a.mp, p);
    reinterpret_cast<unsigned*>(ws + wl.act)[k] = (a.n_ipm > 0) ? M::active_mask(a.mp, p) : 0u;
    float g[NG];
    M::gdot(a.mp, u, g);
#pragma unroll
    for (int j = 0; j < NG; ++j) ws[wl.c + (size_t)k * NG + j] = g[j] - M::h(a.mp, j);
}

template <class M>
__global__ __launch_bounds__(64) void nmpc_linearize_kernel(const SolveArgs a) {
    __shared__ __attribute__((aligned(16))) float lin_lds[LIN_LDS_FLOATS];
    const int N = a.N;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = t < (long long)a.B * (N + 1);
    const int b = in_range ? (int)(t / (N + 1)) : 0;
    const int k = in_range ? (int)(t - (long long)b * (N + 1)) : N;
    linearize_node<M>(a, in_range, b, k, lin_lds);
}

}  // namespace nmpc
