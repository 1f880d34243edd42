// koaf_linear.hip -- nn.Linear on koaf_gemm (split-K for the few-row layers), and the direct kernels of the narrow heads.
#include "koaf_common.h"

// split-K plan for a linear layer with few rows: the 64x64-tile grid of M x N is only a few hundred blocks with
// K/32 serial k-steps each (latency-bound at ~1 block per CU); splitting K 2-8 ways fills the chip.
struct LinTile { int bm, bn; };
static LinTile linear_tile(int M, int N) {
    // 128x128 tiles (half the loader / split work per FLOP of 64x64) once both dimensions offer a few of them; with
    // few rows (200-256 token rows of the per-MRI aggregators) 64x128: the wide N still halves the A traffic per FLOP
    if (M >= 512 && N >= 512) return {128, 128};
    if (N < 1024) return {64, 64};
    return {64, 128};
}
static int linear_splitk(int M, int N, int K) {
    if ((N & 3) || K < 512) return 1;
    const LinTile t = linear_tile(M, N);
    const int64_t tiles = cdiv64(M, t.bm) * cdiv64(N, t.bn);
    const int64_t want = t.bm == 128 ? 512 : (t.bn == 128 ? 768 : 1024);
    if (tiles >= want) return 1;
    int sk = (int)(want / tiles);
    if (sk > 8) sk = 8;
    while (sk > 1 && K / sk < 256) --sk;
    return sk;
}
extern "C" int64_t koaf_linear_ws(int32_t M, int32_t N, int32_t K) {
    const int sk = linear_splitk(M, N, K);
    return sk > 1 ? (int64_t)sk * M * N : 0;
}

// ---- narrow heads (N <= 8 outputs: the 2-class heads) ------------------------------------------------------------
// A 64x64-tile GEMM spends 64 serial k-steps on a handful of useful outputs (81 us per call on the native step);
// these three direct kernels do the same sums on the vector ALUs in a few microseconds, in plain fp32.
__global__ void __launch_bounds__(256) head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ b, const float* __restrict__ res,
                                                       float* __restrict__ y, int M, int N, int K) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;      // one wave per output
    if (o >= M * N) return;
    const int m = o / N, n = o - m * N;
    float a = 0.f;
    for (int k = lane; k < K; k += 64) a += x[(int64_t)m * K + k] * w[(int64_t)n * K + k];
    a = wave_sum(a);
    if (lane == 0) y[o] = a + (b ? b[n] : 0.f) + (res ? res[o] : 0.f);
}
__global__ void __launch_bounds__(256) head_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                         const float* __restrict__ res, float* __restrict__ dx, int M,
                                                         int N, int K) {
    const int64_t total = (int64_t)M * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / K), k = (int)(i - (int64_t)m * K);
        float a = res ? res[i] : 0.f;
        for (int n = 0; n < N; ++n) a += dy[m * N + n] * w[(int64_t)n * K + k];
        dx[i] = a;
    }
}
__global__ void __launch_bounds__(256) head_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         float* __restrict__ dw, int M, int N, int K) {
    const int64_t total = (int64_t)N * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / K), k = (int)(i - (int64_t)n * K);
        float a = 0.f;
        for (int m = 0; m < M; ++m) a += dy[m * N + n] * x[(int64_t)m * K + k];
        dw[i] = a;
    }
}
static inline bool narrow_head(int M, int N, int K) { return N <= 8 && (int64_t)M * N <= 4096 && K >= 64; }

extern "C" int koaf_linear_fwd(const float* x, const float* w, const float* b, const float* residual, float* y,
                               float* ws, int32_t M, int32_t N, int32_t K, void* stream) {
    KOAF_REQUIRE(x && w && y && M > 0 && N > 0 && K > 0, "koaf_linear_fwd: bad args");
    if (narrow_head(M, N, K)) {
        hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)cdiv64((int64_t)M * N, 4)), dim3(256), 0, STREAM, x, w, b, residual,
                           y, M, N, K);
        return koaf_check_launch("koaf_linear_fwd");
    }
    KoafGemm g;
    zero_gemm(&g);
    g.A.ptr = x; g.A.kind = 0; g.A.ld = K;
    g.B.ptr = w; g.B.kind = 0; g.B.ld = K;
    g.M = M; g.N = N; g.K = K;
    const int sk = ws ? linear_splitk(M, N, K) : 1;
    if (sk > 1) {
        g.splitk = sk; g.bm = linear_tile(M, N).bm; g.bn = linear_tile(M, N).bn;
        g.C = ws; g.ldc = N;
        int rc = koaf_gemm(&g, stream);
        if (rc != KOAF_OK) return rc;
        return koaf_slab_reduce_epilogue(ws, sk, M, N, b, residual, N, y, N, stream);
    }
    g.C = y; g.ldc = N;
    g.bias = b;
    g.residual = residual; g.ldr = N;
    return koaf_gemm(&g, stream);
}
extern "C" int koaf_linear_dgrad(const float* dy, const float* w, const float* residual, float* dx, float* ws,
                                 int32_t M, int32_t N, int32_t K, void* stream) {
    KOAF_REQUIRE(dy && w && dx && M > 0 && N > 0 && K > 0, "koaf_linear_dgrad: bad args");
    if (narrow_head(M, N, K)) {
        hipLaunchKernelGGL(head_dgrad_kernel, dim3((unsigned)cdiv64((int64_t)M * K, 256)), dim3(256), 0, STREAM, dy, w,
                           residual, dx, M, N, K);
        return koaf_check_launch("koaf_linear_dgrad");
    }
    KoafGemm g;
    zero_gemm(&g);
    g.prec = 1;
    g.A.ptr = dy; g.A.kind = 0; g.A.ld = N;
    g.B.ptr = w; g.B.kind = 1; g.B.ld = K;  // element (r = k_in, kk = n_out) at w + n_out*K + k_in
    g.M = M; g.N = K; g.K = N;
    const int sk = ws ? linear_splitk(M, K, N) : 1;
    if (sk > 1) {
        g.splitk = sk; g.bm = linear_tile(M, K).bm; g.bn = linear_tile(M, K).bn;
        g.C = ws; g.ldc = K;
        int rc = koaf_gemm(&g, stream);
        if (rc != KOAF_OK) return rc;
        return koaf_slab_reduce_epilogue(ws, sk, M, K, nullptr, residual, K, dx, K, stream);
    }
    g.C = dx; g.ldc = K;
    g.residual = residual; g.ldr = K;
    return koaf_gemm(&g, stream);
}
extern "C" int koaf_linear_wgrad(const float* dy, const float* x, float* dw, float* db, float* ws, int32_t M, int32_t N,
                                 int32_t K, void* stream) {
    KOAF_REQUIRE(dy && x && dw && M > 0 && N > 0 && K > 0, "koaf_linear_wgrad: bad args");
    if (narrow_head(M, N, K)) {
        hipLaunchKernelGGL(head_wgrad_kernel, dim3((unsigned)cdiv64((int64_t)N * K, 256)), dim3(256), 0, STREAM, dy, x, dw, M,
                           N, K);
        int rc = koaf_check_launch("koaf_linear_wgrad");
        if (rc != KOAF_OK || !db) return rc;
        return koaf_colsum(dy, db, M, N, ws, stream);
    }
    KoafGemm g;
    zero_gemm(&g);
    g.prec = 1;
    g.A.ptr = dy; g.A.kind = 1; g.A.ld = N;
    g.B.ptr = x; g.B.kind = 1; g.B.ld = K;
    g.M = N; g.N = K; g.K = M;
    g.C = dw; g.ldc = K;
    int rc = koaf_gemm(&g, stream);
    if (rc != KOAF_OK || !db) return rc;
    return koaf_colsum(dy, db, M, N, ws, stream);
}
