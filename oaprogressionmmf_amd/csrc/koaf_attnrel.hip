// koaf_attnrel.hip -- attention relevance of the FeaT fusion (not in the reference): the per-layer matrices of attention rollout
// (Abnar & Zuidema 2020) and of the gradient-weighted self-attention rule (Chefer et al. 2021), their chain product carried as a
// few rows from the left, and the per-slice / per-modality totals of a relevance row.  Full fp32 products, fp32 or fp64 sums in a
// fixed order, no atomics: two runs give the same bits.
#include "koaf_common.h"

namespace {

constexpr int AR_BLOCK = 256;        // rollout: one block of four waves per attention row
constexpr int AR_T = 64;             // gradient rule: a block owns a 64 x 64 tile of abar ...
constexpr int AR_KC = 16;            // ... and walks d in chunks of 16
constexpr int AR_LD = AR_T + 4;      // LDS row pitch: 16-byte aligned rows, the transposing stores spread over the banks
constexpr int AP_Q = 4;              // apply: rows of r a block carries through one pass over abar
constexpr int AP_S = 16;             // apply: interleaved slices of the m range, one wave each, added as a pairwise tree

// Rollout layer.  One block of four waves per row (b, i): f[j] = fuse_h attn[b][h][i][j] (heads in index order: a running sum
// divided by h, a running max or min), + 1 at j == i; the row is divided by its sum.  Thread t owns the columns t, t + 256, ...: it
// writes f and adds it to an fp64 partial; the 64 partials of a wave meet in a xor butterfly and the four waves as (0 + 1) + (2 + 3)
// (fp64: the sum of n fp32 values carries no fp32 rounding of its own); the thread then re-reads its own f and stores
// (float)(f / sum).  Per element: h - 1 additions and one division (mean), the identity's addition, the final division -- at most
// h + 2 roundings, all on non-negative terms.
__global__ void __launch_bounds__(AR_BLOCK) attn_rollout_kernel(const float* __restrict__ attn, float* __restrict__ abar, int n, int h,
                                                               int mode) {
    __shared__ double red[AR_BLOCK / 64];
    const int64_t row = blockIdx.x;
    const int64_t b = row / n;
    const int i = (int)(row - b * n);
    const int64_t nn = (int64_t)n * n;
    const float* a = attn + b * h * nn + (int64_t)i * n;
    float* o = abar + row * n;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += AR_BLOCK) {
        float f = a[j];
        if (mode == 0) {
#pragma unroll 8
            for (int hh = 1; hh < h; ++hh) f += a[hh * nn + j];
            f = f / (float)h;
        } else if (mode == 1) {
#pragma unroll 8
            for (int hh = 1; hh < h; ++hh) { const float v = a[hh * nn + j]; f = v > f ? v : f; }
        } else {
#pragma unroll 8
            for (int hh = 1; hh < h; ++hh) { const float v = a[hh * nn + j]; f = v < f ? v : f; }
        }
        if (j == i) f += 1.f;
        o[j] = f;
        s += (double)f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    for (int j = threadIdx.x; j < n; j += AR_BLOCK) o[j] = (float)((double)o[j] / s);       // (the thread's own stores: program order)
}

// Gradient rule layer.  abar[b][i][j] = (1 / h) sum_h relu(attn[b][h][i][j] * dP), dP = sum_k dout[b][i][h d + k] *
// qkv[b][j][2 h_all d + h d + k]: a [n, d] x [d, n] product per (b, h) that exists only in registers.  Block (tj, ti, b) owns a
// 64 x 64 tile; per head it stages 64 x 16 chunks of dout and V in LDS k-major, each thread runs one fmaf chain of d links (k
// in index order) for each of its 4 x 4 elements, multiplies by attn, clamps at 0 and adds the head to its running sum (heads in
// index order); the sum is divided by h at the end.  Rows, columns and k beyond n / d are staged as zeros and never stored.
__global__ void __launch_bounds__(256) attn_grad_kernel(const float* __restrict__ attn, const float* __restrict__ dout,
                                                        const float* __restrict__ qkv, float* __restrict__ abar, int n, int h, int d,
                                                        int vec) {
    __shared__ __attribute__((aligned(16))) float As[AR_KC][AR_LD];
    __shared__ __attribute__((aligned(16))) float Bs[AR_KC][AR_LD];
    const int b = blockIdx.z, i0 = blockIdx.y * AR_T, j0 = blockIdx.x * AR_T;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int lr = t >> 2, lk = (t & 3) * 4;                  // staging: row lr of the tile, 4 consecutive k from lk
    const int64_t hd = (int64_t)h * d, nn = (int64_t)n * n;
    const float* dob = dout + (int64_t)b * n * hd;
    const float* vb = qkv + (int64_t)b * n * 3 * hd + 2 * hd;
    const float* ab = attn + (int64_t)b * h * nn;
    const bool ra = i0 + lr < n, rb = j0 + lr < n;
    const float* arow = dob + (int64_t)(i0 + lr) * hd;
    const float* brow = vb + (int64_t)(j0 + lr) * 3 * hd;
    float sum[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) sum[u][v] = 0.f;
    for (int hh = 0; hh < h; ++hh) {
        float acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
        const int c0 = hh * d;
        for (int k0 = 0; k0 < d; k0 += AR_KC) {
            float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
            const int k = k0 + lk;
            if (vec && k + 3 < d) {
                if (ra) { const v4f x = *(const v4f*)(arow + c0 + k); av[0] = x[0]; av[1] = x[1]; av[2] = x[2]; av[3] = x[3]; }
                if (rb) { const v4f x = *(const v4f*)(brow + c0 + k); bv[0] = x[0]; bv[1] = x[1]; bv[2] = x[2]; bv[3] = x[3]; }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ra && k + u < d) av[u] = arow[c0 + k + u];
                    if (rb && k + u < d) bv[u] = brow[c0 + k + u];
                }
            }
            __syncthreads();                                   // (the previous chunk's readers are done)
#pragma unroll
            for (int u = 0; u < 4; ++u) { As[lk + u][lr] = av[u]; Bs[lk + u][lr] = bv[u]; }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < AR_KC; ++kk) {
                const v4f x = *(const v4f*)&As[kk][ty * 4], y = *(const v4f*)&Bs[kk][tx * 4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(x[u], y[v], acc[u][v]);
            }
        }
        const float* ah = ab + hh * nn;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + ty * 4 + u;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = j0 + tx * 4 + v;
                if (i < n && j < n) {
                    const float p = ah[(int64_t)i * n + j] * acc[u][v];
                    sum[u][v] += p < 0.f ? 0.f : p;           // (a NaN fails the comparison and stays)
                }
            }
        }
    }
    const float hf = (float)h;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            if (i < n && j < n) abar[(int64_t)b * nn + (int64_t)i * n + j] = sum[u][v] / hf;
        }
    }
}

// r_out[b][qi][j] = sum_m r_in[b][qi][m] * abar[b][m][j] (+ r_in[b][qi][j]).  Block (tj, tq, b): 64 columns, up to AP_Q rows;
// wave w adds the terms m = w, w + 16, ... in that order as one fmaf chain per row, and the sixteen chains meet in a pairwise tree
// ((0 + 1) + (2 + 3)) + ...: ceil(n / 16) + 4 roundings, then the identity's addition.  abar is read once per AP_Q rows,
// coalesced; the r_in value of a wave is one address (a broadcast).
__global__ void __launch_bounds__(64 * AP_S) attn_apply_kernel(const float* __restrict__ r_in, const float* __restrict__ abar,
                                                               float* __restrict__ r_out, int q, int n, int add_identity) {
    __shared__ float part[AP_S][AP_Q][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.z, q0 = blockIdx.y * AP_Q, j = blockIdx.x * 64 + lane;
    const int nq = min(AP_Q, q - q0);
    const float* A = abar + (int64_t)b * n * n;
    const float* R = r_in + ((int64_t)b * q + q0) * n;
    float acc[AP_Q];
#pragma unroll
    for (int u = 0; u < AP_Q; ++u) acc[u] = 0.f;
    if (j < n) {
#pragma unroll 8
        for (int m = w; m < n; m += AP_S) {
            const float a = A[(int64_t)m * n + j];
#pragma unroll
            for (int u = 0; u < AP_Q; ++u)
                if (u < nq) acc[u] = fmaf(R[(int64_t)u * n + m], a, acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < AP_Q; ++u) part[w][u][lane] = acc[u];
    __syncthreads();
    if (w == 0 && j < n) {
        for (int u = 0; u < nq; ++u) {
            float v[AP_S];
#pragma unroll
            for (int c = 0; c < AP_S; ++c) v[c] = part[c][u][lane];
#pragma unroll
            for (int st = 1; st < AP_S; st *= 2)
#pragma unroll
                for (int c = 0; c < AP_S; c += 2 * st) v[c] += v[c + st];
            if (add_identity) v[0] += R[(int64_t)u * n + j];
            r_out[((int64_t)b * q + q0 + u) * n + j] = v[0];
        }
    }
}

// r_in NULL: the identity from the left -- r_out = abar (+ I), a copy
__global__ void __launch_bounds__(256) attn_apply_eye_kernel(const float* __restrict__ abar, float* __restrict__ r_out, int64_t total,
                                                             int n, int add_identity) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        float v = abar[e];
        if (add_identity) {
            const int64_t r = e / n;
            if (e - r * n == r % n) v += 1.f;
        }
        r_out[e] = v;
    }
}

// out[b][k] = sum_{u < t} r[b][off + k t + u]: one thread per (b, k), the terms in index order into an fp64 sum, rounded once
__global__ void __launch_bounds__(256) attn_segsum_kernel(const float* __restrict__ r, float* __restrict__ out, int64_t total, int n,
                                                          int off, int K, int t) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t b = e / K;
    const int k = (int)(e - b * K);
    const float* p = r + b * n + off + (int64_t)k * t;
    double s = 0.0;
    for (int u = 0; u < t; ++u) s += (double)p[u];
    out[e] = (float)s;
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb * 4 && y < x + (uintptr_t)na * 4;
}

}  // namespace

extern "C" int koaf_attn_layer(const float* attn, const float* dout, const float* qkv, float* abar, int32_t B, int32_t n, int32_t h,
                               int32_t d, int32_t mode, void* stream) {
    KOAF_REQUIRE(mode >= 0 && mode <= 3, "koaf_attn_layer: mode is 0 (mean), 1 (max), 2 (min) or 3 (gradient rule), got %d", mode);
    KOAF_REQUIRE(attn && abar, "koaf_attn_layer: attn and abar are required");
    KOAF_REQUIRE(B >= 1 && n >= 1 && h >= 1 && d >= 1, "koaf_attn_layer: B, n, h, d >= 1 (B = %d, n = %d, h = %d, d = %d)", B, n, h, d);
    KOAF_REQUIRE((int64_t)B * h * n * n < (1ll << 40) && (int64_t)h * d < (1ll << 28), "koaf_attn_layer: tensor too large");
    KOAF_REQUIRE(!overlap(attn, (int64_t)B * h * n * n, abar, (int64_t)B * n * n), "koaf_attn_layer: abar overlaps attn");
    if (mode < 3) {
        KOAF_REQUIRE(!dout && !qkv, "koaf_attn_layer: the rollout modes take no dout / qkv");
        const int64_t rows = (int64_t)B * n;
        KOAF_REQUIRE(rows < (1ll << 31), "koaf_attn_layer: B * n too large");
        hipLaunchKernelGGL(attn_rollout_kernel, dim3((unsigned)rows), dim3(AR_BLOCK), 0, STREAM, attn, abar, n, h, mode);
        return koaf_check_launch("koaf_attn_layer");
    }
    KOAF_REQUIRE(dout && qkv, "koaf_attn_layer: the gradient rule needs dout and qkv");
    KOAF_REQUIRE(B <= 65535 && cdiv64(n, AR_T) <= 65535, "koaf_attn_layer: B <= 65535 and n <= %d in the gradient rule", 65535 * AR_T);
    KOAF_REQUIRE(!overlap(dout, (int64_t)B * n * h * d, abar, (int64_t)B * n * n) &&
                 !overlap(qkv, (int64_t)B * n * 3 * h * d, abar, (int64_t)B * n * n), "koaf_attn_layer: abar overlaps dout / qkv");
    const int vec = d % 4 == 0 && aligned16(dout) && aligned16(qkv);
    const unsigned tiles = (unsigned)cdiv64(n, AR_T);
    hipLaunchKernelGGL(attn_grad_kernel, dim3(tiles, tiles, B), dim3(256), 0, STREAM, attn, dout, qkv, abar, n, h, d, vec);
    return koaf_check_launch("koaf_attn_layer");
}

extern "C" int koaf_attn_apply(const float* r_in, const float* abar, float* r_out, int32_t B, int32_t q, int32_t n, int32_t add_identity,
                               void* stream) {
    KOAF_REQUIRE(abar && r_out, "koaf_attn_apply: abar and r_out are required");
    KOAF_REQUIRE(B >= 1 && B <= 65535 && q >= 1 && n >= 1, "koaf_attn_apply: 1 <= B <= 65535, q >= 1, n >= 1 (B = %d, q = %d, n = %d)", B,
                 q, n);
    KOAF_REQUIRE(add_identity == 0 || add_identity == 1, "koaf_attn_apply: add_identity is 0 or 1");
    KOAF_REQUIRE(r_in || q == n, "koaf_attn_apply: r_in NULL stands for the identity, q == n (q = %d, n = %d)", q, n);
    KOAF_REQUIRE(cdiv64(q, AP_Q) <= 65535 && (int64_t)B * n * n < (1ll << 40) && (int64_t)B * q * n < (1ll << 40),
                 "koaf_attn_apply: q <= %d, tensors below 2^40 elements", 65535 * AP_Q);
    const int64_t nr = (int64_t)B * q * n, na = (int64_t)B * n * n;
    KOAF_REQUIRE(!overlap(r_out, nr, abar, na) && !(r_in && overlap(r_out, nr, r_in, nr)), "koaf_attn_apply: r_out aliases an input");
    if (!r_in) {
        hipLaunchKernelGGL(attn_apply_eye_kernel, dim3(ew_grid(na)), dim3(256), 0, STREAM, abar, r_out, na, n, add_identity);
        return koaf_check_launch("koaf_attn_apply");
    }
    hipLaunchKernelGGL(attn_apply_kernel, dim3((unsigned)cdiv64(n, 64), (unsigned)cdiv64(q, AP_Q), B), dim3(64 * AP_S), 0, STREAM, r_in,
                       abar, r_out, q, n, add_identity);
    return koaf_check_launch("koaf_attn_apply");
}

extern "C" int koaf_attn_segsum(const float* r, float* out, int32_t B, int32_t n, int32_t off, int32_t K, int32_t t, void* stream) {
    KOAF_REQUIRE(r && out, "koaf_attn_segsum: r and out are required");
    KOAF_REQUIRE(B >= 1 && n >= 1 && K >= 1 && t >= 1 && off >= 0, "koaf_attn_segsum: B, n, K, t >= 1 and off >= 0");
    KOAF_REQUIRE((int64_t)off + (int64_t)K * t <= n, "koaf_attn_segsum: the segment [%d, %d + %d * %d) leaves the row of n = %d", off, off,
                 K, t, n);
    const int64_t total = (int64_t)B * K;
    KOAF_REQUIRE(cdiv64(total, 256) < (1ll << 31), "koaf_attn_segsum: B * K too large");
    KOAF_REQUIRE(!overlap(r, (int64_t)B * n, out, total), "koaf_attn_segsum: out overlaps r");
    hipLaunchKernelGGL(attn_segsum_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, STREAM, r, out, total, n, off, K, t);
    return koaf_check_launch("koaf_attn_segsum");
}
