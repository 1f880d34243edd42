// koaf_rows.hip -- row-wise and pointwise kernels of the transformer side: LayerNorm, softmax (attention rows), GELU / ReLU / add,
// both dropouts, the device step counter and fill.
#include "koaf_cols.h"

namespace {
// ------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * D;
    const int D4 = D / 4;
    float s = 0.f;
    for (int i = lane; i < D4; i += 64) { v4f v = *(const v4f*)&xr[i * 4]; s += v[0] + v[1] + v[2] + v[3]; }
    const float m = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int i = lane; i < D4; i += 64) {
        v4f v = *(const v4f*)&xr[i * 4] - m;
        q += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int i = lane; i < D4; i += 64) {
        v4f v = (*(const v4f*)&xr[i * 4] - m) * rs;
        v = v * *(const v4f*)&gamma[i * 4] + *(const v4f*)&beta[i * 4];
        *(v4f*)&y[(int64_t)row * D + i * 4] = v;
    }
    if (lane == 0) { mean[row] = m; rstd[row] = rs; }
}

// dx per row (one wave per row) ...
__global__ void __launch_bounds__(256) layernorm_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dx,
                                                               int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * D;
    const float* gr = dy + (int64_t)row * D;
    const int D4 = D / 4;
    const float m = mean[row], rs = rstd[row];
    float a = 0.f, b = 0.f;
    for (int i = lane; i < D4; i += 64) {
        v4f g = *(const v4f*)&gr[i * 4] * *(const v4f*)&gamma[i * 4];
        v4f xh = (*(const v4f*)&xr[i * 4] - m) * rs;
        a += g[0] + g[1] + g[2] + g[3];
        b += g[0] * xh[0] + g[1] * xh[1] + g[2] * xh[2] + g[3] * xh[3];
    }
    a = wave_sum(a) / (float)D;
    b = wave_sum(b) / (float)D;
    for (int i = lane; i < D4; i += 64) {
        v4f g = *(const v4f*)&gr[i * 4] * *(const v4f*)&gamma[i * 4];
        v4f xh = (*(const v4f*)&xr[i * 4] - m) * rs;
        *(v4f*)&dx[(int64_t)row * D + i * 4] = (g - a - xh * b) * rs;
    }
}
// ... and the parameter gradients as column partials: part[blk][0] = sum dy*xhat, [1] = sum dy
__global__ void __launch_bounds__(256) layernorm_bwd_param_kernel(const float* __restrict__ dy,
                                                                  const float* __restrict__ x,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, int64_t rows, int D,
                                                                  ColGeom geo, float* __restrict__ part) {
    const int t = threadIdx.x, cvx = t % geo.CV, ry = t / geo.CV;
    const int c0 = blockIdx.y * geo.CW + 4 * cvx;
    const int64_t rbeg = (int64_t)blockIdx.x * geo.rpb;
    const int64_t rend = min(rows, rbeg + (int64_t)geo.rpb);
    v4f s[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int64_t r = rbeg + ry; r < rend; r += geo.RP) {
        v4f g = *(const v4f*)&dy[r * D + c0];
        v4f xh = (*(const v4f*)&x[r * D + c0] - mean[r]) * rstd[r];
        s[0] += g * xh;
        s[1] += g;
    }
    col_block_reduce<2>(s, part, blockIdx.x, D, blockIdx.y * geo.CW, geo.CV, geo.RP);
}
}  // namespace

extern "C" int koaf_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                  float* rstd, int32_t rows, int32_t D, float eps, void* stream) {
    KOAF_REQUIRE(x && gamma && beta && y && mean && rstd && rows > 0 && D % 4 == 0, "koaf_layernorm_fwd: bad args");
    hipLaunchKernelGGL(layernorm_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, STREAM, x, gamma, beta, y, mean, rstd,
                       rows, D, eps);
    return koaf_check_launch("koaf_layernorm_fwd");
}
extern "C" int64_t koaf_layernorm_bwd_ws(int32_t rows, int32_t D) {
    ColGeom g;
    if (!col_geom(rows, D, 256, &g)) return -1;
    return (int64_t)g.nblk * 2 * D;
}
extern "C" int koaf_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                                  const float* rstd, float* dx, float* dgamma, float* dbeta, float* part, int32_t rows,
                                  int32_t D, void* stream) {
    ColGeom g;
    KOAF_REQUIRE(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && part && rows > 0,
                 "koaf_layernorm_bwd: bad args");
    KOAF_REQUIRE(col_geom(rows, D, 256, &g), "koaf_layernorm_bwd: unsupported D=%d", D);
    hipLaunchKernelGGL(layernorm_bwd_dx_kernel, dim3((rows + 3) / 4), dim3(256), 0, STREAM, dy, x, gamma, mean, rstd,
                       dx, rows, D);
    hipLaunchKernelGGL(layernorm_bwd_param_kernel, dim3(g.nblk, g.nchunk), dim3(256), 0, STREAM, dy, x, mean, rstd,
                       (int64_t)rows, D, g, part);
    hipLaunchKernelGGL(colfinal_kernel<2>, dim3((D + 63) / 64), dim3(1024), 0, STREAM, part, g.nblk, D, dgamma, dbeta);
    return koaf_check_launch("koaf_layernorm_bwd");
}

namespace {
// ------------------------------------------------------------------------------------------------
// softmax rows (attention), in place; one wave per row
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) softmax_rows_kernel(float* __restrict__ x, int64_t rows, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* xr = x + row * n;
    float m = -INFINITY;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, xr[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += expf(xr[i] - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int i = lane; i < n; i += 64) xr[i] = expf(xr[i] - m) * inv;
}
// ds = p * (dp - sum(dp*p)) * scale, in place on dp
__global__ void __launch_bounds__(256) softmax_bwd_rows_kernel(float* __restrict__ dp, const float* __restrict__ p,
                                                               int64_t rows, int n, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* dr = dp + row * n;
    const float* pr = p + row * n;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += dr[i] * pr[i];
    s = wave_sum(s);
    for (int i = lane; i < n; i += 64) dr[i] = pr[i] * (dr[i] - s) * scale;
}
}  // namespace

extern "C" int koaf_softmax_rows(float* x, int64_t rows, int32_t n, void* stream) {
    KOAF_REQUIRE(x && rows > 0 && n > 0, "koaf_softmax_rows: bad args");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, STREAM, x, rows, n);
    return koaf_check_launch("koaf_softmax_rows");
}
extern "C" int koaf_softmax_bwd_rows(float* dp, const float* p, int64_t rows, int32_t n, float scale, void* stream) {
    KOAF_REQUIRE(dp && p && rows > 0 && n > 0, "koaf_softmax_bwd_rows: bad args");
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, STREAM, dp, p, rows, n,
                       scale);
    return koaf_check_launch("koaf_softmax_bwd_rows");
}

namespace {
// ------------------------------------------------------------------------------------------------
// pointwise
// ------------------------------------------------------------------------------------------------
enum { PW_GELU_F, PW_GELU_B, PW_RELU_F, PW_RELU_B, PW_ADD };
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_d(float x) {
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return cdf + x * pdf;
}
template <int OP>
__global__ void __launch_bounds__(256) pointwise_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ out, int64_t n) {
    const int64_t nvec = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        v4f x = *(const v4f*)&a[i * 4], y = {0, 0, 0, 0}, o;
        if (OP == PW_GELU_B || OP == PW_RELU_B || OP == PW_ADD) y = *(const v4f*)&b[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (OP == PW_GELU_F) o[j] = gelu_f(x[j]);
            else if (OP == PW_GELU_B) o[j] = x[j] * gelu_d(y[j]);       // a = dy, b = x
            else if (OP == PW_RELU_F) o[j] = fmaxf(x[j], 0.f);
            else if (OP == PW_RELU_B) o[j] = y[j] > 0.f ? x[j] : 0.f;   // a = dy, b = y
            else o[j] = x[j] + y[j];
        }
        *(v4f*)&out[i * 4] = o;
    }
    // tail
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = nvec * 4 + threadIdx.x;
        float x = a[i], y = (OP == PW_GELU_B || OP == PW_RELU_B || OP == PW_ADD) ? b[i] : 0.f, o;
        if (OP == PW_GELU_F) o = gelu_f(x);
        else if (OP == PW_GELU_B) o = x * gelu_d(y);
        else if (OP == PW_RELU_F) o = fmaxf(x, 0.f);
        else if (OP == PW_RELU_B) o = y > 0.f ? x : 0.f;
        else o = x + y;
        out[i] = o;
    }
}
}  // namespace

#define PW_LAUNCH(OP, a, b, out, n, name)                                                                      \
    KOAF_REQUIRE((a) && (out) && (n) > 0, name ": bad args");                                                  \
    KOAF_REQUIRE(aligned16(a) && aligned16(out) && (!(b) || aligned16(b)), name ": unaligned");                \
    hipLaunchKernelGGL(pointwise_kernel<OP>, dim3(ew_grid(((n) + 3) / 4)), dim3(EB), 0, STREAM, a, b, out, n); \
    return koaf_check_launch(name)

extern "C" int koaf_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
    PW_LAUNCH(PW_GELU_F, x, (const float*)nullptr, y, n, "koaf_gelu_fwd");
}
extern "C" int koaf_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
    KOAF_REQUIRE(x, "koaf_gelu_bwd: bad args");
    PW_LAUNCH(PW_GELU_B, dy, x, dx, n, "koaf_gelu_bwd");
}
extern "C" int koaf_relu_fwd(const float* x, float* y, int64_t n, void* stream) {
    PW_LAUNCH(PW_RELU_F, x, (const float*)nullptr, y, n, "koaf_relu_fwd");
}
extern "C" int koaf_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream) {
    KOAF_REQUIRE(y, "koaf_relu_bwd: bad args");
    PW_LAUNCH(PW_RELU_B, dy, y, dx, n, "koaf_relu_bwd");
}
extern "C" int koaf_add(const float* a, const float* b, float* out, int64_t n, void* stream) {
    KOAF_REQUIRE(b, "koaf_add: bad args");
    PW_LAUNCH(PW_ADD, a, b, out, n, "koaf_add");
}

namespace {
// (mix64, the counter-based generator's hash: koaf_common.h -- shared with koaf_attr.hip)
// `epoch` (nullable): a device-resident step counter folded into the seed, so that a HIP-graph replay of a captured step
// (whose `seed` argument is frozen) still draws fresh masks every step; forward and backward of one step read the same value
__device__ __forceinline__ uint64_t step_seed(uint64_t seed, const int64_t* epoch) {
    return epoch ? seed ^ mix64(0x9E3779B97F4A7C15ull * (uint64_t)(*epoch + 1)) : seed;
}

__global__ void __launch_bounds__(256) dropout_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                      float p, float inv_keep, uint64_t seed0, const int64_t* epoch) {
    const uint64_t seed = step_seed(seed0, epoch);
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
        const uint64_t h = mix64(seed ^ mix64((uint64_t)i));
        const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
        y[i] = (u >= p) ? x[i] * inv_keep : 0.f;
    }
}

// nn.Dropout2d on an NHWC feature map: one Bernoulli draw per (image, channel), index n*C + c -- the same draw the
// element-wise kernel makes on the (N, C) pooled output, so pooled and spatial encoders share their masks
__global__ void __launch_bounds__(256) dropout2d_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                        int64_t hwc, int C, float p, float inv_keep, uint64_t seed0,
                                                        const int64_t* epoch) {
    const uint64_t seed = step_seed(seed0, epoch);
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
        const int64_t idx = (i / hwc) * C + (i % C);
        const uint64_t h = mix64(seed ^ mix64((uint64_t)idx));
        const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
        y[i] = (u >= p) ? x[i] * inv_keep : 0.f;
    }
}
}  // namespace

extern "C" int koaf_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, const int64_t* epoch, void* stream) {
    KOAF_REQUIRE(x && y && n > 0 && p >= 0.f && p < 1.f, "koaf_dropout: bad args");
    hipLaunchKernelGGL(dropout_kernel, dim3(ew_grid(n)), dim3(EB), 0, STREAM, x, y, n, p, 1.f / (1.f - p), seed, epoch);
    return koaf_check_launch("koaf_dropout");
}
extern "C" int koaf_dropout2d(const float* x, float* y, int32_t N, int32_t HW, int32_t C, float p, uint64_t seed,
                              const int64_t* epoch, void* stream) {
    KOAF_REQUIRE(x && y && N > 0 && HW > 0 && C > 0 && p >= 0.f && p < 1.f, "koaf_dropout2d: bad args");
    const int64_t n = (int64_t)N * HW * C;
    hipLaunchKernelGGL(dropout2d_kernel, dim3(ew_grid(n)), dim3(EB), 0, STREAM, x, y, n, (int64_t)HW * C, C, p,
                       1.f / (1.f - p), seed, epoch);
    return koaf_check_launch("koaf_dropout2d");
}

namespace {
__global__ void counter_add_kernel(int64_t* ctr, int64_t delta) { *ctr += delta; }

__global__ void __launch_bounds__(256) fill_kernel(float* __restrict__ p, float v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) p[i] = v;
}
}  // namespace

extern "C" int koaf_counter_add(int64_t* counter, int64_t delta, void* stream) {
    KOAF_REQUIRE(counter, "koaf_counter_add: null counter");
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, STREAM, counter, delta);
    return koaf_check_launch("koaf_counter_add");
}
extern "C" int koaf_fill(float* p, float value, int64_t n, void* stream) {
    KOAF_REQUIRE(p && n > 0, "koaf_fill: bad args");
    hipLaunchKernelGGL(fill_kernel, dim3(ew_grid(n)), dim3(EB), 0, STREAM, p, value, n);
    return koaf_check_launch("koaf_fill");
}
