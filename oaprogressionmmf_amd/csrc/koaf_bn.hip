// koaf_bn.hip -- the HBM-bound kernels of the convolutional trunk: column statistics and sums, BatchNorm finalize / backward, the
// bottleneck tail, the 3x3 / stride-2 max-pool and GAP (the pool lives here: bn_bwd_reduce_kernel<H, true> gathers its gradient).
// All are float4-vectorised along the channel (fastest) axis and sized for >= 8 blocks per CU.
#include "koaf_cols.h"

namespace {
template <bool H>
__global__ void __launch_bounds__(256) colstats_kernel(const float* __restrict__ x, int64_t rows, int C,
                                                       ColGeom g, float* __restrict__ part, int sq,
                                                       const float* __restrict__ shift) {
    const int t = threadIdx.x, cvx = t % g.CV, ry = t / g.CV;
    const int c0 = blockIdx.y * g.CW;
    const int64_t rbeg = (int64_t)blockIdx.x * g.rpb;
    const int64_t rend = min(rows, rbeg + (int64_t)g.rpb);
    v4f s[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    v4f k = {0, 0, 0, 0};
    if (shift) k = *(const v4f*)&shift[c0 + 4 * cvx];       // sums about the shift (see KoafGemm.stats_shift)
    for (int64_t r = rbeg + ry; r < rend; r += g.RP) {
        v4f v = load4<H>(x, r * C + c0 + 4 * cvx) - k;
        s[0] += v;
        s[1] += v * v;
    }
    if (sq) col_block_reduce<2>(s, part, blockIdx.x, C, c0, g.CV, g.RP);
    else {
        v4f s1[1] = {s[0]};
        col_block_reduce<1>(s1, part, blockIdx.x, C, c0, g.CV, g.RP);
    }
}

// generic tiny-C column sum (C not a multiple of 4, e.g. the 2-class head bias)
__global__ void colsum_small_kernel(const float* __restrict__ x, int rows, int C, float* __restrict__ out) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float a = 0.f;
    for (int r = 0; r < rows; ++r) a += x[(int64_t)r * C + c];
    out[c] = a;
}
}  // namespace

extern "C" int koaf_colstats(const float* x, int64_t rows, int32_t C, float* part, int32_t* part_rows,
                             const float* shift, int32_t act16, void* stream) {
    ColGeom g;
    KOAF_REQUIRE(x && part && part_rows && rows > 0, "koaf_colstats: bad args");
    KOAF_REQUIRE(col_geom(rows, C, 1024, &g), "koaf_colstats: unsupported C=%d", C);
    KOAF_LAUNCH_ACT16(act16, colstats_kernel<A16>, dim3(g.nblk, g.nchunk), dim3(256), 0, STREAM, x, rows, C, g, part, 1, shift);
    *part_rows = g.nblk;
    return koaf_check_launch("koaf_colstats");
}
extern "C" int32_t koaf_colpart_rows(int64_t rows, int32_t C) {
    ColGeom g;
    if (!col_geom(rows, C, 1024, &g)) return -1;
    return g.nblk;
}

extern "C" int koaf_colsum(const float* x, float* out, int32_t rows, int32_t C, float* part, void* stream) {
    KOAF_REQUIRE(x && out && rows > 0 && C > 0, "koaf_colsum: bad args");
    ColGeom g;
    if (part && aligned16(x) && col_geom(rows, C, 256, &g)) {
        hipLaunchKernelGGL(colstats_kernel<false>, dim3(g.nblk, g.nchunk), dim3(256), 0, STREAM, x, (int64_t)rows, C, g, part,
                           0, (const float*)nullptr);
        hipLaunchKernelGGL(colfinal_kernel<1>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, part, g.nblk, C, out,
                           (float*)nullptr);
    } else {
        hipLaunchKernelGGL(colsum_small_kernel, dim3((C + 255) / 256), dim3(256), 0, STREAM, x, rows, C, out);
    }
    return koaf_check_launch("koaf_colsum");
}
extern "C" int64_t koaf_colsum_ws(int32_t rows, int32_t C) {
    ColGeom g;
    if (!col_geom(rows, C, 256, &g)) return 0;
    return (int64_t)g.nblk * C;
}

namespace {
// ------------------------------------------------------------------------------------------------
// BatchNorm finalize (train: from partial column sums; eval: running stats)
// ------------------------------------------------------------------------------------------------
// Stage 1 of the per-channel finalisations when there are many partial rows (one per 128-row GEMM tile: 6400 for a
// layer-1 activation of the native batch): src [rows][nsum][C] fp32 -> ws [S][2][C] fp64, block (bx, s) sums row
// slice s of sums (0, i1) for 64 channels.  Fixed slice boundaries and summation order: deterministic.
__global__ void __launch_bounds__(1024) part_reduce_kernel(const float* __restrict__ src, int rows, int C, int nsum,
                                                           int i1, int chunk, double* __restrict__ ws) {
    __shared__ double red[2][16][64];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const int r0 = blockIdx.y * chunk, r1 = min(rows, r0 + chunk);
    double a = 0.0, b = 0.0;
    if (c < C)
        for (int r = r0 + gy; r < r1; r += 16) {
            a += (double)src[((int64_t)r * nsum + 0) * C + c];
            b += (double)src[((int64_t)r * nsum + i1) * C + c];
        }
    red[0][gy][cx] = a;
    red[1][gy][cx] = b;
    __syncthreads();
    if (gy < 2 && c < C) {
        double t = 0.0;
        for (int j = 0; j < 16; ++j) t += red[gy][j][cx];
        ws[((int64_t)blockIdx.y * 2 + gy) * C + c] = t;
    }
}

// slices of the two-stage reduction: 0 = single stage
static inline int part_slices(int rows) { return rows > 128 ? (rows >= 4096 ? 64 : (rows + 63) / 64) : 0; }

template <typename T>
__global__ void __launch_bounds__(1024) bn_finalize_kernel(const T* __restrict__ stats, int rows, int C,
                                                           double inv_count, double unbias,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* running_mean,
                                                           float* running_var, int64_t* nbt, float momentum,
                                                           float eps, int train, float* mean, float* invstd,
                                                           float* sc, float* sh, const float* __restrict__ shift,
                                                           uint32_t* status) {
    __shared__ double red[2][16][64];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    if (train) {
        double a = 0.0, b = 0.0;
        if (c < C)
            for (int r = gy; r < rows; r += 16) {
                a += (double)stats[((int64_t)r * 2 + 0) * C + c];
                b += (double)stats[((int64_t)r * 2 + 1) * C + c];
            }
        red[0][gy][cx] = a;
        red[1][gy][cx] = b;
        __syncthreads();
    }
    if (gy == 0 && c < C) {
        float m, var;
        if (train) {
            double s1 = 0.0, s2 = 0.0;
            for (int j = 0; j < 16; ++j) { s1 += red[0][j][cx]; s2 += red[1][j][cx]; }
            double dm = s1 * inv_count;                 // mean of (x - k)
            double dv = s2 * inv_count - dm * dm;
            if (dv < 0.0) dv = 0.0;
            if (shift) dm += (double)shift[c];          // (read before running_mean, possibly the same buffer, is updated)
            m = (float)dm;
            var = (float)dv;
            // momentum < 0 = nn.BatchNorm2d(momentum=None): cumulative moving average, factor 1 / num_batches_tracked (which
            // the entry point has already incremented for this batch: torch increments first, torch/nn/modules/batchnorm.py)
            const float f = momentum < 0.f ? 1.f / (float)(*nbt) : momentum;
            running_mean[c] = (1.f - f) * running_mean[c] + f * m;
            running_var[c] = (1.f - f) * running_var[c] + f * (float)(dv * unbias);
        } else {
            m = running_mean[c];
            var = running_var[c];
        }
        float is = 1.0f / sqrtf(var + eps);
        float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
        mean[c] = m;
        invstd[c] = is;
        sc[c] = g * is;
        sh[c] = b - m * g * is;
        // a NaN / Inf in the conv output reaches the statistics, and from there every element of the channel: say so (the
        // consumers' fp16 clamp would turn relu(NaN * x + NaN) into 0)
        if (!koaf_bits_finite(koaf_absbits(g * is)) || !koaf_bits_finite(koaf_absbits(b - m * g * is))) koaf_status_add(status, 1, 1u);
    }
    if (train && nbt && momentum >= 0.f && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}
}  // namespace

extern "C" int64_t koaf_bn_reduce_ws(int32_t rows, int32_t C) {
    const int S = part_slices(rows);
    return S ? (int64_t)S * 2 * C * (int64_t)sizeof(double) : 0;
}

// stage 1 when it pays; returns the slice count (0: the caller reads the fp32 rows itself)
static int part_reduce(const float* src, int rows, int C, int nsum, int i1, double* ws, hipStream_t st) {
    const int S = ws ? part_slices(rows) : 0;
    if (!S) return 0;
    const int chunk = (rows + S - 1) / S;
    hipLaunchKernelGGL(part_reduce_kernel, dim3((C + 63) / 64, S), dim3(1024), 0, st, src, rows, C, nsum, i1, chunk, ws);
    return S;
}

extern "C" int koaf_bn_finalize(const float* stats, int32_t rows, int32_t C, int64_t count, const float* gamma,
                                const float* beta, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float momentum, float eps, int32_t train, float* mean,
                                float* invstd, float* sc, float* sh, const float* shift, double* ws, void* stream) {
    KOAF_REQUIRE(C > 0 && mean && invstd && sc && sh && running_mean && running_var, "koaf_bn_finalize: bad args");
    KOAF_REQUIRE(!train || (stats && rows > 0 && count > 0), "koaf_bn_finalize: train mode needs stats");
    const double inv = train ? 1.0 / (double)count : 0.0;
    const double unbias = (train && count > 1) ? (double)count / (double)(count - 1) : 1.0;
    if (train && momentum < 0.f) {
        // cumulative average (momentum None): the factor is 1 / (the count INCLUDING this batch); the blocks of the kernel
        // below all read it, so the increment is its own stream-ordered launch in front of them
        KOAF_REQUIRE(num_batches_tracked, "koaf_bn_finalize: momentum < 0 (cumulative average) needs num_batches_tracked");
        int rc = koaf_counter_add(num_batches_tracked, 1, stream);
        if (rc != KOAF_OK) return rc;
    }
    const int S = train ? part_reduce(stats, rows, C, 2, 1, ws, STREAM) : 0;
    if (S)
        hipLaunchKernelGGL(bn_finalize_kernel<double>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, ws, S, C, inv, unbias,
                           gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, train, mean,
                           invstd, sc, sh, train ? shift : nullptr, koaf_status_ptr());
    else
        hipLaunchKernelGGL(bn_finalize_kernel<float>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, stats, rows, C, inv,
                           unbias, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, train,
                           mean, invstd, sc, sh, train ? shift : nullptr, koaf_status_ptr());
    return koaf_check_launch("koaf_bn_finalize");
}

namespace {
// y = relu(sc*c+sh [+ identity])   (H: c, idt and y are bf16 activations)
template <bool H>
__global__ void __launch_bounds__(256) bn_add_relu_kernel(const float* __restrict__ c, const float* __restrict__ sc,
                                                          const float* __restrict__ sh, const float* __restrict__ idt,
                                                          const float* __restrict__ idsc,
                                                          const float* __restrict__ idsh, float* __restrict__ y,
                                                          int64_t nvec, int C4, uint32_t* status) {
    unsigned nsat = 0;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        v4f v = load4_nt<H>(c, i * 4);       // (streams: read / written once, kept out of L2's way)
        // (explicit fused multiply-adds: the loader that forms this tail on load -- KoafOperand.tf 3 -- rounds exactly alike)
        const v4f s4 = *(const v4f*)&sc[cv], h4 = *(const v4f*)&sh[cv];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(v[j], s4[j], h4[j]);
        if (idt) {
            v4f d = load4_nt<H>(idt, i * 4);
            if (idsc) {
                const v4f is4 = *(const v4f*)&idsc[cv], ih4 = *(const v4f*)&idsh[cv];
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = fmaf(d[j], is4[j], ih4[j]);
            }
            v += d;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (this tensor feeds convolutions at the fixed activation scale: |y| * KOAF_ACT_SCALE beyond the fp16 range is
            // clamped there -- counted here, where the check is free; a NaN counts too and stays a NaN in y)
            nsat += !(v[j] * KOAF_ACT_SCALE <= 65504.f) ? 1u : 0u;
            v[j] = v[j] != v[j] ? v[j] : fmaxf(v[j], 0.f);
        }
        store4_nt<H>(y, i * 4, v);
    }
    koaf_status_add(status, 0, nsat);
}
}  // namespace

extern "C" int koaf_bn_add_relu(const float* c, const float* sc, const float* sh, const float* idt, const float* idsc,
                                const float* idsh, float* y, int64_t rows, int32_t C, int32_t act16, void* stream) {
    KOAF_REQUIRE(c && sc && sh && y && rows > 0 && C > 0 && C % 4 == 0, "koaf_bn_add_relu: bad args");
    KOAF_REQUIRE(aligned16(c) && aligned16(y) && aligned16(sc) && aligned16(sh) && (!idt || aligned16(idt)), "koaf_bn_add_relu: unaligned");
    KOAF_REQUIRE((idsc == nullptr) == (idsh == nullptr), "koaf_bn_add_relu: idsc/idsh come together");
    const int64_t nvec = rows * (C / 4);
    KOAF_LAUNCH_ACT16(act16, bn_add_relu_kernel<A16>, dim3(ew_grid(nvec)), dim3(EB), 0, STREAM, c, sc, sh, idt, idsc, idsh, y,
                      nvec, C / 4, koaf_status_ptr());
    return koaf_check_launch("koaf_bn_add_relu");
}
extern "C" int koaf_bn_relu(const float* c, const float* sc, const float* sh, float* y, int64_t rows, int32_t C,
                            int32_t act16, void* stream) {
    return koaf_bn_add_relu(c, sc, sh, nullptr, nullptr, nullptr, y, rows, C, act16, stream);
}

namespace {
// BN backward pass 1: masked gradient + column partials of dz and dz*xhat   (H: c and ymask are bf16 activations)
// POOL: g is not a tensor of `rows` rows but the gradient of the 3x3 / stride-2 / pad-1 max-pool that follows this BatchNorm
// (+ReLU): pool_g [N][OH][OW][C] with the window positions pool_am recorded (koaf_maxpool_fwd); the gradient of input pixel
// (n, iy, ix) is gathered here -- the arithmetic of maxpool_bwd_kernel -- instead of being written by it and read back
struct PoolGeom { const float* g; const uint8_t* am; int H, W, OH, OW; };
template <bool H, bool POOL>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ c,
                                                            const float* __restrict__ ymask,
                                                            const float* __restrict__ sc, const float* __restrict__ sh,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, int mask_mode,
                                                            float* __restrict__ dz_out, int64_t rows, int C,
                                                            ColGeom geo, float* __restrict__ part, float* dz_amax, PoolGeom pg) {
    const int t = threadIdx.x, cvx = t % geo.CV, ry = t / geo.CV;
    unsigned am = 0u;       // largest |dz| as magnitude bits (a NaN / Inf wins: koaf_common.h)
    const int c0 = blockIdx.y * geo.CW + 4 * cvx;
    const int64_t rbeg = (int64_t)blockIdx.x * geo.rpb;
    const int64_t rend = min(rows, rbeg + (int64_t)geo.rpb);
    const v4f mu = *(const v4f*)&mean[c0], is = *(const v4f*)&invstd[c0];
    v4f s4 = {0, 0, 0, 0}, h4 = {0, 0, 0, 0};
    if (mask_mode == 2) { s4 = *(const v4f*)&sc[c0]; h4 = *(const v4f*)&sh[c0]; }
    v4f s[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    // POOL: (image, row, column) of this thread's pixel, carried from pass to pass (three 64-bit divisions per pixel cost more
    // than the gather itself)
    int ix = 0, iy = 0, n = 0;
    if constexpr (POOL) {
        int64_t pp = rbeg + ry;
        ix = (int)(pp % pg.W);
        pp /= pg.W;
        iy = (int)(pp % pg.H);
        n = (int)(pp / pg.H);
    }
    for (int64_t r = rbeg + ry; r < rend; r += geo.RP) {
        const int64_t o = r * C + c0;
        v4f gv;
        if constexpr (POOL) {
            gv = (v4f){0.f, 0.f, 0.f, 0.f};
            // output windows covering (iy, ix): oy in {iy / 2, (iy + 1) / 2} (one window row when iy is even), likewise ox.  All four
            // candidates are fetched at once from clamped addresses and masked (a loop with early exits kept one pair of loads in
            // flight per lane: 2.9 TB/s)
            const int oya = iy >> 1, oyb = (iy + 1) >> 1, oxa = ix >> 1, oxb = (ix + 1) >> 1;
            const bool vy[2] = {oya < pg.OH, oyb != oya && oyb < pg.OH}, vx[2] = {oxa < pg.OW, oxb != oxa && oxb < pg.OW};
            const int oys[2] = {oya, oyb}, oxs[2] = {oxa, oxb};
            uint32_t a4[4];
            v4f gg[4];
#pragma unroll
            for (int wy = 0; wy < 2; ++wy)
#pragma unroll
                for (int wx = 0; wx < 2; ++wx) {
                    const bool ok = vy[wy] && vx[wx];
                    const int64_t po = ok ? ((int64_t)(n * pg.OH + oys[wy]) * pg.OW + oxs[wx]) * C + c0 : (int64_t)c0;
                    a4[2 * wy + wx] = *(const uint32_t*)&pg.am[po];
                    gg[2 * wy + wx] = *(const v4f*)&pg.g[po];
                }
#pragma unroll
            for (int wy = 0; wy < 2; ++wy)
#pragma unroll
                for (int wx = 0; wx < 2; ++wx) {
                    const bool ok = vy[wy] && vx[wx];
                    const uint32_t want = (uint32_t)((iy - (oys[wy] * 2 - 1)) * 3 + (ix - (oxs[wx] * 2 - 1)));
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ok && ((a4[2 * wy + wx] >> (8 * j)) & 0xffu) == want) gv[j] += gg[2 * wy + wx][j];
                }
            ix += geo.RP;
            while (ix >= pg.W) { ix -= pg.W; if (++iy == pg.H) { iy = 0; ++n; } }
        } else {
            gv = *(const v4f*)&g[o];
        }
        v4f cvv = load4<H>(c, o);
        if (mask_mode == 1) {
            v4f yv = load4<H>(ymask, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
        } else if (mask_mode == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = (cvv[j] * s4[j] + h4[j]) > 0.f ? gv[j] : 0.f;
        }
        if (dz_out) *(v4f*)&dz_out[o] = gv;
        s[0] += gv;
        s[1] += gv * ((cvv - mu) * is);
#pragma unroll
        for (int j = 0; j < 4; ++j) am = max(am, koaf_absbits(gv[j]));
    }
    col_block_reduce<2>(s, part, blockIdx.x, C, blockIdx.y * geo.CW, geo.CV, geo.RP);
    if (dz_amax) block_amax_raise_bits(am, dz_amax);
}
}  // namespace

extern "C" int koaf_bn_bwd_reduce(const float* g, const float* c, const float* ymask, const float* sc, const float* sh,
                                  const float* mean, const float* invstd, int32_t mask_mode, float* dz_out, float* part,
                                  int32_t* part_rows, int64_t rows, int32_t C, float* dz_amax, int32_t act16, void* stream) {
    ColGeom geo;
    KOAF_REQUIRE(g && c && mean && invstd && part && part_rows && rows > 0, "koaf_bn_bwd_reduce: bad args");
    KOAF_REQUIRE(mask_mode != 1 || ymask, "koaf_bn_bwd_reduce: mask_mode 1 needs ymask");
    KOAF_REQUIRE(mask_mode != 2 || (sc && sh), "koaf_bn_bwd_reduce: mask_mode 2 needs sc/sh");
    KOAF_REQUIRE(col_geom(rows, C, 1024, &geo), "koaf_bn_bwd_reduce: unsupported C=%d", C);
    if (dz_amax && hipMemsetAsync(dz_amax, 0, sizeof(float), STREAM) != hipSuccess) {
        koaf_set_error("koaf_bn_bwd_reduce: memset failed");
        return KOAF_ELAUNCH;
    }
    const PoolGeom nopool{nullptr, nullptr, 0, 0, 0, 0};
    KOAF_LAUNCH_ACT16(act16, (bn_bwd_reduce_kernel<A16, false>), dim3(geo.nblk, geo.nchunk), dim3(256), 0, STREAM, g, c, ymask,
                      sc, sh, mean, invstd, mask_mode, dz_out, rows, C, geo, part, dz_amax, nopool);
    *part_rows = geo.nblk;
    return koaf_check_launch("koaf_bn_bwd_reduce");
}

extern "C" int koaf_bn_bwd_reduce_pool(const float* pool_g, const uint8_t* pool_argmax, const float* c, const float* sc,
                                       const float* sh, const float* mean, const float* invstd, float* dz_out, float* part,
                                       int32_t* part_rows, int32_t N, int32_t H, int32_t W, int32_t C, float* dz_amax,
                                       int32_t act16, void* stream) {
    ColGeom geo;
    KOAF_REQUIRE(pool_g && pool_argmax && c && sc && sh && mean && invstd && dz_out && part && part_rows && N > 0 && H > 0 && W > 0,
                 "koaf_bn_bwd_reduce_pool: bad args");
    const int64_t rows = (int64_t)N * H * W;
    KOAF_REQUIRE(col_geom(rows, C, 1024, &geo), "koaf_bn_bwd_reduce_pool: unsupported C=%d", C);
    if (dz_amax && hipMemsetAsync(dz_amax, 0, sizeof(float), STREAM) != hipSuccess) {
        koaf_set_error("koaf_bn_bwd_reduce_pool: memset failed");
        return KOAF_ELAUNCH;
    }
    const PoolGeom pg{pool_g, pool_argmax, H, W, (H + 2 - 3) / 2 + 1, (W + 2 - 3) / 2 + 1};
    KOAF_LAUNCH_ACT16(act16, (bn_bwd_reduce_kernel<A16, true>), dim3(geo.nblk, geo.nchunk), dim3(256), 0, STREAM, nullptr, c,
                      nullptr, sc, sh, mean, invstd, 2, dz_out, rows, C, geo, part, dz_amax, pg);
    *part_rows = geo.nblk;
    return koaf_check_launch("koaf_bn_bwd_reduce_pool");
}

namespace {
template <typename T>
__global__ void __launch_bounds__(1024) bn_bwd_finalize_kernel(const T* __restrict__ part, int rows, int C,
                                                               double inv_count, const float* __restrict__ sc,
                                                               const float* __restrict__ invstd, float* dgamma,
                                                               float* dbeta, float* coef, int nsum, int i1,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ dz_amax, double sqrt_nm1,
                                                               float* amax) {
    __shared__ double red[2][16][64];
    float bound = 0.f;
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    double a = 0.0, b = 0.0;
    if (c < C)
        for (int r = gy; r < rows; r += 16) {
            a += (double)part[((int64_t)r * nsum + 0) * C + c];
            b += (double)part[((int64_t)r * nsum + i1) * C + c];
        }
    red[0][gy][cx] = a;
    red[1][gy][cx] = b;
    __syncthreads();
    if (gy == 0 && c < C) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < 16; ++j) { s1 += red[0][j][cx]; s2 += red[1][j][cx]; }
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
        const float k0 = sc[c], k1 = (float)(s1 * inv_count), k2 = (float)((double)sc[c] * (double)invstd[c] * s2 * inv_count);
        coef[c] = k0;
        coef[C + c] = k1;
        coef[2 * C + c] = k2;
        if (mean) {
            // dc = k0 * (dz - k1) - k2 * (x - mean) = k0 * dz + k3 - k2 * x: the form the GEMM loaders evaluate (KoafOperand.tf 2)
            coef[3 * C + c] = k2 * mean[c] - k0 * k1;
            // |dc| <= |k0| (max|dz| + |k1|) + |k2| max|x - mean|, and no sample of n lies further than sqrt(n - 1) standard
            // deviations from its mean (Samuelson): a guaranteed bound of the tensor's largest magnitude without a pass
            if (amax) bound = fabsf(k0) * ((dz_amax ? *dz_amax : 0.f) + fabsf(k1)) + fabsf(k2) * (float)(sqrt_nm1 / (double)invstd[c]);
        }
    }
    if (amax && mean) block_amax_raise(bound, amax);
}

// eval-mode BatchNorm (y = sc*c + sh with constant coefficients): dc = sc*dz, so coef = {sc, 0, 0[, 0]}; dgamma / dbeta are
// the sums the train-mode kernel above forms, added in the same order
template <typename T>
__global__ void __launch_bounds__(1024) bn_bwd_finalize_eval_kernel(const T* __restrict__ part, int rows, int C,
                                                                    const float* __restrict__ sc, float* dgamma, float* dbeta,
                                                                    float* coef, int coef_rows, int nsum, int i1,
                                                                    const float* __restrict__ dz_amax, float* amax) {
    __shared__ double red[2][16][64];
    float bound = 0.f;
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    double a = 0.0, b = 0.0;
    if (part && c < C)
        for (int r = gy; r < rows; r += 16) {
            a += (double)part[((int64_t)r * nsum + 0) * C + c];
            b += (double)part[((int64_t)r * nsum + i1) * C + c];
        }
    red[0][gy][cx] = a;
    red[1][gy][cx] = b;
    __syncthreads();
    if (gy == 0 && c < C) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < 16; ++j) { s1 += red[0][j][cx]; s2 += red[1][j][cx]; }
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
        coef[c] = sc[c];
        for (int k = 1; k < coef_rows; ++k) coef[k * C + c] = 0.f;
        if (amax) bound = fabsf(sc[c]) * (dz_amax ? *dz_amax : 0.f);
    }
    if (amax) block_amax_raise(bound, amax);
}
}  // namespace

extern "C" int koaf_bn_bwd_finalize(const float* part, int32_t part_rows, int32_t C, int64_t count, const float* sc,
                                    const float* invstd, float* dgamma, float* dbeta, float* coef, int32_t nsum,
                                    int32_t i1, double* ws, const float* mean, const float* dz_amax, float* amax,
                                    void* stream) {
    KOAF_REQUIRE(part && part_rows > 0 && C > 0 && count > 0 && sc && invstd && coef, "koaf_bn_bwd_finalize: bad args");
    KOAF_REQUIRE(nsum >= 2 && i1 >= 1 && i1 < nsum, "koaf_bn_bwd_finalize: bad (nsum, i1)");
    KOAF_REQUIRE(!amax || mean, "koaf_bn_bwd_finalize: amax needs mean (coef gets its fourth row)");
    if (amax && hipMemsetAsync(amax, 0, sizeof(float), STREAM) != hipSuccess) {
        koaf_set_error("koaf_bn_bwd_finalize: memset failed");
        return KOAF_ELAUNCH;
    }
    const double sq = sqrt((double)(count > 1 ? count - 1 : 1));
    const int S = part_reduce(part, part_rows, C, nsum, i1, ws, STREAM);
    if (S)
        hipLaunchKernelGGL(bn_bwd_finalize_kernel<double>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, ws, S, C,
                           1.0 / (double)count, sc, invstd, dgamma, dbeta, coef, 2, 1, mean, dz_amax, sq, amax);
    else
        hipLaunchKernelGGL(bn_bwd_finalize_kernel<float>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, part, part_rows, C,
                           1.0 / (double)count, sc, invstd, dgamma, dbeta, coef, nsum, i1, mean, dz_amax, sq, amax);
    return koaf_check_launch("koaf_bn_bwd_finalize");
}
extern "C" int koaf_bn_bwd_finalize_eval(const float* part, int32_t part_rows, int32_t C, const float* sc, float* dgamma,
                                         float* dbeta, float* coef, int32_t coef_rows, int32_t nsum, int32_t i1, double* ws,
                                         const float* dz_amax, float* amax, void* stream) {
    KOAF_REQUIRE(C > 0 && sc && coef && (coef_rows == 3 || coef_rows == 4), "koaf_bn_bwd_finalize_eval: bad args");
    KOAF_REQUIRE(part ? part_rows > 0 : (!dgamma && !dbeta), "koaf_bn_bwd_finalize_eval: dgamma / dbeta need the partial sums");
    KOAF_REQUIRE(!part || (nsum >= 2 && i1 >= 1 && i1 < nsum), "koaf_bn_bwd_finalize_eval: bad (nsum, i1)");
    KOAF_REQUIRE(!amax || coef_rows == 4, "koaf_bn_bwd_finalize_eval: amax belongs to the four-row form");
    if (amax && hipMemsetAsync(amax, 0, sizeof(float), STREAM) != hipSuccess) {
        koaf_set_error("koaf_bn_bwd_finalize_eval: memset failed");
        return KOAF_ELAUNCH;
    }
    const int S = part ? part_reduce(part, part_rows, C, nsum, i1, ws, STREAM) : 0;
    if (S)
        hipLaunchKernelGGL(bn_bwd_finalize_eval_kernel<double>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, ws, S, C, sc, dgamma,
                           dbeta, coef, coef_rows, 2, 1, dz_amax, amax);
    else
        hipLaunchKernelGGL(bn_bwd_finalize_eval_kernel<float>, dim3((C + 63) / 64), dim3(1024), 0, STREAM, part, part_rows, C, sc,
                           dgamma, dbeta, coef, coef_rows, nsum, i1, dz_amax, amax);
    return koaf_check_launch("koaf_bn_bwd_finalize_eval");
}

namespace {
template <bool H>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ dz, const float* __restrict__ c,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ coef, float* __restrict__ dc,
                                                           int64_t nvec, int C, float* __restrict__ amax) {
    const int C4 = C / 4;
    unsigned m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        v4f z = *(const v4f*)&dz[i * 4];
        v4f x = load4<H>(c, i * 4);
        v4f k0 = *(const v4f*)&coef[cv], k1 = *(const v4f*)&coef[C + cv], k2 = *(const v4f*)&coef[2 * C + cv];
        v4f mu = *(const v4f*)&mean[cv];
        const v4f o = k0 * (z - k1) - k2 * (x - mu);
        *(v4f*)&dc[i * 4] = o;
#pragma unroll
        for (int j = 0; j < 4; ++j) m = max(m, koaf_absbits(o[j]));
    }
    // max |dc| of the tensor: the scale of dc as an operand of the fp16 contraction scheme
    if (amax) block_amax_raise_bits(m, amax);
}
}  // namespace

extern "C" int koaf_bn_bwd_apply(const float* dz, const float* c, const float* mean, const float* coef, float* dc,
                                 int64_t rows, int32_t C, float* amax, int32_t act16, void* stream) {
    KOAF_REQUIRE(dz && c && mean && coef && dc && rows > 0 && C % 4 == 0, "koaf_bn_bwd_apply: bad args");
    const int64_t nvec = rows * (C / 4);
    KOAF_LAUNCH_ACT16(act16, bn_bwd_apply_kernel<A16>, dim3(ew_grid(nvec)), dim3(EB), 0, STREAM, dz, c, mean, coef, dc, nvec, C,
                      amax);
    return koaf_check_launch("koaf_bn_bwd_apply");
}

namespace {
// ------------------------------------------------------------------------------------------------
// max-pool 3x3 s2 p1 over relu(sc*c+sh); GAP
// ------------------------------------------------------------------------------------------------
template <bool B16>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const float* __restrict__ c, const float* __restrict__ sc,
                                                          const float* __restrict__ sh, float* __restrict__ y,
                                                          uint8_t* __restrict__ am, int N, int H, int W, int C,
                                                          int OH, int OW, uint32_t* status) {
    const int C4 = C / 4;
    unsigned nsat = 0;
    const int64_t total = (int64_t)N * OH * OW * C4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        int64_t p = i / C4;
        const int ox = (int)(p % OW);
        p /= OW;
        const int oy = (int)(p % OH);
        const int n = (int)(p / OH);
        const v4f s4 = *(const v4f*)&sc[cv], h4 = *(const v4f*)&sh[cv];
        v4f best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int iy = oy * 2 - 1 + kh;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ix = ox * 2 - 1 + kw;
                if ((unsigned)ix >= (unsigned)W) continue;
                v4f v = load4<B16>(c, ((int64_t)(n * H + iy) * W + ix) * C + cv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // (a NaN stays a NaN, as in bn_add_relu_kernel -- fmaxf alone would return the 0 -- and takes the window, as in
                    // F.max_pool2d: it is counted below and reaches the consumers instead of turning into a healthy zero)
                    const float z = v[j] * s4[j] + h4[j];
                    const float a = z != z ? z : fmaxf(z, 0.f);
                    if (a > best[j] || a != a) { best[j] = a; bi[j] = kh * 3 + kw; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) nsat += !(best[j] * KOAF_ACT_SCALE <= 65504.f) ? 1u : 0u;    // (as in bn_add_relu_kernel)
        store4<B16>(y, i * 4, best);
        *(uint32_t*)&am[i * 4] = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    }
    koaf_status_add(status, 0, nsat);
}

__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ am,
                                                          float* __restrict__ da, int N, int H, int W, int C, int OH,
                                                          int OW) {
    const int C4 = C / 4;
    const int64_t total = (int64_t)N * H * W * C4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        int64_t p = i / C4;
        const int ix = (int)(p % W);
        p /= W;
        const int iy = (int)(p % H);
        const int n = (int)(p / H);
        v4f acc = {0, 0, 0, 0};
        // output windows covering (iy, ix): oy*2-1 <= iy <= oy*2+1
        for (int oy = (iy) / 2; oy <= (iy + 1) / 2; ++oy) {
            if (oy >= OH) continue;
            const int kh = iy - (oy * 2 - 1);
            if (kh < 0 || kh > 2) continue;
            for (int ox = (ix) / 2; ox <= (ix + 1) / 2; ++ox) {
                if (ox >= OW) continue;
                const int kw = ix - (ox * 2 - 1);
                if (kw < 0 || kw > 2) continue;
                const int64_t o = ((int64_t)(n * OH + oy) * OW + ox) * C + cv;
                const uint32_t a4 = *(const uint32_t*)&am[o];
                const v4f g = *(const v4f*)&dy[o];
                const uint32_t want = (uint32_t)(kh * 3 + kw);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (((a4 >> (8 * j)) & 0xffu) == want) acc[j] += g[j];
            }
        }
        *(v4f*)&da[i * 4] = acc;
    }
}
}  // namespace

extern "C" int koaf_maxpool_fwd(const float* c, const float* sc, const float* sh, float* y, uint8_t* argmax, int32_t N,
                                int32_t H, int32_t W, int32_t C, int32_t act16, void* stream) {
    KOAF_REQUIRE(c && sc && sh && y && argmax && N > 0 && H > 0 && W > 0 && C % 4 == 0, "koaf_maxpool_fwd: bad args");
    const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
    const int64_t nvec = (int64_t)N * OH * OW * (C / 4);
    KOAF_LAUNCH_ACT16(act16, maxpool_fwd_kernel<A16>, dim3(ew_grid(nvec)), dim3(EB), 0, STREAM, c, sc, sh, y, argmax, N, H, W, C,
                      OH, OW, koaf_status_ptr());
    return koaf_check_launch("koaf_maxpool_fwd");
}
extern "C" int koaf_maxpool_bwd(const float* dy, const uint8_t* argmax, float* da, int32_t N, int32_t H, int32_t W,
                                int32_t C, void* stream) {
    KOAF_REQUIRE(dy && argmax && da && N > 0 && C % 4 == 0, "koaf_maxpool_bwd: bad args");
    const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
    const int64_t nvec = (int64_t)N * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_grid(nvec)), dim3(EB), 0, STREAM, dy, argmax, da, N, H, W, C, OH,
                       OW);
    return koaf_check_launch("koaf_maxpool_bwd");
}

namespace {
template <bool H>
__global__ void __launch_bounds__(256) gap_fwd_kernel(const float* __restrict__ y, float* __restrict__ out, int N,
                                                      int HW, int C) {
    const int C4 = C / 4;
    const int64_t total = (int64_t)N * C4;
    const float inv = 1.f / (float)HW;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        const int64_t n = i / C4;
        v4f a = {0, 0, 0, 0};
        for (int p = 0; p < HW; ++p) a += load4<H>(y, (n * HW + p) * C + cv);
        *(v4f*)&out[n * C + cv] = a * inv;
    }
}
__global__ void __launch_bounds__(256) gap_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dy, int N,
                                                      int HW, int C) {
    const int C4 = C / 4;
    const int64_t total = (int64_t)N * HW * C4;
    const float inv = 1.f / (float)HW;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        const int cv = (int)(i % C4) * 4;
        const int64_t n = i / ((int64_t)C4 * HW);
        *(v4f*)&dy[i * 4] = *(const v4f*)&dout[n * C + cv] * inv;
    }
}
}  // namespace

extern "C" int koaf_gap_fwd(const float* y, float* out, int32_t N, int32_t HW, int32_t C, int32_t act16, void* stream) {
    KOAF_REQUIRE(y && out && N > 0 && HW > 0 && C % 4 == 0, "koaf_gap_fwd: bad args");
    KOAF_LAUNCH_ACT16(act16, gap_fwd_kernel<A16>, dim3(ew_grid((int64_t)N * C / 4)), dim3(EB), 0, STREAM, y, out, N, HW, C);
    return koaf_check_launch("koaf_gap_fwd");
}
extern "C" int koaf_gap_bwd(const float* dout, float* dy, int32_t N, int32_t HW, int32_t C, void* stream) {
    KOAF_REQUIRE(dout && dy && N > 0 && HW > 0 && C % 4 == 0, "koaf_gap_bwd: bad args");
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(ew_grid((int64_t)N * HW * C / 4)), dim3(EB), 0, STREAM, dout, dy, N, HW,
                       C);
    return koaf_check_launch("koaf_gap_bwd");
}
