// koaf_mriprep.hip -- from raw MRI series to the model's input volumes (run/prepare_data_mri_oai.py): the weighted log-linear T2 fit of
// a multi-echo series (datasets/_mr_t2_mapping.py fit_t2_map) and the bit shift / percentile clip / narrowing / margin crop of
// preproc_compress_series.  Everything is per voxel and streams whole volumes once; the fp64 arithmetic restates the reference's
// source text operation by operation.
#include "koaf_common.h"

// No fused multiply-add and no reassociation anywhere in this file: the fit is compared against the IEEE evaluation of the
// reference, its rounding and the quantile interpolation bit for bit.  (HIP's __dmul_rn and friends are plain operators that the
// compiler may still contract; this pragma is what keeps every product and sum a separately rounded operation.)
#pragma clang fp contract(off)

namespace {
constexpr int MP_RUN = 64;      // voxels of one wave: 64 consecutive columns of one row of one slice, 64 * E contiguous elements
constexpr int MP_TS1 = 32;      // slices per block of the slice-fastest layout (its transpose tile is [64][MP_TS1 + 1])

// the reference's np.round(x, d): rint(x * 10^d) / 10^d, two separately rounded operations
__device__ __forceinline__ double round_decimals(double v, double scale) {
    return scale > 0.0 ? rint(v * scale) / scale : v;
}

// fit_exp_linear + the branches of fit_t2_map for one voxel whose E echoes lie at ys[0..E)
template <typename T>
__device__ __forceinline__ double t2_voxel(const T* ys, const double* __restrict__ xs, int E, double nan_to, double val_low,
                                           double val_high) {
    double S_x2_y = 0.0, S_y_lny = 0.0, S_x_y = 0.0, S_x_y_lny = 0.0, S_y = 0.0;
    for (int e = 0; e < E; ++e) {
        const double x = xs[e], y = (double)ys[e];
        const double ly = log(y);
        S_x2_y += x * x * y;
        S_y_lny += y * ly;
        S_x_y += x * y;
        S_x_y_lny += x * y * ly;
        S_y += y;
    }
    const double denom = S_y * S_x2_y - S_x_y * S_x_y;
    if (denom == 0.0) return 0.0;
    const double a = (S_x2_y * S_y_lny - S_x_y * S_x_y_lny) / denom;      // exp(a) is NaN exactly when a is
    const double b = (S_y * S_x_y_lny - S_x_y * S_y_lny) / denom;
    if (a != a || b != b) return 0.0;
    const double t = -1.0 / b;
    if (t != t) return nan_to;
    if (t < val_low || t > val_high) return 0.0;
    return t;
}

struct T2Geom {
    int S, R, C, E, margin, RO, CO, runs;      // RO = R - 2 margin, CO = C - 2 margin, runs = ceil(CO / 64)
    double nan_to, val_low, val_high, scale;   // scale = 10^decimals, or 0: no rounding
};

// One wave per (slice, row, run of 64 columns): its input is one contiguous byte range.  The range is read in 16-byte pieces at
// 16-byte aligned addresses (whatever the alignment of the voxel size or of the base pointer), element by element only in the at
// most two pieces that straddle its ends, and laid into LDS at the same offsets; every lane then reads its own E echoes there.
// Block = 4 waves = 4 slices of one run per pass.  LAYOUT 0 stores out[s][r][c] straight from the lanes (64 consecutive fp64);
// LAYOUT 1 collects MP_TS1 slices of the run in a transpose tile and stores out[r][c][s] with the slice index along the lanes.
template <typename T, int LAYOUT>
__global__ void __launch_bounds__(256) t2_fit_kernel(const T* __restrict__ vol, const double* __restrict__ tes,
                                                     double* __restrict__ out, T2Geom g, int stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_lds[];
    constexpr int TS = LAYOUT == 1 ? MP_TS1 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ro = blockIdx.x / g.runs, c0 = (blockIdx.x % g.runs) * MP_RUN;
    const int nv = min(MP_RUN, g.CO - c0);                    // voxels of this run
    const int s0 = blockIdx.y * TS;
    unsigned char* stage = mp_lds + (size_t)wave * stage_bytes;
    double* tile = (double*)(mp_lds + (size_t)4 * stage_bytes);       // [64][MP_TS1 + 1], LAYOUT 1 only
    const int bytes = nv * g.E * (int)sizeof(T);
    for (int j = 0; j < TS / 4; ++j) {
        const int s = s0 + 4 * j + wave;
        if (j > 0) __syncthreads();                           // the previous pass has read its stage
        int head = 0;
        if (s < g.S) {
            const unsigned char* b0 = (const unsigned char*)(vol + (((int64_t)s * g.R + ro + g.margin) * g.C + c0 + g.margin) * g.E);
            head = (int)((uintptr_t)b0 & 15);
            const unsigned char* a0 = b0 - head;
            const int npieces = (head + bytes + 15) >> 4;
            for (int k = lane; k < npieces; k += 64) {
                const int lo = 16 * k - head;                 // byte offset of the piece within the range
                if (lo >= 0 && lo + 16 <= bytes) {
                    *(v4i*)(stage + 16 * k) = __builtin_nontemporal_load((const v4i*)(a0 + 16 * k));
                } else {
#pragma unroll
                    for (int q = 0; q < 16 / (int)sizeof(T); ++q) {
                        const int o = lo + q * (int)sizeof(T);
                        if (o >= 0 && o < bytes) *(T*)(stage + 16 * k + q * sizeof(T)) = *(const T*)(a0 + 16 * k + q * sizeof(T));
                    }
                }
            }
        }
        __syncthreads();
        if (s < g.S && lane < nv) {
            const T* ys = (const T*)(stage + head) + lane * g.E;
            const double t = round_decimals(t2_voxel(ys, tes + (int64_t)s * g.E, g.E, g.nan_to, g.val_low, g.val_high), g.scale);
            if constexpr (LAYOUT == 0) out[((int64_t)s * g.RO + ro) * g.CO + c0 + lane] = t;
            else tile[lane * (MP_TS1 + 1) + 4 * j + wave] = t;
        }
    }
    if constexpr (LAYOUT == 1) {
        __syncthreads();
        const int ns = min(MP_TS1, g.S - s0);
        double* ob = out + ((int64_t)ro * g.CO + c0) * g.S + s0;
        for (int i = threadIdx.x; i < nv * ns; i += 256) {
            const int p = i / ns, sl = i - p * ns;
            ob[(int64_t)p * g.S + sl] = tile[p * (MP_TS1 + 1) + sl];
        }
    }
}

template <typename T>
int t2_fit_launch(const void* vol, const double* tes, double* out, const T2Geom& g, int layout, hipStream_t st) {
    const int stage_bytes = (MP_RUN * g.E * (int)sizeof(T) + 16 + 15) & ~15;
    const dim3 grid((unsigned)(g.RO * g.runs), (unsigned)((g.S + (layout ? MP_TS1 : 4) - 1) / (layout ? MP_TS1 : 4)));
    if (layout == 0)
        hipLaunchKernelGGL((t2_fit_kernel<T, 0>), grid, dim3(256), 4 * stage_bytes, st, (const T*)vol, tes, out, g, stage_bytes);
    else
        hipLaunchKernelGGL((t2_fit_kernel<T, 1>), grid, dim3(256), 4 * stage_bytes + MP_RUN * (MP_TS1 + 1) * (int)sizeof(double), st,
                           (const T*)vol, tes, out, g, stage_bytes);
    return koaf_check_launch("koaf_t2_fit");
}

inline int dtype_size(int dtype) { return dtype == 2 || dtype == 3 ? 2 : dtype == 4 ? 4 : dtype == 5 ? 8 : 0; }
}  // namespace

extern "C" int koaf_t2_fit(const void* vol, int32_t dtype, const double* tes, int32_t S, int32_t R, int32_t C, int32_t E, double nan_to,
                           double val_low, double val_high, int32_t decimals, int32_t margin, int32_t layout, double* out,
                           void* stream) {
    KOAF_REQUIRE(vol && tes && out, "koaf_t2_fit: null pointer");
    KOAF_REQUIRE(dtype >= 2 && dtype <= 5, "koaf_t2_fit: dtype 2 = uint16, 3 = int16, 4 = float32, 5 = float64");
    KOAF_REQUIRE(E >= 2 && E <= 16, "koaf_t2_fit: 2..16 echoes (with one echo the reference's own answer is rounding noise), got %d", E);
    KOAF_REQUIRE(S > 0 && R > 0 && C > 0 && margin >= 0 && 2 * margin < R && 2 * margin < C,
                 "koaf_t2_fit: bad shape [%d][%d][%d] with margin %d", S, R, C, margin);
    KOAF_REQUIRE(layout == 0 || layout == 1, "koaf_t2_fit: layout 0 = [S][R][C], 1 = [R][C][S]");
    KOAF_REQUIRE(decimals <= 22, "koaf_t2_fit: 10^decimals is exact in fp64 up to 22 decimals");
    KOAF_REQUIRE(((uintptr_t)vol) % dtype_size(dtype) == 0 && (((uintptr_t)tes) & 7) == 0 && (((uintptr_t)out) & 7) == 0,
                 "koaf_t2_fit: a pointer is not aligned to its element size");
    T2Geom g;
    g.S = S, g.R = R, g.C = C, g.E = E, g.margin = margin, g.RO = R - 2 * margin, g.CO = C - 2 * margin;
    g.runs = (g.CO + MP_RUN - 1) / MP_RUN;
    g.nan_to = nan_to, g.val_low = val_low, g.val_high = val_high, g.scale = 0.0;
    if (decimals >= 0) {
        g.scale = 1.0;
        for (int i = 0; i < decimals; ++i) g.scale *= 10.0;       // exact
    }
    KOAF_REQUIRE((int64_t)g.RO * g.runs < (1ll << 31) && (S + 3) / 4 <= 65535, "koaf_t2_fit: volume too large for one launch");
    switch (dtype) {
        case 2: return t2_fit_launch<uint16_t>(vol, tes, out, g, layout, STREAM);
        case 3: return t2_fit_launch<int16_t>(vol, tes, out, g, layout, STREAM);
        case 4: return t2_fit_launch<float>(vol, tes, out, g, layout, STREAM);
        default: return t2_fit_launch<double>(vol, tes, out, g, layout, STREAM);
    }
}

namespace {
// ------------------------------------------------------------------------------------------------
// preproc_compress_series: histogram of v >> shift, order statistics from the histogram, clip + narrow + crop
// ------------------------------------------------------------------------------------------------
// the uint16 a stored value becomes under astype(np.uint16): integers reinterpreted, floats truncated toward zero.  -> false
// (and a raised bit: 1 = NaN / Inf, 2 = outside [0, 65535]) for a float that has no such value
template <typename T>
__device__ __forceinline__ bool as_u16(T v, unsigned& u, unsigned& bad) {
    if constexpr (sizeof(T) == 2) {
        u = (unsigned)(uint16_t)v;
        return true;
    } else {
        const double d = (double)v;
        if (!(fabs(d) <= 1.7976931348623157e308)) { bad |= 1u; return false; }
        const double t = trunc(d);
        if (t < 0.0 || t > 65535.0) { bad |= 2u; return false; }
        u = (unsigned)t;
        return true;
    }
}

// Counts per block in LDS (integer atomics), added to the global bins with one integer atomic per non-empty bin: integer sums
// do not depend on their order.  16-byte loads from the first 16-byte aligned element on; the elements before it and behind
// the last whole vector go one by one.
template <typename T>
__global__ void __launch_bounds__(256) series_hist_kernel(const T* __restrict__ x, int64_t n, int shift, int nbins,
                                                          int32_t* __restrict__ bins, uint32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_lds[];
    int* cnt = (int*)mp_lds;
    constexpr int V = 16 / (int)sizeof(T);
    for (int i = threadIdx.x; i < nbins; i += 256) cnt[i] = 0;
    __syncthreads();
    unsigned bad = 0u, u;
    int64_t head = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    const int64_t nvec = (n - head) / V;
    const v4i* xv = (const v4i*)(x + head);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const v4i raw = __builtin_nontemporal_load(xv + i);
        T v[V];
        __builtin_memcpy(v, &raw, 16);
        int bin = -1, run = 0;                 // neighbours along the fastest axis mostly share a bin: one atomic per run of equal bins
#pragma unroll
        for (int q = 0; q < V; ++q) {
            if (!as_u16(v[q], u, bad)) continue;
            const int b = (int)(u >> shift);
            if (b != bin) {
                if (run != 0) atomicAdd(&cnt[bin], run);
                bin = b, run = 0;
            }
            ++run;
        }
        if (run != 0) atomicAdd(&cnt[bin], run);
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + nvec * V;
        for (int64_t i = threadIdx.x; i < head + (n - tail0); i += 256) {
            const int64_t k = i < head ? i : tail0 + (i - head);
            if (as_u16(x[k], u, bad)) atomicAdd(&cnt[u >> shift], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += 256) {
        const int c = cnt[i];
        if (c != 0) atomicAdd(&bins[i], c);
    }
    if (bad != 0u) atomicOr(flag, bad);
}

struct QuantArgs { int K; int64_t k[8]; double gamma[8]; };

// One block.  Thread t owns the contiguous bins [t * per, (t + 1) * per); a fixed scan over the 256 thread sums gives each thread
// the number of elements below its first bin, and the thread whose run holds order statistic q walks to its bin.  An index at or
// beyond the number of counted elements gives the largest counted value.
__global__ void __launch_bounds__(256) series_quantiles_kernel(const int32_t* __restrict__ bins, int nbins, int64_t n, QuantArgs qa,
                                                               double* __restrict__ out) {
    __shared__ int64_t cum[257];
    __shared__ int val[16];
    const int per = nbins / 256, b0 = threadIdx.x * per;
    int64_t mine = 0;
    for (int i = 0; i < per; ++i) mine += bins[b0 + i];
    cum[threadIdx.x + 1] = mine;
    if (threadIdx.x < 16) val[threadIdx.x] = -1;
    __syncthreads();
    if (threadIdx.x == 0) {
        cum[0] = 0;
        for (int i = 1; i <= 256; ++i) cum[i] += cum[i - 1];
    }
    __syncthreads();
    const int64_t below = cum[threadIdx.x], total = cum[256];
    for (int j = 0; j < 2 * qa.K; ++j) {
        int64_t q = qa.k[j >> 1] + (j & 1);
        if (q > n - 1) q = n - 1;
        if (q > total - 1) q = total - 1;
        if (q < 0) q = 0;
        if (q >= below && q < below + mine) {
            int64_t c = below;
            for (int i = 0; i < per; ++i) {
                c += bins[b0 + i];
                if (q < c) { val[j] = b0 + i; break; }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < qa.K) {
        // numpy's _lerp: a + (b - a) * gamma, and b - (b - a) * (1 - gamma) where gamma >= 0.5
        const double a = (double)val[2 * threadIdx.x], b = (double)val[2 * threadIdx.x + 1], gm = qa.gamma[threadIdx.x];
        const double d = b - a;
        double r = a + d * gm;
        if (gm >= 0.5) r = b - d * (1.0 - gm);
        out[threadIdx.x] = total > 0 ? r : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// out[r - m][c - m][s] = narrow(min(max(v >> shift, lo), hi)); V consecutive slices per thread (V = 8 where the rows allow it)
template <typename T, typename O, int V>
__global__ void __launch_bounds__(256) series_pack_kernel(const T* __restrict__ x, O* __restrict__ out, const double* __restrict__ lim,
                                                          int C, int S, int m, int shift, int64_t rowv, int64_t total) {
    const double lo = lim[0], hi = lim[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ro = i / rowv, rem = (i - ro * rowv) * V;          // rowv = (C - 2m) * S / V work items per output row
        const int64_t src = ((ro + m) * C + m) * S + rem, dst = ro * rowv * V + rem;
        T v[V];
        O o[V];
        __builtin_memcpy(v, x + src, sizeof(v));
#pragma unroll
        for (int q = 0; q < V; ++q) {
            unsigned u = 0u, bad = 0u;
            as_u16(v[q], u, bad);                                     // (a float without a uint16 value counts as 0: the histogram flagged it)
            const double w = fmin(fmax((double)(u >> shift), lo), hi);
            o[q] = (O)(int)w;
        }
        __builtin_memcpy(out + dst, o, sizeof(o));
    }
}

template <typename T, typename O>
void series_pack_launch(const void* x, void* out, const double* lim, int R, int C, int S, int m, int shift, hipStream_t st) {
    const int64_t row = (int64_t)(C - 2 * m) * S;
    const bool v8 = row % 8 == 0 && ((int64_t)C * S) % 8 == 0 && ((int64_t)m * S) % 8 == 0 &&
                    ((uintptr_t)x) % (8 * sizeof(T)) == 0 && ((uintptr_t)out) % (8 * sizeof(O)) == 0;
    const int64_t total = (int64_t)(R - 2 * m) * row / (v8 ? 8 : 1);
    if (v8)
        hipLaunchKernelGGL((series_pack_kernel<T, O, 8>), dim3(ew_grid(total)), dim3(EB), 0, st, (const T*)x, (O*)out, lim, C, S, m, shift,
                           row / 8, total);
    else
        hipLaunchKernelGGL((series_pack_kernel<T, O, 1>), dim3(ew_grid(total)), dim3(EB), 0, st, (const T*)x, (O*)out, lim, C, S, m, shift,
                           row, total);
}
template <typename T>
void series_pack_out(const void* x, void* out, int out16, const double* lim, int R, int C, int S, int m, int shift, hipStream_t st) {
    if (out16) series_pack_launch<T, uint16_t>(x, out, lim, R, C, S, m, shift, st);
    else series_pack_launch<T, uint8_t>(x, out, lim, R, C, S, m, shift, st);
}
}  // namespace

extern "C" int koaf_series_hist(const void* x, int32_t dtype, int64_t n, int32_t shift, int32_t* bins, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(x && bins && flag, "koaf_series_hist: null pointer");
    KOAF_REQUIRE(dtype >= 2 && dtype <= 5, "koaf_series_hist: dtype 2 = uint16, 3 = int16, 4 = float32, 5 = float64");
    KOAF_REQUIRE(shift >= 2 && shift <= 8, "koaf_series_hist: shift 2..8 (the block's bins live in LDS), got %d", shift);
    KOAF_REQUIRE(n > 0 && n < (1ll << 31), "koaf_series_hist: 0 < n < 2^31");
    KOAF_REQUIRE(((uintptr_t)x) % dtype_size(dtype) == 0, "koaf_series_hist: the volume is not aligned to its element size");
    const int nbins = 65536 >> shift;
    // few, long-lived blocks: every block zeroes and merges all of its bins, which costs more than the counting once a block's
    // share of the volume is smaller than its histogram
    unsigned grid = ew_grid(cdiv64(n, 8));
    if (grid > 256 * 4) grid = 256 * 4;
    const size_t lds = (size_t)nbins * sizeof(int);
    if (dtype == 2) hipLaunchKernelGGL(series_hist_kernel<uint16_t>, dim3(grid), dim3(256), lds, STREAM, (const uint16_t*)x, n, shift, nbins, bins, flag);
    else if (dtype == 3) hipLaunchKernelGGL(series_hist_kernel<int16_t>, dim3(grid), dim3(256), lds, STREAM, (const int16_t*)x, n, shift, nbins, bins, flag);
    else if (dtype == 4) hipLaunchKernelGGL(series_hist_kernel<float>, dim3(grid), dim3(256), lds, STREAM, (const float*)x, n, shift, nbins, bins, flag);
    else hipLaunchKernelGGL(series_hist_kernel<double>, dim3(grid), dim3(256), lds, STREAM, (const double*)x, n, shift, nbins, bins, flag);
    return koaf_check_launch("koaf_series_hist");
}

extern "C" int koaf_series_quantiles(const int32_t* bins, int32_t shift, int64_t n, const int64_t* k, const double* gamma, int32_t K,
                                     double* out, void* stream) {
    KOAF_REQUIRE(bins && k && gamma && out, "koaf_series_quantiles: null pointer");
    KOAF_REQUIRE(shift >= 2 && shift <= 8, "koaf_series_quantiles: shift 2..8, got %d", shift);
    KOAF_REQUIRE(n > 0 && n < (1ll << 31) && K >= 1 && K <= 8, "koaf_series_quantiles: 0 < n < 2^31, 1..8 quantiles");
    QuantArgs qa;
    qa.K = K;
    for (int i = 0; i < 8; ++i) {
        qa.k[i] = i < K ? k[i] : 0;
        qa.gamma[i] = i < K ? gamma[i] : 0.0;
        KOAF_REQUIRE(qa.k[i] >= 0 && qa.k[i] < n && qa.gamma[i] >= 0.0 && qa.gamma[i] < 1.0,
                     "koaf_series_quantiles: pair %d is not (0 <= k < n, 0 <= gamma < 1)", i);
    }
    hipLaunchKernelGGL(series_quantiles_kernel, dim3(1), dim3(256), 0, STREAM, bins, 65536 >> shift, n, qa, out);
    return koaf_check_launch("koaf_series_quantiles");
}

extern "C" int koaf_series_pack(const void* x, int32_t dtype, int32_t R, int32_t C, int32_t S, int32_t shift, int32_t margin,
                                const double* limits, void* out, int32_t out16, void* stream) {
    KOAF_REQUIRE(x && limits && out, "koaf_series_pack: null pointer");
    KOAF_REQUIRE(dtype >= 2 && dtype <= 5, "koaf_series_pack: dtype 2 = uint16, 3 = int16, 4 = float32, 5 = float64");
    KOAF_REQUIRE(shift >= 2 && shift <= 8, "koaf_series_pack: shift 2..8, got %d", shift);
    KOAF_REQUIRE(R > 0 && C > 0 && S > 0 && (int64_t)R * C * S < (1ll << 31), "koaf_series_pack: bad shape [%d][%d][%d]", R, C, S);
    KOAF_REQUIRE(margin >= 1 && 2 * margin < R && 2 * margin < C, "koaf_series_pack: margin %d of [%d][%d] (numpy's [0:-0] is empty)", margin, R, C);
    KOAF_REQUIRE(out16 == 0 || out16 == 1, "koaf_series_pack: out16 0 = uint8, 1 = uint16");
    KOAF_REQUIRE(((uintptr_t)x) % dtype_size(dtype) == 0 && (((uintptr_t)limits) & 7) == 0 && ((uintptr_t)out) % (out16 ? 2 : 1) == 0,
                 "koaf_series_pack: a pointer is not aligned to its element size");
    if (dtype == 2) series_pack_out<uint16_t>(x, out, out16, limits, R, C, S, margin, shift, STREAM);
    else if (dtype == 3) series_pack_out<int16_t>(x, out, out16, limits, R, C, S, margin, shift, STREAM);
    else if (dtype == 4) series_pack_out<float>(x, out, out16, limits, R, C, S, margin, shift, STREAM);
    else series_pack_out<double>(x, out, out16, limits, R, C, S, margin, shift, STREAM);
    return koaf_check_launch("koaf_series_pack");
}
