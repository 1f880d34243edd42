// koaf_preproc.hip -- the input pipeline on the device: integer volumes to fp32, per-sample range, rotation / gamma /
// normalisation in one pass, resizing, the slice-major layout moves, and the per-sample dot product of the attribution maps.
#include "koaf_common.h"

namespace {
// integer volumes as they come off the disk (uint8 radiographs, uint16 / int16 MRI) -> fp32, 16 elements per thread step
template <typename T>
__global__ void __launch_bounds__(256) widen_kernel(const T* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t nv = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nv; i += (int64_t)gridDim.x * EB) {
        T v[4];
        __builtin_memcpy(v, x + i * 4, sizeof(v));        // one 4- or 8-byte load (4-element alignment checked by the caller)
        *(v4f*)&y[i * 4] = (v4f){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[nv * 4 + threadIdx.x] = (float)x[nv * 4 + threadIdx.x];
}
}  // namespace

extern "C" int koaf_widen(const void* x, int32_t dtype, float* y, int64_t n, void* stream) {
    KOAF_REQUIRE(x && y && n > 0 && dtype >= 1 && dtype <= 3, "koaf_widen: bad args (dtype 1 = uint8, 2 = uint16, 3 = int16)");
    KOAF_REQUIRE(aligned16(y) && (((uintptr_t)x) & 7) == 0, "koaf_widen: unaligned");
    const unsigned grid = ew_grid(n / 4 + 1);
    if (dtype == 1) hipLaunchKernelGGL(widen_kernel<uint8_t>, dim3(grid), dim3(EB), 0, STREAM, (const uint8_t*)x, y, n);
    else if (dtype == 2) hipLaunchKernelGGL(widen_kernel<uint16_t>, dim3(grid), dim3(EB), 0, STREAM, (const uint16_t*)x, y, n);
    else hipLaunchKernelGGL(widen_kernel<int16_t>, dim3(grid), dim3(EB), 0, STREAM, (const int16_t*)x, y, n);
    return koaf_check_launch("koaf_widen");
}

namespace {
// ------------------------------------------------------------------------------------------------
// input pipeline on the device (koafusion/preproc/_pt.py:75-99 PTToUnitRange, :257-345 PTRotate3DInSlice / PTRotate2D,
// :203-232 PTGammaCorrection, :101-135 PTNormalize -- applied per sample by the reference's CPU data-loader workers)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) minmax_part_kernel(const float* __restrict__ x, int64_t n, int nblk,
                                                          float* __restrict__ part) {
    const int b = blockIdx.y;
    const float* xb = x + (int64_t)b * n;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)nblk * 256) {
        const float v = xb[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    __shared__ float red[2][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[((int64_t)b * nblk + blockIdx.x) * 2 + 0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        part[((int64_t)b * nblk + blockIdx.x) * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}
__global__ void __launch_bounds__(64) minmax_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ mm) {
    const int b = blockIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += 64) {
        lo = fminf(lo, part[((int64_t)b * nblk + i) * 2 + 0]);
        hi = fmaxf(hi, part[((int64_t)b * nblk + i) * 2 + 1]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if (threadIdx.x == 0) { mm[2 * b] = lo; mm[2 * b + 1] = hi; }
}

// One thread per V consecutive slices of one (sample, row, column): the slice index is the fastest-varying one in
// memory, so consecutive lanes read consecutive addresses (V = 4 when S % 4 == 0, else 1; radiographs: S = 1, lanes run
// along the columns).  The four bilinear source positions depend on (row, column) only and are recomputed per lane.
template <int V>
__global__ void __launch_bounds__(256) augment_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      const float* __restrict__ mm, const float* __restrict__ prm,
                                                      int B, int R, int C, int S, float mean, float stdv) {
    const int SV = S / V;
    const int64_t total = (int64_t)B * R * C * SV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int sv = (int)(i % SV);
        const int64_t pix = i / SV;
        const int c = (int)(pix % C);
        const int r = (int)((pix / C) % R);
        const int b = (int)(pix / ((int64_t)R * C));
        const float mn = mm[2 * b], den = mm[2 * b + 1] - mn;
        const float cs = prm[4 * b], sn = prm[4 * b + 1], ex = prm[4 * b + 2];
        const bool rot = prm[4 * b + 3] != 0.f;
        const float* xb = x + (int64_t)b * R * C * S + V * sv;
        float v[V];
        if (rot) {
            // F.affine_grid(theta, align_corners=False) then F.grid_sample(bilinear, zeros, align_corners=False)
            const float xn = (2.f * c + 1.f) / C - 1.f, yn = (2.f * r + 1.f) / R - 1.f;
            const float gx = cs * xn - sn * yn, gy = sn * xn + cs * yn;
            const float ix = ((gx + 1.f) * C - 1.f) * 0.5f, iy = ((gy + 1.f) * R - 1.f) * 0.5f;
            const float fx = floorf(ix), fy = floorf(iy);
            const int x0 = (int)fx, y0 = (int)fy;
            const float tx = ix - fx, ty = iy - fy;
            const float w[4] = {(1.f - tx) * (1.f - ty), tx * (1.f - ty), (1.f - tx) * ty, tx * ty};
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
                if ((unsigned)xx < (unsigned)C && (unsigned)yy < (unsigned)R) {
                    const float* src = xb + (int64_t)(yy * C + xx) * S;
                    if constexpr (V == 4) {
                        const v4f q = *(const v4f*)src;
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] += ((q[j] - mn) / den) * w[k];
                    } else {
                        v[0] += ((src[0] - mn) / den) * w[k];
                    }
                }
            }
        } else {
            const float* src = xb + (int64_t)(r * C + c) * S;
            if constexpr (V == 4) {
                const v4f q = *(const v4f*)src;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (q[j] - mn) / den;
            } else {
                v[0] = (src[0] - mn) / den;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (ex != 0.f) v[j] = powf(v[j], ex);
            v[j] = (v[j] - mean) / stdv;
        }
        float* dst = y + pix * S + V * sv;
        if constexpr (V == 4) *(v4f*)dst = (v4f){v[0], v[1], v[2], v[3]};
        else dst[0] = v[0];
    }
}
}  // namespace

extern "C" int64_t koaf_minmax_ws(int64_t n) {
    int64_t nb = cdiv64(n, 256 * 16);
    return (nb < 1 ? 1 : (nb > 256 ? 256 : nb)) * 2;      // floats per sample
}
extern "C" int koaf_minmax(const float* x, int32_t B, int64_t n, float* mm, float* ws, void* stream) {
    KOAF_REQUIRE(x && mm && ws && B > 0 && n > 0, "koaf_minmax: bad args");
    const int nblk = (int)(koaf_minmax_ws(n) / 2);
    hipLaunchKernelGGL(minmax_part_kernel, dim3(nblk, B), dim3(256), 0, STREAM, x, n, nblk, ws);
    hipLaunchKernelGGL(minmax_final_kernel, dim3(B), dim3(64), 0, STREAM, ws, nblk, mm);
    return koaf_check_launch("koaf_minmax");
}
extern "C" int koaf_augment(const float* x, float* y, const float* mm, const float* params, int32_t B, int32_t R,
                            int32_t C, int32_t S, float mean, float stdv, void* stream) {
    KOAF_REQUIRE(x && y && mm && params && B > 0 && R > 0 && C > 0 && S > 0, "koaf_augment: bad args");
    KOAF_REQUIRE((int64_t)R * C * S < (1ll << 31), "koaf_augment: sample too large");
    const bool v4 = (S % 4 == 0) && aligned16(x) && aligned16(y);
    const int64_t total = (int64_t)B * R * C * (v4 ? S / 4 : S);
    if (v4)
        hipLaunchKernelGGL(augment_kernel<4>, dim3(ew_grid(total)), dim3(EB), 0, STREAM, x, y, mm, params, B, R, C, S, mean, stdv);
    else
        hipLaunchKernelGGL(augment_kernel<1>, dim3(ew_grid(total)), dim3(EB), 0, STREAM, x, y, mm, params, B, R, C, S, mean, stdv);
    return koaf_check_launch("koaf_augment");
}

namespace {
// 2x average pooling == F.interpolate(scale 0.5, align_corners=False, linear modes)
__global__ void __launch_bounds__(256) downscale2_kernel(const float* __restrict__ x, float* __restrict__ out, int B,
                                                         int R, int Cc, int S, int fs) {
    const int OR = R / 2, OC = Cc / 2, OS = S / fs;
    const int64_t total = (int64_t)B * OR * OC * OS;
    const float inv = 1.f / (float)(4 * fs);
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        int64_t p = i;
        const int os = (int)(p % OS); p /= OS;
        const int oc = (int)(p % OC); p /= OC;
        const int orr = (int)(p % OR);
        const int b = (int)(p / OR);
        float a = 0.f;
        for (int dr = 0; dr < 2; ++dr)
            for (int dc = 0; dc < 2; ++dc)
                for (int ds = 0; ds < fs; ++ds)
                    a += x[(((int64_t)b * R + 2 * orr + dr) * Cc + 2 * oc + dc) * S + os * fs + ds];
        out[i] = a * inv;
    }
}

// F.interpolate(x, scale_factor, mode = linear | bilinear | trilinear, align_corners=False, recompute_scale_factor=True) for
// ANY scale (preproc/_pt.py:175-192): x [BC][I0][I1][I2] -> out [BC][O0][O1][O2] (absent dimensions have size 1).  torch's rule:
// source coordinate = (in / out) * (dst + 0.5) - 0.5 clamped at 0, its two neighbours (the upper one clamped at in - 1)
// weighted linearly.
struct ResizeGeom { int I[3], O[3]; float rs[3]; };
__device__ __forceinline__ void resize_axis(int dst, int in, float rs, int& i0, int& i1, float& w1) {
    float src = rs * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    w1 = src - (float)i0;
}
__global__ void __launch_bounds__(256) resize_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t BC,
                                                     ResizeGeom g) {
    const int64_t on = (int64_t)g.O[0] * g.O[1] * g.O[2], in = (int64_t)g.I[0] * g.I[1] * g.I[2];
    const int64_t total = BC * on;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += (int64_t)gridDim.x * EB) {
        int64_t p = i;
        const int o2 = (int)(p % g.O[2]); p /= g.O[2];
        const int o1 = (int)(p % g.O[1]); p /= g.O[1];
        const int o0 = (int)(p % g.O[0]);
        const int64_t bc = p / g.O[0];
        int a0, a1, b0, b1, c0, c1;
        float wa, wb, wc;
        resize_axis(o0, g.I[0], g.rs[0], a0, a1, wa);
        resize_axis(o1, g.I[1], g.rs[1], b0, b1, wb);
        resize_axis(o2, g.I[2], g.rs[2], c0, c1, wc);
        const float* xb = x + bc * in;
        auto at = [&](int a, int b, int c) { return xb[((int64_t)a * g.I[1] + b) * g.I[2] + c]; };
        const float v00 = at(a0, b0, c0) * (1.f - wc) + at(a0, b0, c1) * wc, v01 = at(a0, b1, c0) * (1.f - wc) + at(a0, b1, c1) * wc;
        const float v10 = at(a1, b0, c0) * (1.f - wc) + at(a1, b0, c1) * wc, v11 = at(a1, b1, c0) * (1.f - wc) + at(a1, b1, c1) * wc;
        out[i] = (v00 * (1.f - wb) + v01 * wb) * (1.f - wa) + (v10 * (1.f - wb) + v11 * wb) * wa;
    }
}
}  // namespace

extern "C" int koaf_downscale2(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S, int32_t fs,
                               void* stream) {
    KOAF_REQUIRE(x && out && B > 0 && R % 2 == 0 && Cc % 2 == 0 && (fs == 1 || fs == 2) && S % fs == 0,
                 "koaf_downscale2: needs even R,C (and S if fs==2)");
    const int64_t total = (int64_t)B * (R / 2) * (Cc / 2) * (S / fs);
    hipLaunchKernelGGL(downscale2_kernel, dim3(ew_grid(total)), dim3(EB), 0, STREAM, x, out, B, R, Cc, S, fs);
    return koaf_check_launch("koaf_downscale2");
}

extern "C" int koaf_resize(const float* x, float* out, int64_t BC, int32_t ndim, const int32_t* in_size, const int32_t* out_size,
                           void* stream) {
    KOAF_REQUIRE(x && out && BC > 0 && ndim >= 1 && ndim <= 3 && in_size && out_size, "koaf_resize: bad args (1..3 spatial dims)");
    ResizeGeom g;
    for (int d = 0; d < 3; ++d) {
        const int k = d - (3 - ndim);         // leading absent dimensions have size 1
        g.I[d] = k >= 0 ? in_size[k] : 1;
        g.O[d] = k >= 0 ? out_size[k] : 1;
        KOAF_REQUIRE(g.I[d] > 0 && g.O[d] > 0, "koaf_resize: empty dimension");
        g.rs[d] = (float)g.I[d] / (float)g.O[d];
    }
    const int64_t total = BC * g.O[0] * g.O[1] * g.O[2];
    hipLaunchKernelGGL(resize_kernel, dim3(ew_grid(total)), dim3(EB), 0, STREAM, x, out, BC, g);
    return koaf_check_launch("koaf_resize");
}

namespace {
// ------------------------------------------------------------------------------------------------
// layout moves
// ------------------------------------------------------------------------------------------------
// x [B][P][S] -> out [B][S][P]   (P = R*C pixels), 32x32 LDS tiles
__global__ void __launch_bounds__(256) slice_fold_kernel(const float* __restrict__ x, float* __restrict__ out, int P,
                                                         int S) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int p0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 8 rows per pass
    const float* xb = x + (int64_t)b * P * S;
    float* ob = out + (int64_t)b * P * S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int p = p0 + ty + 8 * j, s = s0 + tx;
        tile[ty + 8 * j][tx] = (p < P && s < S) ? xb[(int64_t)p * S + s] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int s = s0 + ty + 8 * j, p = p0 + tx;
        if (p < P && s < S) ob[(int64_t)s * P + p] = tile[tx][ty + 8 * j];
    }
}
}  // namespace

extern "C" int koaf_slice_fold(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S, void* stream) {
    KOAF_REQUIRE(x && out && B > 0 && R > 0 && Cc > 0 && S > 0 && B <= 65535, "koaf_slice_fold: bad args");
    const int P = R * Cc;
    dim3 grid((P + 31) / 32, (S + 31) / 32, B);
    hipLaunchKernelGGL(slice_fold_kernel, grid, dim3(256), 0, STREAM, x, out, P, S);
    return koaf_check_launch("koaf_slice_fold");
}
// the transpose of the transpose: x [B][S][P] -> out [B][P][S], the same tile kernel with the two extents exchanged
extern "C" int koaf_slice_unfold(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S, void* stream) {
    KOAF_REQUIRE(x && out && B > 0 && R > 0 && Cc > 0 && S > 0 && B <= 65535, "koaf_slice_unfold: bad args");
    const int64_t P = (int64_t)R * Cc;
    KOAF_REQUIRE(P <= 65535ll * 32, "koaf_slice_unfold: image too large");
    dim3 grid((S + 31) / 32, (unsigned)((P + 31) / 32), B);
    hipLaunchKernelGGL(slice_fold_kernel, grid, dim3(256), 0, STREAM, x, out, S, (int)P);
    return koaf_check_launch("koaf_slice_unfold");
}

namespace {
// ------------------------------------------------------------------------------------------------
// per-sample dot product (gradient x input totals): out[b] = sum_i a[b][i] * b[b][i].  Stage 1: one block per RD_CHUNK elements,
// fp64 accumulation (a product of two fp32 values is exact there), fixed lane / wave order; stage 2: one wave per sample adds
// the block sums in index order.  No atomics: the bits do not depend on scheduling.
// ------------------------------------------------------------------------------------------------
constexpr int RD_CHUNK = 8192;
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ void __launch_bounds__(256) rowdot_part_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                          int nblk, double* __restrict__ ws) {
    const int s = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * RD_CHUNK, r1 = r0 + RD_CHUNK < n ? r0 + RD_CHUNK : n;
    const float* as = a + (int64_t)s * n;
    const float* bs = b + (int64_t)s * n;
    double acc = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) acc += (double)as[i] * (double)bs[i];
    acc = wave_sum_d(acc);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[(int64_t)s * nblk + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ void __launch_bounds__(64) rowdot_final_kernel(const double* __restrict__ ws, int nblk, float* __restrict__ out) {
    const int s = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) acc += ws[(int64_t)s * nblk + i];
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) out[s] = (float)acc;
}
}  // namespace

extern "C" int64_t koaf_rowdot_ws(int64_t n) { return n > 0 ? 2 * cdiv64(n, RD_CHUNK) : 0; }      // (fp64 block sums)
extern "C" int koaf_rowdot(const float* a, const float* b, int32_t B, int64_t n, float* out, float* ws, void* stream) {
    KOAF_REQUIRE(a && b && out && ws && B > 0 && B <= 65535 && n > 0, "koaf_rowdot: bad args");
    KOAF_REQUIRE((((uintptr_t)ws) & 7) == 0, "koaf_rowdot: the workspace is 8-byte aligned");
    const int64_t nblk = cdiv64(n, RD_CHUNK);
    KOAF_REQUIRE(nblk < (1ll << 31), "koaf_rowdot: rows too long");
    hipLaunchKernelGGL(rowdot_part_kernel, dim3((unsigned)nblk, B), dim3(256), 0, STREAM, a, b, n, (int)nblk, (double*)ws);
    hipLaunchKernelGGL(rowdot_final_kernel, dim3(B), dim3(64), 0, STREAM, (const double*)ws, (int)nblk, out);
    return koaf_check_launch("koaf_rowdot");
}
