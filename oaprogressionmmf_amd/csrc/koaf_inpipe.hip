// koaf_inpipe.hip -- from the STORED integer volumes to the tensor the model consumes: the crop window, the flip, the per-sample
// range, rotation / gamma / normalisation and the 2x average pool, read in place through a per-sample table (koaf.h).  Two
// launches (+ the small second stage of the reduction) instead of widen -> minmax -> augment -> downscale2 on a batch the host
// has cropped, flipped and stacked.
#include "koaf_common.h"

namespace {
// one sample's row of the table, decoded: element strides of the three WINDOW axes in the stored volume (negative on an axis
// walked backwards) and the element offset of window voxel (0, 0, 0)
struct Win {
    const char* base;
    int64_t e0, tR, tC;
    int tS;
    bool ok;
};
// ok = the whole R x C x S window lies inside the stored volume: a table that fails this is never dereferenced
__device__ __forceinline__ Win win_of(const int64_t* __restrict__ tab, int b, int R, int C, int S) {
    const int64_t* t = tab + 8 * (int64_t)b;
    const int64_t R0 = t[1], C0 = t[2], S0 = t[3], r0 = t[4], c0 = t[5], s0 = t[6], back = t[7];
    const int dR = (back & 1) ? -1 : 1, dC = (back & 2) ? -1 : 1, dS = (back & 4) ? -1 : 1;
    const int64_t r1 = r0 + (int64_t)dR * (R - 1), c1 = c0 + (int64_t)dC * (C - 1), s1 = s0 + (int64_t)dS * (S - 1);
    Win w;
    w.base = (const char*)t[0];
    w.ok = w.base != nullptr && R0 > 0 && C0 > 0 && S0 > 0 && r0 >= 0 && r0 < R0 && r1 >= 0 && r1 < R0 && c0 >= 0 && c0 < C0 &&
           c1 >= 0 && c1 < C0 && s0 >= 0 && s0 < S0 && s1 >= 0 && s1 < S0;
    w.e0 = (r0 * C0 + c0) * S0 + s0;
    w.tR = dR * C0 * S0;
    w.tC = dC * S0;
    w.tS = dS;
    return w;
}

// element e of a stored volume as fp32 (dtype 0 = fp32, 1 = uint8, 2 = uint16, 3 = int16; integers below 2^24: exact)
__device__ __forceinline__ float load1(const char* base, int dtype, int64_t e) {
    switch (dtype) {
        case 0: return ((const float*)base)[e];
        case 1: return (float)((const uint8_t*)base)[e];
        case 2: return (float)((const uint16_t*)base)[e];
        default: return (float)((const int16_t*)base)[e];
    }
}
// v[j] = element e + j * step, j < N.  Four elements one apart travel as ONE 4- / 8- / 16-byte load where the lowest address
// is a multiple of that size (the origin and S0 are arbitrary: a uint8 row may start at any byte), one by one otherwise.
template <int N>
__device__ __forceinline__ void load_run(const char* base, int dtype, int64_t e, int64_t step, float (&v)[N]) {
    if constexpr (N == 4) {
        if (step == 1 || step == -1) {
            const int64_t lo = step == 1 ? e : e - 3;
            const int esz = dtype == 0 ? 4 : (dtype == 1 ? 1 : 2);
            const char* p = base + lo * esz;
            if ((((uintptr_t)p) & (uintptr_t)(4 * esz - 1)) == 0) {
                float q[4];
                if (dtype == 0) {
                    const v4f f = *(const v4f*)p;
                    q[0] = f[0]; q[1] = f[1]; q[2] = f[2]; q[3] = f[3];
                } else if (dtype == 1) {
                    const uint32_t u = *(const uint32_t*)p;
                    q[0] = (float)(u & 0xffu); q[1] = (float)((u >> 8) & 0xffu); q[2] = (float)((u >> 16) & 0xffu); q[3] = (float)(u >> 24);
                } else {
                    const uint2 u = *(const uint2*)p;
                    const uint32_t h[4] = {u.x & 0xffffu, u.x >> 16, u.y & 0xffffu, u.y >> 16};
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = dtype == 2 ? (float)h[j] : (float)(int16_t)h[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = step == 1 ? q[j] : q[3 - j];
                return;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = load1(base, dtype, e + j * step);
}

// ---- per-sample (min, max) of the window.  The window is walked as [D0][D1][D2] with D2 the contiguous axis: (R, C, S), or
// (1, R, C) for a radiograph (S = S0 = 1), whose columns are then the vector axis.  NS elements of D2 per thread step. --------
template <int NS>
__global__ void __launch_bounds__(256) window_minmax_part_kernel(const int64_t* __restrict__ tab, int dtype, int R, int C, int S,
                                                                 int flat2d, int nblk, float* __restrict__ part) {
    const int b = blockIdx.y;
    const Win w = win_of(tab, b, R, C, S);
    float lo = INFINITY, hi = -INFINITY;
    if (w.ok) {
        const unsigned D1 = flat2d ? R : C, D2 = flat2d ? C : S;
        const int64_t t0 = flat2d ? 0 : w.tR, t1 = flat2d ? w.tR : w.tC, t2 = flat2d ? w.tC : (int64_t)w.tS;
        const unsigned G = D2 / NS;
        const unsigned n = (unsigned)(flat2d ? 1 : R) * D1 * G;      // (below 2^31: 32-bit divisions)
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned)nblk * 256u) {
            const unsigned g = i % G, row = i / G;
            const int64_t e = w.e0 + (int64_t)(row / D1) * t0 + (int64_t)(row % D1) * t1 + (int64_t)g * NS * t2;
            float v[NS];
            load_run<NS>(w.base, dtype, e, t2, v);
#pragma unroll
            for (int j = 0; j < NS; ++j) { lo = fminf(lo, v[j]); hi = fmaxf(hi, v[j]); }
        }
    } else {
        lo = hi = NAN;      // (fminf / fmaxf drop a NaN operand: set, not folded)
    }
    float l2 = -wave_max(-lo), h2 = wave_max(hi);
    __shared__ float red[2][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = l2; red[1][threadIdx.x >> 6] = h2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)b * nblk + blockIdx.x) * 2;
        o[0] = w.ok ? fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3])) : NAN;
        o[1] = w.ok ? fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3])) : NAN;
    }
}
__global__ void __launch_bounds__(64) window_minmax_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ mm) {
    const int b = blockIdx.x;
    const float* pb = part + (int64_t)b * nblk * 2;
    const bool bad = pb[0] != pb[0];          // a refused table row (every partial of the sample is NaN then)
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += 64) {
        lo = fminf(lo, pb[2 * i + 0]);
        hi = fmaxf(hi, pb[2 * i + 1]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if (threadIdx.x == 0) { mm[2 * b] = bad ? NAN : lo; mm[2 * b + 1] = bad ? NAN : hi; }
}

// ---- the fused pass.  One thread per NS consecutive SOURCE slices of one P x P block of window pixels: the slice index is
// the fastest-varying one in memory, so consecutive lanes read consecutive addresses (NS = 4 when S % 4 == 0, else PS;
// radiographs: S = 1, lanes run along the columns).  f is koaf_augment's arithmetic, statement for statement, at window
// coordinates; the four bilinear neighbours of a rotated pixel are bounded by the WINDOW (the reference rotates the cropped
// tensor) and addressed through the sample's origin and strides.  The pool is koaf_downscale2's sum in its order. ------------
template <int NS, int P, int PS>
__global__ void __launch_bounds__(256) input_pipeline_kernel(const int64_t* __restrict__ tab, int dtype, float* __restrict__ y,
                                                             const float* __restrict__ mm, const float* __restrict__ prm, int B,
                                                             int R, int C, int S, float mean, float stdv, int ncdhw, int vec_out) {
    constexpr int VO = NS / PS;
    // one block column per sample: the sample's row of the table is wave-uniform, and the index of a work item inside one
    // sample fits 32 bits (the window is below 2^31 voxels), which keeps the three divisions cheap
    const unsigned OR = R / P, OC = C / P, OS = S / PS, SG = S / NS;
    const float inv = 1.f / (float)(P * P * PS);
    const int b = blockIdx.y;
    const unsigned it = blockIdx.x * 256u + threadIdx.x;
    if (it >= OR * OC * SG) return;
    const unsigned sg = it % SG, pix_b = it / SG;
    const unsigned oc = pix_b % OC, orr = pix_b / OC;
    const int64_t pix = (int64_t)b * OR * OC + pix_b;
    const Win w = win_of(tab, b, R, C, S);
    const float mn = mm[2 * b], den = mm[2 * b + 1] - mn;
    const float cs = prm[4 * b], sn = prm[4 * b + 1], ex = prm[4 * b + 2];
    const bool rot = prm[4 * b + 3] != 0.f;
    float f[P * P][NS];
#pragma unroll
    for (int q = 0; q < P * P; ++q) {
        const int r = (int)orr * P + q / P, c = (int)oc * P + q % P;
        float (&v)[NS] = f[q];
        const int64_t es = w.e0 + (int64_t)sg * NS * w.tS;
        if (!w.ok) {
#pragma unroll
            for (int j = 0; j < NS; ++j) v[j] = NAN;
        } else if (rot) {
            // F.affine_grid(theta, align_corners=False) then F.grid_sample(bilinear, zeros, align_corners=False)
            const float xn = (2.f * c + 1.f) / C - 1.f, yn = (2.f * r + 1.f) / R - 1.f;
            const float gx = cs * xn - sn * yn, gy = sn * xn + cs * yn;
            const float ix = ((gx + 1.f) * C - 1.f) * 0.5f, iy = ((gy + 1.f) * R - 1.f) * 0.5f;
            const float fx = floorf(ix), fy = floorf(iy);
            const int x0 = (int)fx, y0 = (int)fy;
            const float tx = ix - fx, ty = iy - fy;
            const float wt[4] = {(1.f - tx) * (1.f - ty), tx * (1.f - ty), (1.f - tx) * ty, tx * ty};
#pragma unroll
            for (int j = 0; j < NS; ++j) v[j] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
                if ((unsigned)xx < (unsigned)C && (unsigned)yy < (unsigned)R) {
                    float s[NS];
                    load_run<NS>(w.base, dtype, es + yy * w.tR + xx * w.tC, w.tS, s);
#pragma unroll
                    for (int j = 0; j < NS; ++j) v[j] += ((s[j] - mn) / den) * wt[k];
                }
            }
        } else {
            float s[NS];
            load_run<NS>(w.base, dtype, es + r * w.tR + c * w.tC, w.tS, s);
#pragma unroll
            for (int j = 0; j < NS; ++j) v[j] = (s[j] - mn) / den;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (ex != 0.f) v[j] = powf(v[j], ex);
            v[j] = (v[j] - mean) / stdv;
        }
    }
    float o[VO];
#pragma unroll
    for (int j = 0; j < VO; ++j) {
        if constexpr (P == 1 && PS == 1) {
            o[j] = f[0][j];
        } else {
            float a = 0.f;
#pragma unroll
            for (int q = 0; q < P * P; ++q)
#pragma unroll
                for (int ds = 0; ds < PS; ++ds) a += f[q][j * PS + ds];
            o[j] = a * inv;
        }
    }
    const unsigned os = sg * VO;
    if (ncdhw) {                                             // [B][OS][OR][OC]
        float* dst = y + (((int64_t)b * OS + os) * OR + orr) * (int64_t)OC + oc;
#pragma unroll
        for (int j = 0; j < VO; ++j) dst[(int64_t)j * OR * OC] = o[j];
    } else {                                                 // [B][OR][OC][OS]
        float* dst = y + pix * OS + os;
        if constexpr (VO == 4) {
            if (vec_out) { *(v4f*)dst = (v4f){o[0], o[1], o[2], o[3]}; return; }
        }
        if constexpr (VO == 2) {
            if (vec_out) { *(float2*)dst = make_float2(o[0], o[1]); return; }
        }
#pragma unroll
        for (int j = 0; j < VO; ++j) dst[j] = o[j];
    }
}

bool window_args_ok(const void* table, int dtype, int B, int R, int C, int S) {
    return table && dtype >= 0 && dtype <= 3 && B > 0 && B <= 65535 && R > 0 && C > 0 && S > 0 && (int64_t)R * C * S < (1ll << 31);
}
}  // namespace

extern "C" int64_t koaf_window_minmax_ws(int64_t n) {
    int64_t nb = cdiv64(n, 256 * 16);
    return (nb < 1 ? 1 : (nb > 256 ? 256 : nb)) * 2;      // floats per sample
}
extern "C" int koaf_window_minmax(const int64_t* table, int32_t dtype, int32_t B, int32_t R, int32_t C, int32_t S, float* mm,
                                  float* ws, void* stream) {
    KOAF_REQUIRE(window_args_ok(table, dtype, B, R, C, S) && mm && ws,
                 "koaf_window_minmax: bad args (dtype 0 = fp32, 1 = uint8, 2 = uint16, 3 = int16; B <= 65535; window below 2^31 voxels)");
    const int nblk = (int)(koaf_window_minmax_ws((int64_t)R * C * S) / 2);
    const int flat2d = S == 1;                           // (a one-slice window of a deeper volume: its stride is not 1, load_run copes)
    const bool v4 = (flat2d ? C : S) % 4 == 0;
    if (v4)
        hipLaunchKernelGGL(window_minmax_part_kernel<4>, dim3(nblk, B), dim3(256), 0, STREAM, table, dtype, R, C, S, flat2d, nblk, ws);
    else
        hipLaunchKernelGGL(window_minmax_part_kernel<1>, dim3(nblk, B), dim3(256), 0, STREAM, table, dtype, R, C, S, flat2d, nblk, ws);
    hipLaunchKernelGGL(window_minmax_final_kernel, dim3(B), dim3(64), 0, STREAM, ws, nblk, mm);
    return koaf_check_launch("koaf_window_minmax");
}

extern "C" int koaf_input_pipeline(const int64_t* table, int32_t dtype, float* y, const float* mm, const float* params, int32_t B,
                                   int32_t R, int32_t C, int32_t S, int32_t pool, int32_t pool_s, int32_t layout, float mean,
                                   float stdv, void* stream) {
    KOAF_REQUIRE(window_args_ok(table, dtype, B, R, C, S) && y && mm && params, "koaf_input_pipeline: bad args");
    KOAF_REQUIRE((pool == 1 || pool == 2) && (pool_s == 1 || pool_s == 2) && R % pool == 0 && C % pool == 0 && S % pool_s == 0,
                 "koaf_input_pipeline: pools are 1 or 2 and divide the window");
    KOAF_REQUIRE(layout == 0 || layout == 1, "koaf_input_pipeline: layout 0 = [B][R'][C'][S'], 1 = [B][S'][R'][C']");
    const bool v4 = S % 4 == 0;
    const int ns = v4 ? 4 : pool_s;
    const int64_t per = (int64_t)(R / pool) * (C / pool) * (S / ns);        // work items of one sample
    const int vec_out = aligned16(y) ? 1 : 0;
    const dim3 grid((unsigned)cdiv64(per, EB), B), block(EB);
#define KOAF_INPIPE(NS, P, PS)                                                                                                  \
    hipLaunchKernelGGL((input_pipeline_kernel<NS, P, PS>), grid, block, 0, STREAM, table, dtype, y, mm, params, B, R, C, S, mean, \
                       stdv, layout, vec_out)
    if (pool == 1 && pool_s == 1) { if (v4) KOAF_INPIPE(4, 1, 1); else KOAF_INPIPE(1, 1, 1); }
    else if (pool == 2 && pool_s == 1) { if (v4) KOAF_INPIPE(4, 2, 1); else KOAF_INPIPE(1, 2, 1); }
    else if (pool == 1 && pool_s == 2) { if (v4) KOAF_INPIPE(4, 1, 2); else KOAF_INPIPE(2, 1, 2); }
    else { if (v4) KOAF_INPIPE(4, 2, 2); else KOAF_INPIPE(2, 2, 2); }
#undef KOAF_INPIPE
    return koaf_check_launch("koaf_input_pipeline");
}
