// koaf_cam.hip -- class-activation maps of the slice-wise trunks (Grad-CAM; not in the reference): the weighted channel sum of
// a trunk's last NHWC feature map, and the one write pass that resizes the low-resolution maps, normalises them and lays them
// out as the tensor the model received.  Both kernels are HBM-bound; no atomics, every reduction a fixed-order tree.
#include "koaf_common.h"

namespace {

constexpr int CAM_BLOCK = 256;       // 4 waves; wave w takes pixel rows w, w + 4, ...
constexpr size_t LDS_DYN_MAX = 65536 - 64;                    // 64 KiB a block, less the kernels' static reduction words (<= 32 B)
constexpr int CAM_MAX_C = (int)(LDS_DYN_MAX / sizeof(float)); // the w row sits in LDS
constexpr int UPS_MAX_K = 8192;      // the per-image scales sit in LDS, beside the H + W interpolation taps

// cam[n][p] = sum_c A[n][p][c] * w[n][c].  One block per image; a wave owns one pixel row at a time: lane l multiplies the
// 4-channel vectors l, l + 64, ... into four fmaf chains (ceil(C / 256) links each), adds them as (0 + 1) + (2 + 3) and the 64
// lanes as a xor butterfly -- ceil(C / 256) + 8 roundings on the longest path.  The row results of a wave are dealt round-robin
// to its lanes, which add theirs in row order; a butterfly per wave and ((w0 + w1) + (w2 + w3)) give the image sum: at most
// ceil(HW / 16384) + 7 roundings (log2(HW) + 1 up to HW = 16384).  The maximum runs on the magnitude bits, so a NaN survives.
template <bool H>
__global__ void __launch_bounds__(CAM_BLOCK) cam_kernel(const float* __restrict__ A, const float* __restrict__ w,
                                                        float* __restrict__ cam, float* __restrict__ img_sum,
                                                        float* __restrict__ img_max, int HW, int C, int relu) {
    extern __shared__ v4f cam_w[];
    __shared__ float red_s[CAM_BLOCK / 64];
    __shared__ unsigned red_m[CAM_BLOCK / 64];
    const int n = blockIdx.x, C4 = C / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const v4f* wn = (const v4f*)(w + (int64_t)n * C);
    for (int v = threadIdx.x; v < C4; v += CAM_BLOCK) cam_w[v] = wn[v];
    __syncthreads();
    const int64_t base = (int64_t)n * HW;
    float s = 0.f;
    unsigned m = 0u;
    int it = 0;
    for (int p = wave; p < HW; p += CAM_BLOCK / 64, ++it) {
        const int64_t row = (base + p) * C;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int v = lane; v < C4; v += 64) {
            const v4f a = load4_nt<H>(A, row + 4 * v), wv = cam_w[v];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(a[j], wv[j], acc[j]);
        }
        float r = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
        if (relu) r = r < 0.f ? 0.f : r;          // (a NaN fails the comparison and stays)
        if (lane == (it & 63)) {
            s += r;
            const unsigned b = koaf_absbits(r);
            m = m > b ? m : b;
        }
        if (lane == 0) cam[base + p] = r;
    }
    s = wave_sum(s);
    m = wave_max_u(m);
    if (lane == 0) { red_s[wave] = s; red_m[wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        img_sum[n] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        unsigned mm = red_m[0];
        for (int i = 1; i < CAM_BLOCK / 64; ++i) mm = mm > red_m[i] ? mm : red_m[i];
        img_max[n] = __uint_as_float(mm);
    }
}

// torch's align_corners=False rule: source coordinate = (in / out) * (dst + 0.5) - 0.5 clamped at 0, its two neighbours (the upper
// one clamped at in - 1) weighted linearly -- the rule of koaf_resize, evaluated as ((2 dst + 1) in - out) / (2 out): numerator
// and denominator are exact integers (below 2^24 for every size the trunks meet), so the coordinate carries ONE rounding.
struct CamTap { int i0; float w1; };
__device__ __forceinline__ CamTap cam_axis(int dst, int in, int out) {
    float src = (float)((2ll * dst + 1) * in - out) / (float)(2ll * out);
    if (src < 0.f) src = 0.f;
    const int i0 = min((int)src, in - 1);
    return {i0, src - (float)i0};
}

// The K scales of a sample (normalize 0: 1; 1: 1 / the largest img_max of the sample; 2: 1 / the image's own; a zero maximum
// gives 0, a non-finite one NaN) and the H + W interpolation taps, formed once per block in LDS.  All threads call it.
__device__ __forceinline__ void cam_block_tables(const float* __restrict__ mx, int K, int h, int w, int H, int W, int normalize,
                                                 CamTap* taps, float* scales) {
    __shared__ unsigned ups_red[4];
    unsigned smax = 0u;
    if (normalize == 1) {
        for (int k = threadIdx.x; k < K; k += 256) { const unsigned v = koaf_absbits(mx[k]); smax = smax > v ? smax : v; }
        smax = wave_max_u(smax);
        if ((threadIdx.x & 63) == 0) ups_red[threadIdx.x >> 6] = smax;
        __syncthreads();
        smax = ups_red[0];
        for (int i = 1; i < 4; ++i) smax = smax > ups_red[i] ? smax : ups_red[i];
    }
    for (int k = threadIdx.x; k < K; k += 256) {
        float sc = 1.f;
        if (normalize != 0) {
            const unsigned bits = normalize == 1 ? smax : koaf_absbits(mx[k]);
            sc = bits == 0u ? 0.f : koaf_bits_finite(bits) ? 1.f / __uint_as_float(bits) : __uint_as_float(0x7fc00000u);
        }
        scales[k] = sc;
    }
    for (int t = threadIdx.x; t < H + W; t += 256) taps[t] = t < H ? cam_axis(t, h, H) : cam_axis(t - H, w, W);
    __syncthreads();
}

// a + w (b - a) with one rounding after the difference: w < 1, so the result stays between a and b -- a map divided by its own
// maximum stays in [-1, 1], which a (1 - w) a + w b with its rounded weights does not promise
__device__ __forceinline__ float cam_lerp(float a, float b, float w) { return fmaf(w, b - a, a); }

// Columns (or no axis: V == 1) are the unit-stride axis of out.  Block (x, b) writes part of sample b; a thread produces V
// consecutive columns -- one 16-byte store when V == 4 -- and the grid walks the sample in (k, i, j) order.  An element costs
// its four cached reads of the small source image, three blends and the scale.
template <int V>
__global__ void __launch_bounds__(256) cam_upsample_kernel(const float* __restrict__ cam, const float* __restrict__ img_max,
                                                           float* __restrict__ out, int K, int h, int w, int H, int W, int64_t sb,
                                                           int64_t sk, int64_t si, int64_t sj, int normalize) {
    extern __shared__ CamTap ups_tap[];                        // [H + W] taps, then [K] scales
    float* ups_sc = (float*)(ups_tap + H + W);
    const int b = blockIdx.y;
    cam_block_tables(img_max + (int64_t)b * K, K, h, w, H, W, normalize, ups_tap, ups_sc);
    const unsigned nuv = (unsigned)(W / V);
    const unsigned total = (unsigned)(K * H) * nuv;
    const int64_t hw = (int64_t)h * w;
    const float* cb = cam + (int64_t)b * K * hw;
    float* ob = out + (int64_t)b * sb;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
        const int j = (int)(t % nuv) * V;
        const unsigned r = t / nuv;
        const int i = (int)(r % (unsigned)H), k = (int)(r / (unsigned)H);
        const CamTap ta = ups_tap[i];
        const int r0 = ta.i0 * w, r1 = r0 + (ta.i0 < h - 1 ? w : 0);
        const float* im = cb + k * hw;
        const float sc = ups_sc[k];
        float val[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const CamTap tb = ups_tap[H + j + v];
            const int c0 = tb.i0, c1 = c0 + (c0 < w - 1 ? 1 : 0);
            val[v] = cam_lerp(cam_lerp(im[r0 + c0], im[r0 + c1], tb.w1), cam_lerp(im[r1 + c0], im[r1 + c1], tb.w1), ta.w1) * sc;
        }
        float* o = ob + k * sk + i * si + j * sj;
        if constexpr (V == 4) __builtin_nontemporal_store((v4f){val[0], val[1], val[2], val[3]}, (v4f*)o);
        else o[0] = val[0];
    }
}

// Slices are the unit-stride axis of out (sk == 1: the (B,1,R,C,S) volumes).  Consecutive lanes then want consecutive IMAGES of
// the source, which lie h * w elements apart: read per element that is 64 cache lines per load instruction and bounds the kernel
// at an eighth of this one's rate (measured).  So block (x, b) takes whole output rows i of sample b and first lays the source row it needs
// into LDS slice-fastest, vertically blended and scaled: rowv[c][k] = lerp(cam[k][r0][c], cam[k][r1][c]) * scale[k] (w * K
// floats).  A thread then produces V consecutive slices of one column j from two 16-byte LDS reads and one blend per element.
template <int V>
__global__ void __launch_bounds__(256) cam_upsample_slices_kernel(const float* __restrict__ cam, const float* __restrict__ img_max,
                                                                  float* __restrict__ out, int K, int h, int w, int H, int W,
                                                                  int64_t sb, int64_t si, int64_t sj, int normalize) {
    extern __shared__ v4f ups_rowv4[];                         // [w * K] floats (K % 4 == 0 when V == 4), [H + W] taps, [K] scales
    float* rowv = (float*)ups_rowv4;
    CamTap* ups_tap = (CamTap*)(rowv + ((w * K + 3) & ~3));
    float* ups_sc = (float*)(ups_tap + H + W);
    const int b = blockIdx.y;
    cam_block_tables(img_max + (int64_t)b * K, K, h, w, H, W, normalize, ups_tap, ups_sc);
    const int64_t hw = (int64_t)h * w;
    const float* cb = cam + (int64_t)b * K * hw;
    float* ob = out + (int64_t)b * sb;
    const unsigned nuv = (unsigned)(K / V), total = (unsigned)W * nuv;
    for (int i = blockIdx.x; i < H; i += gridDim.x) {
        const CamTap ta = ups_tap[i];
        const int r0 = ta.i0 * w, r1 = r0 + (ta.i0 < h - 1 ? w : 0);
        __syncthreads();                                       // (the previous row's readers are done with rowv)
        for (int t = threadIdx.x; t < w * K; t += 256) {
            const int k = t % K, c = t / K;
            const float* im = cb + k * hw;
            rowv[c * K + k] = cam_lerp(im[r0 + c], im[r1 + c], ta.w1) * ups_sc[k];
        }
        __syncthreads();
        float* orow = ob + i * si;
        for (unsigned t = threadIdx.x; t < total; t += 256u) {
            const int k = (int)(t % nuv) * V, j = (int)(t / nuv);
            const CamTap tb = ups_tap[H + j];
            const int c0 = tb.i0, c1 = c0 + (c0 < w - 1 ? 1 : 0);
            float* o = orow + j * sj + k;
            if constexpr (V == 4) {
                const v4f a = *(const v4f*)&rowv[c0 * K + k], bb = *(const v4f*)&rowv[c1 * K + k];
                __builtin_nontemporal_store((v4f){cam_lerp(a[0], bb[0], tb.w1), cam_lerp(a[1], bb[1], tb.w1), cam_lerp(a[2], bb[2], tb.w1),
                                                  cam_lerp(a[3], bb[3], tb.w1)}, (v4f*)o);
            } else {
                o[0] = cam_lerp(rowv[c0 * K + k], rowv[c1 * K + k], tb.w1);
            }
        }
    }
}

}  // namespace

extern "C" int koaf_cam(const float* A, const float* w, float* cam, float* img_sum, float* img_max, int32_t N, int32_t HW,
                        int32_t C, int32_t relu, int32_t act16, void* stream) {
    KOAF_REQUIRE(A && w && cam && img_sum && img_max && N > 0 && HW > 0 && C > 0, "koaf_cam: bad args");
    KOAF_REQUIRE(C % 4 == 0 && C <= CAM_MAX_C, "koaf_cam: C %% 4 == 0 and C <= %d (C = %d)", CAM_MAX_C, C);
    KOAF_REQUIRE(aligned16(w) && (act16 ? (((uintptr_t)A) & 7) == 0 : aligned16(A)), "koaf_cam: unaligned");
    const size_t lds = (size_t)C * sizeof(float);
    KOAF_LAUNCH_ACT16(act16, cam_kernel<A16>, dim3(N), dim3(CAM_BLOCK), lds, STREAM, A, w, cam, img_sum, img_max, HW, C, relu);
    return koaf_check_launch("koaf_cam");
}

extern "C" int koaf_cam_upsample(const float* cam, const float* img_max, float* out, int32_t B, int32_t K, int32_t h, int32_t w,
                                 int32_t H, int32_t W, int64_t sb, int64_t sk, int64_t si, int64_t sj, int32_t normalize,
                                 void* stream) {
    KOAF_REQUIRE(cam && out && B > 0 && B <= 65535 && K > 0 && K <= UPS_MAX_K && h > 0 && w > 0 && H > 0 && W > 0,
                 "koaf_cam_upsample: bad args (B <= 65535, K <= %d)", UPS_MAX_K);
    KOAF_REQUIRE(normalize >= 0 && normalize <= 2 && (normalize == 0 || img_max), "koaf_cam_upsample: normalize is 0, 1 or 2 (1, 2 need img_max)");
    KOAF_REQUIRE(sb > 0 && sk > 0 && si > 0 && sj > 0, "koaf_cam_upsample: strides are positive element counts");
    KOAF_REQUIRE((int64_t)K * H * W < (1ll << 31) && (int64_t)h * w < (1ll << 31), "koaf_cam_upsample: sample too large");
    const size_t lds = (size_t)(H + W) * sizeof(CamTap) + (size_t)K * sizeof(float);
    const size_t lds_rows = lds + (((size_t)w * K + 3) & ~(size_t)3) * sizeof(float);
    KOAF_REQUIRE(lds <= LDS_DYN_MAX, "koaf_cam_upsample: H + W = %d taps and K = %d scales do not fit the 64 KiB of LDS", H + W, K);
    // slices on the unit-stride axis: whole output rows from a source row staged in LDS (where that row fits)
    const bool ku = sk == 1 && sj != 1 && lds_rows <= LDS_DYN_MAX;
    const bool v4 = aligned16(out) && sb % 4 == 0 && si % 4 == 0 &&
                    (ku ? (K % 4 == 0 && sj % 4 == 0) : (sj == 1 && W % 4 == 0 && sk % 4 == 0));
    const int64_t cap = cdiv64(256 * ew_blocks_per_cu(), B);
    const dim3 block(256);
    if (ku) {
        const dim3 grid((unsigned)(H < cap ? H : cap), B);
#define KOAF_UPS(V) hipLaunchKernelGGL(cam_upsample_slices_kernel<V>, grid, block, lds_rows, STREAM, cam, img_max, out, K, h, w, H, W, sb, si, sj, normalize)
        if (v4) KOAF_UPS(4);
        else KOAF_UPS(1);
#undef KOAF_UPS
    } else {
        int64_t gx = cdiv64((int64_t)K * H * W / (v4 ? 4 : 1), 256);
        if (gx > cap) gx = cap;
        const dim3 grid((unsigned)gx, B);
#define KOAF_UPS(V) hipLaunchKernelGGL(cam_upsample_kernel<V>, grid, block, lds, STREAM, cam, img_max, out, K, h, w, H, W, sb, sk, si, sj, normalize)
        if (v4) KOAF_UPS(4);
        else KOAF_UPS(1);
#undef KOAF_UPS
    }
    return koaf_check_launch("koaf_cam_upsample");
}
