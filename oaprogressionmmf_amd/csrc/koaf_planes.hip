// koaf_planes.hip -- the cutters of the pre-split fp16 plane images that koaf_gemm_kernel reads by LDS-DMA: the weights of every
// convolution once per optimizer step (koaf_wplanes_build, the M_PS operand) and activations (koaf_act_planes, M_PA / M_PH / M_PT / M_PK).
#include "koaf_pieces.h"

// ================================================================================================
// weight plane images (the M_PS operand): cut once per optimizer step for every convolution weight of the model
// ================================================================================================
namespace {
// block -> (descriptor, tile): the last descriptor whose first tile is <= blockIdx.x; tile = 32 (rows) x 32 (k of one tap)
struct WTile { KoafWPlane d; int idx, rt, tap, ct; };
__device__ __forceinline__ WTile wtile_of_block(const KoafWPlane* __restrict__ tab, int ntab) {
    int lo = 0, hi = ntab - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    WTile w;
    w.d = tab[lo];
    w.idx = lo;
    int tl = (int)((int64_t)blockIdx.x - w.d.tile0);
    const int nct = (w.d.C + 31) / 32;
    w.ct = tl % nct; tl /= nct;
    w.tap = tl % w.d.taps;
    w.rt = tl / w.d.taps;
    return w;
}
__device__ __forceinline__ v4f wtile_load(const float* __restrict__ base, const WTile& w, int r, int c) {
    const KoafWPlane& d = w.d;
    const int64_t K = (int64_t)d.taps * d.C;
    v4f x = {0.f, 0.f, 0.f, 0.f};
    if (r < d.R) {
        const float* s = base + d.src_off + (int64_t)r * K + (int64_t)w.tap * d.C + c;
        if (c + 3 < d.C && ((K | d.C) & 3) == 0) x = *(const v4f*)s;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (c + j < d.C) x[j] = s[j];
        }
    }
    return x;
}

// pass 1: amax[i] = max |w| of weight i (amax zeroed beforehand; float bits of non-negative values order like integers)
__global__ void __launch_bounds__(256) wplanes_amax_kernel(const float* __restrict__ base, const KoafWPlane* __restrict__ tab,
                                                           int ntab, float* __restrict__ amax) {
    const WTile w = wtile_of_block(tab, ntab);
    const int t = threadIdx.x;
    const v4f x = wtile_load(base, w, w.rt * 32 + (t >> 3), w.ct * 32 + 4 * (t & 7));
    block_amax_raise_bits(max(max(koaf_absbits(x[0]), koaf_absbits(x[1])), max(koaf_absbits(x[2]), koaf_absbits(x[3]))), amax + w.idx);
}

// pass 2: the images of w * scale_of_amax(amax[i]) (split2h: bit-identical to the in-kernel split of the same operand)
//   F image [2][R][Kp]         (Kp = taps * C rounded up to 32; forward B operand: rows = output channels)
//   D image [2][C][taps * Rp]  (Rp = R rounded up to 32; the transposed weight, dgrad B operand: rows = input channels,
//                               k = (tap, output channel)); the tile is transposed through LDS.
// Both are zero-filled up to their padded extents.
__global__ void __launch_bounds__(256) wplanes_build_kernel(const float* __restrict__ base, unsigned short* __restrict__ planes,
                                                            const KoafWPlane* __restrict__ tab, int ntab,
                                                            const float* __restrict__ amax) {
    __shared__ unsigned short tile[2][32][36];      // [plane][c][r] (+4 pad)
    const WTile w = wtile_of_block(tab, ntab);
    const KoafWPlane& d = w.d;
    const int t = threadIdx.x, ty = t >> 3, tx = t & 7;
    const int r = w.rt * 32 + ty, c = w.ct * 32 + 4 * tx;
    unsigned pl[2][2];
    {
        v4f x = wtile_load(base, w, r, c);
        const float sc = scale_of_amax(amax[w.idx]);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = __builtin_amdgcn_fmed3f(x[j] * sc, -65504.f, 65504.f);
        split2h(x, pl);
    }
    if (d.f_off >= 0 && r < d.R) {
        // (c + 3 < Kp always: Kp and c are multiples of 4, the tile covers C rounded up to 32 only when taps == 1)
        unsigned short* f = planes + d.f_off + (int64_t)r * d.Kp + (int64_t)w.tap * d.C + c;
        const int64_t ps = (int64_t)d.R * d.Kp;
#pragma unroll
        for (int q = 0; q < 2; ++q) *(uint2*)(f + q * ps) = make_uint2(pl[q][0], pl[q][1]);
    }
    if (d.d_off < 0) return;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        tile[q][4 * tx + 0][ty] = (unsigned short)(pl[q][0] & 0xffffu);
        tile[q][4 * tx + 1][ty] = (unsigned short)(pl[q][0] >> 16);
        tile[q][4 * tx + 2][ty] = (unsigned short)(pl[q][1] & 0xffffu);
        tile[q][4 * tx + 3][ty] = (unsigned short)(pl[q][1] >> 16);
    }
    __syncthreads();
    const int cc = w.ct * 32 + ty;                   // this thread now owns input channel cc, rows rt*32 + 4tx .. +3
    if (cc < d.C) {
        const int64_t ldd = (int64_t)d.taps * d.Rp, ps = (int64_t)d.C * ldd;
        unsigned short* o = planes + d.d_off + (int64_t)cc * ldd + (int64_t)w.tap * d.Rp + w.rt * 32 + 4 * tx;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned short* sr = &tile[q][ty][4 * tx];
            *(uint2*)(o + q * ps) = make_uint2((unsigned)sr[0] | ((unsigned)sr[1] << 16), (unsigned)sr[2] | ((unsigned)sr[3] << 16));
        }
    }
}
}  // namespace

extern "C" int koaf_wplanes_build(const float* base, uint16_t* planes, float* amax, const KoafWPlane* table_dev, int32_t n,
                                  int64_t ntiles, void* stream) {
    KOAF_REQUIRE(base && planes && amax && table_dev && n > 0 && ntiles > 0 && ntiles < (1ll << 31), "koaf_wplanes_build: bad args");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(amax, 0, sizeof(float) * (size_t)n, s) != hipSuccess) {
        koaf_set_error("koaf_wplanes_build: memset failed");
        return KOAF_ELAUNCH;
    }
    hipLaunchKernelGGL(wplanes_amax_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, base, table_dev, n, amax);
    int rc = koaf_check_launch("koaf_wplanes_build/amax");
    if (rc != KOAF_OK) return rc;
    hipLaunchKernelGGL(wplanes_build_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, base, planes, table_dev, n, amax);
    return koaf_check_launch("koaf_wplanes_build");
}


// ================================================================================================
// activation plane images (the M_PA operand): the fp16 piece planes of an NHWC tensor, transform included
// ================================================================================================
namespace {
// TF as in TileLoader (0 none, 1 relu(sc*x+sh), 2 sc*x + sh - sc2*x2); the arithmetic is finish_unit()'s + split2h, so the
// images hold bit for bit what the fp32 loader of the same operand puts into LDS.
// X16: the activation among the sources is stored as bf16 (tf 0 / 1: x; tf 2: x2 = the conv output c)
template <int TF, bool X16>
__global__ void __launch_bounds__(256) act_planes_kernel(const float* __restrict__ x, const float* __restrict__ x2, int64_t n8,
                                                         int C, const float* __restrict__ sc, const float* __restrict__ sh,
                                                         const float* __restrict__ sc2, const float* __restrict__ amax,
                                                         float fscale, unsigned short* __restrict__ planes, int64_t ps,
                                                         uint32_t* status) {
    constexpr float HMAX = 65504.f;
    unsigned nsat = 0;      // elements beyond the fp16 range of the scale (clamped below) or not finite
    const float fsc = amax ? scale_of_amax(*amax) : (fscale != 0.f ? fscale : 1.f);
    if (blockIdx.x == 0 && threadIdx.x == 0) *(uint4*)(planes + 2 * ps) = make_uint4(0u, 0u, 0u, 0u);   // the zero chunk
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 8) % C);
        unsigned pl[2][2][2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            v4f v = load4<X16 && TF != 2>(x, i * 8 + 4 * hf);
            if constexpr (TF == 1) {
                const v4f a = *(const v4f*)(sc + c + 4 * hf) * fsc, b = *(const v4f*)(sh + c + 4 * hf) * fsc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = fmaf(v[j], a[j], b[j]);
                    nsat += !(u <= HMAX) ? 1u : 0u;
                    v[j] = __builtin_amdgcn_fmed3f(u, 0.f, HMAX);
                }
            } else if constexpr (TF == 2) {
                const v4f a = *(const v4f*)(sc + c + 4 * hf) * fsc, b = *(const v4f*)(sh + c + 4 * hf) * fsc;
                const v4f k = *(const v4f*)(sc2 + c + 4 * hf) * fsc;
                const v4f w = load4<X16>(x2, i * 8 + 4 * hf);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = fmaf(a[j], v[j], fmaf(-k[j], w[j], b[j]));
                    nsat += !(fabsf(u) <= HMAX) ? 1u : 0u;
                    v[j] = __builtin_amdgcn_fmed3f(u, -HMAX, HMAX);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = v[j] * fsc;
                    nsat += !(fabsf(u) <= HMAX) ? 1u : 0u;
                    v[j] = __builtin_amdgcn_fmed3f(u, -HMAX, HMAX);
                }
            }
            split2h(v, pl[hf]);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
            *(uint4*)(planes + q * ps + i * 8) = make_uint4(pl[0][q][0], pl[0][q][1], pl[1][q][0], pl[1][q][1]);
    }
    koaf_status_add(status, 0, nsat);
}
}  // namespace

extern "C" int64_t koaf_act_planes_elems(int64_t npix, int32_t C) { return 2 * npix * C + 8; }

extern "C" int koaf_act_planes(const float* x, const float* x2, int64_t npix, int32_t C, int32_t tf, const float* sc,
                               const float* sh, const float* sc2, const float* amax, float fscale, uint16_t* planes,
                               int32_t act16, void* stream) {
    KOAF_REQUIRE(x && planes && npix > 0 && C > 0 && (C & 7) == 0 && tf >= 0 && tf <= 2, "koaf_act_planes: bad args (C %% 8 == 0)");
    KOAF_REQUIRE(tf == 0 || (sc && sh), "koaf_act_planes: tf needs sc / sh");
    KOAF_REQUIRE(tf != 2 || (x2 && sc2), "koaf_act_planes: tf 2 needs x2 / sc2");
    KOAF_REQUIRE(aligned16(x) && aligned16(planes) && (tf != 2 || aligned16(x2)) && (tf == 0 || (aligned16(sc) && aligned16(sh))),
                 "koaf_act_planes: unaligned");
    const int64_t ps = npix * C, n8 = ps / 8;
    int64_t blocks = cdiv64(n8, 256);
    if (blocks > 16384) blocks = 16384;
    hipStream_t s = (hipStream_t)stream;
#define KOAF_AP(TF_, X_) hipLaunchKernelGGL((act_planes_kernel<TF_, X_>), dim3((unsigned)blocks), dim3(256), 0, s, x, x2, n8, C, sc, sh, sc2, amax, fscale, planes, ps, koaf_status_ptr())
    if (tf == 0) { if (act16) KOAF_AP(0, true); else KOAF_AP(0, false); }
    else if (tf == 1) { if (act16) KOAF_AP(1, true); else KOAF_AP(1, false); }
    else { if (act16) KOAF_AP(2, true); else KOAF_AP(2, false); }
#undef KOAF_AP
    return koaf_check_launch("koaf_act_planes");
}
