// koaf_attr.hip -- path attributions over the model's inputs (integrated gradients, SmoothGrad; not in the reference): the J
// modified copies of an input that one model pass consumes, and the weighted sum of the J gradient tensors that comes back.
// Both kernels stream: every operand byte travels once, x and base are read once for all J points, and the fold reads each
// gradient plane once.  Element-wise, no atomics and no cross-thread reduction: the bits do not depend on the grid.  The
// arithmetic is written so that numpy's fp32 restates it bit for bit (koaf.h): every product and sum rounds on its own.
#include "koaf_common.h"

namespace {

constexpr int AT_BLOCK = 256;
constexpr int AT_CHUNK = 4096;          // elements per block: 4 dwordx4 accesses per lane and operand
constexpr int AT_MAX_J = KOAF_ATTR_MAX_J;

// The helpers below keep contraction off: hipcc would otherwise fuse a * b + c, in one function or across inlined ones (both
// instructions need the flag to fuse, and none of these carries it).
__device__ __forceinline__ float at_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float at_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
// c + a * b, the product rounded first
__device__ __forceinline__ float at_muladd(float a, float b, float c) {
#pragma clang fp contract(off)
    const float ab = a * b;
    return c + ab;
}

// ---- the generator (koaf.h: koaf_path_points) ------------------------------------------------------------------------------
// row key of (seed, draw, b); pair hash of (key, i / 2) -> the two standard normals of elements 2p and 2p + 1
__device__ __forceinline__ uint64_t at_row_key(uint64_t seed, uint64_t draw, uint64_t b) {
    return mix64(seed ^ mix64((draw << 32) | b));
}
__device__ __forceinline__ void at_normal_pair(uint64_t key, uint64_t pair_hash, float& z0, float& z1) {
    const uint64_t h = mix64(key ^ pair_hash);
    const float u1 = (float)((uint32_t)(h >> 40) + 1u) * 0x1p-24f;                 // (0, 1]: the logarithm is finite
    const float t = (float)((uint32_t)(h >> 16) & 0xffffffu) * 0x1p-23f;           // 2 u2 in [0, 2): exact
    const float r = sqrtf(at_mul(-2.f, logf(u1)));
    float s, c;
    sincospif(t, &s, &c);                                                          // sin / cos (pi t): no argument reduction
    z0 = at_mul(r, c);
    z1 = at_mul(r, s);
}

// out[j][b][i] = base + alpha[j] * (x - base) (+ sigma_b * z).  Block (c, b) owns elements [c * AT_CHUNK, ...) of row b.
// VEC: rows are 16-byte aligned (n % 4 == 0 and aligned pointers) -- a lane takes 4 elements = 2 generator pairs; else one
// element per lane (the odd one of a pair recomputes its partner's hash: the slow path pays that, the layout stays coalesced).
template <bool VEC, bool NOISE, bool BASE>
__global__ void __launch_bounds__(AT_BLOCK) path_points_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                               float base_value, const float* __restrict__ alpha,
                                                               float* __restrict__ out, int J, int B, int64_t n,
                                                               const float* __restrict__ mm, float noise_level, uint64_t seed,
                                                               int64_t draw0) {
    __shared__ float al[AT_MAX_J];
    __shared__ uint64_t keys[AT_MAX_J];
    const int b = blockIdx.y;
    if ((int)threadIdx.x < J) {
        al[threadIdx.x] = alpha[threadIdx.x];
        if constexpr (NOISE) keys[threadIdx.x] = at_row_key(seed, (uint64_t)(draw0 + threadIdx.x), (uint64_t)b);
    }
    __syncthreads();
    float sigma = 0.f;
    if constexpr (NOISE) sigma = at_mul(noise_level, at_sub(mm[2 * b + 1], mm[2 * b]));
    const int64_t e0 = (int64_t)blockIdx.x * AT_CHUNK, e1 = e0 + AT_CHUNK < n ? e0 + AT_CHUNK : n;
    const int64_t row = (int64_t)b * n, plane = (int64_t)B * n;
    const float* __restrict__ xr = x + row;
    const float* __restrict__ br = BASE ? base + row : nullptr;
    float* __restrict__ orow = out + row;
    if constexpr (VEC) {
#pragma unroll 2
        for (int64_t v = e0 / 4 + threadIdx.x; v < e1 / 4; v += AT_BLOCK) {
            const v4f xv = *(const v4f*)&xr[v * 4];
            v4f bv = {base_value, base_value, base_value, base_value}, d;
            if constexpr (BASE) bv = *(const v4f*)&br[v * 4];
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = at_sub(xv[k], bv[k]);
            uint64_t ph0 = 0, ph1 = 0;
            if constexpr (NOISE) { ph0 = mix64((uint64_t)(2 * v)); ph1 = mix64((uint64_t)(2 * v + 1)); }
            for (int j = 0; j < J; ++j) {
                const float a = al[j];
                v4f r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = at_muladd(a, d[k], bv[k]);
                if constexpr (NOISE) {
                    float z[4];
                    at_normal_pair(keys[j], ph0, z[0], z[1]);
                    at_normal_pair(keys[j], ph1, z[2], z[3]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[k] = at_muladd(sigma, z[k], r[k]);
                }
                __builtin_nontemporal_store(r, (v4f*)&orow[j * plane + v * 4]);      // (written once, read by the model much later)
            }
        }
    } else {
        for (int64_t i = e0 + threadIdx.x; i < e1; i += AT_BLOCK) {
            const float xv = xr[i], bv = BASE ? br[i] : base_value;
            const float d = at_sub(xv, bv);
            uint64_t ph = 0;
            if constexpr (NOISE) ph = mix64((uint64_t)(i >> 1));
            for (int j = 0; j < J; ++j) {
                float r = at_muladd(al[j], d, bv);
                if constexpr (NOISE) {
                    float z0, z1;
                    at_normal_pair(keys[j], ph, z0, z1);
                    r = at_muladd(sigma, (i & 1) ? z1 : z0, r);
                }
                orow[j * plane + i] = r;
            }
        }
    }
}

// one term of the fold: s + w * f(g), f the identity or the square; every operation rounds on its own
__device__ __forceinline__ float at_term(float s, float g, float w, bool sq) {
    return at_muladd(w, sq ? at_mul(g, g) : g, s);
}

// acc[e] (=|+=) sum_j w[j] * f(g[j][e]) over the flat range e in [0, N), N = B * n; FIN 1 / 2: the stored value times
// (x[e] - base_value) / (x[e] - base[e]).  Block c owns elements [c * AT_CHUNK, ...).  VEC: N % 4 == 0 and aligned pointers.
// The gradient planes are read once and never again: their 16-byte loads are non-temporal (measured, DESIGN 3.16: 6.7 against
// 5.4 TB/s with plain loads at J = 4).  w[j] is uniform: a scalar load per plane, no LDS and no barrier in front of the stream.
template <bool VEC, int FIN>
__global__ void __launch_bounds__(AT_BLOCK) attr_fold_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                             const float* __restrict__ w, const float* __restrict__ x,
                                                             const float* __restrict__ base, float base_value, int J, int64_t N,
                                                             int square, int first) {
    const bool sq = square != 0;
    const int64_t e0 = (int64_t)blockIdx.x * AT_CHUNK, e1 = e0 + AT_CHUNK < N ? e0 + AT_CHUNK : N;
    if constexpr (VEC) {
#pragma unroll 2
        for (int64_t v = e0 / 4 + threadIdx.x; v < e1 / 4; v += AT_BLOCK) {
            v4f s = {0.f, 0.f, 0.f, 0.f};
            if (!first) s = *(const v4f*)&acc[v * 4];
#pragma unroll 4
            for (int j = 0; j < J; ++j) {
                const v4f gv = __builtin_nontemporal_load((const v4f*)&g[j * N + v * 4]);
                const float wj = w[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = at_term(s[k], gv[k], wj, sq);
            }
            if constexpr (FIN != 0) {
                const v4f xv = *(const v4f*)&x[v * 4];
                v4f bv = {base_value, base_value, base_value, base_value};
                if constexpr (FIN == 2) bv = *(const v4f*)&base[v * 4];
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = at_mul(s[k], at_sub(xv[k], bv[k]));
            }
            *(v4f*)&acc[v * 4] = s;
        }
    } else {
        for (int64_t i = e0 + threadIdx.x; i < e1; i += AT_BLOCK) {
            float s = first ? 0.f : acc[i];
#pragma unroll 4
            for (int j = 0; j < J; ++j) s = at_term(s, g[j * N + i], w[j], sq);
            if constexpr (FIN != 0) s = at_mul(s, at_sub(x[i], FIN == 2 ? base[i] : base_value));
            acc[i] = s;
        }
    }
}

}  // namespace

extern "C" int koaf_path_points(const float* x, const float* base, float base_value, const float* alpha, float* out, int32_t J,
                                int32_t B, int64_t n, const float* mm, float noise_level, uint64_t seed, int64_t draw0,
                                void* stream) {
    KOAF_REQUIRE(J >= 1 && J <= AT_MAX_J, "koaf_path_points: 1 <= J <= %d (J = %d)", AT_MAX_J, J);
    KOAF_REQUIRE(B >= 1 && B <= 65535, "koaf_path_points: 1 <= B <= 65535 (B = %d)", B);
    KOAF_REQUIRE(n >= 1 && n < (1ll << 40), "koaf_path_points: 1 <= n < 2^40 (n = %lld)", (long long)n);
    KOAF_REQUIRE(x && alpha && out, "koaf_path_points: x, alpha and out are required");
    KOAF_REQUIRE(draw0 >= 0 && draw0 + J <= (1ll << 31), "koaf_path_points: draw indices lie in [0, 2^31)");
    const bool noise = mm != nullptr && noise_level != 0.f;
    const bool vec = n % 4 == 0 && aligned16(x) && aligned16(out) && (!base || aligned16(base));
    const dim3 grid((unsigned)cdiv64(n, AT_CHUNK), (unsigned)B), block(AT_BLOCK);
#define KOAF_PP(V, Z, T)                                                                                                     \
    hipLaunchKernelGGL((path_points_kernel<V, Z, T>), grid, block, 0, STREAM, x, base, base_value, alpha, out, J, B, n, mm,   \
                       noise_level, seed, draw0)
#define KOAF_PP2(V, Z) do { if (base) KOAF_PP(V, Z, true); else KOAF_PP(V, Z, false); } while (0)
    if (vec && noise) KOAF_PP2(true, true);
    else if (vec) KOAF_PP2(true, false);
    else if (noise) KOAF_PP2(false, true);
    else KOAF_PP2(false, false);
#undef KOAF_PP2
#undef KOAF_PP
    return koaf_check_launch("koaf_path_points");
}

extern "C" int koaf_attr_fold(float* acc, const float* g, const float* w, const float* x, const float* base, float base_value,
                              int32_t J, int32_t B, int64_t n, int32_t square, int32_t first, int32_t finish, void* stream) {
    KOAF_REQUIRE(J >= 1 && J <= AT_MAX_J, "koaf_attr_fold: 1 <= J <= %d (J = %d)", AT_MAX_J, J);
    KOAF_REQUIRE(B >= 1, "koaf_attr_fold: B >= 1 (B = %d)", B);
    KOAF_REQUIRE(n >= 1 && n < (1ll << 40), "koaf_attr_fold: 1 <= n < 2^40 (n = %lld)", (long long)n);
    KOAF_REQUIRE(acc && g && w, "koaf_attr_fold: acc, g and w are required");
    KOAF_REQUIRE(!finish || x, "koaf_attr_fold: finish needs x");
    const int64_t N = (int64_t)B * n;
    KOAF_REQUIRE(cdiv64(N, AT_CHUNK) < (1ll << 31), "koaf_attr_fold: range too long");
    const int fin = !finish ? 0 : base ? 2 : 1;
    const bool vec = N % 4 == 0 && aligned16(acc) && aligned16(g) && (fin == 0 || aligned16(x)) && (fin != 2 || aligned16(base));
    const dim3 grid((unsigned)cdiv64(N, AT_CHUNK)), block(AT_BLOCK);
#define KOAF_AF(V, F) hipLaunchKernelGGL((attr_fold_kernel<V, F>), grid, block, 0, STREAM, acc, g, w, x, base, base_value, J, N, square, first)
    if (vec) { if (fin == 0) KOAF_AF(true, 0); else if (fin == 1) KOAF_AF(true, 1); else KOAF_AF(true, 2); }
    else { if (fin == 0) KOAF_AF(false, 0); else if (fin == 1) KOAF_AF(false, 1); else KOAF_AF(false, 2); }
#undef KOAF_AF
    return koaf_check_launch("koaf_attr_fold");
}
