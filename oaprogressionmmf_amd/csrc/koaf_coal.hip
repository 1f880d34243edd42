// koaf_coal.hip -- modality coalitions (not in the reference): the final FeaT's input tokens of a chunk of coalitions,
// spliced from the tokens of the intact inputs and of the baselines, and the Shapley values, pair interactions, leave-one-out and
// stand-alone differences of the 2^M coalition values.  The splice is a copy; the fold sums in fp64 in a fixed order, one thread
// per output element, no atomics -- the bits do not depend on the grid (koaf.h).
#include <limits.h>

#include "koaf_common.h"

namespace {

constexpr int CO_BLOCK = 256;
constexpr int CO_CHUNK = 4096;          // elements per block of the splice: 4 dwordx4 accesses per lane
constexpr int CO_UNITS = CO_CHUNK / 4 / CO_BLOCK;
constexpr int CO_MAX_M = KOAF_COAL_MAX_M;
constexpr int CO_MAX_J = KOAF_COAL_MAX_J;

// the inner segment bounds seg_off[1 .. M - 1], padded with INT_MAX: seg(l) = the number of bounds <= l
struct CoSeg { int off[CO_MAX_M - 1]; };
struct CoMasks { uint32_t m[CO_MAX_J]; };
struct CoWeights { double phi[CO_MAX_M], inter[CO_MAX_M]; };

__device__ __forceinline__ unsigned co_bit(const CoSeg& sg, int l) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < CO_MAX_M - 1; ++i) s += l >= sg.off[i] ? 1 : 0;
    return 1u << s;
}

// out[j][b][e] = (masks[j] & bit(e / D)) ? tx[b][e] : t0[b % B0][e] over the n = L * D elements of a sample.  Block (c, b) owns
// elements [c * CO_CHUNK, ...) of sample b; the J masks sit in LDS.  VEC: n % 4 == 0 and aligned pointers -- a lane takes 4
// elements, which may lie in two or more tokens (D % 4 != 0); else one element per lane.
template <bool VEC>
__global__ void __launch_bounds__(CO_BLOCK) coal_tokens_kernel(const float* __restrict__ tx, const float* __restrict__ t0,
                                                               float* __restrict__ out, int J, int B, int B0, int n, int D, CoSeg sg,
                                                               CoMasks mk) {
    __shared__ unsigned msk[CO_MAX_J];
    if ((int)threadIdx.x < J) msk[threadIdx.x] = mk.m[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const int e0 = blockIdx.x * CO_CHUNK, e1 = min(e0 + CO_CHUNK, n);
    const int64_t plane = (int64_t)B * n;
    const float* __restrict__ xr = tx + (int64_t)b * n;
    const float* __restrict__ br = t0 + (int64_t)(b % B0) * n;
    float* __restrict__ orow = out + (int64_t)b * n;
    if constexpr (VEC) {
        // all of a lane's loads are issued before its first store: CO_UNITS independent 16-byte pairs in flight per lane
        v4f xv[CO_UNITS], bv[CO_UNITS];
#pragma unroll
        for (int q = 0; q < CO_UNITS; ++q) {
            const int v = e0 / 4 + q * CO_BLOCK + threadIdx.x;
            if (v < e1 / 4) { xv[q] = *(const v4f*)&xr[v * 4]; bv[q] = *(const v4f*)&br[v * 4]; }
        }
#pragma unroll
        for (int q = 0; q < CO_UNITS; ++q) {
            const int v = e0 / 4 + q * CO_BLOCK + threadIdx.x;
            if (v >= e1 / 4) break;
            int l = v * 4 / D, c = v * 4 - l * D;
            unsigned bit[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bit[u] = co_bit(sg, l);
                if (++c == D) { c = 0; ++l; }
            }
            for (int j = 0; j < J; ++j) {
                const unsigned m = msk[j];
                v4f r;
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = (m & bit[u]) ? xv[q][u] : bv[q][u];
                *(v4f*)&orow[j * plane + v * 4] = r;          // (read back by the FeaT right away: a plain store)
            }
        }
    } else {
        for (int i = e0 + threadIdx.x; i < e1; i += CO_BLOCK) {
            const float xv = xr[i], bv = br[i];
            const unsigned bit = co_bit(sg, i / D);
            for (int j = 0; j < J; ++j) orow[j * plane + i] = (msk[j] & bit) ? xv : bv;
        }
    }
}

// thread t = (b, r): r < M * M the interaction (i, j), then M each of phi, loo, solo.  Subsets in ascending mask order.
__global__ void __launch_bounds__(CO_BLOCK) shapley_fold_kernel(const float* __restrict__ v, double* __restrict__ phi,
                                                                double* __restrict__ inter, double* __restrict__ loo,
                                                                double* __restrict__ solo, int S, int B, int M, CoWeights w) {
    __shared__ double wp[CO_MAX_M], wi[CO_MAX_M];
    if (threadIdx.x < CO_MAX_M) { wp[threadIdx.x] = w.phi[threadIdx.x]; wi[threadIdx.x] = w.inter[threadIdx.x]; }
    __syncthreads();
    const int per = M * (M + 3);
    const int t = blockIdx.x * CO_BLOCK + threadIdx.x;
    if (t >= B * per) return;
    const int b = t / per;
    int r = t - b * per;
    const unsigned full = (unsigned)S - 1u;
#define CO_V(s) ((double)v[(int64_t)(s) * B + b])
    if (r < M * M) {
        const int i = r / M, j = r - i * M;
        const unsigned bi = 1u << i, bj = 1u << j;
        double acc = 0.0;
        if (i != j)
            for (unsigned s = 0; s <= full; ++s) {
                if (s & (bi | bj)) continue;
                const double d = CO_V(s | bi | bj) - CO_V(s | bi) - CO_V(s | bj) + CO_V(s);
                acc += wi[__popc(s)] * d;
            }
        inter[((int64_t)b * M + i) * M + j] = acc;
        return;
    }
    r -= M * M;
    const int kind = r / M, i = r - kind * M;
    const unsigned bi = 1u << i;
    const int64_t o = (int64_t)b * M + i;
    if (kind == 0) {
        double acc = 0.0;
        for (unsigned s = 0; s <= full; ++s) {
            if (s & bi) continue;
            acc += wp[__popc(s)] * (CO_V(s | bi) - CO_V(s));
        }
        phi[o] = acc;
    } else if (kind == 1) {
        loo[o] = CO_V(full) - CO_V(full & ~bi);
    } else {
        solo[o] = CO_V(bi) - CO_V(0u);
    }
#undef CO_V
}

}  // namespace

extern "C" int koaf_coal_tokens(const float* tx, const float* t0, const int32_t* seg_off, const uint32_t* masks, float* out, int32_t J,
                                int32_t B, int32_t B0, int32_t L, int32_t D, int32_t M, void* stream) {
    KOAF_REQUIRE(M >= 1 && M <= CO_MAX_M, "koaf_coal_tokens: 1 <= M <= %d (M = %d)", CO_MAX_M, M);
    KOAF_REQUIRE(tx && t0 && seg_off && masks && out, "koaf_coal_tokens: tx, t0, seg_off, masks and out are required");
    KOAF_REQUIRE(J >= 1 && L >= 1 && D >= 1, "koaf_coal_tokens: J, L, D >= 1 (J = %d, L = %d, D = %d)", J, L, D);
    KOAF_REQUIRE(B >= 1 && B <= 65535 && (B0 == 1 || B0 == B), "koaf_coal_tokens: 1 <= B <= 65535 and B0 is 1 or B (B = %d, B0 = %d)", B, B0);
    KOAF_REQUIRE((int64_t)L * D < (1ll << 31), "koaf_coal_tokens: L * D stays below 2^31 (L = %d, D = %d)", L, D);
    KOAF_REQUIRE(seg_off[0] == 0 && seg_off[M] == L, "koaf_coal_tokens: seg_off runs from 0 to L = %d, got %d to %d", L, seg_off[0], seg_off[M]);
    CoSeg sg;
    for (int i = 0; i < CO_MAX_M - 1; ++i) sg.off[i] = INT_MAX;
    for (int i = 0; i < M; ++i) {
        KOAF_REQUIRE(seg_off[i] < seg_off[i + 1], "koaf_coal_tokens: seg_off ascends strictly (seg_off[%d] = %d, seg_off[%d] = %d)", i,
                     seg_off[i], i + 1, seg_off[i + 1]);
        if (i > 0) sg.off[i - 1] = seg_off[i];
    }
    for (int j = 0; j < J; ++j)
        KOAF_REQUIRE((masks[j] >> M) == 0u, "koaf_coal_tokens: masks[%d] = 0x%x has a bit at or above M = %d", j, masks[j], M);
    const int n = L * D;
    const bool vec = n % 4 == 0 && aligned16(tx) && aligned16(t0) && aligned16(out);
    const dim3 grid((unsigned)cdiv64(n, CO_CHUNK), (unsigned)B), block(CO_BLOCK);
    for (int j0 = 0; j0 < J; j0 += CO_MAX_J) {              // the masks travel as kernel arguments, CO_MAX_J a launch
        const int Jc = J - j0 < CO_MAX_J ? J - j0 : CO_MAX_J;
        CoMasks mk = {};
        for (int j = 0; j < Jc; ++j) mk.m[j] = masks[j0 + j];
        float* o = out + (int64_t)j0 * B * n;
        if (vec) hipLaunchKernelGGL(coal_tokens_kernel<true>, grid, block, 0, STREAM, tx, t0, o, Jc, B, B0, n, D, sg, mk);
        else hipLaunchKernelGGL(coal_tokens_kernel<false>, grid, block, 0, STREAM, tx, t0, o, Jc, B, B0, n, D, sg, mk);
    }
    return koaf_check_launch("koaf_coal_tokens");
}

extern "C" int koaf_shapley_fold(const float* v, const double* w_phi, const double* w_int, double* phi, double* inter, double* loo,
                                 double* solo, int32_t S, int32_t B, int32_t M, void* stream) {
    KOAF_REQUIRE(M >= 1 && M <= CO_MAX_M, "koaf_shapley_fold: 1 <= M <= %d (M = %d)", CO_MAX_M, M);
    KOAF_REQUIRE(S == (1 << M), "koaf_shapley_fold: v holds S = 2^M coalitions (S = %d, M = %d)", S, M);
    KOAF_REQUIRE(B >= 1 && B <= (1 << 20), "koaf_shapley_fold: 1 <= B <= 2^20 (B = %d)", B);
    KOAF_REQUIRE(v && w_phi && (w_int || M == 1) && phi && inter && loo && solo, "koaf_shapley_fold: v, the weights and the four outputs are required");
    CoWeights w = {};
    for (int t = 0; t < M; ++t) w.phi[t] = w_phi[t];
    for (int t = 0; t + 1 < M; ++t) w.inter[t] = w_int[t];
    const int total = B * M * (M + 3);
    hipLaunchKernelGGL(shapley_fold_kernel, dim3((unsigned)cdiv64(total, CO_BLOCK)), dim3(CO_BLOCK), 0, STREAM, v, phi, inter, loo, solo, S,
                       B, M, w);
    return koaf_check_launch("koaf_shapley_fold");
}
