// koaf_tile256.h -- the 256-row tile schedule that the dedicated convolution kernels of the fp16 scheme share (koaf_wgrad1.hip,
// koaf_fwd_s2.hip, koaf_dgrad_s2.hip, koaf_fwd1.hip), written once: a unit brings its loader and its epilogue.
// The generic kernel (koaf_gemm_kernel) runs these calls on 128 x 128 tiles with ONE LDS image per operand and two block barriers per
// 32-k step: the transform, the piece split and the LDS store sit between the barriers with the matrix pipe idle.  Here a block of 512
// threads (waves 4 x 2) owns a 256 x 256 tile (256 x 128 / 128 x 256 where a dimension is no multiple of 256) -- half the conversions
// and half the L2 reads per operand element -- with two LDS stages per operand and one barrier per k-step:
//     step s:  MFMAs of k-tile s (stage s % 2)  ||  transform + split + store of k-tile s + 1 (registers -> stage (s + 1) % 2),
//              each register unit refilled with its loads of k-tile s + 2 as soon as it is stored
// so a load has a whole k-step to land and the vector work runs in the shadow of the matrix instructions (its own wave's and those of
// the second wave on the SIMD).  Register slots are static (one k-tile in registers, unit by unit); the loads behind the end of the
// k-range are issued unconditionally, into registers whose conversion nobody reads.  Every wave executes every barrier; there is no
// role split, no spin-wait and no hand-off between blocks.
// The bit-identity contract with koaf_gemm_kernel lives here: the transform expressions, scale and split2h of TileLoader::finish_unit
// (t256_finish4, t256_store_kc_unit); the k-tile order and the three piece products per accumulator and 16-k slice of mma()
// (T256_KSTEP); alpha * acc, the + 0 of the zero bias and the statistics tree of the shared epilogue, written as TWO partial rows per
// tile, one per 128-row half, where a 128-row tiling puts them (T256_FWD_EPILOGUE).
// LDS images (koaf_pieces.h): the row-major kernels keep A as plane[row][32 k + 8 pad] and B as the swizzled rows PlaneLoader writes
// (T256FragRow); B travels through registers like A (T256PlaneB), so that hipcc counts every load in flight itself.  The weight
// gradient keeps both operands K-major, plane[k][ROWS + 32 pad] (T256FragKM).
// These kernels have no register to spare, and a piece that is shared must compile like the text it replaced:
// scripts/compare_kernels.py against the tree before a change decides (DESIGN 3.11 has the verdict per piece, and the pieces that
// stayed in the units because they did not).
#pragma once
#include "koaf_pieces.h"

namespace {

constexpr int T256_NT = 512;
constexpr int T256_BM = 256;             // the row-major kernels' tile height
constexpr int T256_TAB_C = 1024;         // forward, tf 1: channels the coefficient table in LDS holds

// block -> slot of the tile order: koaf_gemm_kernel's XCD remap (XCD = block id % 8 works through one contiguous chunk of the order)
__device__ __forceinline__ unsigned t256_xcd_slot(unsigned ntx, unsigned v) {
    const unsigned q = ntx >> 3, rem = ntx & 7, x = v & 7, j = v >> 3;
    return x * q + (x < rem ? x : rem) + j;
}

// end of a k-step: every wave is done reading this stage and has written its part of the next (the loads stay in flight)
__device__ __forceinline__ void t256_lgkm0_barrier() {
    // (the wait is the BUILTIN: hipcc's wait-count pass does not read inline assembly)
    __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
    asm volatile("s_barrier" ::: "memory");
}

// where the k-step finds its fragments: piece plane q of a stage's A / B image, 32 rows from row0, 16-k slice g
template <int BM, int BN>
struct T256FragRow {      // A K-contiguous, B PlaneLoader's swizzled rows
    static constexpr int A_PL = plane_dwords(BM, true), B_PL = BN * 16;
    static __device__ __forceinline__ v4i a(const unsigned* A, int q, int row0, int g, int lane) { return frag_load<BM, true>(A + q * A_PL, row0, g, lane); }
    static __device__ __forceinline__ v4i b(const unsigned* B, int q, int row0, int g, int lane) { return frag_load_ps(B + q * B_PL, row0, g, lane); }
};
template <int BM, int BN>
struct T256FragKM {       // both K-major
    static constexpr int A_PL = plane_dwords(BM, false), B_PL = plane_dwords(BN, false);
    static __device__ __forceinline__ v4i a(const unsigned* A, int q, int row0, int g, int lane) { return frag_load<BM, false>(A + q * A_PL, row0, g, lane); }
    static __device__ __forceinline__ v4i b(const unsigned* B, int q, int row0, int g, int lane) { return frag_load<BN, false>(B + q * B_PL, row0, g, lane); }
};

// The k-step and the forward epilogue are TEXT, not functions.  hipcc optimises a forced-inline function on its own before it inlines
// it, and these two come out of that with other address arithmetic, other merged LDS accesses and other wait counts than the same lines
// standing in the kernel: with every piece of this header a function template, all 42 kernels of the four units moved, 31 of them in
// resources or work (DESIGN 3.11 has the figures); as text the kernels keep their machine code.
//
// T256_KSTEP(F, UNITS, UNIT): the MFMAs of the stage at (Au, Bu) -- per accumulator the order of koaf_gemm_kernel's mma(): 16-k slice g,
// then lo*hi, hi*lo, hi*hi -- with the NUT units of the next k-tile, the statement UNIT for u = 0 .. NUT - 1, dealt out behind its MFMA
// groups (16-k slice x column tile); UNITS false: a k-step without vector work.  F: the fragment policy.  From the scope it stands
// in: TM, TN, NUT (constants), acc[TM][TN], const unsigned *Au, *Bu, wm, wn, lane.
#define T256_KSTEP(F, UNITS, UNIT)                                                                                                        \
    _Pragma("unroll") for (int g = 0; g < 2; ++g) {                                                                                       \
        v4i ap[TM][2];                                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                                    \
            _Pragma("unroll") for (int q = 0; q < 2; ++q) ap[i][q] = F::a(Au, q, wm * (32 * TM) + 32 * i, g, lane);                       \
        _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                                                                               \
            v4i bp[2];                                                                                                                    \
            _Pragma("unroll") for (int q = 0; q < 2; ++q) bp[q] = F::b(Bu, q, wn * (32 * TN) + 32 * jn, g, lane);                         \
            constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};                                                                         \
            _Pragma("unroll") for (int term = 0; term < 3; ++term)                                                                        \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                            \
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, ap[i][PAH[term]]),                      \
                                                                        __builtin_bit_cast(h16x8, bp[PBH[term]]), acc[i][jn], 0, 0, 0);   \
            if constexpr (UNITS) {                                                                                                        \
                const int grp = g * TN + jn;                                                                                              \
                _Pragma("unroll") for (int u = 0; u < NUT; ++u)                                                                           \
                    if (u * (2 * TN) / NUT == grp) { UNIT; }                                                                              \
                /* the scheduler keeps each group's MFMAs, vector work and loads where they are written (only fragment reads and */      \
                /* scalar work may cross): left free, it sinks every global load to the end of the step, in front of its first use */    \
                __builtin_amdgcn_sched_barrier(0x104);                                                                                    \
            }                                                                                                                             \
        }                                                                                                                                 \
    }

// TileLoader::finish_unit's arithmetic for four values: TF 0  x sca;  TF 1  relu(ca x + cb);  TF 2  the two-source apply
// ca x + cb - ck x2 (coefficients already scaled), clamped to the fp16 range; a unit that is not ok (padding, behind the k-range) is
// zeroed BEHIND the transform
template <int TF>
__device__ __forceinline__ v4f t256_finish4(const v4f x, const v4f x2, const v4f ca, const v4f cb, const v4f ck, float sca, bool ok = true) {
    constexpr float HMAX = 65504.f;
    v4f v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y = x[j];
        if constexpr (TF == 1) {
            y = fmaf(y, ca[j], cb[j]);
            y = __builtin_amdgcn_fmed3f(y, 0.f, HMAX);
        } else if constexpr (TF == 2) {
            y = fmaf(ca[j], y, fmaf(-ck[j], x2[j], cb[j]));
            y = __builtin_amdgcn_fmed3f(y, -HMAX, HMAX);
        } else {
            y = __builtin_amdgcn_fmed3f(y * sca, -HMAX, HMAX);
        }
        v[j] = ok ? y : 0.f;
    }
    return v;
}

template <int TF>      // (the one-source transforms)
__device__ __forceinline__ v4f t256_finish4(const v4f x, const v4f ca, const v4f cb, float sca, bool ok = true) {
    static_assert(TF != 2, "the apply has a second source");
    return t256_finish4<TF>(x, x, ca, cb, cb, sca, ok);
}

// split2h + the store of TileLoader::store into the K-contiguous image at S (plane stride A_PL): k = 4 kq .. 4 kq + 3 of `row`.
// WATCH: TileLoader::store's saturation watch (tf 1) between the two -- satmax keeps the largest hi pieces of the live units, two fp16
// per word; a kernel whose satmax reaches the clamp 0x7bff in either half counts one saturated tile in status word 0
template <bool WATCH>
__device__ __forceinline__ void t256_store_kc_unit(unsigned* S, int A_PL, unsigned row, unsigned kq, const v4f v, unsigned& satmax, bool live) {
    unsigned pl[2][2];
    split2h(v, pl);
    if constexpr (WATCH) {
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int d = 0; d < 2; ++d)
            satmax = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, satmax),
                                                                             __builtin_bit_cast(u16x2, live ? pl[0][d] : 0u)));
    }
    const unsigned off = row * 20u + 2u * kq;
#pragma unroll
    for (int q = 0; q < 2; ++q) *(uint2*)&S[q * A_PL + off] = make_uint2(pl[q][0], pl[q][1]);
}
__device__ __forceinline__ void t256_store_kc_unit(unsigned* S, int A_PL, unsigned row, unsigned kq, const v4f v) {
    unsigned none = 0u;
    t256_store_kc_unit<false>(S, A_PL, row, kq, v, none, false);
}

// B from a plane image [2][rows][K] through registers: BN / 64 units per thread and k-tile = 16 B (8 k) of plane u % 2, row
// t / 4 + 128 (u / 2).  The source address is the caller's: plane (u & 1), row 128 (u >> 1) + t / 4, element 8 (t % 4) of the k-tile
template <int BN>
struct T256PlaneB {
    static constexpr int NU = BN / 64, PL = BN * 16;
    v4i rb[NU];
    __device__ __forceinline__ void issue(int u, const unsigned short* src) { rb[u] = *(const v4i*)src; }
    // (b0: B's image in the stage at S; bdst: PlaneLoader's swizzled dword of this thread's chunk, (t / 4) * 16 + 4 * ((t % 4) ^ ((t / 16) % 4)))
    __device__ __forceinline__ void store(int u, unsigned* S, int b0, unsigned bdst) { *(v4i*)&S[b0 + (u & 1) * PL + (u >> 1) * (128 * 16) + bdst] = rb[u]; }
};

// position of a k-tile in the (tap, channel) order of a gathered operand (block-uniform), k0 its first k; past the last tile it
// wraps to k = 0
struct TapWalk {
    int kh, kw, coff, k0;
    __device__ __forceinline__ void next(int C, int nkh, int nkw) {
        coff += BK; k0 += BK;
        if (coff >= C) {
            coff = 0;
            if (++kw == nkw) { kw = 0; ++kh; }
            if (kh == nkh) { kh = 0; k0 = 0; }
        }
    }
};

// what the forward kernels (koaf_fwd1.hip, koaf_fwd_s2.hip) take from a descriptor alike; the dimensions follow in each kernel's own
// struct, where they were, so that no kernel argument moves
struct T256FwdParams {
    const float* x;             // A, fp32
    const float* sc;            // tf 1: in_sc / in_sh per input channel
    const float* sh;
    float a_scale;              // scale of A (fixed)
    const unsigned short* wf;   // F image: plane q at wf + q * w_ps, row co at co * w_ld
    int64_t w_ps, w_ld;
    const float* w_amax;        // scale of B = scale_of_amax(*w_amax)
    float alpha;
    float* y;                   // [M][N]
    float* stats;               // [M / 128][2][stats_ld] or null
    const float* shift;         // per-column shift of the statistics or null
    int64_t stats_ld;
    uint32_t* status;
};

// T256_FWD_EPILOGUE(BN, RELEASE): the forward epilogue with statistics, koaf_gemm_kernel's, the tile as two 128-row halves (waves
// wm = 2 hh, 2 hh + 1 are the 2 x 2 waves of half hh) through a staging half in smem.  All waves passed the k-loop's last barrier:
// the operand stages are dead.  RELEASE: the stages are written again behind the epilogue -- only when every wave has read the sums.
// From the scope it stands in: TM, TN (constants), smem, acc[TM][TN], alpha, the tile (tm, m0, n0), the kernel's parameters p
// (T256FwdParams and N, part_row0), do_stats = p.stats != nullptr, and the thread's indices te (its number), wm, wn, r = lane % 32,
// h = lane / 32.
#define T256_FWD_EPILOGUE(BN, RELEASE)                                                                                                    \
    {                                                                                                                                     \
        constexpr int LDC_S = BN + 4;      /* staging row (floats), 128 rows at a time */                                                 \
        float* Cs = reinterpret_cast<float*>(smem);                                                                                       \
        constexpr int C4 = BN / 4, RPP = T256_NT / C4;                                                                                    \
        const int c4 = te % C4, rr = te / C4;                                                                                             \
        float s1[TM][TN], s2[TM][TN], kshift[TN];                                                                                         \
        _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                                                                               \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) s1[i][jn] = s2[i][jn] = 0.f;                                                   \
            kshift[jn] = (do_stats && p.shift) ? p.shift[n0 + wn * (32 * TN) + 32 * jn + r] : 0.f;                                        \
        }                                                                                                                                 \
        v4f bv = {0.f, 0.f, 0.f, 0.f};                                                                                                    \
        asm volatile("" : "+v"(bv));       /* (the zero bias the shared epilogue adds: -0 becomes +0) */                                  \
        _Pragma("unroll") for (int hh = 0; hh < 2; ++hh) {                                                                                \
            if ((wm >> 1) == hh) {                                                                                                        \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                            \
                    _Pragma("unroll") for (int jn = 0; jn < TN; ++jn)                                                                     \
                        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                  \
                            const float v = alpha * acc[i][jn][e];                                                                        \
                            s1[i][jn] += v - kshift[jn];                                                                                  \
                            s2[i][jn] = fmaf(v - kshift[jn], v - kshift[jn], s2[i][jn]);                                                  \
                            Cs[((wm & 1) * (32 * TM) + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) * LDC_S + wn * (32 * TN) + 32 * jn + r] = v; \
                        }                                                                                                                 \
            }                                                                                                                             \
            __syncthreads();                                                                                                              \
            float* const Yp = p.y + (int64_t)(m0 + 128 * hh) * p.N + n0 + 4 * c4;                                                         \
            _Pragma("unroll 4") for (int row = rr; row < 128; row += RPP) {                                                               \
                const v4f v = *(const v4f*)&Cs[row * LDC_S + 4 * c4] + bv;                                                                \
                __builtin_nontemporal_store(v, (v4f*)(Yp + (int64_t)row * p.N));                                                          \
            }                                                                                                                             \
            __syncthreads();                                                                                                              \
        }                                                                                                                                 \
        if (do_stats) {                                                                                                                   \
            /* column sums: lanes (r, 0) + (r, 1) over the wave's two bands, then the two waves of each 128-row half */                   \
            float* red = Cs;               /* [4][2][BN] */                                                                               \
            _Pragma("unroll") for (int jn = 0; jn < TN; ++jn) {                                                                           \
                float a1 = s1[0][jn] + __shfl_xor(s1[0][jn], 32, 64);                                                                     \
                float a2 = s2[0][jn] + __shfl_xor(s2[0][jn], 32, 64);                                                                     \
                _Pragma("unroll") for (int i = 1; i < TM; ++i) {                                                                          \
                    a1 += s1[i][jn] + __shfl_xor(s1[i][jn], 32, 64);                                                                      \
                    a2 += s2[i][jn] + __shfl_xor(s2[i][jn], 32, 64);                                                                      \
                }                                                                                                                         \
                if (h == 0) {                                                                                                             \
                    red[(wm * 2 + 0) * BN + wn * (32 * TN) + 32 * jn + r] = a1;                                                           \
                    red[(wm * 2 + 1) * BN + wn * (32 * TN) + 32 * jn + r] = a2;                                                           \
                }                                                                                                                         \
            }                                                                                                                             \
            __syncthreads();                                                                                                              \
            if (te < 2 * BN) {                                                                                                            \
                const int hh = te / BN, c = te % BN;                                                                                      \
                float a1 = red[(4 * hh + 0) * BN + c], a2 = red[(4 * hh + 1) * BN + c];                                                   \
                a1 += red[(4 * hh + 2) * BN + c];                                                                                         \
                a2 += red[(4 * hh + 3) * BN + c];                                                                                         \
                float* st = p.stats + (int64_t)(p.part_row0 + 2 * tm + hh) * 2 * p.stats_ld;                                              \
                st[n0 + c] = a1;                                                                                                          \
                st[p.stats_ld + n0 + c] = a2;                                                                                             \
            }                                                                                                                             \
            if constexpr (RELEASE) __syncthreads();                                                                                       \
        }                                                                                                                                 \
    }

// ---- host side ----

// what koaf_fwd1 and koaf_fwd_s2 both require of a descriptor: the fp16 scheme on fp32 tensors, A fp32 with tf 0 | 1 at a fixed scale (no
// plane-image input, no tail), B the F plane image, a plain output with optional statistics (no emission), whole tiles and k-tiles,
// 16-B aligned pointers
inline bool t256_fwd_args_ok(const KoafGemm& g) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    return g.fmt == 1 && g.act16 == 0 && A.kind == 0 && A.ptr && !A.ptr2 && !A.amax &&
           (A.tf == 0 || (A.tf == 1 && A.sc && A.sh && aligned16(A.sc) && aligned16(A.sh))) &&
           B.kind == 2 && B.gather == 0 && B.planes && B.amax && !B.tf && g.C && g.ldc == g.N && g.splitk <= 1 && g.nb0 * g.nb1 <= 1 &&
           !g.bias && !g.residual && !g.cmap && !g.bnb_mode && !g.out_planes && g.m_base == 0 && g.stats_bs == 0 &&
           g.M % T256_BM == 0 && g.N % 128 == 0 && g.K % BK == 0 && B.ld == g.K &&
           aligned16(A.ptr) && aligned16(B.planes) && aligned16(g.C);
}
inline void t256_fwd_params(const KoafGemm& g, T256FwdParams& p) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    p.x = A.ptr; p.sc = A.sc; p.sh = A.sh;
    p.a_scale = A.fscale != 0.f ? A.fscale : 1.f;
    p.wf = B.planes; p.w_ps = B.plane_stride; p.w_ld = B.ld; p.w_amax = B.amax;
    p.alpha = g.alpha;
    p.y = g.C;
    p.stats = g.stats; p.shift = g.stats ? g.stats_shift : nullptr; p.stats_ld = g.stats_ld ? g.stats_ld : g.N;
    p.status = g.status ? g.status : koaf_status_ptr();
}
// tile width of the row-major kernels; the launch record of a call on bm x bn tiles
inline int t256_bn(int N) { return (N % 256) == 0 ? 256 : 128; }
inline void t256_log_launch(const char* variant, const KoafGemm& g, int bm, int bn, dim3 grid, dim3 launched) {
    KoafGemm rec = g;
    rec.bm = bm; rec.bn = bn;
    koaf_log_launch(variant, rec, grid, launched);
}

}  // namespace
