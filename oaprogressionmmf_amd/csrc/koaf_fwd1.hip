// koaf_fwd1.hip -- forward pass of the dense 1x1 / stride-1 / pad-0 convolutions on 256-row tiles:
//     y[m][co] = sum_k x~[m][k] * w[co][k]       m = pixel, k = input channel
// with x fp32 in HBM at pixel stride Cin (tf 0 plain, tf 1 relu(in_sc x + in_sh), formed on load) and the weights from the F plane image
// [2][Cout][K] (KoafWImg.f).  fp16 scheme only (KoafGemm.fmt 1: two pieces per value, three MFMAs per product).
// The streamed kernel (koaf_gemm_kernel, A mode 13) runs these calls on 128 x 128 tiles; a tile's load, convert, multiply and store
// phases follow one another there.  Here fwd_s2_kernel's schedule (koaf_fwd_s2.hip, itself wgrad1_kernel::step's) without its gather --
// row = pixel, so there is no tap walk and no padding mask: a block of 512 threads (waves 4 x 2) owns a 256 x 256 tile (256 x 128 where
// Cout is no multiple of 256) with two LDS stages of both operands and one barrier per k-step:
//     step s:  MFMAs of k-tile s (stage s % 2)  ||  transform + split + store of A's k-tile s + 1 and the store of B's (registers ->
//              stage (s + 1) % 2), each register unit refilled with its loads of k-tile s + 2 as soon as it is stored
// Register slots are static.  Addresses are a block-uniform base plus one 32-bit offset per thread and operand.
// Two forms:
//   WALK 0  one tile per block (koaf_fwd_s2's grid and XCD remap); the loads behind the end of K are issued unconditionally (the walk
//           wraps to k = 0) into registers whose conversion nobody reads.
//   WALK 1  a persistent block (grid = min(tiles, 256)) walks a contiguous run of the tile order, column tiles fastest, so consecutive
//           tiles share their A rows.  The units stored in a tile's last-but-one k-step are refilled with the NEXT tile's first k-tile;
//           the last k-step has no vector work, the loads land under the epilogue and are converted into stage 0 once the epilogue has
//           released the stages.  A block's last tile prefetches its own first k-tile again (in bounds, unused).  K >= 64: the
//           last-but-one step exists.  Every trip count is block-uniform and every wave executes every barrier; there is no role split,
//           no spin-wait, no hand-off between blocks and no flag in memory.
// LDS images: A = plane[row][32 k + 8 pad] (koaf_pieces.h, fragments by frag_load<.., true>), B = the swizzled rows PlaneLoader writes
// (frag_load_ps); B travels through registers like A, so that hipcc counts every load in flight itself.
// Same bits as koaf_gemm_kernel on the same descriptor: transform expressions, scale and split2h; k-tile order and the three piece
// products per accumulator and 16-k slice; alpha * acc and the + 0 of the zero bias; the statistics tree of the shared epilogue, written
// as TWO partial rows per tile, one per 128-row half, where a 128-row tiling puts them (tests/test_fwd1_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "koaf.h"
#include "koaf_pieces.h"

namespace {
struct F1Params {
    const float* x;             // [M][K]
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
    int M, N, K;
    int tiles;                  // (M / 256) (N / BN)
    int part_row0;
};

constexpr int F1_NT = 512;
constexpr int F1_BM = 256;
constexpr int F1_TAB_C = 1024;           // tf 1: channels the coefficient table holds
constexpr int F1_CUS = 256;              // WALK 1: one block per CU

template <int BN, int TF, int WALK>
__global__ void __launch_bounds__(F1_NT) fwd1_kernel(const F1Params p) {
    constexpr int BM = F1_BM, WGN = 2;                                    // waves 4 (M) x 2 (N)
    constexpr int WM = BM / 4, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int A_PL = plane_dwords(BM, true), B_PL = BN * 16;
    constexpr int A_ELEMS = 2 * A_PL, B_ELEMS = 2 * B_PL, STAGE = A_ELEMS + B_ELEMS;
    constexpr int TAB = TF == 1 ? 2 * F1_TAB_C : 0;
    constexpr int LDC_S = BN + 4;                                         // epilogue staging row (floats), 128 rows at a time
    static_assert((2 * STAGE + TAB) * 4 <= 160 * 1024, "two stages of both operands and the table in LDS");
    static_assert(128 * LDC_S <= 2 * STAGE && 8 * BN <= 2 * STAGE, "staging half and statistics reduction reuse the stages");
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * STAGE + (TAB ? TAB : 4)];
    [[maybe_unused]] const float* const tab = reinterpret_cast<const float*>(smem + 2 * STAGE);

    // block -> its run of the tile order (column tiles fastest): koaf_gemm_kernel's XCD remap (XCD x works through one contiguous chunk)
    const int ntn = p.N / BN;
    int tile, tile_end;
    {
        const unsigned ntx = gridDim.x, v = blockIdx.x;
        const unsigned q = ntx >> 3, rem = ntx & 7, x = v & 7, j = v >> 3;
        const unsigned b = x * q + (x < rem ? x : rem) + j;
        if constexpr (WALK) {
            tile = (int)((uint64_t)b * (unsigned)p.tiles / ntx);
            tile_end = (int)((uint64_t)(b + 1u) * (unsigned)p.tiles / ntx);
        } else {
            tile = (int)b;
            tile_end = tile + 1;
        }
    }
    const int K = p.K, nstep = K / BK;

    const float sca = p.a_scale, scb = scale_of_amax(*p.w_amax);
    float alpha = p.alpha / (sca * scb);
    if (!koaf_bits_finite(koaf_absbits(*p.w_amax))) {
        alpha = __uint_as_float(0x7fc00000u);          // (diverged weights: the whole output is NaN, as koaf_gemm does)
        if (blockIdx.x == 0 && threadIdx.x == 0) koaf_status_add(p.status, 1, 1u);
    }

    const int t = threadIdx.x;
    // the k-loop's per-thread indices.  WALK 1 forms them again for every tile from the thread index behind an opaque copy: as loop
    // invariants they would stay live through the epilogue, which carries the next tile's loads and has no registers to spare for them
    int lane, wm, wn;
    unsigned kq, ar;           // A: four units per thread and k-tile = rows ar + 64 i, k = 4 kq .. 4 kq + 3
    unsigned aoff;             // the thread's offset inside a tile of A (< 2^20 floats)
    unsigned boff, bdst;       // B: source offset inside a column tile (w_ld = K: < 2^19 elements) and PlaneLoader's swizzled LDS dword
    auto thread_indices = [&]() {
        int tk = t;
        if constexpr (WALK) asm volatile("" : "+v"(tk));
        lane = tk & 63;
        wm = (tk >> 6) / WGN; wn = (tk >> 6) % WGN;
        kq = (unsigned)tk & 7u; ar = (unsigned)tk >> 3;
        aoff = ar * (unsigned)K + 4u * kq;
        boff = ((unsigned)tk >> 2) * (unsigned)p.w_ld + 8u * ((unsigned)tk & 3u);
        bdst = ((unsigned)tk >> 2) * 16u + 4u * (((unsigned)tk & 3u) ^ (((unsigned)tk >> 4) & 3u));
    };
    thread_indices();

    constexpr int NUA = 4;
    const unsigned arow = 64u * (unsigned)K;               // unit i of A: + i arow (block-uniform)
    v4f ra[NUA];
    [[maybe_unused]] unsigned satmax = 0u;
    v4f ca = {0.f, 0.f, 0.f, 0.f}, cb = ca;      // tf 1: the scaled coefficients of the k-tile being converted
    // the k-tile the next issue fetches: tile bases (block-uniform) and k
    const float* a_base;
    const unsigned short* b_base;
    int ki = 0;
    auto tile_bases = [&](int tl, const float*& ab, const unsigned short*& bb) {
        const int tn_ = tl % ntn, tm_ = tl / ntn;
        ab = p.x + (int64_t)tm_ * BM * K;
        bb = p.wf + (int64_t)tn_ * BN * p.w_ld;
    };
    auto issue_a = [&](int i) { ra[i] = *(const v4f*)(a_base + (ki + i * arow) + aoff); };
    // TileLoader::finish_unit's arithmetic + split2h + the store of TileLoader::store (and its saturation watch) for unit i
    auto convert_a = [&](int i, unsigned* S, bool live) {
        constexpr float HMAX = 65504.f;
        v4f v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = ra[i][j];
            if constexpr (TF == 1) {
                x = fmaf(x, ca[j], cb[j]);
                x = __builtin_amdgcn_fmed3f(x, 0.f, HMAX);
            } else {
                x = __builtin_amdgcn_fmed3f(x * sca, -HMAX, HMAX);
            }
            v[j] = x;
        }
        unsigned pl[2][2];
        split2h(v, pl);
        if constexpr (TF == 1) {
            typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int d = 0; d < 2; ++d)
                satmax = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, satmax),
                                                                                 __builtin_bit_cast(u16x2, live ? pl[0][d] : 0u)));
        }
        const unsigned off = (ar + 64u * i) * 20u + 2u * kq;
#pragma unroll
        for (int q = 0; q < 2; ++q) *(uint2*)&S[q * A_PL + off] = make_uint2(pl[q][0], pl[q][1]);
    };
    auto load_coef = [&](int coff) {
        if constexpr (TF == 1) {
            ca = *(const v4f*)&tab[coff + 4 * (int)kq];
            cb = *(const v4f*)&tab[F1_TAB_C + coff + 4 * (int)kq];
        }
    };

    // ---- B: BN / 64 units per thread and k-tile = 16 B (8 k) of plane u % 2, row (t / 4) + 128 (u / 2) ----
    constexpr int NUB = BN / 64;
    v4i rb[NUB];
    auto issue_b = [&](int u) { rb[u] = *(const v4i*)(b_base + ((u & 1) * p.w_ps + (int64_t)(128 * (u >> 1)) * p.w_ld + ki) + boff); };
    auto store_b = [&](int u, unsigned* S) { *(v4i*)&S[A_ELEMS + (u & 1) * B_PL + (u >> 1) * (128 * 16) + bdst] = rb[u]; };

    v16f acc[TM][TN];

    constexpr int NUT = NUA + NUB, NG = 2 * TN;          // units per k-tile; MFMA groups (16-k slice x column tile) per k-step
    int ccoff = 0;                                       // first channel of the k-tile the next conversion handles
    [[maybe_unused]] const float* a_next = nullptr;      // WALK 1: the bases of the tile behind the one in work
    [[maybe_unused]] const unsigned short* b_next = nullptr;
    // unit u of the k-tile in registers into the stage at S, then the unit's loads of the k-tile at (a_base, b_base, ki)
    auto unit = [&](int u, unsigned* S, bool live) {
        if (u < NUA) { convert_a(u, S, live); issue_a(u); }
        else { store_b(u - NUA, S); issue_b(u - NUA); }
    };
    auto lgkm0_barrier = [&]() {
        // (the wait is the BUILTIN: hipcc's wait-count pass does not read inline assembly)
        __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
        asm volatile("s_barrier" ::: "memory");
    };
    // behind the end of K the issue walk goes on with k = 0 of the same tile (WALK 0) or of the next one (WALK 1)
    auto advance = [&]() {
        ki += BK;
        if (ki >= K) {
            ki = 0;
            if constexpr (WALK) { a_base = a_next; b_base = b_next; }
        }
        ccoff += BK;
        if (ccoff >= K) ccoff = 0;
    };
    // k-step: the MFMAs of the stage at cur -- per accumulator the order of koaf_gemm_kernel's mma(): 16-k slice g, then lo*hi, hi*lo,
    // hi*hi -- with the units of the next k-tile dealt out behind its MFMA groups (UNITS false: a step without vector work)
    auto step = [&](int cur, bool live, auto units_c) {
        constexpr bool UNITS = decltype(units_c)::value;
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        if constexpr (UNITS) load_coef(ccoff);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            v4i ap[TM][2];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 2; ++q) ap[i][q] = frag_load<BM, true>(Au + q * A_PL, wm * WM + 32 * i, g, lane);
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
                v4i bp[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) bp[q] = frag_load_ps(Bu + q * B_PL, wn * WN + 32 * jn, g, lane);
                constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};
#pragma unroll
                for (int term = 0; term < 3; ++term)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
                        acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, ap[i][PAH[term]]),
                                                                            __builtin_bit_cast(h16x8, bp[PBH[term]]), acc[i][jn], 0, 0, 0);
                if constexpr (UNITS) {
                    const int grp = g * TN + jn;
#pragma unroll
                    for (int u = 0; u < NUT; ++u)
                        if (u * NG / NUT == grp) unit(u, Sn, live);
                    // (the scheduler keeps each group's MFMAs, vector work and loads where they are written: koaf_fwd_s2.hip)
                    __builtin_amdgcn_sched_barrier(0x104);
                }
            }
        }
        if constexpr (UNITS) advance();
        // every wave is done reading this stage and has written its part of the next (the loads stay in flight)
        lgkm0_barrier();
    };

    // ---- prologue: the coefficient table, k-tile 0 of the first tile into the registers ----
    if constexpr (TF == 1) {
        float* tw = reinterpret_cast<float*>(smem + 2 * STAGE);
        for (int c = t; c < K; c += F1_NT) { tw[c] = p.sc[c] * sca; tw[F1_TAB_C + c] = p.sh[c] * sca; }
    }
    tile_bases(tile, a_base, b_base);
#pragma unroll
    for (int i = 0; i < NUA; ++i) issue_a(i);
#pragma unroll
    for (int u = 0; u < NUB; ++u) issue_b(u);
    if constexpr (TF == 1) __syncthreads();

    const bool do_stats = p.stats != nullptr;
    float* Cs = reinterpret_cast<float*>(smem);
    constexpr int C4 = BN / 4, RPP = F1_NT / C4;

#pragma unroll 1
    for (; tile < tile_end; ++tile) {
        const int tn = tile % ntn, tm = tile / ntn;
        const int m0 = tm * BM, n0 = tn * BN;
        if constexpr (WALK) {
            tile_bases(tile + 1 < tile_end ? tile + 1 : tile, a_next, b_next);
            thread_indices();
        }
        // the registers hold k-tile 0 of this tile: into stage 0, refilled with k-tile 1
        ki = BK;
        ccoff = 0;
        load_coef(0);
#pragma unroll
        for (int u = 0; u < NUT; ++u) unit(u, smem, true);
        advance();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        lgkm0_barrier();
        if constexpr (WALK) {
#pragma unroll 1
            for (int s = 0; s + 1 < nstep; ++s) step(s & 1, true, std::true_type{});
            step((nstep - 1) & 1, false, std::false_type{});
        } else {
#pragma unroll 1
            for (int s = 0; s < nstep; ++s) step(s & 1, s + 1 < nstep, std::true_type{});
        }

        if constexpr (TF == 1) {
            if (((satmax & 0xffffu) >= 0x7bffu) | ((satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
            satmax = 0u;
        }

        // ---- epilogue: koaf_gemm_kernel's, the tile as two 128-row halves (waves wm = 2 hh, 2 hh + 1 are the 2 x 2 waves of half hh) ----
        // (all waves passed the k-loop's last barrier: the operand stages are dead)
        // WALK 1: the epilogue's per-thread indices are formed again for every tile from the thread index behind an opaque copy -- hoisted
        // out of the tile loop they would stay live through the k-loop, which has no registers to spare for them
        int te = t;
        if constexpr (WALK) asm volatile("" : "+v"(te));
        const int wm = (te >> 6) / WGN, wn = (te >> 6) % WGN, r = te & 31, h = (te >> 5) & 1;
        const int c4 = te % C4, rr = te / C4;
        float s1[TM][TN], s2[TM][TN], kshift[TN];
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
#pragma unroll
            for (int i = 0; i < TM; ++i) s1[i][jn] = s2[i][jn] = 0.f;
            kshift[jn] = (do_stats && p.shift) ? p.shift[n0 + wn * WN + 32 * jn + r] : 0.f;
        }
        v4f bv = {0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(bv));                     // (the zero bias the shared epilogue adds: -0 becomes +0)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            if ((wm >> 1) == hh) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const float v = alpha * acc[i][jn][e];
                            s1[i][jn] += v - kshift[jn];
                            s2[i][jn] = fmaf(v - kshift[jn], v - kshift[jn], s2[i][jn]);
                            Cs[((wm & 1) * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) * LDC_S + wn * WN + 32 * jn + r] = v;
                        }
            }
            __syncthreads();
            float* const Yp = p.y + (int64_t)(m0 + 128 * hh) * p.N + n0 + 4 * c4;
#pragma unroll 4
            for (int row = rr; row < 128; row += RPP) {
                const v4f v = *(const v4f*)&Cs[row * LDC_S + 4 * c4] + bv;
                __builtin_nontemporal_store(v, (v4f*)(Yp + (int64_t)row * p.N));
            }
            __syncthreads();
        }
        if (do_stats) {
            // column sums: lanes (r, 0) + (r, 1) over the wave's two bands, then the two waves of each 128-row half
            float* red = Cs;      // [4][2][BN]
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
                float a1 = s1[0][jn] + __shfl_xor(s1[0][jn], 32, 64);
                float a2 = s2[0][jn] + __shfl_xor(s2[0][jn], 32, 64);
#pragma unroll
                for (int i = 1; i < TM; ++i) {
                    a1 += s1[i][jn] + __shfl_xor(s1[i][jn], 32, 64);
                    a2 += s2[i][jn] + __shfl_xor(s2[i][jn], 32, 64);
                }
                if (h == 0) {
                    red[(wm * 2 + 0) * BN + wn * WN + 32 * jn + r] = a1;
                    red[(wm * 2 + 1) * BN + wn * WN + 32 * jn + r] = a2;
                }
            }
            __syncthreads();
            if (te < 2 * BN) {
                const int hh = te / BN, c = te % BN;
                float a1 = red[(4 * hh + 0) * BN + c], a2 = red[(4 * hh + 1) * BN + c];
                a1 += red[(4 * hh + 2) * BN + c];
                a2 += red[(4 * hh + 3) * BN + c];
                float* st = p.stats + (int64_t)(p.part_row0 + 2 * tm + hh) * 2 * p.stats_ld;
                st[n0 + c] = a1;
                st[p.stats_ld + n0 + c] = a2;
            }
            // (the next tile's first k-tile goes into stage 0 only when every wave has read the sums)
            if constexpr (WALK) __syncthreads();
        }
    }
}

template <int BN, int WALK>
int f1_launch(const F1Params& p, int tf, dim3 grid, hipStream_t s) {
    if (tf) hipLaunchKernelGGL((fwd1_kernel<BN, 1, WALK>), grid, dim3(F1_NT), 0, s, p);
    else hipLaunchKernelGGL((fwd1_kernel<BN, 0, WALK>), grid, dim3(F1_NT), 0, s, p);
    return koaf_check_launch("koaf_fwd1");
}
}  // namespace

void koaf_log_launch(const char* variant, const KoafGemm& g, dim3 grid, dim3 launched);      // koaf_gemm.hip

// the form in which koaf_fwd1 ships for Cin = K, Cout = N: 0 one tile per block, 1 the persistent walk, -1 not at all (the call stays on
// the streamed kernel).  A table of the production shapes with the verdict of the per-call rule, not a heuristic.
int koaf_fwd1_form(int K, int N) {
#ifdef KOAF_FWD1_FORCE      // (benchmark builds only, scripts/bench_fwd1.py: every shape in one form)
    return KOAF_FWD1_FORCE;
#else
    struct Row { int K, N, form; };
    static const Row rows[] = {
        {64, 256, -1},      // conv3 and the shortcut of layer1: 1.09 / 1.07 x in the walk, inside ten spreads of the rounds
        {128, 512, 1}, {256, 1024, 1}, {512, 2048, 0}, {256, 128, 1}, {512, 256, 1},
    };
    for (const Row& r : rows)
        if (r.K == K && r.N == N) return r.form;
    return 1;      // (no production shape, never timed: the form that won or tied on every shape that was; tests/test_fwd1_gpu.py holds it there)
#endif
}

// the 1x1 / stride-1 forward convolution described by g (koaf_conv2d_fwd's descriptor: A = x dense with tf 0 | 1, B = the F plane image,
// fmt 1, act16 0, statistics optional) on 256-row tiles in the given form; the caller has checked the dispatch rule (koaf_conv.hip fwd1_ok)
int koaf_fwd1(const KoafGemm& g, int form, void* stream) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    KOAF_REQUIRE(g.fmt == 1 && g.act16 == 0 && A.kind == 0 && A.gather == 0 && A.ptr && !A.ptr2 && !A.amax &&
                 (A.tf == 0 || (A.tf == 1 && A.sc && A.sh && g.K <= F1_TAB_C)) && A.ld == g.K &&
                 B.kind == 2 && B.gather == 0 && B.planes && B.amax && !B.tf && g.C && g.ldc == g.N && g.splitk <= 1 && g.nb0 * g.nb1 <= 1 &&
                 !g.bias && !g.residual && !g.cmap && !g.bnb_mode && !g.out_planes && g.m_base == 0 && g.stats_bs == 0 &&
                 g.M % F1_BM == 0 && g.N % 128 == 0 && g.K >= 2 * BK && g.K % BK == 0 && g.K <= 8192 && B.ld == g.K && (form == 0 || form == 1),
                 "koaf_fwd1: bad args");
    F1Params p;
    p.x = A.ptr; p.sc = A.sc; p.sh = A.sh;
    p.a_scale = A.fscale != 0.f ? A.fscale : 1.f;
    p.wf = B.planes; p.w_ps = B.plane_stride; p.w_ld = B.ld; p.w_amax = B.amax;
    p.alpha = g.alpha;
    p.y = g.C;
    p.stats = g.stats; p.shift = g.stats ? g.stats_shift : nullptr; p.stats_ld = g.stats_ld ? g.stats_ld : g.N;
    p.status = g.status ? g.status : koaf_status_ptr();
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.part_row0 = g.part_row0;
    const int bn = (g.N % 256) == 0 ? 256 : 128;
    const int64_t tiles = (int64_t)(g.M / F1_BM) * (g.N / bn);
    KOAF_REQUIRE(tiles < (1ll << 31), "koaf_fwd1: too many tiles");
    p.tiles = (int)tiles;
    const dim3 grid((unsigned)tiles), launched(form ? (unsigned)(tiles < F1_CUS ? tiles : F1_CUS) : (unsigned)tiles);
    KoafGemm rec = g;
    rec.bm = F1_BM; rec.bn = bn;
    koaf_log_launch("koaf_fwd1", rec, grid, launched);
    hipStream_t s = (hipStream_t)stream;
    if (form) return bn == 256 ? f1_launch<256, 1>(p, A.tf, launched, s) : f1_launch<128, 1>(p, A.tf, launched, s);
    return bn == 256 ? f1_launch<256, 0>(p, A.tf, launched, s) : f1_launch<128, 0>(p, A.tf, launched, s);
}
