// koaf_fwd_s2.hip -- forward pass of the stride-2 convolutions (1x1 / pad 0 shortcuts, 3x3 / pad 1) on 256-row tiles (k = (tap, ci)):
//     y[m][co] = sum_k x~[m][k] * w[co][k]       m = output pixel (n, oy, ox), x~ = x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its
//                                                transform, 0 outside the image
// with x fp32 in HBM (tf 0 plain, tf 1 relu(in_sc x + in_sh), formed on load) and the weights from the F plane image [2][Cout][K]
// (KoafWImg.f: already cut into fp16 pieces).  fp16 scheme only (KoafGemm.fmt 1: two pieces per value, three MFMAs per product).
// The generic kernel (koaf_gemm_kernel, TileLoader<.., M_KC_G1> x PlaneLoader) runs these calls on 128 x 128 tiles with ONE LDS image of A
// and two block barriers per 32-k step: the prologue, the piece split and the LDS store sit between the barriers with the matrix pipe
// idle.  Here, as in koaf_wgrad1.hip, a block of 512 threads (waves 4 x 2) owns a 256 x 256 tile (256 x 128 where Cout is no multiple of
// 256) with two LDS stages of both operands and one barrier per k-step:
//     step s:  MFMAs of k-tile s (stage s % 2)  ||  transform + split + store of A's k-tile s + 1 and the store of B's (registers ->
//              stage (s + 1) % 2), each register unit refilled with its loads of k-tile s + 2 as soon as it is stored
// so a load has a whole k-step to land and the vector work runs in the shadow of the matrix instructions.  Register slots are static;
// the loads behind the end of K are issued unconditionally (the walk wraps to k = 0) into registers whose conversion nobody reads.
// Every wave executes every barrier; there is no role split, no spin-wait and no hand-off between blocks.
// Gather: a k-tile lies inside one filter tap (Cin % 32 == 0) and a thread owns the same four output-pixel rows for the whole tile: their
// (n, 2 oy - pad, 2 ox - pad) are decoded once; a unit's issue adds the tap and tests the two ranges.  A padding row loads pixel 0 and is
// zeroed BEHIND the transform, as TileLoader::finish_unit does.  The tf 1 coefficients, scaled, sit in an LDS table (Cin <= 1024).
// LDS images: A = plane[row][32 k + 8 pad] (koaf_pieces.h, fragments by frag_load<.., true>), B = the swizzled rows PlaneLoader writes
// (frag_load_ps); B travels through registers like A, so that hipcc counts every load in flight itself.
// Same bits as koaf_gemm_kernel on the same descriptor: transform expressions, scale and split2h; k-tile order and the three piece
// products per accumulator and 16-k slice; alpha * acc and the + 0 of the zero bias; the statistics tree of the shared epilogue, written
// as TWO partial rows per tile, one per 128-row half, where a 128-row tiling puts them (tests/test_fwd_s2_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "koaf.h"
#include "koaf_pieces.h"

namespace {
struct Fs2Params {
    const float* x;             // [n][H][W][C]
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
    int H, W, C, PH, PW, KH, pad;
    int part_row0;
};

constexpr int FS2_NT = 512;
constexpr int FS2_BM = 256;
constexpr int FS2_TAB_C = 1024;          // tf 1: channels the coefficient table holds

// position of a k-tile in the (tap, ci) order (block-uniform); past the last tile it wraps to k = 0
struct Fs2Walk {
    int kh, kw, coff, k0;
    __device__ __forceinline__ void next(int C, int KH) {
        coff += BK; k0 += BK;
        if (coff >= C) {
            coff = 0;
            if (++kw == KH) { kw = 0; ++kh; }
            if (kh == KH) { kh = 0; k0 = 0; }
        }
    }
};

template <int BN, int TF>
__global__ void __launch_bounds__(FS2_NT) fwd_s2_kernel(const Fs2Params p) {
    constexpr int BM = FS2_BM, WGN = 2;                                   // waves 4 (M) x 2 (N)
    constexpr int WM = BM / 4, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int A_PL = plane_dwords(BM, true), B_PL = BN * 16;
    constexpr int A_ELEMS = 2 * A_PL, B_ELEMS = 2 * B_PL, STAGE = A_ELEMS + B_ELEMS;
    constexpr int TAB = TF == 1 ? 2 * FS2_TAB_C : 0;
    constexpr int LDC_S = BN + 4;                                         // epilogue staging row (floats), 128 rows at a time
    static_assert((2 * STAGE + TAB) * 4 <= 160 * 1024, "two stages of both operands and the table in LDS");
    static_assert(128 * LDC_S <= 2 * STAGE && 8 * BN <= 2 * STAGE, "staging half and statistics reduction reuse the stages");
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * STAGE + (TAB ? TAB : 4)];
    [[maybe_unused]] const float* const tab = reinterpret_cast<const float*>(smem + 2 * STAGE);

    // block -> tile: koaf_gemm_kernel's XCD remap (XCD x works through one contiguous chunk of the tile order, column tiles fastest)
    const int ntn = p.N / BN;
    int tm, tn;
    {
        const unsigned ntx = gridDim.x, v = blockIdx.x;
        const unsigned q = ntx >> 3, rem = ntx & 7, x = v & 7, j = v >> 3;
        const unsigned b = x * q + (x < rem ? x : rem) + j;
        tn = (int)(b % (unsigned)ntn);
        tm = (int)(b / (unsigned)ntn);
    }
    const int m0 = tm * BM, n0 = tn * BN;
    const int nstep = p.K / BK;

    const float sca = p.a_scale, scb = scale_of_amax(*p.w_amax);
    float alpha = p.alpha / (sca * scb);
    if (!koaf_bits_finite(koaf_absbits(*p.w_amax))) {
        alpha = __uint_as_float(0x7fc00000u);          // (diverged weights: the whole output is NaN, as koaf_gemm does)
        if (blockIdx.x == 0 && threadIdx.x == 0) koaf_status_add(p.status, 1, 1u);
    }

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w / WGN, wn = w % WGN;

    // ---- A: four units per thread and k-tile = rows ar + 64 i, k = 4 kq .. 4 kq + 3 ----
    constexpr int NUA = 4;
    const unsigned kq = t & 7, ar = t >> 3;
    unsigned pixb[NUA];        // first pixel of the row's image
    int iy0[NUA], ix0[NUA];    // source pixel of tap (0, 0)
    {
        const unsigned ppi = (unsigned)(p.PH * p.PW);
#pragma unroll
        for (int i = 0; i < NUA; ++i) {
            const unsigned row = (unsigned)m0 + ar + 64u * i;
            const unsigned n = row / ppi, rem = row - n * ppi, py = rem / (unsigned)p.PW, px = rem - py * (unsigned)p.PW;
            pixb[i] = n * (unsigned)(p.H * p.W);
            iy0[i] = 2 * (int)py - p.pad;
            ix0[i] = 2 * (int)px - p.pad;
        }
    }
    v4f ra[NUA];
    unsigned vm = 0u;          // bit i = unit i holds a padding row
    [[maybe_unused]] unsigned satmax = 0u;
    v4f ca = {0.f, 0.f, 0.f, 0.f}, cb = ca;      // tf 1: the scaled coefficients of the k-tile being converted
    auto issue_a = [&](int i, const Fs2Walk& wk) {
        const int sy = iy0[i] + wk.kh, sx = ix0[i] + wk.kw;
        const bool ok = (unsigned)sy < (unsigned)p.H && (unsigned)sx < (unsigned)p.W;
        const unsigned pix = ok ? pixb[i] + (unsigned)sy * (unsigned)p.W + (unsigned)sx : 0u;
        vm = (vm & ~(1u << i)) | ((ok ? 0u : 1u) << i);
        ra[i] = *(const v4f*)(p.x + ((uint64_t)pix * (unsigned)p.C + (unsigned)wk.coff + 4u * kq));
    };
    // TileLoader::finish_unit's arithmetic + split2h + the store of TileLoader::store (and its saturation watch) for unit i
    auto convert_a = [&](int i, unsigned* S, bool live) {
        constexpr float HMAX = 65504.f;
        const bool ok = ((vm >> i) & 1u) == 0u;
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
            v[j] = ok ? x : 0.f;
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
            cb = *(const v4f*)&tab[FS2_TAB_C + coff + 4 * (int)kq];
        }
    };

    // ---- B: BN / 64 units per thread and k-tile = 16 B (8 k) of plane u % 2, row (t / 4) + 128 (u / 2) ----
    constexpr int NUB = BN / 64;
    const unsigned short* const bsrc = p.wf + (int64_t)(n0 + (t >> 2)) * p.w_ld + 8 * (t & 3);
    const unsigned bdst = (unsigned)(t >> 2) * 16u + 4u * ((unsigned)(t & 3) ^ ((unsigned)(t >> 4) & 3u));      // (PlaneLoader's swizzle)
    v4i rb[NUB];
    auto issue_b = [&](int u, const Fs2Walk& wk) {
        rb[u] = *(const v4i*)(bsrc + (u & 1) * p.w_ps + (int64_t)(128 * (u >> 1)) * p.w_ld + wk.k0);
    };
    auto store_b = [&](int u, unsigned* S) { *(v4i*)&S[A_ELEMS + (u & 1) * B_PL + (u >> 1) * (128 * 16) + bdst] = rb[u]; };

    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    constexpr int NUT = NUA + NUB, NG = 2 * TN;          // units per k-tile; MFMA groups (16-k slice x column tile) per k-step
    Fs2Walk wi = {0, 0, 0, 0};                           // the k-tile the next issue fetches
    int ccoff = 0;                                       // first channel of the k-tile the next conversion handles
    // unit u of the k-tile in registers into the stage at S, then the unit's loads of the k-tile at wi
    auto unit = [&](int u, unsigned* S, bool live) {
        if (u < NUA) { convert_a(u, S, live); issue_a(u, wi); }
        else { store_b(u - NUA, S); issue_b(u - NUA, wi); }
    };
    auto lgkm0_barrier = [&]() {
        // (the wait is the BUILTIN: hipcc's wait-count pass does not read inline assembly)
        __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
        asm volatile("s_barrier" ::: "memory");
    };
    auto advance = [&]() {
        wi.next(p.C, p.KH);
        ccoff += BK;
        if (ccoff >= p.C) ccoff = 0;
    };
    // k-step: the MFMAs of the stage at cur -- per accumulator the order of koaf_gemm_kernel's mma(): 16-k slice g, then lo*hi, hi*lo,
    // hi*hi -- with the units of the next k-tile dealt out behind its MFMA groups
    auto step = [&](int cur, bool live) {
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        load_coef(ccoff);
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
                const int grp = g * TN + jn;
#pragma unroll
                for (int u = 0; u < NUT; ++u)
                    if (u * NG / NUT == grp) unit(u, Sn, live);
                // the scheduler keeps each group's MFMAs, vector work and loads where they are written (only fragment reads and scalar
                // work may cross): left free, it sinks every global load to the end of the step, in front of its first use
                __builtin_amdgcn_sched_barrier(0x104);
            }
        }
        advance();
        // every wave is done reading this stage and has written its part of the next (the loads stay in flight)
        lgkm0_barrier();
    };

    // ---- prologue: the coefficient table, k-tile 0 into stage 0, k-tile 1 into the registers ----
    if constexpr (TF == 1) {
        float* tw = reinterpret_cast<float*>(smem + 2 * STAGE);
        for (int c = t; c < p.C; c += FS2_NT) { tw[c] = p.sc[c] * sca; tw[FS2_TAB_C + c] = p.sh[c] * sca; }
    }
#pragma unroll
    for (int i = 0; i < NUA; ++i) issue_a(i, wi);
#pragma unroll
    for (int u = 0; u < NUB; ++u) issue_b(u, wi);
    wi.next(p.C, p.KH);
    if constexpr (TF == 1) __syncthreads();
    load_coef(0);
#pragma unroll
    for (int u = 0; u < NUT; ++u) unit(u, smem, true);
    advance();
    lgkm0_barrier();
#pragma unroll 1
    for (int s = 0; s < nstep; ++s) step(s & 1, s + 1 < nstep);

    if constexpr (TF == 1) {
        if (((satmax & 0xffffu) >= 0x7bffu) | ((satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
    }

    // ---- epilogue: koaf_gemm_kernel's, the tile as two 128-row halves (waves wm = 2 hh, 2 hh + 1 are the 2 x 2 waves of half hh) ----
    const int r = lane & 31, h = lane >> 5;
    const bool do_stats = p.stats != nullptr;
    float s1[TM][TN], s2[TM][TN], kshift[TN];
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
#pragma unroll
        for (int i = 0; i < TM; ++i) s1[i][jn] = s2[i][jn] = 0.f;
        kshift[jn] = (do_stats && p.shift) ? p.shift[n0 + wn * WN + 32 * jn + r] : 0.f;
    }
    float* Cs = reinterpret_cast<float*>(smem);      // all waves passed the k-loop's last barrier: the operand stages are dead
    constexpr int C4 = BN / 4, RPP = FS2_NT / C4;
    const int c4 = t % C4, rr = t / C4;
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
        if (t < 2 * BN) {
            const int hh = t / BN, c = t % BN;
            float a1 = red[(4 * hh + 0) * BN + c], a2 = red[(4 * hh + 1) * BN + c];
            a1 += red[(4 * hh + 2) * BN + c];
            a2 += red[(4 * hh + 3) * BN + c];
            float* st = p.stats + (int64_t)(p.part_row0 + 2 * tm + hh) * 2 * p.stats_ld;
            st[n0 + c] = a1;
            st[p.stats_ld + n0 + c] = a2;
        }
    }
}

template <int BN>
int fs2_launch(const Fs2Params& p, int tf, dim3 grid, hipStream_t s) {
    if (tf) hipLaunchKernelGGL((fwd_s2_kernel<BN, 1>), grid, dim3(FS2_NT), 0, s, p);
    else hipLaunchKernelGGL((fwd_s2_kernel<BN, 0>), grid, dim3(FS2_NT), 0, s, p);
    return koaf_check_launch("koaf_fwd_s2");
}
}  // namespace

void koaf_log_launch(const char* variant, const KoafGemm& g, dim3 grid, dim3 launched);      // koaf_gemm.hip

// the stride-2 forward convolution described by g (koaf_conv2d_fwd's descriptor: A = x with gather 1 and tf 0 | 1, B = the F plane image,
// fmt 1, act16 0, statistics optional) on 256-row tiles; the caller has checked the dispatch rule (koaf_conv.hip fwd_s2_ok)
int koaf_fwd_s2(const KoafGemm& g, void* stream) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    KOAF_REQUIRE(g.fmt == 1 && g.act16 == 0 && A.kind == 0 && A.gather == 1 && A.ptr && !A.amax && (A.tf == 0 || (A.tf == 1 && A.sc && A.sh)) &&
                 B.kind == 2 && B.gather == 0 && B.planes && B.amax && !B.tf && g.C && g.ldc == g.N && g.splitk <= 1 && g.nb0 * g.nb1 <= 1 &&
                 !g.bias && !g.residual && !g.cmap && !g.bnb_mode && !g.out_planes && g.m_base == 0 && g.stats_bs == 0 &&
                 g.M % FS2_BM == 0 && g.N % 128 == 0 && g.K >= BK && g.K % BK == 0 && B.ld == g.K,
                 "koaf_fwd_s2: bad args");
    KOAF_REQUIRE(A.stride == 2 && A.KH == A.KW && A.pad == A.pad_w && ((A.KH == 1 && A.pad == 0) || (A.KH == 3 && A.pad == 1)) && A.C % BK == 0 &&
                 (A.CS == 0 || A.CS == A.C) && g.K == A.KH * A.KW * A.C && A.PH > 0 && A.PW > 0 && A.PH == (A.H + 2 * A.pad - A.KH) / 2 + 1 &&
                 A.PW == (A.W + 2 * A.pad_w - A.KW) / 2 + 1 && g.M % (A.PH * A.PW) == 0 &&
                 (int64_t)(g.M / (A.PH * A.PW)) * A.H * A.W < (1ll << 31) && (A.tf == 0 || A.C <= FS2_TAB_C),
                 "koaf_fwd_s2: bad gather");
    Fs2Params p;
    p.x = A.ptr; p.sc = A.sc; p.sh = A.sh;
    p.a_scale = A.fscale != 0.f ? A.fscale : 1.f;
    p.wf = B.planes; p.w_ps = B.plane_stride; p.w_ld = B.ld; p.w_amax = B.amax;
    p.alpha = g.alpha;
    p.y = g.C;
    p.stats = g.stats; p.shift = g.stats ? g.stats_shift : nullptr; p.stats_ld = g.stats_ld ? g.stats_ld : g.N;
    p.status = g.status ? g.status : koaf_status_ptr();
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.H = A.H; p.W = A.W; p.C = A.C; p.PH = A.PH; p.PW = A.PW; p.KH = A.KH; p.pad = A.pad;
    p.part_row0 = g.part_row0;
    const int bn = (g.N % 256) == 0 ? 256 : 128;
    const dim3 grid((unsigned)((g.M / FS2_BM) * (g.N / bn)));
    KoafGemm rec = g;
    rec.bm = FS2_BM; rec.bn = bn;
    koaf_log_launch("koaf_fwd_s2", rec, grid, grid);
    hipStream_t s = (hipStream_t)stream;
    return bn == 256 ? fs2_launch<256>(p, A.tf, grid, s) : fs2_launch<128>(p, A.tf, grid, s);
}
