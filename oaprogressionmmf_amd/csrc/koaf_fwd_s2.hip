// koaf_fwd_s2.hip -- forward pass of the stride-2 convolutions (1x1 / pad 0 shortcuts, 3x3 / pad 1) on 256-row tiles (k = (tap, ci)):
//     y[m][co] = sum_k x~[m][k] * w[co][k]       m = output pixel (n, oy, ox), x~ = x[n][2 oy - pad + kh][2 ox - pad + kw][ci] behind its
//                                                transform, 0 outside the image
// with x fp32 in HBM (tf 0 plain, tf 1 relu(in_sc x + in_sh), formed on load) and the weights from the F plane image [2][Cout][K]
// (KoafWImg.f: already cut into fp16 pieces).  fp16 scheme only (KoafGemm.fmt 1: two pieces per value, three MFMAs per product).
// The generic kernel (koaf_gemm_kernel, TileLoader<.., M_KC_G1> x PlaneLoader) runs these calls on 128 x 128 tiles; here the schedule of
// koaf_tile256.h on 256 x 256 tiles (256 x 128 where Cout is no multiple of 256), one tile per block.
// Gather: a k-tile lies inside one filter tap (Cin % 32 == 0) and a thread owns the same four output-pixel rows for the whole tile: their
// (n, 2 oy - pad, 2 ox - pad) are decoded once; a unit's issue adds the tap and tests the two ranges.  A padding row loads pixel 0 and is
// zeroed BEHIND the transform, as TileLoader::finish_unit does.  The tf 1 coefficients, scaled, sit in an LDS table (Cin <= 1024).  The
// loads behind the end of K go on at k = 0 (the walk wraps).
// Same bits as koaf_gemm_kernel on the same descriptor, statistics rows included (tests/test_fwd_s2_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "koaf.h"
#include "koaf_tile256.h"
#include "koaf_conv_units.h"

namespace {
struct Fs2Params : T256FwdParams {      // x is [n][H][W][C]
    int M, N, K;
    int H, W, C, PH, PW, KH, pad;
    int part_row0;
};

template <int BN, int TF>
__global__ void __launch_bounds__(T256_NT) fwd_s2_kernel(const Fs2Params p) {
    constexpr int BM = T256_BM, WGN = 2;                                  // waves 4 (M) x 2 (N)
    constexpr int WM = BM / 4, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    typedef T256FragRow<BM, BN> Frag;
    constexpr int A_PL = Frag::A_PL, A_ELEMS = 2 * A_PL, B_ELEMS = 2 * Frag::B_PL, STAGE = A_ELEMS + B_ELEMS;
    constexpr int TAB = TF == 1 ? 2 * T256_TAB_C : 0;
    static_assert((2 * STAGE + TAB) * 4 <= 160 * 1024, "two stages of both operands and the table in LDS");
    static_assert(128 * (BN + 4) <= 2 * STAGE && 8 * BN <= 2 * STAGE, "staging half and statistics reduction reuse the stages");
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * STAGE + (TAB ? TAB : 4)];
    [[maybe_unused]] const float* const tab = reinterpret_cast<const float*>(smem + 2 * STAGE);

    // block -> tile, column tiles fastest
    const int ntn = p.N / BN;
    const unsigned b = t256_xcd_slot(gridDim.x, blockIdx.x);
    const int tn = (int)(b % (unsigned)ntn), tm = (int)(b / (unsigned)ntn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int nstep = p.K / BK;

    const float sca = p.a_scale, scb = scale_of_amax(*p.w_amax);
    // (alpha and the diverged-operand count stay in the unit: as a shared function they move the kernels' prologue)
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
    auto issue_a = [&](int i, const TapWalk& wk) {
        const int sy = iy0[i] + wk.kh, sx = ix0[i] + wk.kw;
        const bool ok = (unsigned)sy < (unsigned)p.H && (unsigned)sx < (unsigned)p.W;
        const unsigned pix = ok ? pixb[i] + (unsigned)sy * (unsigned)p.W + (unsigned)sx : 0u;
        vm = (vm & ~(1u << i)) | ((ok ? 0u : 1u) << i);
        ra[i] = *(const v4f*)(p.x + ((uint64_t)pix * (unsigned)p.C + (unsigned)wk.coff + 4u * kq));
    };
    auto convert_a = [&](int i, unsigned* S, bool live) {
        const v4f v = t256_finish4<TF>(ra[i], ca, cb, sca, ((vm >> i) & 1u) == 0u);
        t256_store_kc_unit<TF == 1>(S, A_PL, ar + 64u * i, kq, v, satmax, live);
    };
    auto load_coef = [&](int coff) {
        if constexpr (TF == 1) {
            ca = *(const v4f*)&tab[coff + 4 * (int)kq];
            cb = *(const v4f*)&tab[T256_TAB_C + coff + 4 * (int)kq];
        }
    };

    // ---- B: row n0 + t / 4 + 128 (u / 2) of plane u % 2 ----
    constexpr int NUB = T256PlaneB<BN>::NU;
    const unsigned short* const bsrc = p.wf + (int64_t)(n0 + (t >> 2)) * p.w_ld + 8 * (t & 3);
    const unsigned bdst = (unsigned)(t >> 2) * 16u + 4u * ((unsigned)(t & 3) ^ ((unsigned)(t >> 4) & 3u));      // (PlaneLoader's swizzle)
    T256PlaneB<BN> lb;
    auto issue_b = [&](int u, const TapWalk& wk) { lb.issue(u, bsrc + (u & 1) * p.w_ps + (int64_t)(128 * (u >> 1)) * p.w_ld + wk.k0); };

    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    constexpr int NUT = NUA + NUB;                       // units per k-tile
    TapWalk wi = {0, 0, 0, 0};                           // the k-tile the next issue fetches
    int ccoff = 0;                                       // first channel of the k-tile the next conversion handles
    // unit u of the k-tile in registers into the stage at S, then the unit's loads of the k-tile at wi
    auto unit = [&](int u, unsigned* S, bool live) {
        if (u < NUA) { convert_a(u, S, live); issue_a(u, wi); }
        else { lb.store(u - NUA, S, A_ELEMS, bdst); issue_b(u - NUA, wi); }
    };
    auto advance = [&]() {
        wi.next(p.C, p.KH, p.KH);
        ccoff += BK;
        if (ccoff >= p.C) ccoff = 0;
    };
    auto step = [&](int cur, bool live) {
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        load_coef(ccoff);
        T256_KSTEP(Frag, true, unit(u, Sn, live));
        advance();
        t256_lgkm0_barrier();
    };

    // ---- prologue: the coefficient table, k-tile 0 into stage 0, k-tile 1 into the registers ----
    if constexpr (TF == 1) {
        float* tw = reinterpret_cast<float*>(smem + 2 * STAGE);
        for (int c = t; c < p.C; c += T256_NT) { tw[c] = p.sc[c] * sca; tw[T256_TAB_C + c] = p.sh[c] * sca; }
    }
#pragma unroll
    for (int i = 0; i < NUA; ++i) issue_a(i, wi);
#pragma unroll
    for (int u = 0; u < NUB; ++u) issue_b(u, wi);
    wi.next(p.C, p.KH, p.KH);
    if constexpr (TF == 1) __syncthreads();
    load_coef(0);
#pragma unroll
    for (int u = 0; u < NUT; ++u) unit(u, smem, true);
    advance();
    t256_lgkm0_barrier();
#pragma unroll 1
    for (int s = 0; s < nstep; ++s) step(s & 1, s + 1 < nstep);

    if constexpr (TF == 1) {      // (the watch's report, in the unit for the same reason)
        if (((satmax & 0xffffu) >= 0x7bffu) | ((satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
    }

    const int te = t, r = lane & 31, h = lane >> 5;
    const bool do_stats = p.stats != nullptr;
    T256_FWD_EPILOGUE(BN, false)
}

template <int BN>
int fs2_launch(const Fs2Params& p, int tf, dim3 grid, hipStream_t s) {
    if (tf) hipLaunchKernelGGL((fwd_s2_kernel<BN, 1>), grid, dim3(T256_NT), 0, s, p);
    else hipLaunchKernelGGL((fwd_s2_kernel<BN, 0>), grid, dim3(T256_NT), 0, s, p);
    return koaf_check_launch("koaf_fwd_s2");
}
}  // namespace

// does koaf_fwd_s2 take the forward convolution described by g?  A stride-2 call, 1x1 / pad 0 or 3x3 / pad 1, of the fp16 scheme with the
// F plane image, fp32 tensors at pixel stride Cin, no plane-image input, tail or emission, whole k-tiles inside a tap (Cin % BK == 0),
// whole column tiles (Cout % 128 == 0), whole 256-row tiles (M % T256_BM == 0: a ragged last tile stays with the generic kernel, and so
// do the 128-row tiles its small calls are tested on), 16-B aligned pointers (t256_fwd_args_ok), a source pixel index that fits 31 bits
// and, behind a prologue, no more channels than the kernel's coefficient table holds (T256_TAB_C).  One k-tile is the shortest K the
// pipeline is written for.
bool koaf_fwd_s2_ok(const KoafGemm& g) {
    const KoafOperand& A = g.A;
    if (!t256_fwd_args_ok(g) || A.gather != 1 || g.K < BK) return false;
    if (A.stride != 2 || A.KH != A.KW || A.pad != A.pad_w || !((A.KH == 1 && A.pad == 0) || (A.KH == 3 && A.pad == 1))) return false;
    if (A.C % BK != 0 || A.CS != A.C || g.K != A.KH * A.KW * A.C || (A.tf != 0 && A.C > T256_TAB_C)) return false;
    if (A.PH <= 0 || A.PW <= 0 || A.PH != (A.H + 2 * A.pad - A.KH) / 2 + 1 || A.PW != (A.W + 2 * A.pad_w - A.KW) / 2 + 1) return false;
    return g.M % (A.PH * A.PW) == 0 && (int64_t)(g.M / (A.PH * A.PW)) * A.H * A.W < (1ll << 31);
}

// the stride-2 forward convolution described by g (koaf_conv2d_fwd's descriptor: A = x with gather 1 and tf 0 | 1, B = the F plane image,
// fmt 1, act16 0, statistics optional) on 256-row tiles
int koaf_fwd_s2(const KoafGemm& g, void* stream) {
    const KoafOperand& A = g.A;
    KOAF_REQUIRE(koaf_fwd_s2_ok(g), "koaf_fwd_s2: bad args");
    Fs2Params p;
    t256_fwd_params(g, p);
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.H = A.H; p.W = A.W; p.C = A.C; p.PH = A.PH; p.PW = A.PW; p.KH = A.KH; p.pad = A.pad;
    p.part_row0 = g.part_row0;
    const int bn = t256_bn(g.N);
    const dim3 grid((unsigned)((g.M / T256_BM) * (g.N / bn)));
    t256_log_launch("koaf_fwd_s2", g, T256_BM, bn, grid, grid);
    hipStream_t s = (hipStream_t)stream;
    return bn == 256 ? fs2_launch<256>(p, A.tf, grid, s) : fs2_launch<128>(p, A.tf, grid, s);
}
