// koaf_dgrad_s2.hip -- data gradients of the stride-2 convolutions (1x1 / pad 0 shortcuts, 3x3 / pad 1) on 256-row tiles.  The input
// pixels (y, x) of a stride-2 convolution fall into four parity classes (y % 2, x % 2), each a stride-1 transposed gather over its own
// subset of the filter taps (koaf_conv.hip koaf_conv2d_dgrad_bnb); per class
//     dx_class[m][ci] = sum_k dy~[m][k] * w[ci][k]      m = (n, yy, xx) of the class, k = (tap of the class's subset, co),
//                                                       dy~ = dy[n][yy + offy - kh][xx + offx - kw][co], 0 outside the image
// and row m is stored at input pixel (n, 2 yy + py, 2 xx + px).  fp16 scheme only (KoafGemm.fmt 1: two pieces per value, three MFMAs per
// product), the weights from the class's taps of the D plane image [2][Cin][KH KW Cout].
// The generic kernel runs each class on 128 x 128 tiles with one k-tile in flight and two block barriers per k-step, and its row map sends
// every tile down the one-row-at-a-time epilogue loop.  Here the schedule of koaf_tile256.h on 256 x 256 tiles (256 x 128 where Cin is no
// multiple of 256), one tile per block.
// A, two loaders:
//   AM 0 (3x3): the activation plane images [2][pixels][Cout] of dy (koaf_act_planes: the BatchNorm-backward apply is in the image), 16-B
//     chunks through registers; a k-tile lies inside one tap (Cout % 32 == 0) and a thread owns the same two rows for a whole tile, their
//     (n, yy + offy, xx + offx) decoded once; a source pixel outside the image reads the image's zero chunk.  No conversion in the loop.
//   AM 1 | 2 (1x1): class (0, 0) of an even image is the identity walk over the pixels of dy -- dense fp32 rows, plain at scale(*amax)
//     (AM 1) or behind the apply coef0 dz + coef3 - coef2 c (AM 2), TileLoader::finish_unit's expressions, scale and split2h.  The other
//     three classes have no tap: their rows are exact zeros, written by the block that owns the neighbouring class-(0, 0) rows.
// Epilogue: the row map is decoded once per thread and tile and then advanced; the loads of four rows go out together; 16-B non-temporal
// stores.  Plain, or the BatchNorm-backward reduction mode 2 (mask by c sc + sh > 0, column sums q1 / q2, max |dz|).
// Same bits as koaf_gemm_kernel on the class descriptors, 128 x 128 tiles: k-tile order, the three piece products per accumulator and 16-k
// slice, alpha * acc, the + 0 of the zero bias, mask and sums in the generic loop's order -- a thread of a 128-row half sums its 16 rows
// rr + 8 j in order, then the eight rr are added in order -- so a 256-row tile writes TWO partial rows, at 2 tm and 2 tm + 1
// (tests/test_dgrad_s2_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "koaf.h"
#include "koaf_tile256.h"
#include "koaf_conv_units.h"

namespace {
struct Ds2Params {
    const float* dz;            // AM 1 | 2: dy (AM 1) or dz (AM 2), [M][C]
    const float* c;             // AM 2: the second source
    const float* sc;            // AM 2: coef0 / coef2 / coef3 per output channel
    const float* sc2;
    const float* sh;
    const float* a_amax;        // scale of A = scale_of_amax(*a_amax)
    const unsigned short* apl;  // AM 0: plane q at apl + q * a_ps, pixel p at p * C; the zero chunk at azero
    int64_t a_ps;
    const unsigned short* azero;
    const unsigned short* wd;   // the class's first tap of the D image: plane q at wd + q * w_ps, row ci at ci * w_ld, tap (i, j) at
    int64_t w_ps, w_ld, w_ts, w_tsh;      // i * w_tsh + j * w_ts
    const float* w_amax;
    float alpha;
    float* dx;                  // [N H W][Cin]
    const float *bc, *bsc, *bsh, *bmean, *binv;      // BatchNorm-backward mode 2 (bnb != 0)
    float* part;
    float* dz_amax;
    int bnb;
    uint32_t* status;
    int nrec;                   // launches of the generic path this one stands for (the status word counts them)
    int M, N, K, C;
    int OH, OW, Hc, Wc, nkh, nkw, offy, offx, H, W, py, px;
    int e_a, e_b, e_c;          // eight rows further in the class: 8 = e_a Hc Wc + e_b Wc + e_c
    int part_row0;
};

// a block-uniform value, pinned to scalar registers
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

template <int BN, int AM>
__global__ void __launch_bounds__(T256_NT) dgrad_s2_kernel(const Ds2Params p) {
    constexpr int BM = T256_BM, WGN = 2;                                  // waves 4 (M) x 2 (N)
    constexpr int WM = BM / 4, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    typedef T256FragRow<BM, BN> Frag;
    constexpr int A_PL = Frag::A_PL, A_ELEMS = 2 * A_PL, B_ELEMS = 2 * Frag::B_PL, STAGE = A_ELEMS + B_ELEMS;
    constexpr int LDC_S = BN + 4;                                         // epilogue staging row (floats)
    constexpr int HPS = BN == 128 ? 2 : 1;                                // 128-row halves staged at a time (128 columns: both)
    constexpr int SMEM = 2 * STAGE > 128 * HPS * LDC_S ? 2 * STAGE : 128 * HPS * LDC_S;
    static_assert(SMEM * 4 <= 159 * 1024, "two stages of both operands, or the staged tile, in LDS");
    __shared__ __attribute__((aligned(16))) unsigned smem[SMEM];

    // block -> tile, column tiles fastest
    const int ntn = p.N / BN;
    const unsigned b = t256_xcd_slot(gridDim.x, blockIdx.x);
    const int tn = (int)(b % (unsigned)ntn), tm = (int)(b / (unsigned)ntn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int nstep = p.K / BK;

    const float sca = scale_of_amax(*p.a_amax), scb = scale_of_amax(*p.w_amax);
    // (alpha and the diverged-operand count stay in the unit: as a shared function they move the kernels' prologue)
    float alpha = p.alpha / (sca * scb);
    if (!koaf_bits_finite(koaf_absbits(*p.a_amax)) || !koaf_bits_finite(koaf_absbits(*p.w_amax))) {
        alpha = __uint_as_float(0x7fc00000u);          // (a diverged operand: the whole output is NaN, as koaf_gemm does)
        if (blockIdx.x == 0 && threadIdx.x == 0) koaf_status_add(p.status, 1, (unsigned)p.nrec);
    }

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w / WGN, wn = w % WGN;

    // ---- A ----
    // AM 0: four units per thread and k-tile = the 16 B (8 k) chunk t % 4 of plane u % 2, row t / 4 + 128 (u / 2)
    // AM 1 | 2: four units = rows t / 8 + 64 i, k = 4 (t % 8) .. + 3 of dz (and of c)
    constexpr int NUA = 4;
    [[maybe_unused]] const unsigned kq = t & 7, ar = t >> 3, ck = t & 3, pr = t >> 2;
    [[maybe_unused]] const unsigned avoff = ar * (unsigned)p.C + 4u * kq;      // AM 1 | 2: this thread's element in a unit's 64 rows
    [[maybe_unused]] unsigned pixb[2];       // AM 0: first pixel of the row's image
    [[maybe_unused]] int iy0[2], ix0[2];     //       source pixel of tap (0, 0)
    if constexpr (AM == 0) {
        const unsigned ppi = (unsigned)(p.Hc * p.Wc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned row = (unsigned)m0 + pr + 128u * j;
            const unsigned n = row / ppi, rem = row - n * ppi, yy = rem / (unsigned)p.Wc, xx = rem - yy * (unsigned)p.Wc;
            pixb[j] = n * (unsigned)(p.OH * p.OW);
            iy0[j] = (int)yy + p.offy;
            ix0[j] = (int)xx + p.offx;
        }
    }
    [[maybe_unused]] v4i rp[AM == 0 ? NUA : 1];
    [[maybe_unused]] v4f ra[AM != 0 ? NUA : 1];
    [[maybe_unused]] v4f rc[AM == 2 ? NUA : 1];
    // AM 2: the coefficients of the k-tile being converted (one set: the next tile's are fetched behind the tile's last A unit and
    // have the B units' MFMA groups and the barrier to land)
    [[maybe_unused]] v4f na = {0.f, 0.f, 0.f, 0.f}, nb = na, nc = na;
    auto issue_a = [&](int u, const TapWalk& wk) {
        if constexpr (AM == 0) {
            const int j = u >> 1, q = u & 1;
            const int sy = iy0[j] - wk.kh, sx = ix0[j] - wk.kw;
            const bool ok = (unsigned)sy < (unsigned)p.OH && (unsigned)sx < (unsigned)p.OW;
            const unsigned pix = pixb[j] + (unsigned)sy * (unsigned)p.OW + (unsigned)sx;
            const unsigned short* src = ok ? p.apl + (q * p.a_ps + (int64_t)((uint64_t)pix * (unsigned)p.C + (unsigned)wk.coff + 8u * ck)) : p.azero;
            rp[u] = *(const v4i*)src;
        } else {
            // (a block-uniform 64-bit base in scalar registers and one 32-bit offset per thread: left to itself hipcc hoists one full
            // 64-bit address per unit and source out of the loop and spills them)
            const uint64_t ub = uniform64((uint64_t)(unsigned)(m0 + 64 * u) * (unsigned)p.C + (unsigned)wk.coff);
            ra[u] = *(const v4f*)(p.dz + ub + avoff);
            if constexpr (AM == 2) rc[u] = *(const v4f*)(p.c + ub + avoff);
        }
    };
    // unit u of the k-tile in registers into the A image at S
    auto store_a = [&](int u, unsigned* S) {
        if constexpr (AM == 0) {
            *(v4i*)&S[(u & 1) * A_PL + (pr + 128u * (u >> 1)) * 20u + 4u * ck] = rp[u];
        } else {
            v4f v;
            if constexpr (AM == 2) {
                // (its own copy of t256_finish4<2>'s expression, the coefficients scaled here: through the function the two kernels move)
                constexpr float HMAX = 65504.f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = __builtin_amdgcn_fmed3f(fmaf(na[j] * sca, ra[u][j], fmaf(-(nc[j] * sca), rc[u][j], nb[j] * sca)), -HMAX, HMAX);
            } else
                v = t256_finish4<0>(ra[u], na, nb, sca);
            t256_store_kc_unit(S, A_PL, ar + 64u * u, kq, v);
        }
    };
    auto issue_coef = [&](int coff) {
        if constexpr (AM == 2) {
            na = *(const v4f*)(p.sc + coff + 4 * (int)kq);
            nb = *(const v4f*)(p.sh + coff + 4 * (int)kq);
            nc = *(const v4f*)(p.sc2 + coff + 4 * (int)kq);
        }
    };

    // ---- B: row n0 + t / 4 + 128 (u / 2) of plane u % 2, at the walk's tap ----
    constexpr int NUB = T256PlaneB<BN>::NU;
    const unsigned bvoff = (unsigned)(t >> 2) * (unsigned)p.w_ld + 8u * (unsigned)(t & 3);      // (32 bits: 128 rows of the D image)
    const unsigned bdst = (unsigned)(t >> 2) * 16u + 4u * ((unsigned)(t & 3) ^ ((unsigned)(t >> 4) & 3u));      // (PlaneLoader's swizzle)
    T256PlaneB<BN> lb;
    auto issue_b = [&](int u, const TapWalk& wk) {
        const int64_t koff = wk.kh * p.w_tsh + wk.kw * p.w_ts + wk.coff;
        lb.issue(u, p.wd + uniform64((uint64_t)((u & 1) * p.w_ps + (int64_t)(n0 + 128 * (u >> 1)) * p.w_ld + koff)) + bvoff);
    };

    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    constexpr int NUT = NUA + NUB;                       // units per k-tile
    TapWalk wi = {0, 0, 0, 0};                           // the k-tile the next issue fetches
    int ncoff = 0;                                       // AM 2: first channel of the k-tile whose coefficients the next issue fetches
    auto next_coef = [&]() {
        issue_coef(ncoff);
        ncoff += BK;
        if (ncoff >= p.C) ncoff = 0;
    };
    auto unit = [&](int u, unsigned* S) {
        if (u < NUA) {
            store_a(u, S);
            if (u == NUA - 1) next_coef();
            issue_a(u, wi);
        }
        else { lb.store(u - NUA, S, A_ELEMS, bdst); issue_b(u - NUA, wi); }
    };
    auto step = [&](int cur) {
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        T256_KSTEP(Frag, true, unit(u, Sn));
        wi.next(p.C, p.nkh, p.nkw);
        t256_lgkm0_barrier();
    };

    // ---- prologue: k-tile 0 into stage 0, k-tile 1 into the registers ----
    next_coef();
#pragma unroll
    for (int i = 0; i < NUA; ++i) issue_a(i, wi);
#pragma unroll
    for (int u = 0; u < NUB; ++u) issue_b(u, wi);
    wi.next(p.C, p.nkh, p.nkw);
#pragma unroll
    for (int u = 0; u < NUT; ++u) unit(u, smem);
    wi.next(p.C, p.nkh, p.nkw);
    t256_lgkm0_barrier();
#pragma unroll 1
    for (int s = 0; s < nstep; ++s) step(s & 1);

    // ---- epilogue: the tile as two 128-row halves (waves wm = 2 hh, 2 hh + 1 are the 2 x 2 waves of half hh) ----
    const int r = lane & 31, h = lane >> 5;
    float* Cs = reinterpret_cast<float*>(smem);      // all waves passed the k-loop's last barrier: the operand stages are dead
    constexpr int C4 = BN / 4;
    static_assert(T256_NT / C4 == 8 * HPS, "eight row threads per column vector and staged half");
    const int c4 = t % C4, rq = t / C4, rr = rq & 7, hs = rq >> 3;
    const int col = n0 + 4 * c4;
    v4f bv = {0.f, 0.f, 0.f, 0.f};
    asm volatile("" : "+v"(bv));                     // (the zero bias the shared epilogue adds: -0 becomes +0)
    const v4f zf = (v4f){alpha * 0.f, alpha * 0.f, alpha * 0.f, alpha * 0.f} + bv;      // AM 1 | 2: a row of a class without a tap
    const bool bnb = AM == 0 && p.bnb != 0;          // (the 1x1 shortcuts carry no fused reduction: koaf_dgrad_s2)
    v4f mu = bv, is = bv, ms = bv, mh = bv;
    if (bnb) {
        mu = *(const v4f*)(p.bmean + col);
        is = *(const v4f*)(p.binv + col);
        ms = *(const v4f*)(p.bsc + col);
        mh = *(const v4f*)(p.bsh + col);
    }
    // the row map: this thread's rows are 128 hs + rr + 8 j of the tile (j = 0 .. 15, and on through the second half where the halves
    // are staged one after the other): (n, yy, xx) decoded once, then advanced by eight rows
    int en, ey, ex;
    {
        const unsigned ppi = (unsigned)(p.Hc * p.Wc);
        const unsigned row = (unsigned)m0 + 128u * hs + rr;
        const unsigned n = row / ppi, rem = row - n * ppi, yy = rem / (unsigned)p.Wc;
        en = (int)n; ey = (int)yy; ex = (int)(rem - yy * (unsigned)p.Wc);
    }
    auto next_pixel = [&]() -> int64_t {
        const int64_t pix = ((int64_t)en * p.H + 2 * ey + p.py) * p.W + 2 * ex + p.px;
        ex += p.e_c;
        if (ex >= p.Wc) { ex -= p.Wc; ++ey; }
        ey += p.e_b;
        if (ey >= p.Hc) { ey -= p.Hc; ++en; }
        en += p.e_a;
        return pix;
    };
    v4f qm = bv;                                     // the largest |dz| this thread stored, as magnitude bits
#pragma unroll 1
    for (int pass = 0; pass < 2 / HPS; ++pass) {
        if (HPS == 2 || (wm >> 1) == pass) {
            const int hrow = HPS == 2 ? (wm >> 1) * 128 : 0;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        Cs[(hrow + (wm & 1) * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) * LDC_S + wn * WN + 32 * jn + r] = alpha * acc[i][jn][e];
        }
        __syncthreads();
        v4f q1 = {0.f, 0.f, 0.f, 0.f}, q2 = q1;      // BatchNorm-backward column sums of this thread's rows of the half
        constexpr int U = 4;
#pragma unroll 1
        for (int j0 = 0; j0 < 16; j0 += U) {
            int64_t off[U];
            v4f cv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                off[u] = next_pixel() * p.N + col;
                if (bnb) cv[u] = __builtin_nontemporal_load((const v4f*)(p.bc + off[u]));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                v4f v = *(const v4f*)&Cs[(128 * hs + rr + 8 * (j0 + u)) * LDC_S + 4 * c4] + bv;
                if (bnb) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (cv[u][j] * ms[j] + mh[j]) > 0.f ? v[j] : 0.f;
                    q1 += v;
                    q2 += v * ((cv[u] - mu) * is);
#pragma unroll
                    for (int j = 0; j < 4; ++j) qm[j] = __uint_as_float(max(__float_as_uint(qm[j]), koaf_absbits(v[j])));
                }
                __builtin_nontemporal_store(v, (v4f*)(p.dx + off[u]));
                if constexpr (AM != 0) {
                    // the three input pixels beside this one belong to the classes without a tap
                    __builtin_nontemporal_store(zf, (v4f*)(p.dx + off[u] + p.N));
                    __builtin_nontemporal_store(zf, (v4f*)(p.dx + off[u] + (int64_t)p.W * p.N));
                    __builtin_nontemporal_store(zf, (v4f*)(p.dx + off[u] + (int64_t)(p.W + 1) * p.N));
                }
            }
        }
        __syncthreads();                             // the staged rows are consumed
        if (bnb) {
            // column sums over the rows of each half: its eight row threads per column vector -> LDS -> one partial row per half
            v4f* red4 = reinterpret_cast<v4f*>(smem);      // [2][8 HPS][C4]
            red4[(0 * 8 * HPS + rq) * C4 + c4] = q1;
            red4[(1 * 8 * HPS + rq) * C4 + c4] = q2;
            __syncthreads();
            if (rr < 2) {
                v4f a = red4[(rr * 8 * HPS + 8 * hs) * C4 + c4];
                for (int j = 1; j < 8; ++j) a += red4[(rr * 8 * HPS + 8 * hs + j) * C4 + c4];
                const int hh = HPS == 2 ? hs : pass;
                *(v4f*)(p.part + ((int64_t)(p.part_row0 + 2 * tm + hh) * 2 + rr) * p.N + col) = a;
            }
            __syncthreads();
        }
    }
    if (bnb && p.dz_amax)
        block_amax_raise_bits(max(max(__float_as_uint(qm[0]), __float_as_uint(qm[1])), max(__float_as_uint(qm[2]), __float_as_uint(qm[3]))), p.dz_amax);
}

template <int BN>
int ds2_launch(const Ds2Params& p, int am, dim3 grid, hipStream_t s) {
    if (am == 0) hipLaunchKernelGGL((dgrad_s2_kernel<BN, 0>), grid, dim3(T256_NT), 0, s, p);
    else if (am == 1) hipLaunchKernelGGL((dgrad_s2_kernel<BN, 1>), grid, dim3(T256_NT), 0, s, p);
    else hipLaunchKernelGGL((dgrad_s2_kernel<BN, 2>), grid, dim3(T256_NT), 0, s, p);
    return koaf_check_launch("koaf_dgrad_s2");
}
}  // namespace

// does koaf_dgrad_s2 take the class described by g of a KH x KW filter (and with it the whole call: the rule reads nothing that differs
// between the classes that have a tap)?  The fp16 scheme with the D plane image on fp32 tensors, no residual, no fused reduction or mode 2
// with one BatchNorm; 3x3 / pad 1 from dy's plane images (reduction optional), 1x1 / pad 0 from the fp32 dy (tf 0 | 2) without a reduction;
// whole k-tiles inside a tap (Cout % BK == 0), whole column tiles (Cin % 128 == 0); an even image whose classes are whole 256-row tiles (a
// ragged tile or an odd image stays with the generic kernel, and so do the 128-row tiles its small calls are tested on); 16-B aligned
// pointers; pixel indices that fit 31 bits.  The descriptor carries the class, not the call: pad 1 of a 3x3 is read from the class's taps
// and offsets (class (py, px) has 1 + py by 1 + px taps at offsets py, px); the filter size is given, since class (0, 0) of a 3x3 and of a
// 1x1 both have one tap.  A class without a tap (K = 0) is refused: the 1x1 call's class (0, 0) writes its zeros.
bool koaf_dgrad_s2_ok(const KoafGemm& g, int KH, int KW) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    const bool f11 = KH == 1 && KW == 1, f33 = KH == 3 && KW == 3;
    if (!(f11 || f33) || g.fmt != 1 || g.act16 != 0 || A.gather != 2 || !A.amax || A.stride != 1) return false;
    if (B.kind != 2 || B.gather != 0 || !B.planes || !B.amax || B.tf || !g.C || g.ldc != g.N || g.splitk > 1 || g.nb0 * g.nb1 > 1) return false;
    if (g.bias || g.residual || !g.cmap || g.stats || g.out_planes || g.m_base != 0 || !aligned16(g.C) || !aligned16(B.planes)) return false;
    if (g.M % T256_BM != 0 || g.N % 128 != 0 || g.K < BK || A.C % BK != 0 || A.KH <= 0 || A.KW <= 0 || g.K != A.KH * A.KW * A.C || A.CS != A.C) return false;
    // the row map: an even image (cm_H = 2 PH), whole images per class
    if (A.PH <= 0 || A.PW <= 0 || g.cm_PH != A.PH || g.cm_PW != A.PW || g.cm_H != 2 * A.PH || g.cm_W != 2 * A.PW || g.M % (A.PH * A.PW) != 0 ||
        (int64_t)(g.M / (A.PH * A.PW)) * g.cm_H * g.cm_W >= (1ll << 31) || (unsigned)g.cm_py >= 2u || (unsigned)g.cm_px >= 2u)
        return false;
    if (g.bnb_mode && (g.bnb_mode != 2 || g.bnb2_c || !g.bnb_c || !g.bnb_sc || !g.bnb_sh || !g.bnb_mean || !g.bnb_invstd || !g.bnb_part ||
                       !aligned16(g.bnb_c) || !aligned16(g.bnb_sc) || !aligned16(g.bnb_sh) || !aligned16(g.bnb_mean) || !aligned16(g.bnb_invstd) ||
                       !aligned16(g.bnb_part)))
        return false;
    if (f33)      // pad 1, from dy's plane images
        return A.kind == 2 && A.planes && A.zeros && !A.tf && aligned16(A.planes) && aligned16(A.zeros) && !(A.plane_stride & 7) &&
               A.KH == 1 + g.cm_py && A.KW == 1 + g.cm_px && A.pad == g.cm_py && A.pad_w == g.cm_px;
    // fp32 A: the identity walk of class (0, 0) of a 1x1 / pad 0 filter, without a fused reduction
    if (A.kind != 0 || !A.ptr || !aligned16(A.ptr) || A.KH != 1 || A.KW != 1 || A.pad != 0 || A.pad_w != 0 || A.H != A.PH || A.W != A.PW ||
        g.cm_py != 0 || g.cm_px != 0 || g.bnb_mode)
        return false;
    return A.tf == 0 || (A.tf == 2 && A.ptr2 && A.sc && A.sh && A.sc2 && aligned16(A.ptr2) && aligned16(A.sc) && aligned16(A.sh) && aligned16(A.sc2));
}

// One parity class of a stride-2 data gradient, described by g as koaf_conv2d_dgrad_bnb builds it (A = dy with gather 2 at stride 1, from
// plane images or fp32 with tf 0 | 2; B = the class's taps of the D plane image; the row map; BatchNorm-backward mode 2 optional), on
// 256-row tiles.  A call whose A is fp32 is class (0, 0) of a 1x1 shortcut: it also writes the zeros of the three classes without a tap
// and leaves their launch records (K = 0) behind its own.
int koaf_dgrad_s2(const KoafGemm& g, int KH, int KW, void* stream) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    const bool pl = A.kind == 2;
    KOAF_REQUIRE(koaf_dgrad_s2_ok(g, KH, KW), "koaf_dgrad_s2: bad args");
    Ds2Params p;
    p.dz = A.ptr; p.c = A.ptr2; p.sc = A.sc; p.sc2 = A.sc2; p.sh = A.sh; p.a_amax = A.amax;
    p.apl = A.planes; p.a_ps = A.plane_stride; p.azero = A.zeros;
    p.wd = B.planes; p.w_ps = B.plane_stride; p.w_ld = B.ld; p.w_ts = B.tap_stride; p.w_tsh = B.tap_stride_h; p.w_amax = B.amax;
    p.alpha = g.alpha;
    p.dx = g.C;
    p.bc = g.bnb_c; p.bsc = g.bnb_sc; p.bsh = g.bnb_sh; p.bmean = g.bnb_mean; p.binv = g.bnb_invstd; p.part = g.bnb_part; p.dz_amax = g.bnb_amax;
    p.bnb = g.bnb_mode;
    p.status = g.status ? g.status : koaf_status_ptr();
    p.nrec = pl ? 1 : 4;
    p.M = g.M; p.N = g.N; p.K = g.K; p.C = A.C;
    p.OH = A.H; p.OW = A.W; p.Hc = A.PH; p.Wc = A.PW; p.nkh = A.KH; p.nkw = A.KW; p.offy = A.pad; p.offx = A.pad_w;
    p.H = g.cm_H; p.W = g.cm_W; p.py = g.cm_py; p.px = g.cm_px;
    {
        const int ppi = A.PH * A.PW, rem = 8 % ppi;
        p.e_a = 8 / ppi; p.e_b = rem / A.PW; p.e_c = rem % A.PW;
    }
    p.part_row0 = g.part_row0;
    const int bn = t256_bn(g.N);
    const dim3 grid((unsigned)((g.M / T256_BM) * (g.N / bn)));
    t256_log_launch("koaf_dgrad_s2", g, T256_BM, bn, grid, grid);
    if (!pl) {
        KoafGemm rec = g;
        rec.K = 0;
        for (int i = 0; i < 3; ++i) t256_log_launch("koaf_dgrad_s2", rec, T256_BM, bn, grid, grid);
    }
    hipStream_t s = (hipStream_t)stream;
    const int am = pl ? 0 : (A.tf == 2 ? 2 : 1);
    return bn == 256 ? ds2_launch<256>(p, am, grid, s) : ds2_launch<128>(p, am, grid, s);
}
