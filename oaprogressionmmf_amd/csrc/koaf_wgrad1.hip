// koaf_wgrad1.hip -- weight gradient of the 1x1 / stride-1 convolutions, and of the stride-2 ones (1x1 shortcuts, 3x3 / pad 1), on
// 256-wide tiles (k = pixel):
//     dw[co][ci] = sum_p dc[p][co] * x~[p][ci]                  (stride 2: dw[co][tap][ci], x~ at the tap's source pixel of p, 0 outside)
// with both operands K-major fp32 in HBM and the transforms of koaf_gemm's loaders formed on load: dc = dy, or the BatchNorm-backward
// apply k0 dz + k3 - k2 c of two sources (KoafOperand.tf 2); x~ = x, or relu(in_sc x + in_sh) (tf 1).  fp16 scheme only
// (KoafGemm.fmt 1: two fp16 pieces per value, three MFMAs per product).
// The generic kernel (koaf_gemm_kernel, M_KM x M_KM) runs these calls on 128 x 128 tiles, and every element of an operand is converted
// once per tile of the OTHER dimension.  Here the schedule of koaf_tile256.h, where it began, on 256 x 256 tiles (256 x 128 / 128 x 256
// where a dimension is 128 wide); the loads behind the end of the k-range are clamped into the tensor.
// Arithmetic, pieces, LDS images (plane[k][ROWS + 32 pad], koaf_pieces.h) and the order of the piece products per accumulator and
// 16-k slice are those of TileLoader + koaf_gemm_kernel's mma(): slabs and dw are bit-identical to the generic path
// (tests/test_wgrad1x1_gpu.py).  Split-K plan, slab layout and the XCD remap are koaf_gemm's.
// Stride 2 (GB = true): B is x gathered on the k index as TileLoader<.., M_KM_G1> gathers it.  Cin is a whole number of column tiles,
// so a block works on ONE filter tap (kh, kw).  The source pixel of a k-row costs no persistent register: the first 32 lanes of wave 0
// compute, three k-steps ahead, the 32 pixel indices of a k-tile (the divisions: once per k-step and block) into a ring of four table
// rows in LDS; a loader thread reads its unit's entry when it issues the unit and keeps one validity bit per unit until it converts it.
// A row that is padding or lies behind the k-range loads pixel 0 and is zeroed behind the transform, as finish_unit does; the zero
// contributions enter the accumulators where the generic kernel's do (tests/test_wgrad1_gather_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "koaf.h"
#include "koaf_tile256.h"
#include "koaf_conv_units.h"

namespace {
struct Wg1Params {
    const float* a;        // dy (tf 0) or dz (tf 2), [K][M]
    const float* a2;       // tf 2: the conv output c, same layout
    const float* asc;      // tf 2: k0, k3, k2 per output channel (KoafOperand.sc / sh / sc2)
    const float* ash;
    const float* asc2;
    const float* a_amax;   // scale of A = scale_of_amax(*a_amax)
    const float* b;        // x, [K][N]
    const float* bsc;      // tf 1: in_sc / in_sh per input channel
    const float* bsh;
    float b_scale;         // scale of B (fixed)
    float* out;            // slabs [splitk][M][N], or dw [M][N] when splitk == 1
    uint32_t* status;
    int M, N, K, splitk;
    // gathered B (stride 2): x is [n][H][W][C] (pixel stride C), k = (n, oy, ox) of the PH x PW output grid, column = (tap, ci)
    int H, W, C, PH, PW, KW, stride, pad, pad_w;
};

constexpr int WG1_TAB = 4 * BK;          // gathered B: ring of four table rows (k-tiles s + 1 .. s + 3 are live during step s)
constexpr unsigned WG1_INVALID = 0x80000000u;

// one K-major fp32 operand of the block: R columns of the 32 rows of a k-tile, 4 columns x (R / 64) rows ("units") per thread
// G: the rows are gathered through the block's table of source pixels (issue_g); ld is then the pixel stride of the source
template <int R, int TF, bool G = false>
struct Wg1Loader {
    static constexpr int NU = R / 64;                 // units per thread and k-tile
    static constexpr int CV = R / 4;                  // threads across a k-row
    static constexpr int RP = T256_NT / CV;            // k-rows per pass of the block
    static constexpr int SK = R / 2 + 16;             // dwords per k-row of a plane image
    static constexpr int PL = plane_dwords(R, false);
    v4f r[NU];
    v4f r2[TF == 2 ? NU : 1];
    v4f ca, cb, ck;        // transform coefficients of this thread's four columns, scaled
    const float* src;
    const float* src2;
    float fsc;
    unsigned ld, col, kr;
    unsigned vm;           // G: bit i = unit i holds a row that is padding or lies behind the k-range

    __device__ __forceinline__ void init(const float* p, const float* p2, const float* sc, const float* sh, const float* sc2,
                                         int c0, int ldim, float scale) {
        const unsigned t = threadIdx.x;
        src = p; src2 = p2;
        fsc = scale;
        ld = (unsigned)ldim;
        col = (unsigned)c0 + 4u * (t % CV);
        kr = t / CV;
        vm = 0u;
        ca = cb = ck = (v4f){0.f, 0.f, 0.f, 0.f};
        if constexpr (TF != 0) {
            ca = *(const v4f*)(sc + col) * fsc;
            cb = *(const v4f*)(sh + col) * fsc;
            if constexpr (TF == 2) ck = *(const v4f*)(sc2 + col) * fsc;
        }
    }
    // loads of unit i of the k-tile at k0 (any k0 >= 0: rows past the tensor's last re-read it)
    __device__ __forceinline__ void issue(int i, int k0, int K) {
        const int kb = min(k0, K - 1);                                  // (block-uniform)
        const unsigned rowmax = (unsigned)(K - 1 - kb);
        const unsigned row = min(kr + (unsigned)(RP * i), rowmax);
        const unsigned off = __umul24(row, ld) + col;                  // (< 32 * 2^16: the tile's base is added as a 64-bit scalar)
        const int64_t base = (int64_t)kb * ld;
        r[i] = *(const v4f*)(src + base + off);
        if constexpr (TF == 2) r2[i] = *(const v4f*)(src2 + base + off);
    }
    // G: loads of unit i of the k-tile whose table row is T -- entry = source pixel index, or WG1_INVALID (the load then re-reads pixel 0)
    __device__ __forceinline__ void issue_g(int i, const unsigned* T) {
        const unsigned e = T[kr + (unsigned)(RP * i)];
        vm = (vm & ~(1u << i)) | ((e >> 31) << i);
        const uint64_t off = (uint64_t)(e & ~WG1_INVALID) * ld + col;  // (N H W C reaches 3 G elements)
        r[i] = *(const v4f*)(src + off);
    }
    // TileLoader::finish_unit's arithmetic + split2h + the store of TileLoader::store, for unit i of the k-tile whose klim first
    // rows lie inside the k-range (G: validity is the unit's bit, border taps included; there is no FULL form)
    template <bool FULL>
    __device__ __forceinline__ void convert(int i, int klim, unsigned* S) {
        // (its own copy of t256_finish4's expressions: through the function hipcc commutes the TF 0 products of twelve kernels here)
        constexpr float HMAX = 65504.f;
        const bool ok = G ? ((vm >> i) & 1u) == 0u : (FULL || (int)(kr + (unsigned)(RP * i)) < klim);
        v4f v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = r[i][j];
            if constexpr (TF == 1) {
                x = fmaf(x, ca[j], cb[j]);
                x = __builtin_amdgcn_fmed3f(x, 0.f, HMAX);
            } else if constexpr (TF == 2) {
                x = fmaf(ca[j], x, fmaf(-ck[j], r2[i][j], cb[j]));
                x = __builtin_amdgcn_fmed3f(x, -HMAX, HMAX);
            } else {
                x = __builtin_amdgcn_fmed3f(x * fsc, -HMAX, HMAX);
            }
            v[j] = ok ? x : 0.f;
        }
        unsigned pl[2][2];
        split2h(v, pl);
        const unsigned off = (kr + (unsigned)(RP * i)) * SK + 2u * (threadIdx.x % CV);
#pragma unroll
        for (int q = 0; q < 2; ++q) *(uint2*)&S[q * PL + off] = make_uint2(pl[q][0], pl[q][1]);
    }
};

template <int BM, int BN, int TFA, int TFB, bool GB>
__global__ void __launch_bounds__(T256_NT) wgrad1_kernel(const Wg1Params p) {
    constexpr int WGM = 4, WGN = 2;                                   // waves along M x N
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    typedef Wg1Loader<BM, TFA> LA;
    typedef Wg1Loader<BN, TFB, GB> LB;
    typedef T256FragKM<BM, BN> Frag;
    constexpr int A_ELEMS = 2 * LA::PL, B_ELEMS = 2 * LB::PL, STAGE = A_ELEMS + B_ELEMS;
    static_assert((2 * STAGE + WG1_TAB) * 4 <= 160 * 1024, "two stages of both operands in LDS");
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * STAGE + (GB ? WG1_TAB : 0)];
    [[maybe_unused]] unsigned* const tab = smem + 2 * STAGE;

    // block -> (k-range, tile): koaf_gemm_kernel's split-K remap -- XCD = linear id % 8 takes the splits = x (mod 8), all tiles of a
    // split in consecutive slots of one XCD (one L2)
    const int ntn = p.N / BN;
    unsigned bid = blockIdx.x;
    int split = blockIdx.y;
    if (gridDim.y > 1 && (gridDim.y & 7) == 0) {
        const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, x = lin & 7, slot = lin >> 3;
        bid = slot % gridDim.x;
        split = (int)((slot / gridDim.x) * 8 + x);
    }
    const int tn = bid % ntn, tm = bid / ntn;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kchunk = (((p.K + p.splitk - 1) / p.splitk + BK - 1) / BK) * BK;
    const int kbeg = split * kchunk;
    const int kend = min(p.K, kbeg + kchunk);
    const int klen = max(kend - kbeg, 0), nstep = (klen + BK - 1) / BK;

    const float sca = scale_of_amax(*p.a_amax), scb = p.b_scale;
    // (alpha and the diverged-operand count stay in the unit: as a shared function they move the kernels' prologue)
    float alpha = 1.f / (sca * scb);
    if (!koaf_bits_finite(koaf_absbits(*p.a_amax))) {
        alpha = __uint_as_float(0x7fc00000u);          // (a diverged dy: the whole gradient is NaN, as koaf_gemm does)
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) koaf_status_add(p.status, 1, 1u);
    }

    LA la;
    LB lb;
    la.init(p.a, p.a2, p.asc, p.ash, p.asc2, m0, p.M, sca);
    // gathered B: the block's filter tap and its first channel (C % BN == 0); table row j & 3 holds the source pixels of k-tile j
    [[maybe_unused]] int g_kh = 0, g_kw = 0;
    if constexpr (GB) {
        const int tap = n0 / p.C;
        g_kh = tap / p.KW;
        g_kw = tap - g_kh * p.KW;
        lb.init(p.b, nullptr, p.bsc, p.bsh, nullptr, n0 - tap * p.C, p.C, scb);
    } else
        lb.init(p.b, nullptr, p.bsc, p.bsh, nullptr, n0, p.N, scb);
    [[maybe_unused]] auto table = [&](int j, int lane32) {
        const int k = kbeg + j * BK + lane32;
        const unsigned kk = (unsigned)min(k, p.K - 1), ppi = (unsigned)(p.PH * p.PW);
        const unsigned n = kk / ppi, rem = kk - n * ppi, oy = rem / (unsigned)p.PW, ox = rem - oy * (unsigned)p.PW;
        const int sy = (int)oy * p.stride - p.pad + g_kh, sx = (int)ox * p.stride - p.pad_w + g_kw;
        const bool ok = k < kend && (unsigned)sy < (unsigned)p.H && (unsigned)sx < (unsigned)p.W;
        tab[(j & 3) * BK + lane32] = ok ? (n * (unsigned)p.H + (unsigned)sy) * (unsigned)p.W + (unsigned)sx : WG1_INVALID;
    };

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w / WGN, wn = w % WGN;

    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // conversion unit u of the k-tile in registers (A units first) into the stage at S, then the unit's loads of the k-tile at k2
    constexpr int NUT = LA::NU + LB::NU;                              // units per k-tile
    auto unit = [&](int u, auto full, int klim, unsigned* S, int k2) {
        constexpr bool FULL = decltype(full)::value;
        if (u < LA::NU) {
            la.template convert<FULL>(u, klim, S);
            la.issue(u, k2, p.K);
        } else {
            lb.template convert<FULL>(u - LA::NU, klim, S + A_ELEMS);
            if constexpr (GB) lb.issue_g(u - LA::NU, tab + (((k2 - kbeg) / BK) & 3) * BK);
            else lb.issue(u - LA::NU, k2, p.K);
        }
    };
    // (this unit keeps the inline-assembly wait it was tuned with; the other three take the builtin, t256_lgkm0_barrier)
    auto lgkm0_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    auto step = [&](auto full, int cur, int klim, int k2) {
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        if constexpr (GB) {
            // the table row of the k-tile after k2: its readers pass this step's barrier first; the row it replaces was last read three steps ago
            if (threadIdx.x < BK) table((k2 - kbeg) / BK + 1, threadIdx.x);
        }
        T256_KSTEP(Frag, true, unit(u, full, klim, Sn, k2));
        lgkm0_barrier();
    };

    if (nstep > 0) {
        if constexpr (GB) {
            if (threadIdx.x < 3 * BK) table(threadIdx.x / BK, threadIdx.x % BK);
            lgkm0_barrier();
        }
#pragma unroll
        for (int i = 0; i < LA::NU; ++i) la.issue(i, kbeg, p.K);
#pragma unroll
        for (int i = 0; i < LB::NU; ++i) {
            if constexpr (GB) lb.issue_g(i, tab);
            else lb.issue(i, kbeg, p.K);
        }
#pragma unroll
        for (int u = 0; u < NUT; ++u) unit(u, std::false_type{}, klen, smem, kbeg + BK);
        lgkm0_barrier();
    }
    // steps whose NEXT k-tile lies wholly inside the range convert without zero fill
    const int nfull = max(klen / BK - 1, 0);
    int s = 0;
#pragma unroll 1
    for (; s < nfull; ++s) step(std::true_type{}, s & 1, BK, kbeg + (s + 2) * BK);
#pragma unroll 1
    for (; s < nstep; ++s) step(std::false_type{}, s & 1, klen - (s + 1) * BK, kbeg + (s + 2) * BK);

    // ---- partial tile -> slab (dw itself when splitk == 1): v = alpha * acc, plus the zero bias the shared epilogue adds ----
    float* out = p.out + (p.splitk > 1 ? (int64_t)split * p.M * p.N : (int64_t)0);
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float v = alpha * acc[i][jn][e];
                asm volatile("" : "+v"(v));            // (the product is rounded before the add, as through the staging tile)
                v += 0.f;
                const int row = m0 + wm * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                const int col = n0 + wn * WN + 32 * jn + r;
                out[(int64_t)row * p.N + col] = v;
            }
}

template <int BM, int BN, bool GB>
int wg1_launch(const Wg1Params& p, int tfa, int tfb, dim3 grid, hipStream_t s) {
#define WG1_GO(TA, TB) hipLaunchKernelGGL((wgrad1_kernel<BM, BN, TA, TB, GB>), grid, dim3(T256_NT), 0, s, p)
    if (tfa == 2) { if (tfb) WG1_GO(2, 1); else WG1_GO(2, 0); }
    else { if (tfb) WG1_GO(0, 1); else WG1_GO(0, 0); }
#undef WG1_GO
    return koaf_check_launch("koaf_wgrad1");
}
template <bool GB>
int wg1_tile(const Wg1Params& p, int bm, int bn, int tfa, int tfb, dim3 grid, hipStream_t s) {
    if (bm == 256 && bn == 256) return wg1_launch<256, 256, GB>(p, tfa, tfb, grid, s);
    if (bm == 256) return wg1_launch<256, 128, GB>(p, tfa, tfb, grid, s);
    return wg1_launch<128, 256, GB>(p, tfa, tfb, grid, s);
}
}  // namespace

// does koaf_wgrad1 take the weight gradient described by g, split g.splitk ways, and on which tile (bm_ / bn_, optional)?  The
// fp16 scheme on fp32 tensors, channel counts in whole tiles of 128 with at least one side 256 wide, and k-ranges of at least
// WGRAD1_MIN_KCHUNK pixels -- shorter launches stay with the generic kernel's more and smaller blocks.  B is dense (1x1 / stride 1) or the
// stride-2 gather of a 1x1 / pad 0 or 3x3 / pad 1 filter over whole pixels whose Cin is a whole number of column tiles (a block then works
// on one filter tap), k = whole images of the output grid and a source pixel index that fits the table's 31 bits; layer2's 3x3 / stride 2
// at 128 -> 128 (N = 1152: no whole number of 256-wide tiles beside M = 128) and every other gather stay on koaf_gemm
constexpr int WGRAD1_MIN_KCHUNK = 1024;
bool koaf_wgrad1_ok(const KoafGemm& g, int* bm_, int* bn_) {
    const KoafOperand& A = g.A;
    const KoafOperand& B = g.B;
    if (g.fmt != 1 || g.act16 != 0 || A.kind != 1 || B.kind != 1 || A.gather || (B.gather != 0 && B.gather != 1)) return false;
    if (!A.amax || !A.ptr || !B.ptr || !g.C || g.K < BK || g.K >= (1 << 30) || g.splitk < 1 || g.splitk > 65535) return false;
    if (g.M % 128 || g.N % 128 || (g.M < 256 && g.N < 256)) return false;
    const int bm = g.M >= 256 ? 256 : 128, bn = g.N >= 256 ? 256 : 128;
    if (g.M % bm || g.N % bn || A.ld != g.M || g.ldc != g.N || (B.gather == 0 && B.ld != g.N)) return false;
    if (B.gather == 1) {
        const bool f11 = B.KH == 1 && B.KW == 1 && B.pad == 0 && B.pad_w == 0, f33 = B.KH == 3 && B.KW == 3 && B.pad == 1 && B.pad_w == 1;
        if (B.stride != 2 || !(f11 || f33) || B.CS != B.C || B.C % bn || g.N != B.KH * B.KW * B.C || B.PH <= 0 || B.PW <= 0) return false;
        if (B.PH != (B.H + 2 * B.pad - B.KH) / 2 + 1 || B.PW != (B.W + 2 * B.pad_w - B.KW) / 2 + 1 || g.K % (B.PH * B.PW) != 0) return false;
        if ((int64_t)(g.K / (B.PH * B.PW)) * B.H * B.W >= (1ll << 31)) return false;      // (the kernel's table holds 31-bit pixel indices)
    }
    if ((cdiv64(g.K, g.splitk) + BK - 1) / BK * BK < WGRAD1_MIN_KCHUNK) return false;
    // (what koaf_gemm's vector path asks of the pointers; an unaligned call takes the generic kernel's scalar path)
    if (!aligned16(A.ptr) || !aligned16(B.ptr) || !aligned16(g.C)) return false;
    if (A.tf && (A.tf != 2 || !A.ptr2 || !A.sc || !A.sh || !A.sc2 || !aligned16(A.ptr2) || !aligned16(A.sc) || !aligned16(A.sh) || !aligned16(A.sc2)))
        return false;
    if (B.tf && (B.tf != 1 || !B.sc || !B.sh || !aligned16(B.sc) || !aligned16(B.sh))) return false;
    if (bm_) { *bm_ = bm; *bn_ = bn; }
    return true;
}

// the weight gradient described by g (koaf_conv2d_wgrad's descriptor: A = dy [K][M] K-major with tf 0 | 2, B = x with tf 0 | 1 -- [K][N]
// K-major for 1x1 / stride 1, or gather 1 over the NHWC tensor for stride 2 --, fmt 1, act16 0, C = slabs or dw) on the rule's tile
int koaf_wgrad1(const KoafGemm& g, void* stream) {
    const KoafOperand& B = g.B;
    const bool gb = B.gather == 1;
    int bm = 0, bn = 0;
    KOAF_REQUIRE(koaf_wgrad1_ok(g, &bm, &bn), "koaf_wgrad1: bad args");
    Wg1Params p;
    p.a = g.A.ptr; p.a2 = g.A.ptr2; p.asc = g.A.sc; p.ash = g.A.sh; p.asc2 = g.A.sc2; p.a_amax = g.A.amax;
    p.b = B.ptr; p.bsc = B.sc; p.bsh = B.sh;
    p.b_scale = B.fscale != 0.f ? B.fscale : 1.f;
    p.out = g.C;
    p.status = g.status ? g.status : koaf_status_ptr();
    p.M = g.M; p.N = g.N; p.K = g.K; p.splitk = g.splitk;
    p.H = B.H; p.W = B.W; p.C = B.C; p.PH = B.PH; p.PW = B.PW; p.KW = B.KW; p.stride = B.stride; p.pad = B.pad; p.pad_w = B.pad_w;
    const dim3 grid((unsigned)((g.M / bm) * (g.N / bn)), (unsigned)g.splitk);
    t256_log_launch("koaf_wgrad1", g, bm, bn, grid, grid);
    hipStream_t s = (hipStream_t)stream;
    return gb ? wg1_tile<true>(p, bm, bn, g.A.tf, B.tf, grid, s) : wg1_tile<false>(p, bm, bn, g.A.tf, B.tf, grid, s);
}
