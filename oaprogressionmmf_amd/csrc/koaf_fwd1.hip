// koaf_fwd1.hip -- forward pass of the dense 1x1 / stride-1 / pad-0 convolutions on 256-row tiles:
//     y[m][co] = sum_k x~[m][k] * w[co][k]       m = pixel, k = input channel
// with x fp32 in HBM at pixel stride Cin (tf 0 plain, tf 1 relu(in_sc x + in_sh), formed on load) and the weights from the F plane image
// [2][Cout][K] (KoafWImg.f).  fp16 scheme only (KoafGemm.fmt 1: two pieces per value, three MFMAs per product).
// The streamed kernel (koaf_gemm_kernel, A mode 13) runs these calls on 128 x 128 tiles; a tile's load, convert, multiply and store
// phases follow one another there.  Here the schedule of koaf_tile256.h on 256 x 256 tiles (256 x 128 where Cout is no multiple of 256)
// -- row = pixel, so there is no tap walk and no padding mask.  Addresses are a block-uniform base plus one 32-bit offset per thread
// and operand.
// Two forms:
//   WALK 0  one tile per block (koaf_fwd_s2's grid and XCD remap); the loads behind the end of K are issued unconditionally (the walk
//           wraps to k = 0) into registers whose conversion nobody reads.
//   WALK 1  a persistent block (grid = min(tiles, 256)) walks a contiguous run of the tile order, column tiles fastest, so consecutive
//           tiles share their A rows.  The units stored in a tile's last-but-one k-step are refilled with the NEXT tile's first k-tile;
//           the last k-step has no vector work, the loads land under the epilogue and are converted into stage 0 once the epilogue has
//           released the stages.  A block's last tile prefetches its own first k-tile again (in bounds, unused).  K >= 64: the
//           last-but-one step exists.  Every trip count is block-uniform and every wave executes every barrier; there is no role split,
//           no spin-wait, no hand-off between blocks and no flag in memory.
// Same bits as koaf_gemm_kernel on the same descriptor, statistics rows included (tests/test_fwd1_gpu.py: torch.equal).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "koaf.h"
#include "koaf_tile256.h"
#include "koaf_conv_units.h"

namespace {
struct F1Params : T256FwdParams {       // x is [M][K]
    int M, N, K;
    int tiles;                  // (M / 256) (N / BN)
    int part_row0;
};

constexpr int F1_CUS = 256;              // WALK 1: one block per CU
constexpr int F1_MAX_K = 8192;           // the rule's cap on Cin: longer rows were never admitted, timed or tested

template <int BN, int TF, int WALK>
__global__ void __launch_bounds__(T256_NT) fwd1_kernel(const F1Params p) {
    constexpr int BM = T256_BM, WGN = 2;                                  // waves 4 (M) x 2 (N)
    constexpr int WM = BM / 4, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    typedef T256FragRow<BM, BN> Frag;
    constexpr int A_PL = Frag::A_PL, A_ELEMS = 2 * A_PL, B_ELEMS = 2 * Frag::B_PL, STAGE = A_ELEMS + B_ELEMS;
    constexpr int TAB = TF == 1 ? 2 * T256_TAB_C : 0;
    static_assert((2 * STAGE + TAB) * 4 <= 160 * 1024, "two stages of both operands and the table in LDS");
    static_assert(128 * (BN + 4) <= 2 * STAGE && 8 * BN <= 2 * STAGE, "staging half and statistics reduction reuse the stages");
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * STAGE + (TAB ? TAB : 4)];
    [[maybe_unused]] const float* const tab = reinterpret_cast<const float*>(smem + 2 * STAGE);

    // block -> its run of the tile order (column tiles fastest): koaf_gemm_kernel's XCD remap (XCD x works through one contiguous chunk)
    const int ntn = p.N / BN;
    int tile, tile_end;
    {
        const unsigned ntx = gridDim.x, b = t256_xcd_slot(ntx, blockIdx.x);
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
    // (alpha and the diverged-operand count stay in the unit: as a shared function they move the kernels' prologue)
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
    auto convert_a = [&](int i, unsigned* S, bool live) {
        const v4f v = t256_finish4<TF>(ra[i], ca, cb, sca);
        t256_store_kc_unit<TF == 1>(S, A_PL, ar + 64u * i, kq, v, satmax, live);
    };
    auto load_coef = [&](int coff) {
        if constexpr (TF == 1) {
            ca = *(const v4f*)&tab[coff + 4 * (int)kq];
            cb = *(const v4f*)&tab[T256_TAB_C + coff + 4 * (int)kq];
        }
    };

    // ---- B: row t / 4 + 128 (u / 2) of the column tile, plane u % 2 ----
    constexpr int NUB = T256PlaneB<BN>::NU;
    T256PlaneB<BN> lb;
    auto issue_b = [&](int u) { lb.issue(u, b_base + ((u & 1) * p.w_ps + (int64_t)(128 * (u >> 1)) * p.w_ld + ki) + boff); };

    v16f acc[TM][TN];

    constexpr int NUT = NUA + NUB;                       // units per k-tile
    int ccoff = 0;                                       // first channel of the k-tile the next conversion handles
    [[maybe_unused]] const float* a_next = nullptr;      // WALK 1: the bases of the tile behind the one in work
    [[maybe_unused]] const unsigned short* b_next = nullptr;
    // unit u of the k-tile in registers into the stage at S, then the unit's loads of the k-tile at (a_base, b_base, ki)
    auto unit = [&](int u, unsigned* S, bool live) {
        if (u < NUA) { convert_a(u, S, live); issue_a(u); }
        else { lb.store(u - NUA, S, A_ELEMS, bdst); issue_b(u - NUA); }
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
    // a k-step on the stage at cur (UNITS false: without vector work)
    auto step = [&](int cur, bool live, auto units_c) {
        constexpr bool UNITS = decltype(units_c)::value;
        const unsigned* Au = smem + cur * STAGE;
        const unsigned* Bu = Au + A_ELEMS;
        unsigned* Sn = smem + (cur ^ 1) * STAGE;
        if constexpr (UNITS) load_coef(ccoff);
        T256_KSTEP(Frag, UNITS, unit(u, Sn, live));
        if constexpr (UNITS) advance();
        t256_lgkm0_barrier();
    };

    // ---- prologue: the coefficient table, k-tile 0 of the first tile into the registers ----
    if constexpr (TF == 1) {
        float* tw = reinterpret_cast<float*>(smem + 2 * STAGE);
        for (int c = t; c < K; c += T256_NT) { tw[c] = p.sc[c] * sca; tw[T256_TAB_C + c] = p.sh[c] * sca; }
    }
    tile_bases(tile, a_base, b_base);
#pragma unroll
    for (int i = 0; i < NUA; ++i) issue_a(i);
#pragma unroll
    for (int u = 0; u < NUB; ++u) issue_b(u);
    if constexpr (TF == 1) __syncthreads();

    const bool do_stats = p.stats != nullptr;

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
        t256_lgkm0_barrier();
        if constexpr (WALK) {
#pragma unroll 1
            for (int s = 0; s + 1 < nstep; ++s) step(s & 1, true, std::true_type{});
            step((nstep - 1) & 1, false, std::false_type{});
        } else {
#pragma unroll 1
            for (int s = 0; s < nstep; ++s) step(s & 1, s + 1 < nstep, std::true_type{});
        }

        if constexpr (TF == 1) {      // (the watch's report, in the unit for the same reason)
            if (((satmax & 0xffffu) >= 0x7bffu) | ((satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
            satmax = 0u;
        }

        // ---- epilogue ----
        // WALK 1: its per-thread indices are formed again for every tile from the thread index behind an opaque copy -- hoisted out of
        // the tile loop they would stay live through the k-loop, which has no registers to spare for them; the next tile's first k-tile
        // goes into stage 0 only when every wave has read the sums
        int te = t;
        if constexpr (WALK) asm volatile("" : "+v"(te));
        const int wm = (te >> 6) / WGN, wn = (te >> 6) % WGN, r = te & 31, h = (te >> 5) & 1;
        T256_FWD_EPILOGUE(BN, WALK != 0)
    }
}

template <int BN, int WALK>
int f1_launch(const F1Params& p, int tf, dim3 grid, hipStream_t s) {
    if (tf) hipLaunchKernelGGL((fwd1_kernel<BN, 1, WALK>), grid, dim3(T256_NT), 0, s, p);
    else hipLaunchKernelGGL((fwd1_kernel<BN, 0, WALK>), grid, dim3(T256_NT), 0, s, p);
    return koaf_check_launch("koaf_fwd1");
}
}  // namespace

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

// the form in which koaf_fwd1 takes the forward convolution described by g, -1 if it does not.  A pointwise call of the fp16 scheme with
// the F plane image, fp32 tensors at pixel stride Cin, no plane-image input, tail or emission, whole k-tiles and at least two of them
// (Cin % BK == 0, K >= 2 BK: the walk's last-but-one k-step exists), whole column tiles (Cout % 128 == 0), 16-B aligned pointers
// (t256_fwd_args_ok), no more than F1_MAX_K channels and, behind a prologue, no more than the coefficient table holds (T256_TAB_C), the
// streamed kernels switched on (koaf_set_stream(0) keeps these calls on the block-wide loader) -- and whole 256-row tiles, at least one
// per CU (M % T256_BM == 0, M >= F1_CUS T256_BM = 65536): below that a 256-row tiling cannot fill the chip, and the small calls the
// tests pin to koaf_gemm/stream from their launch records stay there.  Among these, the (Cin, Cout) of koaf_fwd1_form's table: the
// production shapes that passed the per-call rule.
int koaf_fwd1_ok(const KoafGemm& g) {
    const KoafOperand& A = g.A;
    if (!t256_fwd_args_ok(g) || A.gather != 0 || A.ld != g.K || !koaf_stream_on()) return -1;
    if (g.K < 2 * BK || g.K > F1_MAX_K || (A.tf != 0 && g.K > T256_TAB_C) || g.M < F1_CUS * T256_BM) return -1;
    return koaf_fwd1_form(g.K, g.N);
}

// the 1x1 / stride-1 forward convolution described by g (koaf_conv2d_fwd's descriptor: A = x dense with tf 0 | 1, B = the F plane image,
// fmt 1, act16 0, statistics optional) on 256-row tiles, in the form the rule names
int koaf_fwd1(const KoafGemm& g, void* stream) {
    const KoafOperand& A = g.A;
    const int form = koaf_fwd1_ok(g);
    KOAF_REQUIRE(form == 0 || form == 1, "koaf_fwd1: bad args");
    F1Params p;
    t256_fwd_params(g, p);
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.part_row0 = g.part_row0;
    const int bn = t256_bn(g.N);
    const int64_t tiles = (int64_t)(g.M / T256_BM) * (g.N / bn);
    KOAF_REQUIRE(tiles < (1ll << 31), "koaf_fwd1: too many tiles");
    p.tiles = (int)tiles;
    const dim3 grid((unsigned)tiles), launched(form ? (unsigned)(tiles < F1_CUS ? tiles : F1_CUS) : (unsigned)tiles);
    t256_log_launch("koaf_fwd1", g, T256_BM, bn, grid, launched);
    hipStream_t s = (hipStream_t)stream;
    if (form) return bn == 256 ? f1_launch<256, 1>(p, A.tf, launched, s) : f1_launch<128, 1>(p, A.tf, launched, s);
    return bn == 256 ? f1_launch<256, 0>(p, A.tf, launched, s) : f1_launch<128, 0>(p, A.tf, launched, s);
}
