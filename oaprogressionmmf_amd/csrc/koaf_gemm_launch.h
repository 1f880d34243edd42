// koaf_gemm_launch.h -- between koaf_gemm.hip, which plans a call, and the family files koaf_gemm_*.hip, which hold the
// koaf_gemm_kernel instantiations (host only).  A family function turns an already-made plan into hipLaunchKernelGGL; it
// returns KOAF_NO_KERNEL where its family has no instantiation for the call, and koaf_gemm.hip words the error.
//   koaf_gemm_stream.hip        M_KS x M_PS: the streamed 1x1 convolutions and their data gradients
//   koaf_gemm_wplanes_act0.hip  every other A mode x M_PS (weight plane images): fp32 loader M_KC | M_KC_G1 | M_KC_G2, gathered activation
//   koaf_gemm_wplanes_act1.hip    planes M_PA1 | M_PA2, the 3x3 kernels M_PH | M_PT -- one file per activation-storage role (act16 0 | 1 | 2);
//   koaf_gemm_wplanes_act2.hip    the lists themselves: koaf_gemm_wplanes.h
//   koaf_gemm_kmajor.hip        M_PK x M_PK | M_PKG: K-major plane pairs (weight gradients)
//   koaf_gemm_fp16.hip          fp32 operands on both sides, fp16 scheme (fmt 1)
//   koaf_gemm_bf16.hip          fp32 operands on both sides, bf16 x 3 scheme (fmt 0), the unaligned 64 x 64 path included
#pragma once
#include "koaf_gemm_kernel.h"

constexpr int KOAF_NO_KERNEL = -1000;

// part_rows: row tiles of the call (koaf_gemm_part_rows); halo / t2d: the 3x3 plane-image kernels M_PH / M_PT; stream: M_KS
struct TilePlan { int bm, bn; bool vec; int part_rows; bool halo; bool t2d; bool stream; };

int koaf_launch_stream(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_wplanes_act0(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_wplanes_act1(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_wplanes_act2(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_kmajor(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_fp16(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);
int koaf_launch_bf16(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s);

namespace {

// the access mode (koaf_gemm_loaders.h) that an operand descriptor asks for
inline int operand_mode(const KoafOperand& o) {
    if (o.kind == 3) return o.gather ? M_PKG : M_PK;
    if (o.kind == 2) return o.gather == 0 ? M_PS : (o.gather == 1 ? M_PA1 : M_PA2);
    if (o.kind == 0) return o.gather == 0 ? M_KC : (o.gather == 1 ? M_KC_G1 : M_KC_G2);
    return o.gather == 0 ? M_KM : (o.gather == 1 ? M_KM_G1 : M_KM_G3);
}

constexpr unsigned PERSIST_BLOCKS = 512;      // 2 per CU x 256 CUs; a multiple of 8 (virtual tile ids keep their XCD)
// the grid of a persistent variant: at most two blocks per CU, each walking its tiles
inline dim3 persist_grid(dim3 grid) {
    if (grid.y == 1 && grid.x > PERSIST_BLOCKS) grid.x = PERSIST_BLOCKS;
    return grid;
}

// A family's launch list is a class template F<BM, BN, ACT> (ACT = KoafGemm.act16) with a static run(g, grid, s), written with the
// macros below: BM, BN, VEC, F16, ACT, g, grid, pgrid and s are names of the enclosing run().
template <template <int, int, int> class F, int ACT>
int launch_tile(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    if (tp.bm == 128 && tp.bn == 128) return F<128, 128, ACT>::run(g, grid, s);
    if (tp.bm == 128 && tp.bn == 64) return F<128, 64, ACT>::run(g, grid, s);
    if (tp.bm == 64 && tp.bn == 128) return F<64, 128, ACT>::run(g, grid, s);
    return F<64, 64, ACT>::run(g, grid, s);
}
template <template <int, int, int> class F>
int launch_tile_act(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    switch (g.act16) {
        case 0: return launch_tile<F, 0>(g, tp, grid, s);
        case 1: return launch_tile<F, 1>(g, tp, grid, s);
        case 2: return launch_tile<F, 2>(g, tp, grid, s);
        case 3: return launch_tile<F, 3>(g, tp, grid, s);
    }
    return KOAF_NO_KERNEL;
}

}  // namespace

#define KOAF_LAUNCH(AMODE, BMODE, TA, TB)                                                                        \
    koaf_log_launch("koaf_gemm", g, grid, grid);                                                                 \
    hipLaunchKernelGGL((koaf_gemm_kernel<BM, BN, AMODE, BMODE, TA, TB, VEC, F16, 256, ACT>), grid, dim3(256), 0, s, g);      \
    return koaf_check_launch("koaf_gemm")
// the persistent variants (fp32 A loader + weight tiles by DMA): at most two blocks per CU, each walking its tiles
#define KOAF_LAUNCH_P(AMODE, BMODE, TA, TB)                                                                      \
    koaf_log_launch("koaf_gemm", g, grid, persist_mode(AMODE, BMODE, F16, TA) ? pgrid : grid);                   \
    hipLaunchKernelGGL((koaf_gemm_kernel<BM, BN, AMODE, BMODE, TA, TB, VEC, F16, 256, ACT>), (persist_mode(AMODE, BMODE, F16, TA) ? pgrid : grid), dim3(256), 0, s, g);     \
    return koaf_check_launch("koaf_gemm")

// KoafGemm.out_planes (the epilogue also cuts the consumer's plane images): the instantiations with EMIT, for the calls that use it
// -- dense 1x1 forward convolutions with weight plane images (plain, BatchNorm-prologue and bottleneck-tail loaders)
#define KOAF_LAUNCH_E(AMODE, BMODE, TA, TB)                                                                      \
    koaf_log_launch("koaf_gemm/emit", g, grid, grid);                                                            \
    hipLaunchKernelGGL((koaf_gemm_kernel<BM, BN, AMODE, BMODE, TA, TB, VEC, F16, 256, ACT, true>), grid, dim3(256), 0, s, g);      \
    return koaf_check_launch("koaf_gemm/emit")
#define KOAF_LAUNCH_PE(AMODE, BMODE, TA, TB)                                                                     \
    koaf_log_launch("koaf_gemm/emit", g, grid, persist_mode(AMODE, BMODE, F16, TA) ? pgrid : grid);              \
    hipLaunchKernelGGL((koaf_gemm_kernel<BM, BN, AMODE, BMODE, TA, TB, VEC, F16, 256, ACT, true>), (persist_mode(AMODE, BMODE, F16, TA) ? pgrid : grid), dim3(256), 0, s, g);     \
    return koaf_check_launch("koaf_gemm/emit")

// the streamed dense A operand (M_KS, StreamA) in front of weight plane images: SD = 2 k-tiles in flight per wave
#define KOAF_LAUNCH_S(TA, EM)                                                                                    \
    koaf_log_launch("koaf_gemm/stream", g, grid, (TA) < 2 ? pgrid : grid);                                       \
    hipLaunchKernelGGL((koaf_gemm_kernel<BM, BN, M_KS, M_PS, TA, 0, VEC, F16, 256, ACT, EM, 2>), ((TA) < 2 ? pgrid : grid), dim3(256), 0, s, g);      \
    return koaf_check_launch("koaf_gemm/stream")
// (SD = 4 -- four k-tiles in flight, one tile per block, for the one-source loaders with K >= 256 -- builds without spills (213
// registers) and was measured on the headline step: 1977.2 ms against 1974.4 ms with SD = 2 everywhere; not instantiated.)
