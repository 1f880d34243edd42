// koaf_gemm_wplanes.h -- the launch lists of every koaf_gemm_kernel instantiation whose B operand is weight plane images (M_PS),
// the streamed A operand aside (koaf_gemm_stream.hip): the convolutions, forward and data gradient, with the A operand
//   - through the fp32 loader (M_KC | M_KC_G1 | M_KC_G2: 1x1 and strided convolutions; persistent and out_planes variants),
//   - as gathered activation plane images (M_PA1 forward, M_PA2 data gradient),
//   - as activation plane images of a 3x3 / stride 1 / pad 1 convolution: M_PH, the tile's pixel rows + halo in LDS for all nine
//     taps (256 rows x 512 threads, or 128 rows x 256 threads), and M_PT, 8 x 16 pixel rectangle tiles (TilePlan.t2d).
// It is the heaviest group, and it is cut by activation-storage role, one file per ACT (koaf_gemm_wplanes_act0 / 1 / 2.hip), not by
// A mode: kernels of different A modes share the epilogue instantiation of their (tile, ACT), and hipcc compiles a kernel that is
// the only user of one in its file slightly differently (a few registers, reordered instructions) from one that shares it.
#pragma once
#include "koaf_gemm_launch.h"

namespace {
template <int BM, int BN, int ACT>
struct WplaneModes {
    static int run(const KoafGemm& g, dim3 grid, hipStream_t s) {
        constexpr bool VEC = true, F16 = true;
        const int am = operand_mode(g.A), ta = g.A.tf;
        [[maybe_unused]] const dim3 pgrid = persist_grid(grid);
        if (g.out_planes) {
            if constexpr (ACT == 0 || ACT == 1) {
                if (am == M_KC && ta == 3) { KOAF_LAUNCH_E(M_KC, M_PS, 3, 0); }
                if (am == M_KC && ta < 2) { if (ta == 1) { KOAF_LAUNCH_PE(M_KC, M_PS, 1, 0); } else { KOAF_LAUNCH_PE(M_KC, M_PS, 0, 0); } }
            }
            return KOAF_NO_KERNEL;
        }
        if constexpr (ACT == 0 || ACT == 1) {
            if (am == M_KC && ta == 3) { KOAF_LAUNCH(M_KC, M_PS, 3, 0); }
            if (am == M_KC && ta < 2) { if (ta == 1) { KOAF_LAUNCH_P(M_KC, M_PS, 1, 0); } else { KOAF_LAUNCH_P(M_KC, M_PS, 0, 0); } }
            if (am == M_KC_G1 && ta < 2) { if (ta) { KOAF_LAUNCH_P(M_KC_G1, M_PS, 1, 0); } else { KOAF_LAUNCH_P(M_KC_G1, M_PS, 0, 0); } }
            if (am == M_PA1) { KOAF_LAUNCH(M_PA1, M_PS, 0, 0); }
        }
        if constexpr (ACT == 0 || ACT == 2) {
            if (am == M_KC && ta == 2) { KOAF_LAUNCH(M_KC, M_PS, 2, 0); }
            if (am == M_KC_G2 && ta != 1) { if (ta) { KOAF_LAUNCH(M_KC_G2, M_PS, 2, 0); } else { KOAF_LAUNCH_P(M_KC_G2, M_PS, 0, 0); } }
            if (am == M_PA2) { KOAF_LAUNCH(M_PA2, M_PS, 0, 0); }
        }
        if constexpr (ACT == 2) {       // (a data gradient whose dy is a tensor: only the epilogue's operands are bf16)
            if (am == M_KC && ta == 0) { KOAF_LAUNCH(M_KC, M_PS, 0, 0); }
        }
        return KOAF_NO_KERNEL;
    }
};

// the 3x3 plane-image kernels (they read plane images: only their epilogue sees the storage type -- forward (1): the output; data
// gradient (2): the BatchNorm-backward operands)
template <int ACT>
int conv3_run(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    if (tp.t2d) {
        koaf_log_launch("koaf_gemm/t2d", g, grid, grid);
        hipLaunchKernelGGL((koaf_gemm_kernel<128, 64, M_PT, M_PS, 0, 0, true, true, 256, ACT>), grid, dim3(256), 0, s, g);
        return koaf_check_launch("koaf_gemm/t2d");
    }
    koaf_log_launch(tp.bm == 128 ? "koaf_gemm/halo128" : "koaf_gemm/halo", g, grid, grid);
    if (tp.bm == 128) {
        if (tp.bn == 128) hipLaunchKernelGGL((koaf_gemm_kernel<128, 128, M_PH, M_PS, 0, 0, true, true, 256, ACT>), grid, dim3(256), 0, s, g);
        else hipLaunchKernelGGL((koaf_gemm_kernel<128, 64, M_PH, M_PS, 0, 0, true, true, 256, ACT>), grid, dim3(256), 0, s, g);
        return koaf_check_launch("koaf_gemm/halo128");
    }
    if (tp.bn == 128) hipLaunchKernelGGL((koaf_gemm_kernel<256, 128, M_PH, M_PS, 0, 0, true, true, 512, ACT>), grid, dim3(512), 0, s, g);
    else hipLaunchKernelGGL((koaf_gemm_kernel<256, 64, M_PH, M_PS, 0, 0, true, true, 512, ACT>), grid, dim3(512), 0, s, g);
    return koaf_check_launch("koaf_gemm/halo");
}

template <int ACT>
int wplanes_run(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    if (tp.t2d || tp.halo) return conv3_run<ACT>(g, tp, grid, s);
    return launch_tile<WplaneModes, ACT>(g, tp, grid, s);
}
}  // namespace
