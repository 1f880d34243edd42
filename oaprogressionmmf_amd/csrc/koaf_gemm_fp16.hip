// koaf_gemm_fp16.hip -- the koaf_gemm_kernel instantiations with fp32 operands on both sides (TileLoader x TileLoader) on the fp16
// scheme (fmt 1): convolutions on fp32 weights -- forward (KC | KC_G1 x KC), data gradient (KC x KM, KC_G2 x KM_G3) -- and the weight
// gradients (KM x KM | KM_G1), also with the BatchNorm-backward apply formed in the A loader (tf 2).  tf only where a BatchNorm
// prologue exists.  ACT (bf16 activation storage): only the weight gradients (3) have a role here.
#include "koaf_gemm_launch.h"

namespace {
template <int BM, int BN, int ACT>
struct Fp16Modes {
    static int run(const KoafGemm& g, dim3 grid, hipStream_t s) {
        constexpr bool VEC = true, F16 = true;
        const int am = operand_mode(g.A), bm = operand_mode(g.B);
        const int ta = g.A.tf, tb = g.B.tf;
        if constexpr (ACT == 0) {
            if (am == M_KC && bm == M_KC && !tb) { if (ta == 1) { KOAF_LAUNCH(M_KC, M_KC, 1, 0); } else if (!ta) { KOAF_LAUNCH(M_KC, M_KC, 0, 0); } }
            if (am == M_KC && bm == M_KM && !ta && !tb) { KOAF_LAUNCH(M_KC, M_KM, 0, 0); }
            if (am == M_KM && bm == M_KM && !ta) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM, 0, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM, 0, 0); } }
            if (am == M_KC_G1 && bm == M_KC && !tb) { if (ta == 1) { KOAF_LAUNCH(M_KC_G1, M_KC, 1, 0); } else if (!ta) { KOAF_LAUNCH(M_KC_G1, M_KC, 0, 0); } }
            if (am == M_KC_G2 && bm == M_KM_G3 && !ta && !tb) { KOAF_LAUNCH(M_KC_G2, M_KM_G3, 0, 0); }
            if (am == M_KM && bm == M_KM_G1 && !ta) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM_G1, 0, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM_G1, 0, 0); } }
        }
        if constexpr (ACT == 0 || ACT == 3) {
            // weight gradient with the BatchNorm-backward apply formed in the A loader (dy = sc * dz + sh - sc2 * c)
            if (am == M_KM && bm == M_KM && ta == 2) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM, 2, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM, 2, 0); } }
            if (am == M_KM && bm == M_KM_G1 && ta == 2) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM_G1, 2, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM_G1, 2, 0); } }
        }
        return KOAF_NO_KERNEL;
    }
};
}  // namespace

int koaf_launch_fp16(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) { return launch_tile_act<Fp16Modes>(g, tp, grid, s); }
