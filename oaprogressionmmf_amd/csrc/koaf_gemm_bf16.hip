// koaf_gemm_bf16.hip -- the koaf_gemm_kernel instantiations on the bf16 x 3 scheme (fmt 0; fp32 operands on both sides): linear
// layers and attention contractions (dense pairs), convolutions without scale information, and the one scalar-path kernel set
// (VEC = false: unaligned operands, 64 x 64 tiles).  ACT (bf16 activation storage): the pairs of its role only -- 1 forward
// convolutions, 3 weight gradients.
#include "koaf_gemm_launch.h"

namespace {
template <int BM, int BN, int ACT, bool VEC>
struct Bf16Modes {
    static int run(const KoafGemm& g, dim3 grid, hipStream_t s) {
        constexpr bool F16 = false;
        const int am = operand_mode(g.A), bm = operand_mode(g.B);
        const int ta = g.A.tf, tb = g.B.tf;
        if constexpr (ACT == 0) {
            if (am == M_KC && bm == M_KC && !tb) { if (ta == 1) { KOAF_LAUNCH(M_KC, M_KC, 1, 0); } else if (!ta) { KOAF_LAUNCH(M_KC, M_KC, 0, 0); } }
            if (am == M_KC && bm == M_KM && !ta && !tb) { KOAF_LAUNCH(M_KC, M_KM, 0, 0); }
            if (am == M_KM && bm == M_KM && !ta) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM, 0, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM, 0, 0); } }
        }
        if constexpr (VEC) {
            if constexpr (ACT == 0 || ACT == 1) {
                if (am == M_KC_G1 && bm == M_KC && !tb) { if (ta == 1) { KOAF_LAUNCH(M_KC_G1, M_KC, 1, 0); } else if (!ta) { KOAF_LAUNCH(M_KC_G1, M_KC, 0, 0); } }
            }
            if constexpr (ACT == 0) {
                if (am == M_KC_G2 && bm == M_KM_G3 && !ta && !tb) { KOAF_LAUNCH(M_KC_G2, M_KM_G3, 0, 0); }
            }
            if constexpr (ACT == 0 || ACT == 3) {
                if (am == M_KM && bm == M_KM_G1 && !ta) { if (tb == 1) { KOAF_LAUNCH(M_KM, M_KM_G1, 0, 1); } else if (!tb) { KOAF_LAUNCH(M_KM, M_KM_G1, 0, 0); } }
            }
        }
        return KOAF_NO_KERNEL;
    }
};
template <int BM, int BN, int ACT> using Bf16VecModes = Bf16Modes<BM, BN, ACT, true>;
}  // namespace

int koaf_launch_bf16(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    if (!tp.vec) return g.act16 == 0 ? Bf16Modes<64, 64, 0, false>::run(g, grid, s) : KOAF_NO_KERNEL;
    return launch_tile_act<Bf16VecModes>(g, tp, grid, s);
}
