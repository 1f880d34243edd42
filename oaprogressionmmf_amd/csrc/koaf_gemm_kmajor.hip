// koaf_gemm_kmajor.hip -- the M_PK x M_PK | M_PKG instantiations of koaf_gemm_kernel: both operands K-major from activation plane
// images by LDS-DMA (PlaneKLoader) -- the weight gradients of the convolutions whose activations live as plane images (k = pixel).
#include "koaf_gemm_launch.h"

namespace {
template <int BM, int BN, int ACT>
struct KmajorModes {
    static int run(const KoafGemm& g, dim3 grid, hipStream_t s) {
        constexpr bool VEC = true, F16 = true;
        if (operand_mode(g.B) == M_PKG) { KOAF_LAUNCH(M_PK, M_PKG, 0, 0); }
        KOAF_LAUNCH(M_PK, M_PK, 0, 0);
    }
};
}  // namespace

int koaf_launch_kmajor(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    return g.act16 == 0 ? launch_tile<KmajorModes, 0>(g, tp, grid, s) : KOAF_NO_KERNEL;
}
