// koaf_gemm_stream.hip -- the M_KS x M_PS instantiations of koaf_gemm_kernel: the dense K-contiguous fp32 A operand streamed per
// wave (StreamA) in front of weight plane images -- the 1x1 / stride-1 convolutions and their data gradients.  One shape: 128-row
// tiles, fp16 scheme, fp32 activation storage (TilePlan.stream says when).
#include "koaf_gemm_launch.h"

namespace {
template <int BN>
int stream_run(const KoafGemm& g, dim3 grid, hipStream_t s) {
    constexpr int BM = 128, ACT = 0;
    constexpr bool VEC = true, F16 = true;
    const int ta = g.A.tf;
    const dim3 pgrid = persist_grid(grid);
    if (g.out_planes) {
        if (ta == 0) { KOAF_LAUNCH_S(0, true); }
        if (ta == 1) { KOAF_LAUNCH_S(1, true); }
        if (ta == 3) { KOAF_LAUNCH_S(3, true); }
    } else {
        if (ta == 0) { KOAF_LAUNCH_S(0, false); }
        if (ta == 1) { KOAF_LAUNCH_S(1, false); }
        if (ta == 2) { KOAF_LAUNCH_S(2, false); }
        if (ta == 3) { KOAF_LAUNCH_S(3, false); }
    }
    return KOAF_NO_KERNEL;
}
}  // namespace

int koaf_launch_stream(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    return tp.bn == 128 ? stream_run<128>(g, grid, s) : stream_run<64>(g, grid, s);
}
