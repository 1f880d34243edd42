// koaf_gemm_wplanes_act2.hip -- A x weight plane images (koaf_gemm_wplanes.h), data gradients with bf16 activation storage
// (act16 2: A.ptr2 and the BatchNorm-backward operands of the epilogue)
#include "koaf_gemm_wplanes.h"

int koaf_launch_wplanes_act2(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) { return wplanes_run<2>(g, tp, grid, s); }
