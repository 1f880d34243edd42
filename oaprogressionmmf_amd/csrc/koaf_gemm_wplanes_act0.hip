// koaf_gemm_wplanes_act0.hip -- A x weight plane images (koaf_gemm_wplanes.h) with fp32 activation storage (act16 0)
#include "koaf_gemm_wplanes.h"

int koaf_launch_wplanes_act0(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) { return wplanes_run<0>(g, tp, grid, s); }
