// koaf_gemm_wplanes_act1.hip -- A x weight plane images (koaf_gemm_wplanes.h), forward convolutions with bf16 activation storage
// (act16 1: A.ptr and C)
#include "koaf_gemm_wplanes.h"

int koaf_launch_wplanes_act1(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) { return wplanes_run<1>(g, tp, grid, s); }
