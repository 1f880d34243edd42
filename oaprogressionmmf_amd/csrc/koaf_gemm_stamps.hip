// koaf_gemm_stamps.hip -- the diagnostic build with in-kernel phase stamps (make stamps -> libkoaf_stamps.so, scripts/stamps_*.py;
// never loaded by the product: KOAF_LIB selects it).  The stamp table is a __device__ variable, of which every translation unit's
// code object would get its own copy, so this is the one place where all GEMM families are compiled as ONE unit, beside the
// function that reads the table.  Built with -DKOAF_STAMPS.
#include "koaf_gemm_stream.hip"
#include "koaf_gemm_wplanes_act0.hip"
#include "koaf_gemm_wplanes_act1.hip"
#include "koaf_gemm_wplanes_act2.hip"
#include "koaf_gemm_kmajor.hip"
#include "koaf_gemm_fp16.hip"
#include "koaf_gemm_bf16.hip"

// out[8] = {prologue, k-loop, staging, stores, tile, chunk waits, -, tiles} summed over blocks, in 10 ns ticks; reset: zero the table
extern "C" int koaf_debug_stamps(unsigned long long* out, int reset) {
    static unsigned long long h[64][8];
    if (hipDeviceSynchronize() != hipSuccess) return KOAF_ELAUNCH;
    if (out) {
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(koaf_stamp_tab), sizeof(h)) != hipSuccess) return KOAF_ELAUNCH;
        for (int k = 0; k < 8; ++k) { out[k] = 0; for (int r = 0; r < 64; ++r) out[k] += h[r][k]; }
    }
    if (reset) {
        for (int r = 0; r < 64; ++r) for (int k = 0; k < 8; ++k) h[r][k] = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(koaf_stamp_tab), h, sizeof(h)) != hipSuccess) return KOAF_ELAUNCH;
    }
    return KOAF_OK;
}
