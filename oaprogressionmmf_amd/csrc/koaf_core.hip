// koaf_core.hip -- what every other unit of libkoaf links against: the error text of the last refused call, the numerics
// status pointer and the library version.  Host only, no kernel.
#include <stdarg.h>
#include "koaf_common.h"

static thread_local char g_err[512] = "";
void koaf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* koaf_last_error(void) { return g_err; }
static uint32_t* g_status = nullptr;
uint32_t* koaf_status_ptr() { return g_status; }
extern "C" int koaf_set_status_buffer(uint32_t* dev4) { g_status = dev4; return KOAF_OK; }

// KOAF_VERSION (koaf.h), what each step added:
//   2.0  koaf_sgd_step / koaf_rmsprop_step / koaf_optim_hyper (koaf_optim.hip), koaf_bce_loss / koaf_bce_ws (koaf_bce.hip)
//   1.9  koaf_launch_log / koaf_launch_log_read (host-side record of the koaf_gemm launches, for tests)
//   1.8  koaf_set_stream (streamed kernel of the dense 1x1 convolutions, KoafGemm A mode M_KS)
//   1.7  KoafEmit / KoafGemm.out_planes (epilogue cuts the consumer's plane images), loss labels outside [0, C)
//   1.6  KoafTail.idt_sc / idt_sh (tails behind a downsample branch), koaf_stem_fwd statistics, koaf_stem_wgrad dy_apply,
//        koaf_bn_bwd_reduce_pool
extern "C" int koaf_version(void) { return KOAF_VERSION; }
