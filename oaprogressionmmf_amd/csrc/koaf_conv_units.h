// koaf_conv_units.h -- the dedicated convolution units behind koaf_conv.hip: per unit its dispatch rule and its entry point.
// A rule is defined ONCE, next to its kernel, with its prose.  It reads the descriptor koaf_conv.hip builds (plus the one fact that does
// not carry, where there is one) and holds both halves: what the kernel can run, and the policy that decides which of those calls it
// should run.  koaf_conv.hip asks the rule and calls the entry, which opens with KOAF_REQUIRE(<the same rule>): no second list.
#pragma once
#include "koaf_common.h"

bool koaf_stream_on();      // koaf_gemm.hip: koaf_set_stream's switch

// koaf_fwd_s2.hip: the stride-2 forward convolutions (1x1 / pad 0, 3x3 / pad 1) on 256-row tiles
bool koaf_fwd_s2_ok(const KoafGemm& g);
int koaf_fwd_s2(const KoafGemm& g, void* stream);

// koaf_fwd1.hip: the dense 1x1 / stride-1 forward convolutions on 256-row tiles; _form: the form of a (Cin, Cout), _ok: of g; -1: none
int koaf_fwd1_form(int K, int N);
int koaf_fwd1_ok(const KoafGemm& g);
int koaf_fwd1(const KoafGemm& g, void* stream);

// koaf_dgrad_s2.hip: one parity class of a stride-2 data gradient on 256-row tiles; KH x KW is the filter of the whole call
bool koaf_dgrad_s2_ok(const KoafGemm& g, int KH, int KW);
int koaf_dgrad_s2(const KoafGemm& g, int KH, int KW, void* stream);

// koaf_wgrad1.hip: 1x1 / stride 1, and stride 2 (1x1 / pad 0, 3x3 / pad 1), on 256-wide tiles under the split-K plan in g.splitk
bool koaf_wgrad1_ok(const KoafGemm& g, int* bm = nullptr, int* bn = nullptr);
int koaf_wgrad1(const KoafGemm& g, void* stream);

// koaf_wgrad3.hip: 3x3 / stride 1 / pad 1 over plane images, both tensors walked once in padded raster order
bool koaf_wgrad3_ring_ok(int N, int H, int W, int Cin, int Cout);
int64_t koaf_wgrad3_ring_ws(int N, int H, int W, int Cin, int Cout);
int koaf_wgrad3_ring(const uint16_t* dy_planes, const uint16_t* x_planes, float* dw, float* slabs, const float* dy_amax,
                     float x_scale, int N, int H, int W, int Cin, int Cout, void* stream);
