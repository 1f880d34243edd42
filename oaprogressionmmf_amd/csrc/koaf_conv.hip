// koaf_conv.hip -- dense and grouped convolution entry points built on koaf_gemm: the operand descriptors of the forward pass, the
// data gradients and the weight gradients (split-K plan: wgrad_plan), plus the grouped-conv weight expansion.
#include "koaf_common.h"
#include "koaf_conv_units.h"

namespace {

inline int64_t rup32(int64_t v) { return (v + 31) / 32 * 32; }

// fp16 scheme with the activations at their fixed scale; B operand = the F plane image [2][R][Kp] of a weight [R][K]
// (koaf_wplanes_build) when the image is there, else the fp32 weight split in the kernel at the same scale
inline void set_fimg(KoafGemm* g, const KoafWImg* w, int R, int64_t K) {
    g->fmt = 1;
    g->A.fscale = KOAF_ACT_SCALE;
    g->B.amax = w->amax;
    if (!w->f) return;
    g->B.kind = 2; g->B.gather = 0;
    g->B.planes = w->f; g->B.ld = rup32(K); g->B.plane_stride = (int64_t)R * g->B.ld;
}

// A operand from activation plane images (koaf_act_planes): the transform is in the image
inline void set_aplanes(KoafOperand* a, const uint16_t* planes, int64_t plane_elems) {
    a->kind = 2; a->planes = planes; a->plane_stride = plane_elems; a->zeros = planes + 2 * plane_elems;
    a->ptr = nullptr; a->ptr2 = nullptr; a->tf = 0; a->sc = a->sh = a->sc2 = nullptr;
}

// operand gathered from an NHWC image: H x W pixels of C channels at channel stride CS, walked by a KH x KW filter over a PH x PW grid
// (gather 1: the forward / weight-gradient walk of the input; 2: the transposed walk of the data gradient)
inline void set_gather(KoafOperand* o, int gather, int H, int W, int C, int CS, int PH, int PW, int KH, int KW, int stride, int pad_h,
                       int pad_w) {
    o->gather = gather;
    o->H = H; o->W = W; o->C = C; o->CS = CS;
    o->PH = PH; o->PW = PW;
    o->KH = KH; o->KW = KW; o->stride = stride; o->pad = pad_h; o->pad_w = pad_w;
}

// a 1x1 / stride-1 / unpadded convolution is a plain GEMM over the pixels: no gather
inline bool is_pointwise(int KH, int KW, int stride, int pad) { return KH == 1 && KW == 1 && stride == 1 && pad == 0; }

// split-K plan for weight gradients: M x N output, K = pixels.  ~1024 blocks, >= 512 k-rows per split.
struct WgradPlan { int bm, bn, splitk; };
inline WgradPlan wgrad_plan(int M, int N, int64_t K, int ctap, int batch) {
    WgradPlan p;
    p.bn = (N >= 128 && (ctap % 4) == 0) ? 128 : 64;      // (a B tile may span filter taps)
    p.bm = (M >= 128) ? 128 : 64;
    int64_t tiles = cdiv64(M, p.bm) * cdiv64(N, p.bn) * batch;
    int64_t sk = 1024 / tiles;
    int64_t kmax = cdiv64(K, 512);
    if (sk > kmax) sk = kmax;
    if (sk < 1) sk = 1;
    if (sk > 4096) sk = 4096;
    if (sk > 8) {
        // multiples of 8 (the kernel then keeps all tiles of a k-range on one XCD = one L2); among those between 3/4 and
        // twice the target, the count that fills whole rounds of the chip's 512 block slots best
        int64_t best = sk & ~7ll;
        double beff = 0.0;
        for (int64_t c = ((sk * 3 / 4) + 7) & ~7ll; c <= 2 * sk && c <= kmax && c <= 4096; c += 8) {
            const int64_t blocks = tiles * c;
            const double eff = (double)blocks / (double)(cdiv64(blocks, 512) * 512);
            if (eff > beff + 0.02) { beff = eff; best = c; }
        }
        sk = best;
    }
    p.splitk = (int)sk;
    return p;
}

// ---------------------------------------------------------------------------------------------
// slab reduce with batch: slabs [nb][ns][n] -> out [nb][n]
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) slab_reduce_b_kernel(const float* __restrict__ slabs, int ns, int64_t n,
                                                            float* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float* sb = slabs + (int64_t)blockIdx.y * ns * n;
    v4f a = *(const v4f*)(sb + i);
    for (int s = 1; s < ns; ++s) a += *(const v4f*)(sb + (int64_t)s * n + i);
    *(v4f*)(out + (int64_t)blockIdx.y * n + i) = a;
}

// ---------------------------------------------------------------------------------------------
// grouped 3x3: weights [C][9][Cg] <-> block-diagonal 64-channel slabs [C/64][64][9][64]
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gconv_expand_kernel(const float* __restrict__ w, float* __restrict__ wexp,
                                                           int C, int Cg, float* __restrict__ amax) {
    const int64_t total = (int64_t)C * 9 * 64;
    unsigned mb = 0u;          // largest magnitude seen by this thread, as bits (a NaN / Inf compares above every finite value)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i & 63);
        int64_t r = i >> 6;
        const int tap = (int)(r % 9);
        const int co = (int)(r / 9);  // global output channel; slab = co/64
        const int col = co & 63;
        const int g0 = (col / Cg) * Cg;  // first slab-local input channel of co's group
        float v = 0.f;
        if (ci >= g0 && ci < g0 + Cg) v = w[((int64_t)co * 9 + tap) * Cg + (ci - g0)];
        wexp[i] = v;
        mb = max(mb, koaf_absbits(v));
    }
    if (amax != nullptr) block_amax_raise_bits(mb, amax);
}
__global__ void __launch_bounds__(256) gconv_compress_kernel(const float* __restrict__ dwexp, float* __restrict__ dw,
                                                             int C, int Cg) {
    const int64_t total = (int64_t)C * 9 * Cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cg = (int)(i % Cg);
        int64_t r = i / Cg;
        const int tap = (int)(r % 9);
        const int co = (int)(r / 9);
        const int g0 = ((co & 63) / Cg) * Cg;
        dw[i] = dwexp[((int64_t)co * 9 + tap) * 64 + g0 + cg];
    }
}

}  // namespace

// ================================================================================================
// dense convolution
// ================================================================================================
// (the 256-row units and their dispatch rules: koaf_conv_units.h; each rule is written next to its kernel)
extern "C" int koaf_conv2d_fwd(const float* x, const float* w, float* y, int32_t N, int32_t H, int32_t W, int32_t Cin,
                               int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, const float* in_sc,
                               const float* in_sh, float* stats, int32_t* stats_rows, const float* stats_shift,
                               const KoafWImg* wimg, const uint16_t* x_planes, const KoafTail* tail, const KoafEmit* emit,
                               int32_t act16, void* stream) {
    KOAF_REQUIRE((x || x_planes) && w && y && N > 0 && Cin % 32 == 0 && Cout % 4 == 0, "koaf_conv2d_fwd: bad args (Cin=%d Cout=%d)",
                 Cin, Cout);
    KOAF_REQUIRE(!tail || (tail->idt && x && in_sc && in_sh && !x_planes && is_pointwise(KH, KW, stride, pad) && wimg &&
                           wimg->amax && wimg->f && (tail->idt_sc == nullptr) == (tail->idt_sh == nullptr)),
                 "koaf_conv2d_fwd: the fused bottleneck tail serves 1x1 / stride-1 convolutions with weight plane images, from x / in_sc / in_sh");
    KOAF_REQUIRE((in_sc == nullptr) == (in_sh == nullptr), "koaf_conv2d_fwd: in_sc/in_sh come together");
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    const int64_t M = (int64_t)N * OH * OW;
    KOAF_REQUIRE(M < (1ll << 31), "koaf_conv2d_fwd: too many output pixels");
    KoafGemm g;
    zero_gemm(&g);
    g.A.ptr = x;
    g.A.kind = 0;
    if (is_pointwise(KH, KW, stride, pad) && !x_planes) {
        g.A.gather = 0;
        g.A.ld = Cin;
    } else          // (plane images are always addressed as a gather, a 1x1 kernel being its one-tap case)
        set_gather(&g.A, 1, H, W, Cin, Cin, OH, OW, KH, KW, stride, pad, pad);
    if (in_sc) { g.A.tf = 1; g.A.sc = in_sc; g.A.sh = in_sh; }
    if (tail) { g.A.tf = 3; g.A.ptr2 = tail->idt; g.A.side = tail->y_out; g.A.sc2 = tail->idt_sc; g.A.sh2 = tail->idt_sc ? tail->idt_sh : nullptr; }
    g.B.ptr = w;
    g.B.kind = 0;
    g.B.ld = (int64_t)KH * KW * Cin;
    g.M = (int)M; g.N = Cout; g.K = KH * KW * Cin;
    if (wimg && wimg->amax) set_fimg(&g, wimg, Cout, g.K);
    if (x_planes) {
        KOAF_REQUIRE(g.A.gather == 1 && g.B.kind == 2, "koaf_conv2d_fwd: x_planes serve the gathered kernels and need wimg->f");
        set_aplanes(&g.A, x_planes, (int64_t)N * H * W * Cin);
    }
    g.C = y; g.ldc = Cout;
    g.stats = stats;
    g.stats_shift = stats ? stats_shift : nullptr;
    g.act16 = act16 ? 1 : 0;            // (x and y are bf16 activations)
    if (emit) {
        KOAF_REQUIRE(emit->planes && emit->sc && emit->sh && (Cout % 8) == 0, "koaf_conv2d_fwd: emit needs planes / sc / sh and Cout %% 8 == 0");
        g.out_planes = emit->planes; g.out_sc = emit->sc; g.out_sh = emit->sh; g.out_ps = M * Cout;
    }
    const bool s2 = koaf_fwd_s2_ok(g);
    if (s2 || koaf_fwd1_ok(g) >= 0) {
        if (stats_rows) *stats_rows = g.M / 128;        // two partial rows per 256-row tile: the rows of a 128-row tiling
        return s2 ? koaf_fwd_s2(g, stream) : koaf_fwd1(g, stream);
    }
    if (stats_rows) *stats_rows = koaf_gemm_part_rows(&g);
    return koaf_gemm(&g, stream);
}

// upper bound of the statistics rows koaf_conv2d_fwd writes for M output pixels (64-row tiles everywhere)
extern "C" int32_t koaf_conv2d_stats_rows(int64_t M, int32_t Cout) { return (int32_t)cdiv64(M, 64); }

// A operand = dy formed on load from (dz, c): dy = coef0 * dz + coef3 - coef2 * c (koaf_bn_bwd_finalize)
static void set_apply(KoafOperand* a, const KoafBnApply* ap, int C) {
    a->ptr = ap->dz; a->ptr2 = ap->c; a->tf = 2;
    a->sc = ap->coef; a->sc2 = ap->coef + 2 * (int64_t)C; a->sh = ap->coef + 3 * (int64_t)C;
    a->amax = ap->amax;
}

static void set_bnb(KoafGemm* g, const KoafBnb* b, float* part) {
    if (!b) return;
    g->bnb_amax = b->dz_amax;
    g->bnb_mode = b->mode;
    g->bnb_c = b->c; g->bnb_y = b->y; g->bnb_sc = b->sc; g->bnb_sh = b->sh;
    g->bnb_mean = b->mean; g->bnb_invstd = b->invstd;
    g->bnb2_c = b->c2; g->bnb2_mean = b->mean2; g->bnb2_invstd = b->invstd2;
    g->bnb_part = part;
}

extern "C" int32_t koaf_conv2d_dgrad_bnb_rows(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t stride) {
    // upper bound: 64-row tiles; stride 2 = four parity classes
    if (stride == 2) {
        int64_t r = 0;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) r += cdiv64((int64_t)N * ((H - py + 1) / 2) * ((W - px + 1) / 2), 64);
        return (int32_t)r;
    }
    return (int32_t)cdiv64((int64_t)N * H * W, 64);
}

extern "C" int koaf_conv2d_dgrad_bnb(const float* dy, const float* w, float* dx, int32_t N, int32_t H, int32_t W,
                                     int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                     const float* residual, const KoafBnb* bnb, float* part, int32_t* part_rows,
                                     const KoafWImg* wimg, const float* dy_amax, const KoafBnApply* dy_apply,
                                     const uint16_t* dy_planes, int32_t act16, void* stream) {
    KOAF_REQUIRE(!dy_planes || (wimg && wimg->amax && wimg->d && (dy_amax || dy_apply) && KH * KW > 1),
                 "koaf_conv2d_dgrad: dy_planes need the weight's D plane image, dy_amax and a gathered (KH*KW > 1) kernel");
    KOAF_REQUIRE((dy || dy_apply || dy_planes) && w && dx && N > 0 && Cout % 32 == 0 && Cin % 4 == 0, "koaf_conv2d_dgrad: bad args");
    KOAF_REQUIRE(!dy_apply || (dy_apply->dz && dy_apply->c && dy_apply->coef && dy_apply->amax && wimg && wimg->amax && wimg->d),
                 "koaf_conv2d_dgrad: dy_apply needs dz / c / coef / amax and the weight's D plane image");
    if (dy_apply) { dy = dy_apply->dz; dy_amax = dy_apply->amax; }
    if (bnb && bnb->dz_amax && hipMemsetAsync(bnb->dz_amax, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) {
        koaf_set_error("koaf_conv2d_dgrad_bnb: memset failed");
        return KOAF_ELAUNCH;
    }
    // fp16 scheme when both operands' magnitudes are known; the weight tiles then come from the D image [2][Cin][KH*KW*Cout]
    // (rows = input channels, k = (tap, output channel): the k order of the gathered dy) if it is there
    const bool f16 = wimg && wimg->amax && dy_amax;
    const bool ps = f16 && wimg->d != nullptr;
    const uint16_t* w_dimg = ps ? wimg->d : nullptr;
    const int64_t dld = (int64_t)KH * KW * Cout, dps = (int64_t)Cin * dld;
    KOAF_REQUIRE(!bnb || (part && part_rows), "koaf_conv2d_dgrad_bnb: part / part_rows required");
    const int nsum = (bnb && bnb->c2) ? 3 : 2;
    int rows_done = 0;
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    const int64_t M = (int64_t)N * H * W;
    KOAF_REQUIRE(M < (1ll << 31), "koaf_conv2d_dgrad: too many pixels");
    KoafGemm g;
    if (stride == 2) {
        // Parity decomposition: input pixel (y, x) only sees taps kh = (y+pad) mod 2 (+2, +4, ...), so the four
        // classes (y%2, x%2) are four stride-1 transposed gathers over their own tap subsets -- 4x less MFMA work
        // than multiplying the structural zeros of the plain gather.  Each class scatters its rows straight from
        // the epilogue (row map); a class with no tap (1x1 kernels) just writes residual / zero.
        // (koaf_dgrad_s2 on class (0, 0) of a 1x1 shortcut also writes the three classes without a tap: all_done)
        bool all_done = false;
        for (int py = 0; py < 2 && !all_done; ++py)
            for (int px = 0; px < 2 && !all_done; ++px) {
                const int Hc = (H - py + 1) / 2, Wc = (W - px + 1) / 2;
                if (Hc <= 0 || Wc <= 0) continue;
                const int khs = (py + pad) & 1, kws = (px + pad) & 1;
                const int nkh = khs < KH ? (KH - khs + 1) / 2 : 0, nkw = kws < KW ? (KW - kws + 1) / 2 : 0;
                const int offy = (py + pad - khs) / 2, offx = (px + pad - kws) / 2;
                zero_gemm(&g);
                g.prec = 1;
                if (f16) { g.fmt = 1; g.A.amax = dy_amax; g.B.amax = wimg->amax; }
                g.A.ptr = dy; g.A.kind = 0;
                if (dy_apply) set_apply(&g.A, dy_apply, Cout);
                set_gather(&g.A, 2, OH, OW, Cout, Cout, Hc, Wc, nkh > 0 ? nkh : 1, nkw > 0 ? nkw : 1, 1, offy, offx);
                g.B.ptr = w + ((int64_t)khs * KW + kws) * Cin; g.B.kind = 1; g.B.gather = 3;
                g.B.C = Cout; g.B.ld = (int64_t)KH * KW * Cin;
                g.B.KW = g.A.KW; g.B.tap_stride = 2ll * Cin; g.B.tap_stride_h = 2ll * KW * Cin;
                if (ps) {   // the class's tap subset of the D image: taps (khs + 2i, kws + 2j)
                    g.B.kind = 2; g.B.gather = 0;
                    g.B.planes = w_dimg + ((int64_t)khs * KW + kws) * Cout; g.B.ld = dld; g.B.plane_stride = dps;
                    g.B.tap_stride = 2ll * Cout; g.B.tap_stride_h = 2ll * KW * Cout;
                }
                if (dy_planes && nkh > 0 && nkw > 0) set_aplanes(&g.A, dy_planes, (int64_t)N * OH * OW * Cout);
                g.M = N * Hc * Wc; g.N = Cin; g.K = nkh * nkw * Cout;
                g.C = dx; g.ldc = Cin;
                g.residual = residual; g.ldr = Cin;
                g.cmap = 1; g.cm_PH = Hc; g.cm_PW = Wc; g.cm_H = H; g.cm_W = W; g.cm_py = py; g.cm_px = px;
                g.act16 = act16 ? 2 : 0;
                if (bnb) set_bnb(&g, bnb, part + (int64_t)rows_done * nsum * Cin);
                if (koaf_dgrad_s2_ok(g, KH, KW)) {
                    if (bnb) rows_done += g.M / 128;        // two partial rows per 256-row tile: the rows of a 128-row tiling
                    int rc = koaf_dgrad_s2(g, KH, KW, stream);
                    if (rc != KOAF_OK) return rc;
                    all_done = KH == 1;
                    continue;
                }
                if (bnb) rows_done += koaf_gemm_part_rows(&g);
                int rc = koaf_gemm(&g, stream);
                if (rc != KOAF_OK) return rc;
            }
        if (part_rows) *part_rows = rows_done;
        return KOAF_OK;
    }
    zero_gemm(&g);
    g.prec = 1;
    if (f16) { g.fmt = 1; g.A.amax = dy_amax; g.B.amax = wimg->amax; }
    g.A.ptr = dy;
    g.A.kind = 0;
    if (dy_apply) set_apply(&g.A, dy_apply, Cout);
    g.B.ptr = w;
    g.B.kind = 1;
    if (is_pointwise(KH, KW, stride, pad)) {
        g.A.gather = 0;
        g.A.ld = Cout;
        g.B.gather = 0;
        g.B.ld = Cin;  // element (cin, k=cout) at w + cout*Cin + cin
    } else {
        set_gather(&g.A, 2, OH, OW, Cout, Cout, H, W, KH, KW, stride, pad, pad);
        g.B.gather = 3;
        g.B.C = Cout;
        g.B.ld = (int64_t)KH * KW * Cin;
        g.B.KW = KW;
        g.B.tap_stride = Cin;
        g.B.tap_stride_h = (int64_t)KW * Cin;
    }
    if (ps) {   // all taps in order: k is simply the row offset of the D image
        g.B.kind = 2; g.B.gather = 0; g.B.C = 0; g.B.tap_stride = g.B.tap_stride_h = 0;
        g.B.planes = w_dimg; g.B.ld = dld; g.B.plane_stride = dps;
    }
    if (dy_planes) set_aplanes(&g.A, dy_planes, (int64_t)N * OH * OW * Cout);
    g.M = (int)M; g.N = Cin; g.K = KH * KW * Cout;
    g.C = dx; g.ldc = Cin;
    g.residual = residual; g.ldr = Cin;
    if (bnb) {
        set_bnb(&g, bnb, part);
        *part_rows = koaf_gemm_part_rows(&g);
    }
    g.act16 = act16 ? 2 : 0;            // (dy_apply->c and the BatchNorm-backward operands c / y / c2 are bf16 activations)
    return koaf_gemm(&g, stream);
}

extern "C" int koaf_conv2d_dgrad(const float* dy, const float* w, float* dx, int32_t N, int32_t H, int32_t W,
                                 int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                 const float* residual, const KoafWImg* wimg, const float* dy_amax,
                                 const KoafBnApply* dy_apply, const uint16_t* dy_planes, int32_t act16, void* stream) {
    return koaf_conv2d_dgrad_bnb(dy, w, dx, N, H, W, Cin, Cout, KH, KW, stride, pad, residual, nullptr, nullptr,
                                 nullptr, wimg, dy_amax, dy_apply, dy_planes, act16, stream);
}

static inline bool wgrad3_ring_shape(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    return KH == 3 && KW == 3 && stride == 1 && pad == 1 && koaf_wgrad3_ring_ok(N, H, W, Cin, Cout);
}

extern "C" int64_t koaf_conv2d_wgrad_ws(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                                        int32_t KW, int32_t stride, int32_t pad) {
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    WgradPlan p = wgrad_plan(Cout, KH * KW * Cin, (int64_t)N * OH * OW, Cin, 1);
    int64_t ws = p.splitk > 1 ? (int64_t)(p.splitk + 16) * Cout * KH * KW * Cin : 0;   // +16: koaf_slab_reduce level-1 partials
    if (wgrad3_ring_shape(N, H, W, Cin, Cout, KH, KW, stride, pad)) {
        const int64_t w3 = koaf_wgrad3_ring_ws(N, H, W, Cin, Cout);
        if (w3 > ws) ws = w3;
    }
    return ws;
}

extern "C" int koaf_conv2d_wgrad(const float* dy, const float* x, float* dw, int32_t N, int32_t H, int32_t W,
                                 int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                 const float* in_sc, const float* in_sh, float* slabs, const float* dy_amax,
                                 const KoafBnApply* dy_apply, const uint16_t* dy_planes, const uint16_t* x_planes,
                                 int32_t act16, void* stream) {
    KOAF_REQUIRE((dy_planes == nullptr) == (x_planes == nullptr) && (!dy_planes || dy_amax || dy_apply),
                 "koaf_conv2d_wgrad: dy_planes and x_planes come together, with dy_amax (or dy_apply)");
    KOAF_REQUIRE((dy || dy_apply || dy_planes) && (x || x_planes) && dw && N > 0 && Cin % 64 == 0 && Cout % 4 == 0, "koaf_conv2d_wgrad: bad args");
    KOAF_REQUIRE(!dy_apply || (dy_apply->dz && dy_apply->c && dy_apply->coef && dy_apply->amax),
                 "koaf_conv2d_wgrad: dy_apply needs dz / c / coef / amax");
    if (dy_apply) { dy = dy_apply->dz; dy_amax = dy_apply->amax; }
    KOAF_REQUIRE((in_sc == nullptr) == (in_sh == nullptr), "koaf_conv2d_wgrad: in_sc/in_sh come together");
    const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
    const int64_t P = (int64_t)N * OH * OW;
    KOAF_REQUIRE(P < (1ll << 31), "koaf_conv2d_wgrad: too many pixels");
    const int Ntot = KH * KW * Cin;
    if (dy_planes && slabs && wgrad3_ring_shape(N, H, W, Cin, Cout, KH, KW, stride, pad))
        return koaf_wgrad3_ring(dy_planes, x_planes, dw, slabs, dy_amax, KOAF_ACT_SCALE, N, H, W, Cin, Cout, stream);
    WgradPlan p = wgrad_plan(Cout, Ntot, P, Cin, 1);
    KOAF_REQUIRE(p.splitk == 1 || slabs, "koaf_conv2d_wgrad: workspace required");
    KoafGemm g;
    zero_gemm(&g);
    g.prec = 1;
    if (dy_amax) { g.fmt = 1; g.A.amax = dy_amax; g.B.fscale = KOAF_ACT_SCALE; }   // fp16 scheme: dy at its own scale, x fixed
    g.A.ptr = dy; g.A.kind = 1; g.A.ld = Cout;
    if (dy_apply) set_apply(&g.A, dy_apply, Cout);
    g.B.ptr = x; g.B.kind = 1;
    if (is_pointwise(KH, KW, stride, pad)) {
        g.B.gather = 0;
        g.B.ld = Cin;
    } else
        set_gather(&g.B, 1, H, W, Cin, Cin, OH, OW, KH, KW, stride, pad, pad);
    if (in_sc) { g.B.tf = 1; g.B.sc = in_sc; g.B.sh = in_sh; }
    if (dy_planes) {        // both operands from plane images, K-major (the 1x1 case as a one-tap gather)
        set_aplanes(&g.A, dy_planes, P * Cout);
        g.A.kind = 3; g.A.ld = Cout;
        set_aplanes(&g.B, x_planes, (int64_t)N * H * W * Cin);
        g.B.kind = 3;
        set_gather(&g.B, 1, H, W, Cin, Cin, OH, OW, KH, KW, stride, pad, pad);
    }
    g.M = Cout; g.N = Ntot; g.K = (int)P;
    g.bm = p.bm; g.bn = p.bn; g.splitk = p.splitk;
    g.C = p.splitk > 1 ? slabs : dw;
    g.ldc = Ntot;
    g.act16 = (act16 && !dy_planes) ? 3 : 0;      // (x and dy_apply->c are bf16 activations; plane images carry no storage type)
    int rc = koaf_wgrad1_ok(g) ? koaf_wgrad1(g, stream) : koaf_gemm(&g, stream);
    if (rc != KOAF_OK || p.splitk == 1) return rc;
    return koaf_slab_reduce(slabs, p.splitk, (int64_t)Cout * Ntot, dw, stream);
}

// ================================================================================================
// grouped 3x3 (ResNeXt) as 64-channel block-diagonal slabs through the same GEMM
// ================================================================================================
extern "C" int koaf_gconv_expand_w(const float* w, float* wexp, int32_t C, int32_t groups, float* amax, void* stream) {
    KOAF_REQUIRE(w && wexp && C % 64 == 0 && groups > 0 && C % groups == 0 && 64 % (C / groups) == 0,
                 "koaf_gconv_expand_w: C=%d groups=%d unsupported", C, groups);
    hipLaunchKernelGGL(gconv_expand_kernel, dim3(1024), dim3(256), 0, STREAM, w, wexp, C, C / groups, amax);
    return koaf_check_launch("koaf_gconv_expand_w");
}
extern "C" int koaf_gconv_compress_dw(const float* dwexp, float* dw, int32_t C, int32_t groups, void* stream) {
    KOAF_REQUIRE(dwexp && dw && C % 64 == 0 && groups > 0 && C % groups == 0 && 64 % (C / groups) == 0,
                 "koaf_gconv_compress_dw: C=%d groups=%d unsupported", C, groups);
    hipLaunchKernelGGL(gconv_compress_kernel, dim3(512), dim3(256), 0, STREAM, dwexp, dw, C, C / groups);
    return koaf_check_launch("koaf_gconv_compress_dw");
}

extern "C" int koaf_gconv3x3_fwd(const float* x, const float* wexp, float* y, int32_t N, int32_t H, int32_t W,
                                 int32_t C, int32_t stride, const float* in_sc, const float* in_sh, float* stats,
                                 int32_t* stats_rows, const float* stats_shift, const float* w_amax, int32_t act16, void* stream) {
    KOAF_REQUIRE(x && wexp && y && N > 0 && C % 64 == 0, "koaf_gconv3x3_fwd: bad args");
    const int OH = conv_out(H, 3, stride, 1), OW = conv_out(W, 3, stride, 1);
    const int64_t M = (int64_t)N * OH * OW;
    KOAF_REQUIRE(M < (1ll << 31), "koaf_gconv3x3_fwd: too many pixels");
    KoafGemm g;
    zero_gemm(&g);
    g.nb1 = C / 64;
    g.A.ptr = x; g.A.kind = 0; g.A.bs1 = 64;
    set_gather(&g.A, 1, H, W, 64, C, OH, OW, 3, 3, stride, 1, 1);
    if (in_sc) { g.A.tf = 1; g.A.sc = in_sc; g.A.sh = in_sh; }
    g.B.ptr = wexp; g.B.kind = 0; g.B.ld = 576; g.B.bs1 = 64 * 576;
    g.M = (int)M; g.N = 64; g.K = 576;
    g.C = y; g.ldc = C; g.cbs1 = 64;
    g.stats = stats; g.stats_ld = C; g.stats_bs = 64;
    g.stats_shift = stats ? stats_shift : nullptr;
    g.bn = 64; g.bm = 128;
    if (stats_rows) *stats_rows = (int)cdiv64(M, g.bm);
    g.A.tf_bs = 64;
    g.act16 = act16 ? 1 : 0;
    if (w_amax && !act16) { g.fmt = 1; g.A.fscale = KOAF_ACT_SCALE; g.B.amax = w_amax; }      // (fp16 scheme: both magnitudes known)
    return koaf_gemm(&g, stream);
}

extern "C" int koaf_gconv3x3_dgrad(const float* dy, const float* wexp, float* dx, int32_t N, int32_t H, int32_t W,
                                   int32_t C, int32_t stride, const float* w_amax, const float* dy_amax, void* stream) {
    KOAF_REQUIRE(dy && wexp && dx && N > 0 && C % 64 == 0, "koaf_gconv3x3_dgrad: bad args");
    const int OH = conv_out(H, 3, stride, 1), OW = conv_out(W, 3, stride, 1);
    const int64_t M = (int64_t)N * H * W;
    KOAF_REQUIRE(M < (1ll << 31), "koaf_gconv3x3_dgrad: too many pixels");
    KoafGemm g;
    zero_gemm(&g);
    g.prec = 1;
    g.nb1 = C / 64;
    g.A.ptr = dy; g.A.kind = 0; g.A.bs1 = 64;
    set_gather(&g.A, 2, OH, OW, 64, C, H, W, 3, 3, stride, 1, 1);
    g.B.ptr = wexp; g.B.kind = 1; g.B.gather = 3; g.B.C = 64; g.B.ld = 576; g.B.tap_stride = 64;
    g.B.tap_stride_h = 3 * 64; g.B.KW = 3;
    g.B.bs1 = 64 * 576;
    g.M = (int)M; g.N = 64; g.K = 576;
    g.C = dx; g.ldc = C; g.cbs1 = 64;
    g.bn = 64; g.bm = 128;
    if (w_amax && dy_amax) { g.fmt = 1; g.A.amax = dy_amax; g.B.amax = w_amax; }
    return koaf_gemm(&g, stream);
}

extern "C" int64_t koaf_gconv3x3_wgrad_ws(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride) {
    const int OH = conv_out(H, 3, stride, 1), OW = conv_out(W, 3, stride, 1);
    WgradPlan p = wgrad_plan(64, 576, (int64_t)N * OH * OW, 64, C / 64);
    return (int64_t)p.splitk * C * 576;
}

// dwexp [C/64][64][9][64]
extern "C" int koaf_gconv3x3_wgrad(const float* dy, const float* x, float* dwexp, int32_t N, int32_t H, int32_t W,
                                   int32_t C, int32_t stride, const float* in_sc, const float* in_sh, float* slabs,
                                   const float* dy_amax, int32_t act16, void* stream) {
    KOAF_REQUIRE(dy && x && dwexp && slabs && N > 0 && C % 64 == 0, "koaf_gconv3x3_wgrad: bad args");
    const int OH = conv_out(H, 3, stride, 1), OW = conv_out(W, 3, stride, 1);
    const int64_t P = (int64_t)N * OH * OW;
    KOAF_REQUIRE(P < (1ll << 31), "koaf_gconv3x3_wgrad: too many pixels");
    const int nz = C / 64;
    WgradPlan p = wgrad_plan(64, 576, P, 64, nz);
    {
        // one launch: the C/64 slabs are the batch dimension (split-K slabs laid out [slab][split][64][576])
        KoafGemm g;
        zero_gemm(&g);
        g.prec = 1;
        g.A.ptr = dy; g.A.kind = 1; g.A.ld = C; g.A.bs1 = 64;
        g.B.ptr = x; g.B.kind = 1; g.B.bs1 = 64;
        set_gather(&g.B, 1, H, W, 64, C, OH, OW, 3, 3, stride, 1, 1);
        if (in_sc) { g.B.tf = 1; g.B.sc = in_sc; g.B.sh = in_sh; g.B.tf_bs = 64; }
        g.M = 64; g.N = 576; g.K = (int)P;
        g.nb0 = 1; g.nb1 = nz;
        g.bm = 64; g.bn = 64; g.splitk = p.splitk;
        g.C = slabs;
        g.ldc = 576; g.cbs1 = 64 * 576;      // (unsplit case; split-K slabs are addressed by the kernel)
        g.act16 = act16 ? 3 : 0;
        if (dy_amax && !act16) { g.fmt = 1; g.A.amax = dy_amax; g.B.fscale = KOAF_ACT_SCALE; }
        int rc = koaf_gemm(&g, stream);
        if (rc != KOAF_OK) return rc;
    }
    const int64_t n = 64 * 576;
    hipLaunchKernelGGL(slab_reduce_b_kernel, dim3((unsigned)cdiv64(n / 4, 256), nz), dim3(256), 0, STREAM, slabs,
                       p.splitk, n, dwexp);
    return koaf_check_launch("koaf_gconv3x3_wgrad");
}
