// koaf_gemm.hip -- the one MFMA GEMM under every dense contraction of the koafusion train step:
// implicit-GEMM conv forward / dgrad / wgrad (NHWC), nn.Linear forward / dgrad / wgrad and the
// attention contractions.  fp32 in, fp32 out, fp32 accumulate.
//
// This file is the C entry point and every DECISION of a call: validation, defaults, the vector-path tests, the tile plan (tile shape,
// 3x3 halo / rectangle-tile kernels, the streamed A operand), the launch record and the run-time switches, plus the split-K slab
// reductions.  All mutable host state lives here.  The kernel template is koaf_gemm_kernel.h (arithmetic: koaf_pieces.h); its
// instantiations and their launches are the family files koaf_gemm_*.hip, declared in koaf_gemm_launch.h.
#include "koaf_gemm_launch.h"
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <vector>

namespace {

// out[i] = sum_s slabs[s][i]: block = 64 float4-columns x 4 slab groups (LDS tree), so small outputs (a 64x64
// weight gradient split 1024 ways) still spread over many waves instead of 4 blocks doing 1024 serial loads
// out[m][c] = sum_s slabs[s][m][c] + bias[c] + residual[m][c]   (split-K combine of a small-grid linear layer)
__global__ void __launch_bounds__(256) slab_reduce_epi_kernel(const float* __restrict__ slabs, int nslab, int M, int N,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ residual, int64_t ldr,
                                                              float* __restrict__ out, int64_t ldo) {
    const int N4 = N / 4;
    const int64_t total = (int64_t)M * N4;
    const int64_t n = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / N4), c = (int)(i - (int64_t)m * N4) * 4;
        v4f a = *(const v4f*)(slabs + (int64_t)m * N + c);
        for (int s = 1; s < nslab; ++s) a += *(const v4f*)(slabs + (int64_t)s * n + (int64_t)m * N + c);
        if (bias) a += *(const v4f*)(bias + c);
        if (residual) a += *(const v4f*)(residual + (int64_t)m * ldr + c);
        *(v4f*)(out + (int64_t)m * ldo + c) = a;
    }
}

__global__ void __launch_bounds__(256) slab_reduce_kernel(const float* __restrict__ slabs, int nslab,
                                                          int64_t n, float* __restrict__ out) {
    __shared__ v4f red[4][64];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int64_t i = ((int64_t)blockIdx.x * 64 + cx) * 4;
    const int s_per = (nslab + gridDim.y - 1) / gridDim.y;
    const int s0 = blockIdx.y * s_per, s1 = min(nslab, s0 + s_per);
    v4f a = {0.f, 0.f, 0.f, 0.f};
    if (i < n)
        for (int s = s0 + gy; s < s1; s += 4) a += *(const v4f*)(slabs + (int64_t)s * n + i);
    red[gy][cx] = a;
    __syncthreads();
    if (gy == 0 && i < n) {
        a = red[0][cx] + red[1][cx] + red[2][cx] + red[3][cx];
        if (gridDim.y == 1) *(v4f*)(out + i) = a;
        else *(v4f*)(out + (int64_t)blockIdx.y * n + i) = a;   // second-level slabs
    }
}

bool operand_vec_ok(const KoafOperand& o, int R, int K) {
    if (o.kind == 3) {
        // K-major activation plane images: 16-B chunks of 8 channels along the rows
        return aligned16(o.planes) && aligned16(o.zeros) && o.zeros && !(o.plane_stride & 7) && !(o.bs0 & 7) && !(o.bs1 & 7) &&
               !(R & 7) && (o.gather ? (o.C > 0 && !(o.C & 7) && !(o.CS & 7) && o.KW > 0) : !(o.ld & 7));
    }
    if (o.kind == 2 && o.gather) {
        // activation plane images: 16-B chunks of 8 channels, k-tiles never straddle a tap
        return aligned16(o.planes) && aligned16(o.zeros) && o.zeros && !(o.plane_stride & 7) && !(o.bs0 & 7) && !(o.bs1 & 7) &&
               o.C > 0 && !(o.C & 31) && !(o.CS & 7) && o.KW > 0 && (K % BK) == 0;
    }
    if (o.kind == 2) {
        // pre-split plane images: rows and taps start on 16-B boundaries, k-tiles never straddle a tap
        if (!aligned16(o.planes) || (o.ld & 7) || (o.plane_stride & 7) || (o.bs0 & 7) || (o.bs1 & 7)) return false;
        if ((o.tap_stride & 7) || (o.tap_stride_h & 7) || o.C <= 0 || (o.C & 31) || o.KW <= 0) return false;
        return true;
    }
    if (!aligned16(o.ptr)) return false;
    if ((o.ld & 3) || (o.bs0 & 3) || (o.bs1 & 3)) return false;
    if (o.kind == 0) {
        if (K & 3) return false;
        if (o.gather && ((o.C & 31) || (o.CS & 3))) return false;
    } else {
        if (R & 3) return false;
        if (o.gather == 3 && ((o.C & 31) || (o.tap_stride & 3) || (o.tap_stride_h & 3))) return false;
        if (o.gather == 1 && ((o.C & 3) || (o.CS & 3))) return false;
    }
    if (o.tf && (!aligned16(o.sc) || !aligned16(o.sh))) return false;
    if (o.tf == 2 && (!aligned16(o.sc2) || !aligned16(o.ptr2))) return false;
    return true;
}

}  // namespace

// the launch record (koaf.h koaf_launch_log): host memory only, written before the launch; one relaxed load when switched off
namespace {
std::atomic<int> g_log_on{0};
std::mutex g_log_mutex;
std::vector<KoafLaunchRec> g_log;
int64_t g_log_seen = 0;
constexpr size_t LOG_CAP = 4096;

}  // namespace

void koaf_log_launch(const char* variant, const KoafGemm& g, dim3 grid, dim3 launched) {
    if (!g_log_on.load(std::memory_order_relaxed)) return;
    KoafLaunchRec r;
    memset(&r, 0, sizeof(r));
    strncpy(r.variant, variant, sizeof(r.variant) - 1);
    r.bm = g.bm; r.bn = g.bn;
    r.tiles = (int32_t)grid.x; r.grid_x = (int32_t)launched.x;
    r.splitk = (int32_t)launched.y; r.nbatch = (int32_t)launched.z;
    r.fmt = g.fmt; r.a_tf = g.A.tf; r.b_tf = g.B.tf; r.act16 = g.act16;
    r.M = g.M - g.m_base; r.N = g.N; r.K = g.K;
    r.emit = g.out_planes != nullptr;
    std::lock_guard<std::mutex> lock(g_log_mutex);
    ++g_log_seen;
    if (g_log.size() < LOG_CAP) g_log.push_back(r);
}

namespace {
int g_stream_mode = 1;      // koaf_set_stream: the streamed A operand for the dense 1x1 kernels, 1 on (default), 0 off
// dense K-contiguous fp32 A (1x1 / stride-1 convolutions and their data gradients) in whole k-tiles, an even number of them
bool stream_ok(const KoafGemm& g) {
    return g_stream_mode == 1 && g.A.kind == 0 && g.A.gather == 0 && g.K >= 2 * BK && (g.K % (2 * BK)) == 0 && g.splitk == 1 &&
           g.nb0 * g.nb1 == 1 && (g.A.tf != 1 || g.K <= STREAM_TAB_K);
}
}  // namespace

// koaf_set_stream's switch for the dispatch rules outside this file (koaf_fwd1.hip koaf_fwd1_ok)
bool koaf_stream_on() { return g_stream_mode == 1; }

extern "C" int koaf_gemm_pick_tile(const KoafGemm* g, int32_t* bm, int32_t* bn) {
    int b_m = g->bm, b_n = g->bn;
    const int64_t batch = (int64_t)g->nb0 * g->nb1 * (g->splitk > 0 ? g->splitk : 1);
    if (b_n == 0) {
        b_n = (g->N >= 128) ? 128 : 64;
        // (a gathered K-major B tile may span filter taps: every thread derives the tap of its own 4 columns)
        if (g->B.kind == 1 && g->B.gather == 1 && (g->B.C % 64) != 0) b_n = 64;
    }
    if (b_m == 0) b_m = (g->M >= 128) ? 128 : 64;
    if (g->bm == 0 || g->bn == 0) {
        auto tiles = [&](int m, int n) { return cdiv64(g->M, m) * cdiv64(g->N, n) * batch; };
        // fill the 256 CUs: shrink the tile while the grid is under 384 blocks (1.5 per CU: a single 78 %-full round of
        // 128x128 tiles beats two rounds of the 1.25x costlier 64-row tiles; measured 512 / 384 / 256)
        constexpr int64_t fill = 384;
        if (g->bm == 0 && tiles(b_m, b_n) < fill && b_m == 128) b_m = 64;
        if (g->bn == 0 && tiles(b_m, b_n) < fill && b_n == 128) b_n = 64;
    }
    *bm = b_m;
    *bn = b_n;
    return KOAF_OK;
}

namespace {
int g_halo_mode = 1;        // koaf_set_conv3x3_halo: 0 off, 1 pick the shape per layer, 2 always 256 rows, 3 always 128 rows

// 3x3 / stride 1 / pad 1 over activation plane images with the whole pixel range as rows: the halo kernel (M_PH)
bool halo_ok(const KoafGemm& g) {
    const KoafOperand& a = g.A;
    return g_halo_mode != 0 && a.kind == 2 && (a.gather == 1 || a.gather == 2) && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 &&
           a.pad_w == 1 && a.PH == a.H && a.PW == a.W && a.W <= halo_max_w(g.N >= 128 ? 128 : 64, 256) && a.H * a.W > 0 && (g.M % (a.H * a.W)) == 0 &&
           g.nb0 * g.nb1 == 1 && g.m_base == 0 && g.K == 9 * a.C && g.B.kind == 2 && g.fmt == 1 && !g.cmap && g.splitk == 1;
}

bool gemm_vec_ok(const KoafGemm& g) {
    bool vec = operand_vec_ok(g.A, g.M, g.K) && operand_vec_ok(g.B, g.N, g.K);
    // vector epilogue: 16-B aligned rows of C / residual / bias
    if ((g.N & 3) || !aligned16(g.C) || (g.ldc & 3) || (g.cbs0 & 3) || (g.cbs1 & 3)) vec = false;
    if (g.residual && (!aligned16(g.residual) || (g.ldr & 3) || (g.rbs0 & 3) || (g.rbs1 & 3))) vec = false;
    if (g.bias && !aligned16(g.bias)) vec = false;
    return vec;
}

// g must already have its defaults filled (nb*, splitk, CS, stats_ld)
TilePlan plan_tiles(const KoafGemm& g) {
    TilePlan t;
    KoafGemm q = g;
    koaf_gemm_pick_tile(&q, &t.bm, &t.bn);
    t.vec = gemm_vec_ok(g);
    if (!t.vec) { t.bm = 64; t.bn = 64; }
    t.halo = t.vec && halo_ok(g);
    // 64 channels in (one halo chunk), 64 / 128 out, images of whole 8 x 16 tiles: the rectangle-tile kernel (halo_ok: 3x3 / stride 1 /
    // pad 1 over plane images, one GEMM over all pixels, every pixel a row).  (128 input channels -- two chunks, the halo fetched twice
    // per 64-column tile -- measured no faster than the 128-row raster kernel, 2.59 vs 2.55 ms, and stay with that kernel.)
    t.t2d = t.halo && g_halo_mode == 1 && g.A.C == 64 && (g.N == 64 || g.N == 128) && (g.A.W % 16) == 0 && (g.A.H % 8) == 0 &&
            g.A.zeros != nullptr;
    if (t.t2d) {
        t.halo = false;
        t.bm = 128;
        t.bn = 64;
    } else if (t.halo) {
        t.bn = g.N >= 128 ? 128 : 64;
        // 128 rows x two blocks per CU where the k-loop is short (few channel chunks) and the row fits its halo buffer
        const bool fits128 = g.A.W <= halo_max_w(t.bn, 128);
        t.bm = (g_halo_mode == 3 || (g_halo_mode == 1 && g.A.C <= 64)) && fits128 ? 128 : 256;
    }
    t.part_rows = (int)cdiv64(g.M - g.m_base, t.bm);
    // the streamed A operand (M_KS): the dense fp32 A x weight plane images calls of the fp16 scheme on 128-row tiles whose
    // transform the streamed kernels are built for (with out_planes: not the BatchNorm-backward apply)
    t.stream = t.vec && g.fmt == 1 && g.act16 == 0 && t.bm == 128 && operand_mode(g.A) == M_KC && operand_mode(g.B) == M_PS && !g.B.tf &&
               !(g.out_planes && g.A.tf == 2) && stream_ok(g);
    return t;
}
}  // namespace

// defaults of the optional descriptor fields (shared by the launch and by the planning queries, which must agree)
static void fill_defaults(KoafGemm& g) {
    if (g.nb0 < 1) g.nb0 = 1;
    if (g.nb1 < 1) g.nb1 = 1;
    if (g.splitk < 1) g.splitk = 1;
    if (g.A.CS == 0) g.A.CS = g.A.C;
    if (g.B.CS == 0) g.B.CS = g.B.C;
    if (g.stats_ld == 0) g.stats_ld = g.N;
    if (g.B.kind == 2 && g.B.C == 0) { g.B.C = ((g.K + BK - 1) / BK) * BK; g.B.KW = 1; }   // dense: one "tap" spanning the padded K
}

namespace {
// From the plan to a family: every koaf_gemm_kernel instantiation lives in exactly one of the koaf_gemm_*.hip files (koaf_gemm_launch.h),
// which turn (plan, operand modes, transforms) into its launch or answer KOAF_NO_KERNEL.
int launch_wplanes(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    switch (g.act16) {
        case 0: return koaf_launch_wplanes_act0(g, tp, grid, s);
        case 1: return koaf_launch_wplanes_act1(g, tp, grid, s);
        case 2: return koaf_launch_wplanes_act2(g, tp, grid, s);
    }
    return KOAF_NO_KERNEL;
}

int launch_planned(const KoafGemm& g, const TilePlan& tp, dim3 grid, hipStream_t s) {
    const int am = operand_mode(g.A), bm = operand_mode(g.B);
    if (g.out_planes && (tp.t2d || tp.halo)) { koaf_set_error("koaf_gemm: out_planes is not built for the 3x3 plane-image kernels"); return KOAF_EINVAL; }
    if ((tp.t2d || tp.halo) && g.act16 == 3) {
        koaf_set_error(tp.t2d ? "koaf_gemm: 2-D tile kernel with act16 = 3" : "koaf_gemm: halo kernel with act16 = 3");
        return KOAF_EINVAL;
    }
    if (tp.t2d || tp.halo) return launch_wplanes(g, tp, grid, s);
    if (g.fmt == 1) KOAF_REQUIRE(tp.vec, "koaf_gemm: the fp16 scheme needs the vector path (16-B aligned operands, K %% 4 == 0, N %% 4 == 0)");
    else if (!tp.vec && g.act16 != 0) { koaf_set_error("koaf_gemm: bf16 activation storage needs the vector path"); return KOAF_EINVAL; }
    int rc = KOAF_NO_KERNEL;
    if (tp.stream) rc = koaf_launch_stream(g, tp, grid, s);
    else if (g.out_planes) {
        if (g.fmt == 1 && am == M_KC && bm == M_PS) rc = launch_wplanes(g, tp, grid, s);
        if (rc == KOAF_NO_KERNEL) {
            koaf_set_error("koaf_gemm: out_planes is built for dense K-contiguous A x weight plane images on the fp16 scheme (1x1 forward convolutions); "
                           "got operand modes (%d,%d) tf=%d fmt=%d act16=%d", am, bm, g.A.tf, (int)(g.fmt == 1), g.act16);
            return KOAF_EINVAL;
        }
    }
    else if (bm == M_PS) rc = launch_wplanes(g, tp, grid, s);
    else if (am == M_PK) rc = koaf_launch_kmajor(g, tp, grid, s);
    else rc = g.fmt == 1 ? koaf_launch_fp16(g, tp, grid, s) : koaf_launch_bf16(g, tp, grid, s);
    if (rc == KOAF_NO_KERNEL) {
        koaf_set_error("koaf_gemm: operand mode pair (%d,%d) tf=(%d,%d) fmt=%d vec=%d act16=%d is not instantiated", am, bm, g.A.tf, g.B.tf,
                       (int)(g.fmt == 1), (int)tp.vec, g.act16);
        return KOAF_EINVAL;
    }
    return rc;
}
}  // namespace

extern "C" int koaf_gemm_part_rows(const KoafGemm* gp) {
    KoafGemm g = *gp;
    fill_defaults(g);
    return plan_tiles(g).part_rows;
}

extern "C" int koaf_gemm(const KoafGemm* gp, void* stream) {
    KoafGemm g = *gp;
    KOAF_REQUIRE(g.M > 0 && g.N > 0 && g.K >= 0, "koaf_gemm: bad dims M=%d N=%d K=%d", g.M, g.N, g.K);
    KOAF_REQUIRE((g.A.kind >= 2 ? (const void*)g.A.planes : (const void*)g.A.ptr) &&
                 (g.B.kind >= 2 ? (const void*)g.B.planes : (const void*)g.B.ptr) && g.C, "koaf_gemm: null operand");
    fill_defaults(g);
    if (!g.status) g.status = koaf_status_ptr();
    KOAF_REQUIRE(!g.cmap || (g.splitk == 1 && !g.stats), "koaf_gemm: row map excludes split-K / stats");
    KOAF_REQUIRE(!g.bnb_mode || (g.splitk == 1 && !g.stats && g.nb0 * g.nb1 == 1 && g.bnb_c && g.bnb_mean &&
                                 g.bnb_invstd && g.bnb_part && (g.bnb_mode == 1 ? g.bnb_y != nullptr
                                                                                 : (g.bnb_sc && g.bnb_sh))),
                 "koaf_gemm: fused BN-backward epilogue needs c/mean/invstd/part (+y or sc/sh), no split-K/batch");
    KOAF_REQUIRE(g.splitk == 1 || (!g.bias && !g.residual && !g.stats),
                 "koaf_gemm: split-K writes raw slabs (no epilogue)");
    KOAF_REQUIRE((int64_t)g.nb0 * g.nb1 <= 65535 && g.splitk <= 65535, "koaf_gemm: batch/splitk too large");
    KOAF_REQUIRE(g.A.kind == 0 || (g.A.kind == 1 && g.A.gather == 0) || g.A.kind == 2 || (g.A.kind == 3 && g.A.gather == 0),
                 "koaf_gemm: A is K-contiguous fp32, K-major without gather, or activation plane images");
    KOAF_REQUIRE((g.A.kind == 3) == (g.B.kind == 3), "koaf_gemm: K-major plane images (kind 3) come as a pair");
    if (g.A.kind == 3)
        KOAF_REQUIRE(g.fmt == 1 && !g.A.tf && !g.B.tf && g.A.zeros && g.B.zeros && (g.B.gather == 0 || g.B.gather == 1),
                     "koaf_gemm: K-major plane images need fmt 1, no transform, the zero chunks; B.gather 0 | 1");
    if (g.A.kind == 2)
        KOAF_REQUIRE((g.A.gather == 1 || g.A.gather == 2) && g.B.kind == 2 && g.fmt == 1 && !g.A.tf && g.splitk == 1 && g.A.zeros,
                     "koaf_gemm: activation plane images (A.kind 2) need gather 1|2, a pre-split B, fmt 1, no transform, no split-K");
    KOAF_REQUIRE(!(g.A.kind == 0 && g.A.gather == 3) && !(g.B.kind == 0 && g.B.gather == 3),
                 "koaf_gemm: tapped gather needs a K-major operand");
    KOAF_REQUIRE(!(g.B.kind == 0 && g.B.gather), "koaf_gemm: K-contiguous B cannot be gathered");
    KOAF_REQUIRE(g.fmt == 0 || g.fmt == 1, "koaf_gemm: fmt must be 0 (bf16 x 3) or 1 (fp16 x 2)");
    KOAF_REQUIRE(g.A.tf >= 0 && g.A.tf <= 3 && g.B.tf >= 0 && g.B.tf <= 1, "koaf_gemm: tf is 0 | 1 (A, B) | 2 | 3 (A)");
    KOAF_REQUIRE(g.A.tf != 3 || (g.A.kind == 0 && g.A.gather == 0 && g.A.ptr2 && g.A.sc && g.A.sh && g.fmt == 1 && g.B.kind == 2 &&
                                 g.nb0 * g.nb1 == 1 && g.splitk == 1 && aligned16(g.A.ptr2) && (!g.A.side || aligned16(g.A.side)) &&
                                 (!g.A.sc2 || (g.A.sh2 && aligned16(g.A.sc2) && aligned16(g.A.sh2)))),
                 "koaf_gemm: the bottleneck-tail prologue (tf 3) needs a dense K-contiguous A, ptr2 / sc / sh, the fp16 scheme with a pre-split B");
    KOAF_REQUIRE(g.A.tf != 2 || (g.A.ptr2 && g.A.sc && g.A.sh && g.A.sc2 && g.fmt == 1),
                 "koaf_gemm: the two-source prologue needs ptr2 / sc / sh / sc2 and the fp16 scheme");
    if (g.B.kind == 2) {
        KOAF_REQUIRE(g.fmt == 1 && g.B.amax, "koaf_gemm: plane images are fp16 pieces of B * scale(*B.amax): fmt 1, amax required");
        KOAF_REQUIRE((g.A.kind == 0 || g.A.kind == 2) && !g.B.tf, "koaf_gemm: a pre-split B pairs with a K-contiguous A and takes no transform");
    }
    const TilePlan tp = plan_tiles(g);
    const bool vec = tp.vec;
    KOAF_REQUIRE(!g.out_planes || (tp.vec && g.out_sc && g.out_sh && g.ldc == g.N && !(g.N & 7) && g.nb0 * g.nb1 == 1 && g.splitk == 1 && !g.cmap &&
                                   !g.residual && !g.bnb_mode && g.out_ps == (int64_t)g.M * g.N && aligned16(g.out_planes) && aligned16(g.out_sc) &&
                                   aligned16(g.out_sh)),
                 "koaf_gemm: out_planes needs the vector epilogue of a plain forward call (ldc == N, N %% 8 == 0, no batch / split-K / row map / "
                 "residual / BatchNorm-backward), out_ps == M * N and 16-B aligned out_planes / out_sc / out_sh");
    KOAF_REQUIRE(((tp.bm == 64 || tp.bm == 128) && (tp.bn == 64 || tp.bn == 128)) || tp.halo || tp.t2d, "koaf_gemm: tile must be 64|128");
    if (g.A.gather || g.B.gather) KOAF_REQUIRE(vec, "koaf_gemm: gathered operands need aligned, C%%32==0 tensors");
    if (g.B.kind >= 2 || g.A.kind >= 2) KOAF_REQUIRE(vec, "koaf_gemm: pre-split operands need 16-B aligned images (and C %% 32 == 0 per tap)");
    if (g.B.kind == 1 && g.B.gather == 1)
        KOAF_REQUIRE(g.B.C % 4 == 0, "koaf_gemm: gathered K-major operand needs channels per tap (%d) %% 4 == 0", g.B.C);
    KOAF_REQUIRE(!g.cmap || vec, "koaf_gemm: row map needs the vector epilogue");
    KOAF_REQUIRE(!g.bnb_mode || vec, "koaf_gemm: fused BN-backward needs the vector epilogue");
    hipStream_t s = (hipStream_t)stream;
    g.bm = tp.bm;
    g.bn = tp.bn;
    const int64_t tiles = cdiv64(g.M - g.m_base, tp.bm) * cdiv64(g.N, tp.bn);
    if (tiles <= 0) return KOAF_OK;
    if (tiles >= (1ll << 31)) { koaf_set_error("koaf_gemm: grid too large"); return KOAF_EINVAL; }
    dim3 grid((unsigned)tiles, (unsigned)g.splitk, (unsigned)(g.nb0 * g.nb1));
    if (g.act16 < 0 || g.act16 > 3) { koaf_set_error("koaf_gemm: act16 must be 0 .. 3"); return KOAF_EINVAL; }
    return launch_planned(g, tp, grid, s);
}

extern "C" int koaf_slab_reduce(const float* slabs, int32_t nslab, int64_t n, float* out, void* stream) {
    KOAF_REQUIRE(slabs && out && nslab >= 1 && n > 0 && (n & 3) == 0, "koaf_slab_reduce: bad args (n %% 4 == 0)");
    KOAF_REQUIRE((((uintptr_t)slabs | (uintptr_t)out) & 15) == 0, "koaf_slab_reduce: unaligned");
    const unsigned bx = (unsigned)cdiv64(n / 4, 64);
    // two-level when one level would leave the chip idle: nslab -> 16 partial slabs written BEHIND the input
    // slabs (the workspace holds (nslab + 16) * n floats), then 16 -> out
    hipStream_t s = (hipStream_t)stream;
    if (nslab >= 64 && bx < 256) {
        float* part = const_cast<float*>(slabs) + (int64_t)nslab * n;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(bx, 16), dim3(256), 0, s, slabs, nslab, n, part);
        int rc = koaf_check_launch("koaf_slab_reduce/1");
        if (rc != KOAF_OK) return rc;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(bx, 1), dim3(256), 0, s, part, 16, n, out);
        return koaf_check_launch("koaf_slab_reduce/2");
    }
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(bx, 1), dim3(256), 0, s, slabs, nslab, n, out);
    return koaf_check_launch("koaf_slab_reduce");
}

extern "C" int koaf_slab_reduce_epilogue(const float* slabs, int32_t nslab, int32_t M, int32_t N, const float* bias,
                                         const float* residual, int64_t ldr, float* out, int64_t ldo, void* stream) {
    KOAF_REQUIRE(slabs && out && nslab >= 1 && M > 0 && N > 0 && (N & 3) == 0 && (ldo & 3) == 0 && (ldr & 3) == 0,
                 "koaf_slab_reduce_epilogue: bad args");
    const int64_t total = (int64_t)M * (N / 4);
    int64_t blocks = cdiv64(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(slab_reduce_epi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, slabs, nslab, M,
                       N, bias, residual, ldr, out, ldo);
    return koaf_check_launch("koaf_slab_reduce_epilogue");
}

extern "C" int koaf_set_stream(int on) {
    const int was = g_stream_mode;
    g_stream_mode = on ? 1 : 0;
    return was;
}

extern "C" int koaf_launch_log(int on) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    const int was = g_log_on.load(std::memory_order_relaxed);
    g_log.clear();
    g_log_seen = 0;
    g_log_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return was;
}

extern "C" int koaf_launch_log_read(KoafLaunchRec* out, int32_t cap) {
    std::lock_guard<std::mutex> lock(g_log_mutex);
    for (size_t i = 0; out && i < g_log.size() && (int64_t)i < cap; ++i) out[i] = g_log[i];
    return (int)(g_log_seen < INT32_MAX ? g_log_seen : INT32_MAX);
}

extern "C" int koaf_set_conv3x3_halo(int on) {
    const int was = g_halo_mode;
    g_halo_mode = (on >= 0 && on <= 3) ? on : 1;
    return was;
}
