/*
 * koaf.h -- C ABI of libkoaf.so: the hand-written gfx950 (MI355X / CDNA4) kernels under the
 * koafusion train-step hot path.
 *
 * The reference (imedslab/OAProgressionMMF) has no FFI: its hot path is stock torch.nn called from
 *   koafusion/models/_torchvision.py:118-138,141-246   (conv / BatchNorm2d / ReLU / MaxPool / GAP)
 *   koafusion/models/_core_trf.py:118-205               (Linear / LayerNorm / GELU / attention)
 *   koafusion/various/_losses.py:89-108                 (focal softmax-CE)
 *   koafusion/preproc/_pt.py:75-345                     (F.interpolate x0.5 downscale; the per-sample tensor transforms)
 *   torch.optim.Adam / SGD / RMSprop via koafusion/various/_optimizers.py:47-52
 *   nn.BCELoss / nn.BCEWithLogitsLoss via koafusion/various/_losses.py:111-117
 * Each entry point below names the reference call site it replaces.  All pointers are DEVICE
 * pointers to fp32 (unless stated), all tensors are dense; activations are NHWC ("(n,h,w,c)",
 * c fastest).  Nothing allocates; every call is asynchronous on `stream` (a hipStream_t passed as
 * void*).  Return value: 0 = ok, negative = error (text via koaf_last_error()).
 *
 * Not thread-safe on one stream; re-entrant across devices/streams.
 */
#ifndef KOAF_H
#define KOAF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define KOAF_OK 0
#define KOAF_EINVAL (-1)
#define KOAF_ELAUNCH (-2)

/* The ABI version of this header, 100 * major + 10 * minor.  Any change to a prototype or a struct below bumps it: the binding
 * refuses a library whose koaf_version() differs from the header it parsed. */
#define KOAF_VERSION 200
int koaf_version(void);          /* KOAF_VERSION of the header the library was built from */
const char* koaf_last_error(void);
/* Numerics status words: a device uint32[4] (zeroed by the caller; NULL = off, the default) that kernels bump with atomics when
 *   [0] an activation operand left the fp16 range of the fixed activation scale and was CLAMPED (KOAF_ACT_SCALE: |x| > 4094), or
 *       was not finite: counted per element by koaf_act_planes / koaf_bn_add_relu / koaf_bn_relu / koaf_maxpool_fwd (the
 *       producers of every tensor the convolutions read at that scale), and per GEMM tile by the fp32 loader that applies
 *       relu(sc*x+sh) on load (KoafOperand.tf 1; there a NaN becomes 0 and is not counted -- the BatchNorm coefficients are, [1]);
 *   [1] a NaN / Inf reached an operand's amax scalar (weights, gradients: the GEMM then returns NaN everywhere, see KoafGemm)
 *       or a BatchNorm's sc / sh came out non-finite (koaf_bn_finalize).
 * Process-wide (one process per GPU); read it back with a device-to-host copy whenever convenient (e.g. once per epoch). */
int koaf_set_status_buffer(uint32_t* dev4);

/* ---------------------------------------------------------------------------------------------
 * Generic MFMA GEMM  C[M,N] = alpha * sum_k A(m,k) B(n,k)  (+bias[n]) (+residual[m,n])
 * fp32 in / fp32 out / fp32 accumulate.  Products are formed on the bf16 matrix pipe from exact bf16 pieces of the
 * fp32 operands (KoafGemm.fmt: three bf16 pieces / six products, or two scaled fp16 pieces / three products): error at
 * fp32 rounding level either way.  Non-finite operands: fmt 0 -- an Inf operand yields NaN, NaN stays NaN.  fmt 1 -- the
 * scaled pieces are clamped to +-65504 (a NaN piece becomes the lower clamp bound), so a non-finite ELEMENT does not
 * propagate by itself; instead (a) operands scaled by a device amax (weights, gradients) carry their NaN / Inf into that
 * scalar (all amax reductions propagate non-finite values) and a GEMM that finds a non-finite amax returns NaN in EVERY
 * output element, and (b) activation operands at the fixed scale are watched by the numerics status words
 * (koaf_set_status_buffer): clamped / non-finite elements are counted, non-finite BatchNorm coefficients too.
 * Each operand is either K-contiguous ("KC": element (r,k) at ptr + r*ld + k) or K-major
 * ("KM": element (r,k) at ptr + k*ld + r).  Operands can be gathered on the fly from an NHWC
 * tensor (implicit-GEMM convolution) and transformed on load with relu(sc[c]*x+sh[c]) -- the
 * previous layer's BatchNorm+ReLU, so normalised activations never touch HBM.
 * ------------------------------------------------------------------------------------------- */
typedef struct KoafOperand {
    const float* ptr;
    int64_t ld;       /* KC: stride between rows; KM: stride between k-rows */
    int64_t bs0, bs1; /* batch strides (elements) for batch index z = z0*nb1 + z1 */
    int64_t tap_stride;   /* gather 3 (K-major weights [C][taps][rows]): offset between taps in a tap row */
    int64_t tap_stride_h; /* gather 3: offset between tap rows; tap index = th*KW + tw */
    int32_t kind;     /* 0 = KC, 1 = KM, 2 = pre-split fp16 plane images (B: weights, see `planes`; A: activations, see `zeros`),
                         3 = activation plane images read K-major (both operands of a weight gradient, see `zeros`) */
    int32_t gather;   /* 0 none; 1 conv forward gather; 2 transposed-conv (dgrad) gather;
                         3 (KM only) tapped weights: k = (tap, c), element at c*ld + tap*tap_stride + r */
    int32_t H, W, C;  /* source NHWC tensor dims for a gathered operand (C = channels per tap) */
    int32_t CS;       /* channels per source pixel (0 = C); > C when the GEMM sees a channel slab */
    int32_t PH, PW;   /* pixel grid the GEMM rows (KC) or the k index (KM) enumerate: (n,py,px) */
    int32_t KH, KW, stride, pad; /* pad = row (y) padding */
    int32_t pad_w;               /* column (x) padding (set = pad for square padding) */
    int32_t _pad1;
    int32_t tf;       /* transform on load (c = source channel): 0 none; 1 relu(sc[c]*x + sh[c]); 2 (A operand, fmt 1, vector
                         path) sc[c]*x + sh[c] - sc2[c]*x2 with x2 read from ptr2 (same layout and strides as ptr): the
                         BatchNorm-backward apply formed on load, see koaf_bn_bwd_finalize; 3 (A operand, dense K-contiguous,
                         fmt 1 with a pre-split B) y = relu(sc[c]*x + sh[c] + x2): the BOTTLENECK TAIL relu(bn3(c3) + identity)
                         (_torchvision.py:132-136) formed in the loader of the next block's conv1 -- koaf_bn_add_relu's
                         arithmetic bit for bit -- with y written once to `side` by the blocks of the first column tile; with
                         sc2 / sh2 the identity is sc2[c]*x2 + sh2[c] (a downsample branch's raw conv output and BatchNorm) */
    int32_t tf_bs;    /* channel offset of sc/sh per batch index z1 (grouped-conv slabs) */
    const float* sc;
    const float* sh;
    /* kind 2 (B operand, KoafGemm.fmt 1): `planes` -> plane 0 of the two fp16 plane images (hi, lo) of a K-contiguous matrix
       scaled by scale(*amax) (cut by koaf_wplanes_build): element (r, k) of plane q at planes + q*plane_stride + r*ld + k,
       every row zero-filled up to a multiple of 32 k.  All strides (ld, plane_stride, bs0, bs1, tap_stride, tap_stride_h)
       count 16-bit elements and are multiples of 8.  Tapped addressing as for conv weights: with C > 0 the GEMM's
       k = (tap, c), tap = th*KW + tw, lives at th*tap_stride_h + tw*tap_stride + c of the row (C % 32 == 0); C == 0: k is
       the row offset.  The kernel moves these planes global -> LDS directly (global_load_lds): no split arithmetic in
       the k-loop. */
    const uint16_t* planes;
    int64_t plane_stride;
    /* fp16 scheme (KoafGemm.fmt == 1): the operand is multiplied by a power of two before it is cut into fp16 pieces:
       amax != NULL: scale(*amax) = 2^e with *amax * 2^e in [2^14, 2^15) (1 for *amax == 0) -- *amax = max |element| of the
       tensor, written on the device by its producer; amax == NULL: fscale (0 = 1).  Scaled magnitudes are clamped to 65504. */
    const float* amax;
    float fscale;
    int32_t _pad4;
    const float* ptr2;  /* tf 2: second source tensor */
    const float* sc2;   /* tf 2: its per-channel coefficient */
    /* kind 2 with gather 1 | 2 (A operand): ACTIVATION plane images cut by koaf_act_planes -- the two fp16 piece planes
       [pixel][CS] of an NHWC tensor (plane q at planes + q*plane_stride), transform already applied (tf must be 0), scaled
       by the operand's scale (amax / fscale as above).  Gathered like the fp32 operand of the same `gather`; padding taps
       and rows past M read `zeros` (16 B of zeros, 16-B aligned: koaf_act_planes leaves them at planes + 2*plane_stride).
       C % 32 == 0, CS % 8 == 0; needs a pre-split B (kind 2), fmt 1, K % 32 == 0, no split-K. */
    /* kind 3 (A and B together, fmt 1): the same images read K-MAJOR -- k = pixel, rows = channels: element (k, r) of plane q
       at planes + q*plane_stride + k*ld + r (A, gather 0; ld = channels per pixel), or gathered like a kind-1 gather-1 operand
       (B: column = tap*C + c, k = output pixel -> source pixel by H/W/PH/PW/KH/KW/stride/pad; C % 8 == 0).  Rows % 8 == 0. */
    const uint16_t* zeros;
    float* side;        /* tf 3: where the loader stores y (same layout as ptr; nullable: y is then not kept) */
    const float* sh2;   /* tf 3 with sc2 != NULL: the identity is sc2[c]*x2 + sh2[c] (the BatchNorm of a downsample branch) */
} KoafOperand;

typedef struct KoafGemm {
    KoafOperand A, B;
    int32_t M, N, K;
    int32_t nb0, nb1; /* batch = nb0*nb1 (>=1 each) */
    int32_t splitk;   /* >=1; >1: C is a slab buffer [splitk][M][N] (ldc == N), no epilogue */
    int32_t bm, bn;   /* block tile (64|128); 0 = pick */
    float* C;
    int64_t ldc, cbs0, cbs1;
    float alpha;
    int32_t prec;            /* 0: a forward contraction; 1: a data / weight gradient contraction (informational) */
    const float* bias;     /* [N] or NULL */
    const float* residual; /* [M][ldr] (+batch strides) or NULL */
    int64_t ldr, rbs0, rbs1;
    float* stats;          /* [ceil(M/bm)][2][stats_ld] per-M-tile column sum / sum of squares, or NULL */
    int64_t stats_ld;      /* 0 = N */
    int64_t stats_bs;      /* column offset per batch index (grouped conv slabs) */
    /* output row map (stride-2 dgrad parity classes): GEMM row (n, y', x') over a cm_PH x cm_PW grid is
       written to pixel row (n*cm_H + 2y'+cm_py)*cm_W + 2x'+cm_px of C / residual.  cmap = 0: identity. */
    int32_t cmap, cm_PH, cm_PW, cm_H, cm_W, cm_py, cm_px, _pad2;
    /* Fused BatchNorm(+ReLU)-backward reduction (dgrad epilogue).  The GEMM output g (after bias/residual) is the
       gradient w.r.t. relu(bn(c)); the epilogue masks it (bnb_mode 1: bnb_y > 0; 2: bnb_sc*c+bnb_sh > 0), stores
       dz instead of g, and emits per-M-tile column sums  bnb_part[tile][k][N]:  k=0: sum dz, k=1: sum dz*xhat with
       xhat = (c-mean)*invstd, k=2 (if bnb2_c): sum dz*xhat2 for a second BatchNorm fed by the same dz (the
       downsample branch).  c / y / c2 are laid out like C (same ldc, same row map).  bnb_mode 0 = off. */
    int32_t bnb_mode;
    int32_t fmt;             /* how the fp32 x fp32 products are formed on the matrix pipe:
                              * 0: three exact bf16 pieces per operand, the six piece products of weight >= 2^-16
                              *    (v_mfma_f32_32x32x16_bf16): any fp32 operand, no scale information needed;
                              * 1: two fp16 pieces of operand * 2^e (hi = fp16(x'), lo = fp16(x' - hi): x' = hi + lo to 2^-24
                              *    relative down to |x'| = 2^-2, 2^-25 absolute below) and the three products hi*hi, hi*lo,
                              *    lo*hi (v_mfma_f32_32x32x16_f16; each exact in fp32, the dropped lo*lo <= 2^-24 of the
                              *    product): the same fp32-level accuracy from half the matrix instructions, for operands
                              *    whose magnitude is known (KoafOperand.amax / fscale).  Needs the vector path. */
    const float* bnb_c;
    const float* bnb_y;
    const float* bnb_sc;
    const float* bnb_sh;
    const float* bnb_mean;
    const float* bnb_invstd;
    const float* bnb2_c;
    const float* bnb2_mean;
    const float* bnb2_invstd;
    float* bnb_part;
    float* bnb_amax;       /* nullable: device scalar raised (atomic max; zero it beforehand) to the largest |dz| stored */
    /* row-space origin of this launch (mixed-height tiling: one GEMM = a 128-row-tile launch over rows
       [0, M1) + a 64-row-tile launch over [M1, M)); partial-statistics rows continue at part_row0 */
    int32_t m_base, part_row0;
    /* per-column shift k[N] (+ stats_bs per batch index) of the statistics: stats rows hold sum (v - k) and
       sum (v - k)^2 (NULL: k = 0).  With k near the column mean -- the BatchNorm's running mean -- the variance
       E[(v-k)^2] - E[v-k]^2 keeps its digits when |mean| >> std. */
    const float* stats_shift;
    uint32_t* status;      /* numerics status words (koaf_set_status_buffer); NULL = the registered buffer */
    /* bf16 ACTIVATION STORAGE: which tensors of this call are forward activations kept in HBM as bf16 instead of fp32 (the
       pointers stay typed float*; strides / offsets count elements).  0: none.  1 (forward convolution): A.ptr and C -- the
       loader widens (exact), the epilogue rounds the output to nearest even; statistics come from the fp32 accumulators.
       2 (data gradient): A.ptr2 (the conv output c of a tf-2 apply) and bnb_c / bnb_y / bnb2_c.  3 (weight gradient): A.ptr2
       and B.ptr.  Gradients, weights, statistics and all arithmetic stay fp32; needs the vector path. */
    int32_t act16;
    int32_t _pad5;
    /* Epilogue side output (nullable; forward convolutions whose OUTPUT BatchNorm is already known -- eval mode, stages rebuilt in
       backward): besides C, the epilogue writes the activation plane images of relu(out_sc[n] * C + out_sh[n]) at the scale
       KOAF_ACT_SCALE -- exactly what koaf_act_planes (tf 1) would cut from C in a pass of its own: [2][M][N] fp16 pieces,
       plane stride out_ps = M * N elements, the 16-B zero chunk behind them.  Needs the vector epilogue, ldc == N, no batch, no
       split-K, no row map. */
    uint16_t* out_planes;
    const float* out_sc;
    const float* out_sh;
    int64_t out_ps;
} KoafGemm;

int koaf_gemm(const KoafGemm* g, void* stream);
/* block tile koaf_gemm picks for (M, N, batch) when bm = bn = 0 */
int koaf_gemm_pick_tile(const KoafGemm* g, int32_t* bm, int32_t* bn);
/* number of per-tile partial rows (stats / bnb_part) koaf_gemm writes for this descriptor (mixed-height tiling
 * included); callers size / slice their buffers with it */
int koaf_gemm_part_rows(const KoafGemm* g);
/* Launch record (tests; off by default): which kernel variant served each koaf_gemm call.  While switched on, every koaf_gemm
 * launch appends one entry -- plain host memory, written before the launch; no device work, nothing when off.  `variant` is the
 * tag koaf_gemm reports launch errors under ("koaf_gemm", "koaf_gemm/stream", "/emit", "/halo", "/halo128", "/t2d"; "koaf_fwd1": the 256-row kernel of the dense 1x1 forward convolutions; "koaf_wgrad3/ring": the 3x3 weight-gradient ring kernel
 * behind koaf_conv2d_wgrad leaves an entry too -- 64 x 64 tiles, splitk = its k-ranges, K = the padded positions); `tiles` the
 * block tiles of one (split, batch) slice and `grid_x` the blocks launched for them (grid_x < tiles: persistent blocks that walk
 * several tiles).  A convolution entry point that issues several GEMMs (a stride-2 data gradient: one per phase) leaves one
 * entry per GEMM.  koaf_launch_log(on) clears the record, switches it on / off and returns the previous setting;
 * koaf_launch_log_read copies the first `cap` entries to `out` (NULL with cap 0: count only) and returns how many launches were
 * seen since the record was cleared (the record itself keeps the first 4096).  Process-wide, guarded by a mutex. */
typedef struct KoafLaunchRec {
    char variant[24];
    int32_t bm, bn;           /* block tile (halo kernels: 128 | 256 rows) */
    int32_t tiles, grid_x;
    int32_t splitk, nbatch;   /* grid.y, grid.z */
    int32_t fmt, a_tf, b_tf, act16;
    int32_t M, N, K;
    int32_t emit;             /* KoafGemm.out_planes != NULL */
} KoafLaunchRec;
int koaf_launch_log(int on);
int koaf_launch_log_read(KoafLaunchRec* out, int32_t cap);
/* out[i] = sum_s slabs[s][i], i < n, n % 4 == 0 (deterministic split-K combine).  The slab workspace must
 * hold (nslab + 16) * n floats: large counts are folded in two levels through the 16 trailing slabs. */
int koaf_slab_reduce(const float* slabs, int32_t nslab, int64_t n, float* out, void* stream);
/* out[m][c] = sum_s slabs[s][m][c] + bias[c] + residual[m][c]  (split-K combine with the linear epilogue) */
int koaf_slab_reduce_epilogue(const float* slabs, int32_t nslab, int32_t M, int32_t N, const float* bias,
                              const float* residual, int64_t ldr, float* out, int64_t ldo, void* stream);

/* ---- Weight plane images ---------------------------------------------------------------------
 * Every convolution weight of the model ([Cout][KH*KW][Cin] packed) is cut once per optimizer step into the two fp16
 * piece planes of w * scale(amax(w)) that the MFMA kernel multiplies (KoafGemm.fmt 1), in two arrangements:
 *   F image [2][R][Kp]          Kp = taps*C rounded up to 32: B operand of the forward GEMM (rows = output channels)
 *   D image [2][C][taps*Rp]     Rp = R rounded up to 32: the transposed weight, B operand of the data-gradient GEMM
 * Two launches handle a whole table of descriptors (device memory): max |w| per weight -> amax[i], then the images.
 * tile0 = running sum of ceil(R/32) * taps * ceil(C/32) over the preceding entries, `ntiles` the total.  taps > 1 needs
 * C % 32 == 0.  src_off counts floats from `base`, f_off / d_off 16-bit elements from `planes` (multiples of 8; -1 =
 * image not wanted). */
typedef struct KoafWPlane {
    int64_t src_off, f_off, d_off, tile0;
    int32_t R, taps, C, Kp, Rp, _pad;
} KoafWPlane;
int koaf_wplanes_build(const float* base, uint16_t* planes, float* amax, const KoafWPlane* table_dev, int32_t n,
                       int64_t ntiles, void* stream);
/* Activation plane images (KoafOperand.kind 2 on the A side): planes[q][pixel][C], q = 0 (hi), 1 (lo), of
 *   tf 0: x          tf 1: relu(sc[c]*x + sh[c])          tf 2: sc[c]*x + sh[c] - sc2[c]*x2
 * times the operand scale (scale(*amax) if amax != NULL, else fscale), clamped to +-65504, cut like the GEMM's own loader
 * cuts them (bit-identical), followed by the 16-B zero chunk.  `planes` holds koaf_act_planes_elems(npix, C) 16-bit
 * elements.  One HBM pass (read 4 or 8 B, write 4 B per element) that saves the convolution's k-loop the KH*KW-fold
 * conversion of every element. */
/* Gathered 3x3 / stride 1 / pad 1 convolutions over activation plane images (image rows up to 96 pixels) run the HALO
 * kernel: 256-pixel tiles in raster order whose source pixels for all nine taps are one contiguous range kept in LDS, so
 * the input tile is fetched 1.8 times instead of nine (k runs (channel chunk, tap, channel): the sums are reassociated
 * against the per-tap gather kernel, same accuracy).  Two shapes: 256 rows / 8 waves / one block per CU (halo double-
 * buffered across channel chunks) and 128 rows / 4 waves / two blocks per CU (one halo buffer; the 64-channel layers).
 * koaf_set_conv3x3_halo(mode): 0 sends them through the gather kernel instead, 1 (default) picks the shape per layer,
 * 2 / 3 force the 256- / 128-row shape where it fits (tests / A-B measurements); returns the previous mode.  Process-wide;
 * not meant to be flipped while other threads launch. */
int koaf_set_conv3x3_halo(int on);
/* Dense K-contiguous fp32 A operands in front of weight plane images -- the 1x1 / stride-1 convolutions (plain, BatchNorm-prologue,
 * bottleneck-tail loaders: koafusion/models/_torchvision.py:118-138) and their data gradients with the BatchNorm-backward apply --
 * with 128-row tiles and K a multiple of 64 run the STREAMED kernel: the four waves of a block each load, transform and split their
 * own 32 rows, two k-tiles ahead in registers, the weight tiles arrive through a three-stage LDS ring, and a persistent block
 * prefetches across tile boundaries.  Same pieces, same MFMA order per accumulator: bit-identical to the block-wide loader.
 * koaf_set_stream(0) sends them through the block-wide loader instead (tests / A-B measurements); on by default; returns the
 * previous setting.  Process-wide; not meant to be flipped while other threads launch. */
int koaf_set_stream(int on);
int64_t koaf_act_planes_elems(int64_t npix, int32_t C);
int koaf_act_planes(const float* x, const float* x2, int64_t npix, int32_t C, int32_t tf, const float* sc, const float* sh,
                    const float* sc2, const float* amax, float fscale, uint16_t* planes, int32_t act16, void* stream);
/* what the convolution entry points take for a weight whose images are current (all device pointers) */
typedef struct KoafWImg {
    const uint16_t* f;      /* F image or NULL */
    const uint16_t* d;      /* D image or NULL */
    const float* amax;      /* max |w| the images were scaled by */
} KoafWImg;
/* dy given as its BatchNorm-backward apply (KoafOperand.tf 2): dy = coef0*dz + coef3 - coef2*c with coef [4][Cout] and amax
 * from koaf_bn_bwd_finalize; dz and c are [N,OH,OW,Cout] like dy.  Needs the fp16 scheme (amax; for dgrad also wimg). */
typedef struct KoafBnApply {
    const float* dz;
    const float* c;
    const float* coef;
    const float* amax;
} KoafBnApply;

/* ---- bf16 ACTIVATION STORAGE (`act16` of the entry points below; BASELINE.json config 2 "bf16") -------------------
 * A trunk may keep its FORWARD ACTIVATIONS -- stem / conv outputs, block outputs, max-pool output -- in HBM as bf16 instead of
 * fp32: half the bytes on every HBM-bound call, half the memory saved for backward.  act16 != 0 says that the activation tensors
 * among a call's arguments (named at each entry point) are bf16 behind their float* type; everything else stays fp32: weights,
 * BatchNorm statistics and coefficients, every gradient, all accumulation and all arithmetic -- a kernel widens the bf16 values
 * on load (exact), computes exactly as in the fp32 mode, and only a producer's store rounds (to nearest even).  It is a storage
 * mode, selected per model (config key `activation_storage: bf16`, default fp32), reported by bench.py as a named secondary
 * with its measured error against the fp32 mode; the parity gate (1e-3 of the reference) is the fp32 mode's.
 * Activation arguments per entry point: koaf_conv2d_fwd / koaf_gconv3x3_fwd x, y; koaf_conv2d_dgrad(_bnb) dy_apply->c and
 * bnb->c / y / c2; koaf_conv2d_wgrad / koaf_gconv3x3_wgrad x and dy_apply->c; koaf_stem_fwd y; koaf_stem_wgrad / koaf_stem_dgrad dy_apply->c; koaf_colstats x; koaf_bn_add_relu /
 * koaf_bn_relu c, idt, y; koaf_bn_bwd_reduce c, ymask; koaf_bn_bwd_apply c; koaf_maxpool_fwd c, y; koaf_gap_fwd y; koaf_act_planes
 * x (tf 0 / 1) or x2 (tf 2).  The activation arguments of ONE call share one storage: the entry points cannot tell (every pointer is
 * a float*), a caller that mixed them would have a two-byte tensor read four bytes per element, past its end -- the Python
 * wrappers refuse such a call before anything is launched (ops/_base.py _act16). */

/* ---- Convolution (nn.Conv2d, bias-free; _torchvision.py:23-31) as implicit GEMM on NHWC -------
 * x [N,H,W,Cin], w packed [Cout,KH,KW,Cin] (the memory of a channels_last (Cout,Cin,KH,KW)
 * parameter), y [N,OH,OW,Cout].  in_sc/in_sh (nullable): fused BatchNorm+ReLU of the producer
 * applied to x on load.  stats (nullable): per-M-tile column sums / sums of squares of y for the
 * following BatchNorm (train mode), *stats_rows rows of [2][Cout], summed about stats_shift[Cout] (nullable = 0; pass
 * that BatchNorm's running_mean and hand the same pointer to koaf_bn_finalize).  wimg (nullable): plane images of w
 * (koaf_wplanes_build; they must be current): the contraction then runs on the fp16 scheme (KoafGemm.fmt 1) with the
 * activations at the fixed scale KOAF_ACT_SCALE and the weight tiles DMA'd from wimg->f (wimg->f NULL: weight split in
 * the kernel with the same scale -- bit-identical, slower).  x_planes (nullable; needs wimg->f, Cin % 32 == 0): activation
 * plane images of the TRANSFORMED input (koaf_act_planes: tf 1 with in_sc / in_sh, or tf 0; fscale KOAF_ACT_SCALE): the
 * gathered input tiles are then DMA'd as well and x / in_sc / in_sh are not read -- bit-identical, and what the 3x3
 * convolutions use: their fp32 loader converts every element nine times.  */
#define KOAF_ACT_SCALE 16.0f   /* activations are O(1) behind BatchNorm: |x| * 16 clamps at 65504, 2^-29 absolute resolution */
/* tail (nullable; 1x1 / stride 1 convolutions on the fp16 scheme with wimg->f): x is the raw output c3 of the PREVIOUS block's
 * last convolution, in_sc / in_sh its BatchNorm's coefficients, tail->idt that block's identity: the convolution's input
 * y = relu(in_sc*x + in_sh + idt) -- the bottleneck tail, _torchvision.py:132-136 -- is formed on load (KoafOperand.tf 3) and
 * written once to tail->y_out [N,H,W,Cin] (nullable), so the element-wise tail pass (koaf_bn_add_relu: 12 B per element) and
 * this convolution's own read of y (4 B) become one read of c3 + idt and one write of y.  idt_sc / idt_sh (nullable pair): the
 * block had a downsample branch -- idt is that branch's raw convolution output and these its BatchNorm coefficients. */
typedef struct KoafTail {
    const float* idt;
    float* y_out;
    const float* idt_sc;   /* nullable pair: the identity is idt_sc[c]*idt + idt_sh[c] -- the raw output of a downsample */
    const float* idt_sh;   /* convolution and its BatchNorm coefficients (koaf_bn_add_relu's idsc / idsh)             */
} KoafTail;
/* emit (nullable): the BatchNorm behind THIS convolution is already known (eval mode; a stage rebuilt in backward from its saved
 * statistics: _torchvision.py:118-138 with running / saved statistics): the epilogue also cuts the activation plane images of
 * relu(sc * y + sh) -- what the following 3x3 convolution's koaf_act_planes pre-pass would read y back for -- into `planes`
 * (koaf_act_planes_elems(N * OH * OW, Cout) elements, bit-identical to that pass). */
typedef struct KoafEmit {
    uint16_t* planes;
    const float* sc;
    const float* sh;
} KoafEmit;
int koaf_conv2d_fwd(const float* x, const float* w, float* y, int32_t N, int32_t H, int32_t W,
                    int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                    const float* in_sc, const float* in_sh, float* stats, int32_t* stats_rows,
                    const float* stats_shift, const KoafWImg* wimg, const uint16_t* x_planes, const KoafTail* tail,
                    const KoafEmit* emit, int32_t act16, void* stream);
/* rows of the stats buffer koaf_conv2d_fwd writes for M output pixels */
int32_t koaf_conv2d_stats_rows(int64_t M, int32_t Cout);
/* dx [N,H,W,Cin] = conv_transpose(dy [N,OH,OW,Cout], w) (+residual: the other branch's gradient);
 * w is read K-major in place (no re-packed copy).  With wimg AND dy_amax (device scalar: max |dy|, e.g. from
 * koaf_bn_bwd_apply) the contraction runs on the fp16 scheme, the weight tiles DMA'd from wimg->d.  dy_apply (nullable, needs
 * wimg->d; dy may then be NULL): dy is formed on load from (dz, c), see KoafBnApply.  dy_planes (nullable; needs wimg->d,
 * dy_amax, Cout % 32 == 0): activation plane images of dy (koaf_act_planes with amax = dy_amax; tf 2 for an applied dy):
 * dy / dy_apply are then not read.  */
int koaf_conv2d_dgrad(const float* dy, const float* w, float* dx, int32_t N, int32_t H, int32_t W,
                      int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                      int32_t pad, const float* residual, const KoafWImg* wimg, const float* dy_amax,
                      const KoafBnApply* dy_apply, const uint16_t* dy_planes, int32_t act16, void* stream);
/* Same, with the BatchNorm(+ReLU) backward reduction of the layer that PRODUCED x fused into the epilogue (see
 * KoafGemm.bnb_*): dx receives the masked gradient dz; part [*part_rows][nsum][Cin] (nsum = 2, or 3 with c2) feeds
 * koaf_bn_bwd_finalize.  koaf_conv2d_dgrad_bnb_rows() bounds *part_rows for sizing. */
typedef struct KoafBnb {
    int32_t mode, _pad;     /* 1: mask y > 0; 2: mask sc*c+sh > 0 */
    float* dz_amax;         /* nullable: device scalar set to max |dz| (zeroed by the call) -> koaf_bn_bwd_finalize */
    const float* c;
    const float* y;
    const float* sc;
    const float* sh;
    const float* mean;
    const float* invstd;
    const float* c2;        /* optional second BatchNorm on the same dz */
    const float* mean2;
    const float* invstd2;
} KoafBnb;
int32_t koaf_conv2d_dgrad_bnb_rows(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t stride);
int koaf_conv2d_dgrad_bnb(const float* dy, const float* w, float* dx, int32_t N, int32_t H, int32_t W,
                          int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                          const float* residual, const KoafBnb* bnb, float* part, int32_t* part_rows,
                          const KoafWImg* wimg, const float* dy_amax, const KoafBnApply* dy_apply,
                          const uint16_t* dy_planes, int32_t act16, void* stream);
/* dw packed [Cout,KH,KW,Cin] = sum_pixels dy^T x, x optionally transformed on load.  Deterministic
 * split-K: slabs = workspace of koaf_conv2d_wgrad_ws() floats (0 = none needed).  dy_amax (nullable): max |dy| on the
 * device -> fp16 scheme.  dy_planes + x_planes (nullable, together; need dy_amax or dy_apply, Cin % 8 == 0, Cout % 8 == 0):
 * activation plane images of dy (amax = dy_amax; tf 2 for an applied dy) and of the transformed x (fscale KOAF_ACT_SCALE):
 * both operand tiles are then DMA'd, K-major, and dy / x / in_sc / in_sh are not read.  */
int64_t koaf_conv2d_wgrad_ws(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                             int32_t KH, int32_t KW, int32_t stride, int32_t pad);
int koaf_conv2d_wgrad(const float* dy, const float* x, float* dw, int32_t N, int32_t H, int32_t W,
                      int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                      int32_t pad, const float* in_sc, const float* in_sh, float* slabs,
                      const float* dy_amax, const KoafBnApply* dy_apply, const uint16_t* dy_planes,
                      const uint16_t* x_planes, int32_t act16, void* stream);

/* ---- Grouped 3x3 convolution (ResNeXt 32x4d; _torchvision.py:110,327-330) -------------------
 * Runs on the same MFMA GEMM as 64-channel block-diagonal slabs: packed weights [C][3][3][C/groups]
 * are expanded to wexp [C/64][64][9][64] (zeros off the group blocks), gradients compressed back.
 * Contraction scheme (KoafGemm.fmt): with the operands' largest magnitudes known the three calls run on the fp16 scheme (two
 * scaled fp16 pieces, three products: half the matrix instructions of the bf16 scheme, same accuracy) -- w_amax = device scalar
 * max |w| (koaf_gconv_expand_w leaves it when given `amax`, which the caller zeroes beforehand), dy_amax = device scalar max |dy|
 * (koaf_bn_bwd_apply leaves it); activations x use the fixed activation scale KOAF_ACT_SCALE.  NULL scalars (and every call with
 * act16 != 0): the bf16 scheme. */
int koaf_gconv_expand_w(const float* w, float* wexp, int32_t C, int32_t groups, float* amax, void* stream);
int koaf_gconv_compress_dw(const float* dwexp, float* dw, int32_t C, int32_t groups, void* stream);
int koaf_gconv3x3_fwd(const float* x, const float* wexp, float* y, int32_t N, int32_t H, int32_t W,
                      int32_t C, int32_t stride, const float* in_sc, const float* in_sh,
                      float* stats, int32_t* stats_rows, const float* stats_shift, const float* w_amax, int32_t act16, void* stream);
int koaf_gconv3x3_dgrad(const float* dy, const float* wexp, float* dx, int32_t N, int32_t H,
                        int32_t W, int32_t C, int32_t stride, const float* w_amax, const float* dy_amax, void* stream);
int64_t koaf_gconv3x3_wgrad_ws(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride);
int koaf_gconv3x3_wgrad(const float* dy, const float* x, float* dwexp, int32_t N, int32_t H,
                        int32_t W, int32_t C, int32_t stride, const float* in_sc,
                        const float* in_sh, float* slabs, const float* dy_amax, int32_t act16, void* stream);

/* ---- Stem: 7x7 s2 p3 conv on the 1->3 channel-repeated image (_torchvision.py:170; the
 * `repeat "b ch r c -> b (k ch) r c", k=3` of _xrNmrMcP.py:211-213 is folded: w1t = sum_c w[:,c]).
 * x [N,H,W] (single channel), w1t [49][64], y [N,OH,OW,64].  */
/* stats (nullable): koaf_stem_stats_rows(N, H) rows of [2][64] -- column sums and sums of squares of y about stats_shift[64]
 * (nullable = 0), the partials koaf_bn_finalize takes for the BatchNorm behind the stem (as koaf_conv2d_fwd's stats) */
int32_t koaf_stem_stats_rows(int32_t N, int32_t H);
int koaf_stem_fwd(const float* x, const float* w1t, float* y, int32_t N, int32_t H, int32_t W,
                  float* stats, const float* stats_shift, int32_t act16, void* stream);
int64_t koaf_stem_wgrad_ws(int32_t N, int32_t H, int32_t W);
/* dy_apply (nullable; dy may then be NULL): dy is formed on load from (dz, c, coef) as coef0*dz + coef3 - coef2*c -- the
 * BatchNorm-backward apply of the stem's BatchNorm (koaf_bn_bwd_finalize with mean) -- and never written; act16: c is bf16 */
int koaf_stem_wgrad(const float* dy, const float* x, float* dw1t, int32_t N, int32_t H, int32_t W,
                    float* slabs, const KoafBnApply* dy_apply, int32_t act16, void* stream);
/* w [64,7,7,3] packed -> w1t [49][64] (sum over the 3 channels); gradient un-fold (copy x3) */
int koaf_stem_fold_w(const float* w, float* w1t, void* stream);
int koaf_stem_unfold_dw(const float* dw1t, float* dw, void* stream);
/* Data gradient of the stem (input-gradient / saliency path; the train step's inputs are leaves and never call it):
 *   dx[n][iy][ix] = sum over (kh, kw, co) with (iy+3-kh), (ix+3-kw) even and in range of
 *                   dy[n][(iy+3-kh)/2][(ix+3-kw)/2][co] * w1t[kh*7+kw][co]
 * dx [N,H,W]: the gradient of the single-channel image (the three repeated channels fold into one as in forward); every element
 * is written.  Gather form -- a 16 x 16 tile of dy pixels forms its 49 tap sums with fp32 FMAs, the four input-pixel parity
 * classes then collect their 3x3 / 3x4 / 4x3 / 4x4 windows through LDS in a fixed order: no atomics, run-to-run identical bits.
 * dy_apply / act16: as for koaf_stem_wgrad (dy formed on load, never written). */
int koaf_stem_dgrad(const float* dy, const float* w1t, float* dx, int32_t N, int32_t H, int32_t W,
                    const KoafBnApply* dy_apply, int32_t act16, void* stream);

/* ---- BatchNorm2d (nn.BatchNorm2d; _torchvision.py:172,121-131) ------------------------------- */
/* per-block column sums / sums of squares of x [rows][C] -> part [*part_rows][2][C]
 * (koaf_colpart_rows(rows, C) rows), summed about shift[C] (nullable = 0); for producers without a GEMM epilogue
 * (stem). */
int koaf_colstats(const float* x, int64_t rows, int32_t C, float* part, int32_t* part_rows,
                  const float* shift, int32_t act16, void* stream);
int32_t koaf_colpart_rows(int64_t rows, int32_t C);
/* Bytes of the fp64 workspace `ws` the two finalisations below use to spread a long list of partial rows over
 * the chip (two-stage, fixed-order reduction); 0 = not needed for this row count.  ws may always be NULL
 * (single-stage). */
int64_t koaf_bn_reduce_ws(int32_t rows, int32_t C);
/* stats [rows][2][C] -> mean, invstd, sc = gamma*invstd, sh = beta - mean*sc; train: updates
 * running_mean/var (momentum, unbiased var) and ++num_batches_tracked (int64).  eval (train==0):
 * stats ignored, uses running stats.  shift (nullable): the per-channel shift k the statistics were summed about
 * (KoafGemm.stats_shift / koaf_colstats): mean = k + E[x-k], var = E[(x-k)^2] - E[x-k]^2; it may alias running_mean
 * (read before the update).  */
int koaf_bn_finalize(const float* stats, int32_t rows, int32_t C, int64_t count,
                     const float* gamma, const float* beta, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                     int32_t train, float* mean, float* invstd, float* sc, float* sh,
                     const float* shift, double* ws, void* stream);
/* y = relu(sc*c + sh + identity-term); identity-term = idt (materialised) or idsc*idt+idsh
 * (downsample branch BN folded).  Bottleneck tail, _torchvision.py:132-136.  */
int koaf_bn_add_relu(const float* c, const float* sc, const float* sh, const float* idt,
                     const float* idsc, const float* idsh, float* y, int64_t rows, int32_t C,
                     int32_t act16, void* stream);
/* y = relu(sc*c+sh) materialised */
int koaf_bn_relu(const float* c, const float* sc, const float* sh, float* y, int64_t rows,
                 int32_t C, int32_t act16, void* stream);
/* backward reduce: dz = g * mask, partial sums of dz and dz*(c-mean)*invstd.
 * mask_mode 0: none; 1: y>0 from tensor `ymask`; 2: sc*c+sh>0 recomputed.  If dz_out != NULL
 * writes the masked gradient.  part [*part_rows][2][C] (koaf_colpart_rows rows).  dz_amax (nullable): device scalar set to
 * max |dz| (for koaf_bn_bwd_finalize's bound). */
int koaf_bn_bwd_reduce(const float* g, const float* c, const float* ymask, const float* sc,
                       const float* sh, const float* mean, const float* invstd, int32_t mask_mode,
                       float* dz_out, float* part, int32_t* part_rows, int64_t rows, int32_t C,
                       float* dz_amax, int32_t act16, void* stream);
/* the same reduction for a BatchNorm(+ReLU) that is followed by the 3x3 / stride-2 / pad-1 max-pool (the stem,
 * _torchvision.py:172-174): the upstream gradient is gathered from the POOL's gradient pool_g [N,OH,OW,C] and the window
 * positions pool_argmax of koaf_maxpool_fwd (the arithmetic of koaf_maxpool_bwd), masked by sc*c+sh > 0 and written to dz_out
 * [N,H,W,C] -- the pool's input gradient is never written and read back */
int koaf_bn_bwd_reduce_pool(const float* pool_g, const uint8_t* pool_argmax, const float* c, const float* sc,
                            const float* sh, const float* mean, const float* invstd, float* dz_out, float* part,
                            int32_t* part_rows, int32_t N, int32_t H, int32_t W, int32_t C, float* dz_amax,
                            int32_t act16, void* stream);
/* part [rows][nsum][C] -> dgamma (= sum index i1), dbeta (= sum index 0), and apply coefficients
 * coef [3][C] = {sc, dbeta/M, sc*invstd*dgamma/M}.  (nsum, i1) = (2, 1) for the plain layout.
 * With mean: coef is [4][C], the fourth row = coef2*mean - coef0*coef1, so that dc = coef0*dz + coef3 - coef2*c -- the form
 * the GEMM loaders evaluate on load (KoafOperand.tf 2: the dgrad / wgrad convolutions then read dz and c and dc is never
 * written).  amax (nullable, needs mean): device scalar set to a guaranteed bound of max |dc|, the scale of that operand on
 * the fp16 scheme: max_c |coef0| (dz_amax + |coef1|) + |coef2| sqrt(M - 1) / invstd  (dz_amax: device scalar max |dz| from
 * koaf_bn_bwd_reduce / KoafBnb.dz_amax; no sample lies further than sqrt(M - 1) standard deviations from its mean). */
int koaf_bn_bwd_finalize(const float* part, int32_t part_rows, int32_t C, int64_t count,
                         const float* sc, const float* invstd, float* dgamma, float* dbeta,
                         float* coef, int32_t nsum, int32_t i1, double* ws, const float* mean,
                         const float* dz_amax, float* amax, void* stream);
/* The same finalisation for a BatchNorm in EVAL mode (running statistics: y = sc*c + sh with constant sc, sh), whose backward
 * is dc = sc*dz: coef [coef_rows][C] = {sc, 0, 0[, 0]} (coef_rows 3 | 4: the layouts koaf_bn_bwd_apply / KoafBnApply read),
 * dgamma / dbeta (nullable) the same sums as in train mode -- with xhat formed from the running statistics the reductions
 * already used -- and amax (nullable, coef_rows 4) = max_c |sc| * *dz_amax.  part may be NULL when neither dgamma nor dbeta is
 * wanted (frozen parameters): nothing is reduced then. */
int koaf_bn_bwd_finalize_eval(const float* part, int32_t part_rows, int32_t C, const float* sc, float* dgamma, float* dbeta,
                              float* coef, int32_t coef_rows, int32_t nsum, int32_t i1, double* ws, const float* dz_amax,
                              float* amax, void* stream);
/* dc = coef0*(dz - coef1) - coef2*(c - mean), materialised (consumers that are not GEMMs: the stem's weight gradient; GEMMs
 * without scale information).  amax (nullable): device scalar raised to max |dc| (atomic max; zero it beforehand). */
int koaf_bn_bwd_apply(const float* dz, const float* c, const float* mean, const float* coef,
                      float* dc, int64_t rows, int32_t C, float* amax, int32_t act16, void* stream);

/* ---- input pipeline on the device (koafusion/preproc/_pt.py; applied per sample by the reference's CPU loader
 * workers, koafusion/datasets/_data_provider.py:295-335) ------------------------------------------------------- */
/* Integer volumes as stored on disk (dtype 1 = uint8: radiograph PNGs, 2 = uint16, 3 = int16: MRI NIfTI) -> fp32.  The loader
 * ships the raw integers over PCIe (4x / 2x fewer bytes than the fp32 tensors the reference's workers produce,
 * _data_provider.py:460-498) and the device widens them ahead of koaf_minmax / koaf_augment. */
int koaf_widen(const void* x, int32_t dtype, float* y, int64_t n, void* stream);
/* per-sample minimum and maximum of x [B][n] -> mm [B][2]; ws: B * koaf_minmax_ws(n) floats.  PTToUnitRange :75-99 */
int64_t koaf_minmax_ws(int64_t n);
int koaf_minmax(const float* x, int32_t B, int64_t n, float* mm, float* ws, void* stream);
/* y = ((gamma(rotate(unit(x)))) - mean) / std on a batch x [B][R][C][S] (S = 1: radiographs):
 *   unit(v) = (v - min_b) / (max_b - min_b)                                   PTToUnitRange        :75-99
 *   rotate: in-plane (R, C) bilinear resampling, zero padding, F.affine_grid + F.grid_sample with
 *           align_corners=False and [[cos,-sin,0],[sin,cos,0]]                PTRotate3DInSlice / PTRotate2D :257-345
 *   gamma(v) = pow(v, e)                                                      PTGammaCorrection    :203-232
 * params [B][4] = {cos(theta), sin(theta), e (0 = no gamma), rotate flag (0 = copy)}.  */
int koaf_augment(const float* x, float* y, const float* mm, const float* params, int32_t B, int32_t R, int32_t C,
                 int32_t S, float mean, float stdv, void* stream);

/* ---- the same pipeline from the STORED volumes (koaf_inpipe.hip): np.flip of RIGHT knees (datasets/oai/_dataset.py:298-321),
 * RandomCrop | CenterCrop (preproc/_np_nd.py:62-144), NumpyToTensor, the four transforms above and PTInterpolate(0.5, 0.5[, 0.5 |
 * 1.0]) (run/train_prog_fus.py:111-116) without a cropped, flipped or widened copy.  Every sample is read in place through a
 * DEVICE table of 8 x int64 per sample:
 *   [0] address of stored voxel (0, 0, 0)        [1..3] stored extents R0, C0, S0 (contiguous, S fastest; a radiograph: S0 = 1)
 *   [4..6] origin r0, c0, s0: the stored index of window voxel 0 on each axis
 *   [7] bit mask of the axes walked backwards (1 = R, 2 = C, 4 = S): window index i is stored index origin - i there, + i elsewhere
 * The window R x C x S (S = 1: radiographs) is the same for the whole batch; stored extents and origins are per sample, so ragged
 * volumes need no stacking.  dtype of the stored elements: 0 = fp32, 1 / 2 / 3 = uint8 / uint16 / int16 as in koaf_widen; the
 * address is aligned to the element, nothing more.  The caller checks every window against its volume before the table is
 * uploaded (ops.window_rows refuses such a row on the host, so the Python layer never reaches what follows).  As a defence only, for
 * a caller of this ABI that did not, the kernels re-read the row's extents and do not dereference a row whose window leaves them:
 * its (min, max) and its output are NaN.  The extents themselves and the address are taken on trust.
 * koaf_window_minmax  mm [B][2] = (min, max) over the window only, exact (integers below 2^24 convert exactly); two stages in a
 *   fixed order, no atomics; ws: B * koaf_window_minmax_ws(R * C * S) floats.
 * koaf_input_pipeline  y = mean over pool x pool x pool_s window voxels of f, pool and pool_s in {1, 2} dividing R, C and S:
 *   f = koaf_augment's arithmetic at window coordinates with mm and params [B][4] as there; a bilinear neighbour outside the
 *   WINDOW reads as zero whatever the stored volume holds there (the reference rotates the cropped tensor).  The pool is
 *   koaf_downscale2's sum in its order times 1 / (pool * pool * pool_s).  layout 0: y [B][R/pool][C/pool][S/pool_s], the
 *   reference's; 1: y [B][S/pool_s][R/pool][C/pool], slice-major.  A constant window divides 0 by 0: NaN, as the reference. */
int64_t koaf_window_minmax_ws(int64_t n);
int koaf_window_minmax(const int64_t* table, int32_t dtype, int32_t B, int32_t R, int32_t C, int32_t S, float* mm, float* ws,
                       void* stream);
int koaf_input_pipeline(const int64_t* table, int32_t dtype, float* y, const float* mm, const float* params, int32_t B, int32_t R,
                        int32_t C, int32_t S, int32_t pool, int32_t pool_s, int32_t layout, float mean, float stdv, void* stream);

/* ---- MaxPool2d 3x3 s2 p1 over relu(sc*c+sh) (_torchvision.py:173-174), GAP (:182) ------------
 * A NaN pre-activation stays a NaN (as in koaf_bn_add_relu) and takes its windows (as in F.max_pool2d; argmax = its last position
 * in the window), so it reaches y and status word 0 instead of turning into a zero. */
int koaf_maxpool_fwd(const float* c, const float* sc, const float* sh, float* y, uint8_t* argmax,
                     int32_t N, int32_t H, int32_t W, int32_t C, int32_t act16, void* stream);
/* da [N,H,W,C] (gradient wrt relu(bn(c))) gathered from dy via argmax (every element written) */
int koaf_maxpool_bwd(const float* dy, const uint8_t* argmax, float* da, int32_t N, int32_t H,
                     int32_t W, int32_t C, void* stream);
int koaf_gap_fwd(const float* y, float* out, int32_t N, int32_t HW, int32_t C, int32_t act16, void* stream);
int koaf_gap_bwd(const float* dout, float* dy, int32_t N, int32_t HW, int32_t C, void* stream);

/* ---- Class-activation maps of the slice-wise trunks (koaf_cam.hip; not in the reference) -------
 * cam[n][p] = sum_c A[n][p][c] * w[n][c], clamped at 0 when `relu`; A [N][HW][C] the trunk's NHWC feature map (fp32, or bf16
 * when act16: widened on load, exact), w [N][C] fp32 (Grad-CAM: the gradient of the logit with respect to the pooled token,
 * over HW).  img_sum[n] = sum_p of the stored cam[n][p]; img_max[n] = max_p |cam[n][p]|.  One block per image, one wave per
 * pixel row at a time; every reduction is a fixed-order tree (no atomics): run-to-run identical bits.  A NaN in a row gives a
 * NaN in that pixel, in img_sum[n] and in img_max[n] (integer maximum over the magnitude bits).  C % 4 == 0, C <= 16384. */
int koaf_cam(const float* A, const float* w, float* cam, float* img_sum, float* img_max, int32_t N, int32_t HW, int32_t C,
             int32_t relu, int32_t act16, void* stream);
/* image n = b*K + k of cam [B*K][h][w] resized to H x W (torch's align_corners=False bilinear rule, as koaf_resize), divided by a
 * maximum and written to out[b*sb + k*sk + i*si + j*sj] (strides in elements, all > 0): resize, normalise and the unfold into the
 * layout the model received in one write pass.  normalize 0: none; 1: by the largest img_max among the sample's K images;
 * 2: by the image's own img_max.  A maximum of 0 writes zeros, a non-finite one NaN for everything it scales.  Consecutive
 * lanes walk the unit-stride axis of out: columns (sj == 1) or slices (sk == 1, the (B,1,R,C,S) volumes: whole output rows from
 * a source row staged in LDS, where its w * K floats fit).  K <= 8192 and 8 (H + W) + 4 K <= 65536 (taps and scales sit in LDS). */
int koaf_cam_upsample(const float* cam, const float* img_max, float* out, int32_t B, int32_t K, int32_t h, int32_t w, int32_t H,
                      int32_t W, int64_t sb, int64_t sk, int64_t si, int64_t sj, int32_t normalize, void* stream);

/* ---- Path attributions over the inputs: integrated gradients, SmoothGrad (koaf_attr.hip; not in the reference) -------
 * All tensors are contiguous fp32 rows [B][n], any n >= 1; rows need not be 16-byte aligned (16-byte accesses where n % 4 == 0
 * and the pointers are aligned, one element per lane otherwise).  Element-wise, no atomics: the bits do not depend on the grid.
 * No operation is fused: every difference, product and sum below is rounded to fp32 on its own, in the order written, so that
 * numpy's fp32 restates both kernels bit for bit.  1 <= J <= KOAF_ATTR_MAX_J (alpha and the generator keys sit in LDS).
 *
 * koaf_path_points  out[j][b][i] = (bs + alpha[j] * (x[b][i] - bs)) + sigma_b * z(seed, draw0 + j, b, i),  j in [0, J)
 *   bs = base[b][i], or base_value when base is NULL;  alpha: device [J];  out: [J][B][n];  x and base are read once for all J.
 *   sigma_b = noise_level * (mm[b][1] - mm[b][0]), mm [B][2] as koaf_minmax leaves it.  mm NULL or noise_level == 0: no noise
 *   term at all (nothing is drawn, nothing added).  B <= 65535; draw0 >= 0, draw0 + J <= 2^31.
 *   z: a standard normal, a function of (seed, draw index d = draw0 + j, b, i) only -- not of J, B, n, the grid, or how the
 *   draws are split over calls.  With mix64(v): v += 0x9E3779B97F4A7C15; v = (v ^ v >> 30) * 0xBF58476D1CE4E5B9;
 *   v = (v ^ v >> 27) * 0x94D049BB133111EB; return v ^ v >> 31  (64-bit wrap-around; the dropout kernels' hash):
 *     key = mix64(seed ^ mix64(d << 32 | b));   h = mix64(key ^ mix64(i >> 1))          one hash per PAIR of elements
 *     u1 = ((h >> 40) + 1) / 2^24  in (0, 1];   u2 = ((h >> 16) & 0xFFFFFF) / 2^24  in [0, 1)
 *     r = sqrt(-2 ln u1);   z = r cos(2 pi u2) for even i,  r sin(2 pi u2) for odd i     (Box-Muller)
 *   evaluated in fp32 as sqrtf(-2 * logf(u1)) and sincospif(2 u2) (2 u2 is exact; the pi-scaled functions need no argument
 *   reduction).  |z| <= sqrt(2 ln 2^24) = 5.77.
 * koaf_attr_fold  s = first ? +0 : acc[b][i];  for j = 0 .. J-1 in order: s = s + w[j] * f(g[j][b][i]);  f(v) = v, or v * v when
 *   `square`;  g: [J][B][n], w: device [J].  acc[b][i] = s, or, with `finish`, s * (x[b][i] - bs) (bs as above): the
 *   integrated-gradients map, written by the last chunk's call without another pass.  Without `finish`, x and base are not read
 *   (and may be NULL). */
#define KOAF_ATTR_MAX_J 64
int koaf_path_points(const float* x, const float* base, float base_value, const float* alpha, float* out, int32_t J, int32_t B,
                     int64_t n, const float* mm, float noise_level, uint64_t seed, int64_t draw0, void* stream);
int koaf_attr_fold(float* acc, const float* g, const float* w, const float* x, const float* base, float base_value, int32_t J,
                   int32_t B, int64_t n, int32_t square, int32_t first, int32_t finish, void* stream);

/* ---- Occlusion sensitivity maps (koaf_occl.hip; captum's Occlusion, named by the reference's recipe and never built there) -------
 * An input row is a box of four extents dims[4] (an input of lower rank is padded IN FRONT with ones), win[4] the window and str[4]
 * the strides, 1 <= str <= win <= dims: host arrays of four.  cnt[a] = 1 + ceil((dims[a] - win[a]) / str[a]) windows along
 * dimension a; window k, flat and row-major over cnt with the last dimension fastest, covers [j str, min(j str + win, dims)) along
 * every dimension (the last window is clipped).  K = prod cnt.  Rows and K stay below 2^31.  All four kernels are element-wise or
 * row-wise, with no atomics and fixed orders: the bits do not depend on the grid.
 *
 * koaf_occl_points  out[j][b][i] = (i in window k0 + j) ? bs : x[b][i],  j in [0, J), k0 + J <= K;  bs = base[b][i], or base_value
 *   when base is NULL.  x, base: [B][n], out: [J][B][n]; x and base are read once for all J.  16-byte accesses where n % 4 == 0 and
 *   the pointers are aligned, one element per lane otherwise.  1 <= J <= KOAF_ATTR_MAX_J (the windows sit in LDS), B <= 65535.
 * koaf_occl_slices  out[r] = the H x W slice image n of x with window k set to the baseline, (k, n) = rows[r] -- a device int32
 *   table [nrows][2], n = b * K_img + kk: pixel (i, j) is element b*sb + kk*sk + i*si + j*sj of x, the strides of
 *   koaf_cam_upsample, so out[r] is the image the slice fold of the occluded volume would hand the trunk.  Consecutive lanes walk
 *   the unit-stride axis of the source: columns where sj == 1; where sk == 1 (the (B,1,R,C,S) volumes) 16 table rows x 64 pixels
 *   pass through LDS, so that the read (consecutive table rows = consecutive slices of one sample, as run.occlusion lists them)
 *   and the write are both coalesced.  A table row outside [0, K) x [0, B * K_img) is written as zeros, never read through.
 * koaf_occl_rows  out[j][n] = src[j][n] in [0, F) ? fresh[src[j][n]] : cache[n];  cache [N], fresh [F], out [J][N] rows of
 *   row_bytes bytes, row_bytes % 4 == 0 (a byte copy: fp32 and bf16 feature rows alike); src: device int32 [J][N], negative =
 *   the cached row.
 * koaf_occl_fold  out[b][i] = (sum of delta[k][b] over the windows k that cover element i, in ascending k, fp32) / their number
 *   (one fp32 division; every element is covered, str <= win).  delta: [K][B].  No products: numpy's fp32 restates it bit for bit. */
int koaf_occl_points(const float* x, const float* base, float base_value, float* out, int32_t J, int32_t B, const int32_t* dims,
                     const int32_t* win, const int32_t* str, int32_t k0, void* stream);
int koaf_occl_slices(const float* x, const float* base, float base_value, float* out, const int32_t* rows, int32_t nrows, int32_t B,
                     const int32_t* dims, const int32_t* win, const int32_t* str, int32_t K_img, int32_t H, int32_t W, int64_t sb,
                     int64_t sk, int64_t si, int64_t sj, void* stream);
int koaf_occl_rows(const void* cache, const void* fresh, const int32_t* src, void* out, int32_t J, int32_t N, int32_t F,
                   int64_t row_bytes, void* stream);
int koaf_occl_fold(const float* delta, float* out, int32_t K, int32_t B, const int32_t* dims, const int32_t* win, const int32_t* str,
                   void* stream);

/* ---- Attention relevance of the FeaT fusion: rollout and the gradient-weighted rule (koaf_attnrel.hip; not in the reference) ----
 * All tensors are contiguous fp32, any n, h, d >= 1 (tiles are guarded, nothing needs a multiple).  Full fp32 products; sums in a
 * fixed order in fp32 or fp64; no atomics: run-to-run identical bits.  Outputs may not overlap inputs (refused).
 *
 * koaf_attn_layer  the per-layer matrix abar [B][n][n] from koaf_attention_fwd's attn [B][h][n][n].
 *   mode 0 | 1 | 2 (rollout, Abnar & Zuidema 2020): f[i][j] = mean | max | min over heads of attn (heads in index order; the mean
 *   is the running sum divided by h), + 1 at j == i; abar[i][j] = f[i][j] / sum_j f[i][j], the row sum formed in fp64 and the
 *   quotient rounded once.  dout and qkv are NULL.  At most h + 2 roundings per element, all terms >= 0.
 *   mode 3 (Chefer et al. 2021, self-attention rule): abar[i][j] = (1 / h) sum_h relu(attn[h][i][j] * dP[h][i][j]),
 *   dP[h][i][j] = sum_k dout[i][h d + k] * qkv[j][2 h_all d + h d + k]  (dout [B][n][h d]: the gradient with respect to the
 *   attention core's output; qkv [B][n][3 h d]: the fused projection in the '(qkv h d)' split, whose third part is V) -- one fmaf
 *   chain over k in index order per element, held in registers: dP is never stored.  Heads are added in index order and the sum
 *   is divided by h.  A NaN in a product stays.  B <= 65535.
 * koaf_attn_apply  r_out[b][qi][j] = sum_m r_in[b][qi][m] * abar[b][m][j]  (+ r_in[b][qi][j] when add_identity): a few relevance
 *   rows carried through one layer from the left.  r_in [B][q][n], or NULL for the identity (q == n: r_out = abar, + I when
 *   add_identity, exactly).  The m range is cut into sixteen interleaved fmaf chains added as a pairwise tree.  B <= 65535.
 * koaf_attn_segsum  out[b][k] = sum_{u < t} r[b][off + k t + u], k in [0, K): per-slice (t tokens a slice) and per-modality
 *   (K = 1) totals of a relevance row r [B][n]; off + K t <= n.  Terms in index order into an fp64 sum, rounded once. */
int koaf_attn_layer(const float* attn, const float* dout, const float* qkv, float* abar, int32_t B, int32_t n, int32_t h, int32_t d,
                    int32_t mode, void* stream);
int koaf_attn_apply(const float* r_in, const float* abar, float* r_out, int32_t B, int32_t q, int32_t n, int32_t add_identity,
                    void* stream);
int koaf_attn_segsum(const float* r, float* out, int32_t B, int32_t n, int32_t off, int32_t K, int32_t t, void* stream);

/* ---- Modality coalitions and their Shapley values (koaf_coal.hip; not in the reference) ------------------------------------------
 * A coalition is a bit mask over the M inputs of a fusion model, bit i set = input i present; 1 <= M <= KOAF_COAL_MAX_M.
 *
 * koaf_coal_tokens  out[j][b][l][:] = (masks[j] >> seg(l) & 1) ? tx[b][l][:] : t0[b % B0][l][:] -- the final FeaT's input tokens of
 *   coalition j, spliced from the tokens of the intact inputs tx [B][L][D] and of the baselines t0 [B0][L][D], B0 == 1 (one
 *   baseline row for every sample) or B0 == B;  out: [J][B][L][D], all fp32.  seg_off: HOST int32 [M + 1], seg_off[0] == 0 <
 *   seg_off[1] < ... < seg_off[M] == L: token l belongs to input seg(l) = i where seg_off[i] <= l < seg_off[i + 1].  masks: HOST
 *   uint32 [J], J >= 1, no bit at or above M.  Both tables travel as kernel arguments (KOAF_COAL_MAX_J masks a launch), so every
 *   refusal comes ahead of the first launch.  tx and t0 are read once per launch for all of its coalitions; 16-byte accesses where
 *   L * D % 4 == 0 and the pointers are aligned, one element per lane otherwise.  A copy: no value changes.  L * D < 2^31,
 *   B <= 65535.
 * koaf_shapley_fold  from the coalition values v [S][B] (fp32, S == 2^M, row s = the coalition with mask s), in fp64, one thread
 *   per output element, the subsets T taken in ascending mask order (|T| = its number of players):
 *     phi[b][i]      = sum over T without i     of w_phi[|T|] * (v[T + i] - v[T]),                      w_phi[t] = t! (M - t - 1)! / M!
 *     inter[b][i][j] = sum over T without i, j  of w_int[|T|] * (v[T + i + j] - v[T + i] - v[T + j] + v[T]),
 *                      w_int[t] = t! (M - t - 2)! / (M - 1)!;  inter[b][i][i] = 0, and at M == 1 all of it is 0
 *     loo[b][i]      = v[N] - v[N - i],   solo[b][i] = v[{i}] - v[{}]
 *   w_phi: HOST fp64 [M];  w_int: HOST fp64 [M - 1] (NULL at M == 1): the caller's table, the kernel does no factorial arithmetic.
 *   phi, loo, solo: [B][M];  inter: [B][M][M], all fp64. */
#define KOAF_COAL_MAX_M 8
#define KOAF_COAL_MAX_J 64
int koaf_coal_tokens(const float* tx, const float* t0, const int32_t* seg_off, const uint32_t* masks, float* out, int32_t J, int32_t B,
                     int32_t B0, int32_t L, int32_t D, int32_t M, void* stream);
int koaf_shapley_fold(const float* v, const double* w_phi, const double* w_int, double* phi, double* inter, double* loo, double* solo,
                      int32_t S, int32_t B, int32_t M, void* stream);

/* ---- Input plumbing -------------------------------------------------------------------------- */
/* "b ch r c s -> (b s) ch r c" (_xrNmrMcP.py:209-210): x [B,R,C,S] -> out [B*S,R,C] */
int koaf_slice_fold(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S,
                    void* stream);
/* its transpose "(b s) r c -> b r c s": x [B*S,R,C] -> out [B,R,C,S] (the slice fold's backward) */
int koaf_slice_unfold(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S,
                      void* stream);
/* out[b] = sum_i a[b][i] * b[b][i] over a, b [B][n] (gradient x input totals).  Two fixed-order stages, no atomics: run-to-run
 * identical bits.  ws: B * koaf_rowdot_ws(n) floats. */
int64_t koaf_rowdot_ws(int64_t n);
int koaf_rowdot(const float* a, const float* b, int32_t B, int64_t n, float* out, float* ws, void* stream);
/* F.interpolate(scale 0.5, align_corners=False, (bi|tri)linear) == 2x average pooling
 * (preproc/_pt.py:189-192).  x [B,R,C,S] -> out [B,R/2,C/2,S/fs], fs in {1,2}; S==1 for XR. */
int koaf_downscale2(const float* x, float* out, int32_t B, int32_t R, int32_t Cc, int32_t S,
                    int32_t fs, void* stream);

/* F.interpolate(x, scale_factor, mode = linear | bilinear | trilinear, align_corners=False, recompute_scale_factor=True) for any
 * scale factor (preproc/_pt.py:175-192): x [BC, in_size...] -> out [BC, out_size...], ndim = 1 .. 3 spatial dimensions,
 * out_size[d] = floor(in_size[d] * scale[d]) (computed by the caller as torch does). */
int koaf_resize(const float* x, float* out, int64_t BC, int32_t ndim, const int32_t* in_size, const int32_t* out_size,
                void* stream);

/* ---- Transformer pieces (_core_trf.py) ------------------------------------------------------- */
/* nn.Linear: y[M,N] = x[M,K] w[N,K]^T + b (+residual).  Small grids (few tokens) run split-K: ws = workspace
 * of koaf_linear_ws(M, N, K) floats (0 = not needed; NULL ws falls back to the unsplit kernel). */
int64_t koaf_linear_ws(int32_t M, int32_t N, int32_t K);
int koaf_linear_fwd(const float* x, const float* w, const float* b, const float* residual,
                    float* y, float* ws, int32_t M, int32_t N, int32_t K, void* stream);
/* dx[M,K] = dy[M,N] w[N,K]  (w read K-major, no re-pack) (+residual); ws: koaf_linear_ws(M, K, N) floats */
int koaf_linear_dgrad(const float* dy, const float* w, const float* residual, float* dx, float* ws,
                      int32_t M, int32_t N, int32_t K, void* stream);
/* dw[N,K] = dy^T x ; db[N] = column sums of dy (db nullable; ws: koaf_colsum_ws(M,N) floats) */
int koaf_linear_wgrad(const float* dy, const float* x, float* dw, float* db, float* ws, int32_t M,
                      int32_t N, int32_t K, void* stream);
/* nn.LayerNorm(D) rows: y, save mean/rstd (_core_trf.py:190-192,198,202) */
int koaf_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                       float* mean, float* rstd, int32_t rows, int32_t D, float eps, void* stream);
/* dx; dgamma/dbeta written (part: workspace of koaf_layernorm_bwd_ws floats) */
int64_t koaf_layernorm_bwd_ws(int32_t rows, int32_t D);
int koaf_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                       const float* rstd, float* dx, float* dgamma, float* dbeta, float* part,
                       int32_t rows, int32_t D, void* stream);
/* Attention core (_core_trf.py:170-180): qkv [B,n,3*h*d] with '(qkv h d)' split; scale applied to
 * QK^T; attn [B,h,n,n] emitted (it is returned by the reference, :182); out [B,n,h*d].  One launch
 * for n <= 512 and d % 4 == 0 (scores kept in LDS); larger n: two batched GEMMs + koaf_softmax_rows. */
int koaf_attention_fwd(const float* qkv, float* attn, float* out, int32_t B, int32_t n, int32_t h,
                       int32_t d, float scale, void* stream);
/* dqkv (every element written) from dout; ws: workspace of B*h*n*n floats (dS).  */
int koaf_attention_bwd(const float* dout, const float* qkv, const float* attn, float* dqkv,
                       float* ws, int32_t B, int32_t n, int32_t h, int32_t d, float scale,
                       void* stream);
int koaf_softmax_rows(float* x, int64_t rows, int32_t n, void* stream);
int koaf_softmax_bwd_rows(float* dp, const float* p, int64_t rows, int32_t n, float scale,
                          void* stream);
/* exact (erf) GELU, nn.GELU default (_core_trf.py:146) */
int koaf_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int koaf_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int koaf_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int koaf_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* inverted dropout with a counter-based generator: y = x * keep(seed, i) / (1-p).  The same call
 * with x := dy is the backward.  (nn.Dropout / nn.Dropout2d on (N,C,1,1); streams differ from
 * torch's by construction -- SURVEY a10.)  */
/* epoch (nullable, both dropouts): device-resident step counter folded into the seed -- a captured (HIP-graph) step replays with
 * frozen arguments, the counter (koaf_counter_add) is what changes from step to step */
int koaf_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, const int64_t* epoch, void* stream);
int koaf_counter_add(int64_t* counter, int64_t delta, void* stream);   /* *counter += delta on the device */
/* nn.Dropout2d on an NHWC map x [N][HW][C] (_xrNmrMcP.py:62-72 with with_gap false): one draw per (image, channel),
 * generator index n*C + c -- identical to koaf_dropout on the pooled [N][C] output.  Backward = same call on dy. */
int koaf_dropout2d(const float* x, float* y, int32_t N, int32_t HW, int32_t C, float p, uint64_t seed,
                   const int64_t* epoch, void* stream);
/* out = a + b */
int koaf_add(const float* a, const float* b, float* out, int64_t n, void* stream);
/* p[0..n) = value */
int koaf_fill(float* p, float value, int64_t n, void* stream);
/* column sums of x [rows][C] -> out [C] (bias gradients); part: koaf_colsum_ws floats or NULL */
int64_t koaf_colsum_ws(int32_t rows, int32_t C);
int koaf_colsum(const float* x, float* out, int32_t rows, int32_t C, float* part, void* stream);

/* ---- FocalLoss (_losses.py:89-108): loss = mean|sum( -(1-pt)^gamma * logpt ), logpt = -F.cross_entropy(x, t, weight, 'none') ----
 * logits [B,C,S] -- S = product of the spatial dims of a (b, ch, d0, d1, ...) input, 1 for (b, ch) --, target int64 [B,S],
 * class_weight [C] or NULL; writes the scalar loss and dlogits (= d loss / d logits, same layout).
 * ws: koaf_loss_ws(B, S) floats or NULL.  Up to 8192 elements (the models' (b, 2) logits) one block does everything; beyond that,
 * with a workspace, the same arithmetic runs on a grid of 4096-element blocks whose partial sums are added by one block in index
 * order (two fixed-order stages: the result does not depend on scheduling; without a workspace the one block walks everything). */
int64_t koaf_loss_ws(int32_t B, int64_t S);
int koaf_focal_loss(const float* logits, const int64_t* target, const float* class_weight, float* loss, float* dlogits,
                    int32_t B, int32_t C, int64_t S, float gamma, int32_t reduction_mean, float* ws, void* stream);
/* softmax-CE (CrossEntropyLoss wrapper = nn.CrossEntropyLoss(weight=class_weight), _losses.py:13-49): weighted mean
 * sum_i w[t_i] * (-log p_i[t_i]) / sum_i w[t_i] */
int koaf_ce_loss(const float* logits, const int64_t* target, const float* class_weight, float* loss, float* dlogits,
                 int32_t B, int32_t C, int64_t S, float* ws, void* stream);

/* ---- torch.optim.Adam (coupled L2) over a flat arena (_optimizers.py:47-52) ------------------ */
/* vmax (nullable): amsgrad -- the running maximum of the second moment, updated in place and used in the denominator */
int koaf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int32_t step, int32_t adamw,
                   const float* hyper, float* vmax, void* stream);
/* Device-resident optimizer step state for captured (HIP-graph) train steps: ++*step; hyper[3] = {lr, lr / (1 - beta1^step),
 * sqrt(1 - beta2^step)} from the device scalars; hand `hyper` to koaf_adam_step (its host lr / step are then ignored). */
int koaf_adam_hyper(int32_t* step, const float* lr, double beta1, double beta2, float* hyper, void* stream);

/* ---- torch.optim.SGD over a flat arena (_optimizers.py:47-52, the "SGD" key) -------------------
 * g' = (maximize ? -g : g) + weight_decay * p;  with a momentum: buf = first ? g' : momentum * buf + (1 - dampening) * g' and
 * the step is g' + momentum * buf (nesterov) or buf;  without: the step is g';  p -= lr * step.  buf: the momentum buffer
 * (NULL exactly when momentum == 0); `first`: this is the first update of these elements (buf is written, not read).
 * hyper (nullable): device float[2] from koaf_optim_hyper -- lr and first then come from the device, the host values are
 * ignored.  One pass: p, g (and buf) read once, p (and buf) written once. */
int koaf_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, double momentum, double dampening,
                  float weight_decay, int32_t nesterov, int32_t maximize, int32_t first, const float* hyper, void* stream);
/* ---- torch.optim.RMSprop over a flat arena (_optimizers.py:47-52, the "RMSprop" key) -----------
 * g' as above;  sq = alpha * sq + (1 - alpha) * g'^2;  centered (gavg non-NULL): gavg += (1 - alpha) * (g' - gavg) and
 * avg = sqrt(sq - gavg^2) + eps, else avg = sqrt(sq) + eps;  with a momentum (buf non-NULL exactly when momentum > 0):
 * buf = momentum * buf + g' / avg, p -= lr * buf;  without: p -= lr * g' / avg.  hyper (nullable): as for koaf_sgd_step
 * (only lr is used). */
int koaf_rmsprop_step(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, float lr, double alpha, float eps,
                      float weight_decay, double momentum, int32_t maximize, const float* hyper, void* stream);
/* Device-resident step state of both, for captured (HIP-graph) train steps -- the counterpart of koaf_adam_hyper: ++*step;
 * hyper[2] = {*lr, *step == 1 ? 1 : 0}. */
int koaf_optim_hyper(int32_t* step, const float* lr, float* hyper, void* stream);

/* ---- gradient accumulation over micro-batches and global-norm clipping (torch.nn.utils.clip_grad_norm_) over flat fp32
 * ranges of the arena: 16-byte aligned, any n.  Every block owns one fixed chunk of the range and every reduction is
 * fixed-order and two-stage (no atomics): the same bits from run to run.  Nothing reads a value back to the host.
 * norm_kind: 0 = 2-norm (each square and the sums in fp64: |g| ~ 1e25 does not overflow), 1 = inf-norm (integer maximum over
 * the magnitude bits: a NaN anywhere reaches the result).
 * koaf_grad_fold  mode 0: acc = w * g;  1: acc = acc + w * g;  2: g = acc + w * g (acc unchanged).  The product is rounded to
 *   fp32, then the sum (no fused multiply-add).  ws (nullable, mode 2 only): koaf_grad_norm_ws(n) floats, receives the block
 *   partials of the norm of the values written to g, as koaf_grad_norm_part would give them.
 * koaf_grad_norm_part  the block partials of g's norm -> ws (koaf_grad_norm_ws(n) floats, 8-byte aligned).
 * koaf_grad_norm_final  ws: the partials of one or several ranges laid end to end, nws floats in all, combined in index order
 *   -> norm[0];  coef[0] (nullable) = min(1, max_norm / (norm + 1e-6f)) in fp32 as written: a NaN norm gives NaN, +Inf gives 0.
 * koaf_grad_scale  g *= coef[0] (a device scalar); a block leaves without touching memory when coef[0] == 1. */
int64_t koaf_grad_norm_ws(int64_t n);
int koaf_grad_fold(float* acc, float* g, int64_t n, float w, int32_t mode, int32_t norm_kind, float* ws, void* stream);
int koaf_grad_norm_part(const float* g, int64_t n, int32_t norm_kind, float* ws, void* stream);
int koaf_grad_norm_final(const float* ws, int64_t nws, int32_t norm_kind, float max_norm, float* norm, float* coef, void* stream);
int koaf_grad_scale(float* g, int64_t n, const float* coef, void* stream);

/* ---- nn.BCELoss / nn.BCEWithLogitsLoss (_losses.py:111-117, the "bce_loss" / "bce_wlogits_loss" keys) ----
 * x, target [n] (any equal shape, flattened), weight [n] (already expanded to x's shape) or NULL, pos_weight [C] or NULL (logits
 * form only; C = the last dimension, n % C == 0).  Loss and gradient in one launch:
 *   from_logits 0:  l = -w * (t * max(log x, -100) + (1 - t) * max(log(1 - x), -100)),  dl/dx = w * (x - t) / max((1 - x) * x, 1e-12)
 *                   (torch's clamps).  A probability outside [0, 1], where torch raises a device assert, gets zero loss and
 *                   zero gradient and is counted in status word [1].
 *   from_logits 1:  l = w * ((1 - t) * x + (1 + (pw - 1) * t) * (log1p(exp(-|x|)) + max(-x, 0)))
 * reduction 0: loss [n] per element; 1: mean, 2: sum (loss a scalar).  dx [n] = d loss / d x for an upstream gradient of 1 (it
 * carries the mean's 1 / n).  ws: koaf_bce_ws(n) floats or NULL.  Up to 8192 elements one block does everything; beyond that,
 * with a workspace, a grid of 4096-element blocks whose partial sums one block adds in index order (two fixed-order stages:
 * the result does not depend on scheduling; without a workspace the one block walks everything). */
int64_t koaf_bce_ws(int64_t n);
int koaf_bce_loss(const float* x, const float* target, const float* weight, const float* pos_weight, float* loss, float* dx,
                  int64_t n, int32_t C, int32_t from_logits, int32_t reduction, float* ws, void* stream);

/* ---- calc_metrics_v2 / calc_bootstrap on the device (koaf_metrics.hip; various/_metrics_stat_anlys.py:28-216,
 * _metrics_wissam.py:113-172): ROC-AUC, average precision, prevalence-calibrated average precision, the Youden cutoff and the
 * confusion counts of n <= KOAF_METRICS_MAX_N binary-labelled scores, for the sample itself and for R bootstrap resamples.
 * The scores are ranked once; a resample changes only how often a sample counts, so it is a histogram over the rank bins.
 * Arithmetic contract: ranks, histograms, prefix sums and the Mann-Whitney sum are INTEGER (LDS integer atomics: exact and
 * order-independent); every fp64 value is a quotient of such integers or a sum of such quotients taken in a fixed order (per
 * thread in bin order over a contiguous run of bins, then a fixed tree over the 256 threads), without fused multiply-add.  No
 * floating-point atomics: the same bits from run to run, on any grid.
 * flag: a device uint32 the caller zeroed; bit 0 = a NaN / Inf score, bit 1 = a label other than 0 / 1, bit 2 = an index of the
 * index matrix (or a rank of `packed`) outside [0, n), which is skipped, never followed.
 *
 * koaf_score_ranks  rank[i] = #{ j : s[j] > s[i] } over s[i] = scores[i * stride] (fp32, or fp64 when f64): tied scores get equal
 *   ranks, rank 0 is the largest score, and the ranks in use are sklearn's distinct thresholds in descending order.  The
 *   comparison is made in the scores' own precision (fp64 scores are NOT narrowed: that would merge near-ties).  All-pairs
 *   counting, the scores tiled through LDS; a sample's count does not depend on the grid.  labels (int32 [n], nullable) and
 *   packed go together: packed[i] = rank[i] << 1 | (labels[i] == pos_label), the word the two kernels below gather.  rank is
 *   nullable when packed is given.
 * koaf_curve_metrics  one block per row of out [rows][8] fp64, rows = R + (with_identity ? 1 : 0).  Row r counts the samples
 *   idx[r'][0..m) (int32, r' = r - with_identity), the identity row (row 0 when with_identity; idx may be NULL when R == 0)
 *   counts every sample once.  With (tp_g, fp_g) the positives / negatives of rank bin g, tp / fp their running sums including
 *   g, P / N the totals:
 *     out[r] = { P, N,  sum_g fp_g * (2 * tp_before_g + tp_g) / (2 P N),  sum_g (tp_g / P) * (tp / (tp + fp)),
 *                sum_g (tp_g / P) * (tp / (tp + ratio * fp)),  0, 0, 0 }
 *   ratio = pi * (1 - pi0) / (pi0 * (1 - pi)), pi = P / (P + N) of the row itself; a term whose denominator is 0 counts 0
 *   (_metrics_wissam.py:150-157).  That is roc_auc_score (the Mann-Whitney form of its trapezoid sum), average_precision_score
 *   and average_precision_score_calib(pi0) with the positive class `pos_label` of koaf_score_ranks; P == 0 or N == 0 writes NaN
 *   for the three metrics and the counts.  m <= KOAF_METRICS_MAX_N: a bin's two 16-bit counters cannot carry.
 * koaf_point_metrics  one block, the identity resample.  out [9] fp64:
 *   out[0] the Youden cutoff of sensitivity_specificity_cutoff (:224-254): the threshold of the FIRST maximum of tp / P - fp / N
 *     over the points roc_curve(drop_intermediate=True) keeps -- the first threshold, the last, and every threshold whose
 *     (tp_g, fp_g) differs from the next threshold's (a non-zero second difference of tps or of fps) -- behind the leading
 *     (0, 0, +inf) point.  A score value widened to fp64 (exact), or +inf.
 *   out[1..5) = tn, fp, fn, tp of the prediction s > thr (compared in fp64), out[5..9) = the same of s >= cutoff (in the scores'
 *     precision; nothing is predicted positive at +inf).  "Positive" is packed's label bit. */
#define KOAF_METRICS_MAX_N 16384
int koaf_score_ranks(const void* scores, int32_t f64, int64_t stride, int32_t n, const int32_t* labels, int32_t pos_label,
                     int32_t* rank, int32_t* packed, uint32_t* flag, void* stream);
int koaf_curve_metrics(const int32_t* packed, int32_t n, const int32_t* idx, int32_t R, int32_t m, int32_t with_identity,
                       double pi0, double* out, uint32_t* flag, void* stream);
int koaf_point_metrics(const void* scores, int32_t f64, int64_t stride, const int32_t* packed, int32_t n, double thr, double* out,
                       uint32_t* flag, void* stream);

/* ---- paired permutation test of two models' ROC-AUC / average precision on the same samples (koaf_metrics.hip; the
 * "Permutation testing" cell of run/Analysis_Visualization.ipynb: scipy.stats.permutation_test(permutation_type="samples") around
 * metric(cmp) - metric(ref)).  A permutation swaps the two predictions of some samples.  That does not change the order of the
 * union of the 2n scores, so the union is ranked once and each permutation is, per side, a histogram over the 2n rank bins; the
 * labels do not move, so both sides of every row share P and N.  n <= KOAF_METRICS_MAX_N / 2 = 8192: the 2n bins are the
 * histogram of the kernels above.  The arithmetic contract above holds unchanged: integer ranks, histograms, prefix sums and
 * Mann-Whitney sums, fp64 sums in the fixed per-thread-run-then-tree order without fused multiply-add, no floating-point atomics,
 * the same bits from run to run.  flag as above (bit 2: a rank of `packed` outside [0, 2n), which is skipped).
 *
 * koaf_pair_ranks  ranks the union s[j] = a[j * stride_a] (j < n), s[n + j] = b[j * stride_b], both columns fp32, or both fp64
 *   when f64, compared in their own precision: rank[j] = #{ k < 2n : s[k] > s[j] }, so equal scores of the two models share a
 *   bin.  packed[j] = rank[j] << 1 | (labels[j mod n] == pos_label) for j in [0, 2n); labels (int32 [n]) and packed go together,
 *   rank is nullable when packed is given.
 * koaf_perm_metrics  two blocks (one per side) per row of out [rows][8] fp64, rows = R + (with_identity ? 1 : 0).  masks is
 *   uint32 [R][W], W = ceil(n / 32): row r' = r - with_identity swaps sample i when bit (i & 31) of word (i >> 5) is set; bits at
 *   or beyond n are ignored; the identity row (row 0 when with_identity; masks may be NULL when R == 0) swaps nothing.  Side A
 *   ("ref") counts packed[i] of an unswapped and packed[n + i] of a swapped sample, side B ("cmp") the other word.  With
 *   (tp_g, fp_g) the positives / negatives of union bin g on a side:
 *     out[r] = { P, N,  U_A, U_B,  ap_A, ap_B,  0, 0 },   U = sum_g fp_g * (2 * tp_before_g + tp_g)  (= 2 P N roc_auc, an integer
 *     below 2^27, exact in fp64),   ap = sum_g (tp_g / P) * (tp / (tp + fp))
 *   P == 0 or N == 0 writes the counts, and NaN for the four values U_A, U_B, ap_A, ap_B. */
int koaf_pair_ranks(const void* a, int64_t stride_a, const void* b, int64_t stride_b, int32_t f64, int32_t n, const int32_t* labels,
                    int32_t pos_label, int32_t* rank, int32_t* packed, uint32_t* flag, void* stream);
int koaf_perm_metrics(const int32_t* packed, int32_t n, const uint32_t* masks, int32_t R, int32_t with_identity, double* out,
                      uint32_t* flag, void* stream);

/* ---- the ROC / PR curves themselves, recall-range average precision, best calibrated F1 and confusion counts
 * (koaf_metrics.hip; calc_metrics_v2(with_curves=True) of _metrics_stat_anlys.py:190-202, avg_precision_at_recall_range :11-25,
 * mc_bacc :219-221, precision_recall_curve_calib / f1score_calib / bestf1score_calib of _metrics_wissam.py:113-231).  The same
 * pieces as above -- `packed` of koaf_score_ranks, the histogram over the rank bins, the ordered walk -- with the walk's points
 * written out, or folded into other scalars.  The arithmetic contract above holds unchanged: integer ranks, histograms and prefix
 * sums; every fp64 value a quotient of such integers, one IEEE operation chain on them, or a sum of such chains in the fixed
 * per-thread-run-then-tree order; no fused multiply-add, no floating-point atomics, the same bits from run to run.  n <=
 * KOAF_METRICS_MAX_N; flag as above.
 *
 * koaf_curve_points  one block, the identity sample.  out is fp64 [koaf_curve_points_len(n)] = 8 + 8 * (n + 1): a length known
 *   from n alone, so the points ride in the caller's one device-to-host copy.  With the T non-empty rank bins (sklearn's distinct
 *   thresholds) in descending score order, tp / fp the running counts including the bin, P / N the totals:
 *     out[0..8) = { P, N, T, K, last_ind, 0, 0, 0 }: K the number of thresholds roc_curve(drop_intermediate=True) keeps (the
 *       first, the last, and every one whose (tp_g, fp_g) differs from the next threshold's), last_ind the index of the first
 *       threshold with tp == P (tps.searchsorted(tps[-1]), where precision_recall_curve_calib truncates).
 *     then eight arrays of n + 1 slots each:
 *       0 thr       [j] = the score of threshold j, widened exactly                                            j in [0, T)
 *       1 rec       [0] = 0,  [1 + j] = tp / P
 *       2 prec      [0] = 1,  [1 + j] = tp / (tp + fp)
 *       3 prec_cal  [0] = 1,  [1 + j] = tp / (tp + ratio * fp), 0 where that is NaN;  ratio = pi * (1 - pi0) / (pi0 * (1 - pi))
 *                   in that order, pi = P / (P + N) -- or N / (P + N) when pi_of_negatives: the reference takes np.sum(y_true) / n,
 *                   the share of LABEL 1, whichever class is called positive
 *       4 fpr  5 tpr  6 roc thr   [0] = (0, 0, +inf),  [1 + k] = (fp / N, tp / P, score) of the k-th kept threshold   k in [0, K)
 *       7 scratch (the score of each rank bin)
 *     Slot 0 of arrays 1-3 is the closing point of the PR curves, so sklearn's precision_recall_curve is the reversed slice
 *     [T .. 0] and the reference's calibrated curve the reversed slice [last_ind + 1 .. 0]: the host only slices and reverses.
 *     Positions are counted (per-thread counts, an exclusive prefix over the 256 threads), never decided by an atomic.  Every
 *     value is what numpy computes from the same integers, to the last bit.  Slots beyond T / K are not written.
 * koaf_range_metrics  one block per row of out [rows][8] fp64; rows, idx, m and with_identity as for koaf_curve_metrics.  Along
 *   the row's PR curve in ascending recall -- the leading (rec 0, prec 1) point, then the thresholds; bins empty in the resample
 *   are no thresholds --
 *     out[r] = { P, N, ap_range, best_f1_calib, rec_at_low, rec_at_high, 0, 0 }
 *   rec_at_low = the largest rec <= lo, rec_at_high = the smallest rec >= hi (0 <= lo <= hi <= 1), ap_range = the sum of
 *   (rec - rec_prev) * (prec + prec_prev) / 2.0 over the segments prev -> cur with rec > lo and rec_prev < hi (recall does not
 *   decrease, so these are the segments between those two points; the comparisons are made on the quotients tp / P themselves),
 *   divided by (rec_at_high - rec_at_low): scipy's trapezoid over sklearn's curve; 0 / 0 is NaN as on the host.
 *   best_f1_calib = the maximum of (2 * p * r) / (p + r), NaN / Inf counting 0, over the points (p = prec_cal, r = rec) of the
 *   calibrated curve up to the first threshold of full recall and its closing point (worth 0); pi = P / (P + N) of the row;
 *   pi0 == 0 means pi0=None: no calibration, p = prec.  P == 0 or N == 0 writes the counts and NaN.
 * koaf_confusion  counts[t * K + p] += 1 (int64 [K][K], zeroed by the caller) for each of the n < 2^31 samples with
 *   t = y_true[i], p = y_pred[i] (int32 class indices), K <= 32: per-block LDS integer atomics, then global integer atomics.  A
 *   label outside [0, K) raises flag bit 1 and the sample is skipped. */
int64_t koaf_curve_points_len(int32_t n);
int koaf_curve_points(const void* scores, int32_t f64, int64_t stride, const int32_t* packed, int32_t n, double pi0,
                      int32_t pi_of_negatives, double* out, uint32_t* flag, void* stream);
int koaf_range_metrics(const int32_t* packed, int32_t n, const int32_t* idx, int32_t R, int32_t m, int32_t with_identity, double pi0,
                       double lo, double hi, double* out, uint32_t* flag, void* stream);
int koaf_confusion(const int32_t* y_true, const int32_t* y_pred, int64_t n, int32_t K, int64_t* counts, uint32_t* flag,
                   void* stream);

/* ---- calibration of the predicted probabilities (koaf_calib.hip; scikit-learn's brier_score_loss, log_loss and
 * calibration_curve, numpy's percentile, and the usual companions of a clinical prediction model: ECE / MCE, calibration
 * intercept and slope, temperature scaling, net benefit): for the sample itself and for R bootstrap resamples, one block of 256
 * threads per row; rows, idx, m and with_identity as for koaf_curve_metrics (m <= KOAF_METRICS_MAX_N).  scores are fp32, or fp64
 * when f64, read in place as scores[i * stride] and widened to fp64 (exact); labels is int32 [n] of 0 / 1.
 * Arithmetic contract: everything is fp64; counts are INTEGER (LDS integer atomics, per-thread counters); every fp64 sum has one
 * owner and a fixed order -- thread t adds the draws [t L, (t + 1) L) of its row, L = ceil(draws / 256), in row order, then a
 * fixed tree runs over the 256 threads -- without fused multiply-add.  No floating-point atomics: the same bits from run to run.
 * Every loop bound is a constant or an argument.  `draws` below is the row's length: n for the identity row, m otherwise.
 * flag: bits 0-2 as for koaf_score_ranks / koaf_curve_metrics (a NaN / Inf score; a label other than 0 / 1, which counts as 0;
 * an index outside [0, n), which is skipped and never followed); bit 3: a row of koaf_recalib_fit ended with a status other than 0.
 *
 * koaf_calib_edges  one block.  edges[k] = np.percentile(scores, 100 q[k]) (default linear method) for the nbins + 1 fractions q
 *   (device fp64, in [0, 1]; the quantile strategy of calibration_curve passes np.linspace(0, 1, nbins + 1)): virtual index
 *   h = q * (n - 1), lo = floor(h), the order statistics a = x_(lo), b = x_(min(lo + 1, n - 1)) found by all-pairs counting (no
 *   sort: element i is x_(k) for every k with #{s < s_i} <= k < #{s <= s_i}), t = h - lo, and numpy's two-sided lerp
 *   a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5; h >= n - 1 gives the largest score.  Bit-equal to numpy
 *   on fp64 scores; fp32 scores are widened first (numpy would interpolate in fp32).
 * koaf_calib_metrics  edges is device fp64 [nbins + 1] (only the inner edges are read), thr device fp64 [T] (nullable with
 *   T = 0; each in (0, 1), any order), 1 <= nbins <= KOAF_CALIB_MAX_BINS, 0 <= T <= KOAF_CALIB_MAX_THR.  The bin of p is
 *   #{ k in 1 .. nbins - 1 : edges[k] < p } compared in fp64 -- np.searchsorted(edges[1:-1], p, side="left"): a score on an edge
 *   goes to the lower bin.  With y the label, n_b / S_y,b / S_p,b the count, the positives and the score sum of bin b:
 *     out[r] = { P, N,  sum (p - y)^2 / draws,  sum -log(clip(p_y, eps, 1 - eps)) / draws,  sum p / draws,
 *                (sum_b |S_y,b - S_p,b|) / draws  (b ascending),  max over non-empty b of |S_y,b - S_p,b| / n_b,  bins in use }
 *   p_y = p for y = 1 and 1 - p otherwise.  A one-class row keeps every value (they are defined there); only P or N is 0.
 *   bins [rows][nbins][3] (nullable) = (n_b, S_y,b, S_p,b), the two counts held as fp64.
 *   nb [rows][T][4] (nullable) = (tp, fp, tp / draws - (fp / draws) * (t / (1 - t)), P / draws - (N / draws) * (t / (1 - t))) of
 *   the prediction p >= t: the net benefit of the model and, from the same expression at tp = P, fp = N, of treating everyone.
 * koaf_recalib_fit  unpenalised logistic regression of y on eta = a + b x, one block per row.  kind 0: x = log(q) - log1p(-q),
 *   q = clip(p, eps, 1 - eps), the scores being probabilities; kind 1: x = the score, minus scores0[i * stride0] when scores0 (same
 *   dtype; the logit difference of a (B, 2) logits tensor read in place) is given.  mode 0: a and b free (calibration intercept and
 *   slope); mode 1: b only, a = 0 (temperature scaling of two classes, T = 1 / b); mode 2: a only, b = 1 (calibration in the
 *   large).  From (0, 1), Newton steps on L = sum softplus(eta) - y eta with the Hessian from sigma (1 - sigma), solved in closed
 *   form; the step is halved, at most 30 times, until L does not increase (beyond 2^-45 |L|, the rounding of the sum itself: near
 *   the optimum a Newton step changes L by less); it stops when max|g_free| / draws <= tol (status 0),
 *   after max_iter <= KOAF_RECALIB_MAX_ITER steps or when no halved step keeps L from increasing (status 1), when the Hessian is
 *   not positive, a value leaves the finite range or -- modes 0 and 1 -- the current line puts every draw strictly on its class's
 *   side (complete separation: L has no finite minimum) (status 2), or at once when the row holds one class (status 3).
 *     report[r] = { a, b, steps taken, max|g_free| / draws, L / draws, status, P, N };  a and b are NaN for status >= 2.
 * koaf_recalib_apply  out[i] = sigma(a + b x_i) (fp64 [n], n < 2^31), x as in the fit; element-wise. */
#define KOAF_CALIB_MAX_BINS 64
#define KOAF_CALIB_MAX_THR 128
#define KOAF_RECALIB_MAX_ITER 200
int koaf_calib_edges(const void* scores, int32_t f64, int64_t stride, int32_t n, const double* q, int32_t nbins, double* edges,
                     uint32_t* flag, void* stream);
int koaf_calib_metrics(const void* scores, int32_t f64, int64_t stride, const int32_t* labels, int32_t n, const double* edges,
                       int32_t nbins, const double* thr, int32_t T, const int32_t* idx, int32_t R, int32_t m, int32_t with_identity,
                       double eps, double* out, double* bins, double* nb, uint32_t* flag, void* stream);
int koaf_recalib_fit(const void* scores, int32_t f64, int64_t stride, const void* scores0, int64_t stride0, const int32_t* labels,
                     int32_t n, int32_t kind, int32_t mode, const int32_t* idx, int32_t R, int32_t m, int32_t with_identity,
                     double eps, double tol, int32_t max_iter, double* report, uint32_t* flag, void* stream);
int koaf_recalib_apply(const void* scores, int32_t f64, int64_t stride, const void* scores0, int64_t stride0, int64_t n, int32_t kind,
                       double a, double b, double eps, double* out, uint32_t* flag, void* stream);

/* ---- the clinical logistic-regression baseline (koaf_clin.hip; run/train_prog_clin.py with scikit-learn's StandardScaler,
 * OneHotEncoder and LogisticRegression(lbfgs, L2, fit_intercept) behind it).  Everything is fp64.  Every sum has one owner and a
 * fixed order and there are no floating-point atomics: the same bits from run to run.  *flag is a device word the caller zeroed;
 * bit 0: a NaN / Inf in the table, in a weight, or a fit that left the finite range; bit 1: a category that is not in the list;
 * bit 2: a problem whose weighted rows hold one class; bit 3: a label other than 0 / 1 under a non-zero weight, a negative
 * weight, or a fitting-row index outside [0, n).
 *
 * koaf_clin_design  raw [V][n] holds one column per variable; ncat (HOST, [V]) is 0 for a continuous variable and the number of
 *   categories otherwise; cats (HOST) holds the strictly increasing categories of the categorical variables one after another
 *   (np.unique of the fitting rows).  fit = 1: stats[v] = (mean, population standard deviation) of every continuous variable over
 *   the rows fit_idx[0 .. nfit) (device int32; NULL: all rows, nfit = n) is computed first (two passes, ddof = 0) and left in
 *   stats [V][2]; fit = 0: stats is read.  X [n][D] row-major: (x - mean) / std for a continuous variable (std 0 divides by 1),
 *   one 0 / 1 column per category in list order otherwise, the variables in the caller's order; D + 1 <= KOAF_LOGREG_MAX_P.
 * koaf_logreg_fit  K problems over the same X [n][D] and y [n] (int32 0 / 1), problem k with the weights sw[k][0 .. n): a weight
 *   of 0 takes the row out of the problem (its X values enter no sum, whatever they are), so fold masks and class weights are one mechanism.
 *   Minimises  f(w) = (1/S) sum_i s_i [log(1 + e^{r_i}) - y_i r_i] + |w[:D]|^2 / (2 C S),  r_i = x_i . w[:D] + w[D],  S = sum_i s_i,
 *   by Newton steps (Cholesky of the exact Hessian) damped by Armijo backtracking t = 1, 1/2, ...:  f(w + t d) <= f(w) +
 *   1e-4 t g.d + 4 eps |f(w)|.  It stops at |g|_inf <= tol, when no t >= 2^-30 passes, or after max_iter steps.  One block per
 *   problem, all K in one launch.  W [K][D + 1], the intercept last; report [K][4] = (steps taken, final |g|_inf, final f, step
 *   halvings).  A problem whose weights or labels raise a bit (0, 2 or 3) leaves NaN in its rows of W and report.  2 <= n, D + 1 <= KOAF_LOGREG_MAX_P.
 * koaf_logreg_predict  decision [K][m] = Xt [m][D] . W[k][:D] + W[k][D], proba [K][m][2] = (1 - p, p) with p = 1 / (1 + e^-decision).
 *   logloss != NULL: logloss[k] = -mean over the rows with mask[k][i] != 0 (int32 [K][m]) of log(clip(p of class y[i], eps,
 *   1 - eps)), sklearn.metrics.log_loss; NaN without such a row.  ensemble = 1: ens_proba [m][2] = the mean over the K problems
 *   (added in problem order, then divided) and ens_pred [m] its argmax, the first index winning a tie. */
#define KOAF_LOGREG_MAX_P 32
int koaf_clin_design(const double* raw, int64_t n, int32_t V, const int32_t* ncat, const double* cats, const int32_t* fit_idx,
                     int64_t nfit, int32_t fit, double* stats, double* X, uint32_t* flag, void* stream);
int koaf_logreg_fit(const double* X, const int32_t* y, const double* sw, int64_t n, int32_t D, int32_t K, double C, int32_t max_iter,
                    double tol, double* W, double* report, uint32_t* flag, void* stream);
int koaf_logreg_predict(const double* W, const double* Xt, int64_t m, int32_t D, int32_t K, const int32_t* y, const int32_t* mask,
                        int32_t ensemble, double* decision, double* proba, double* logloss, double* ens_proba, int32_t* ens_pred,
                        void* stream);

/* ---- from raw MRI series to the model's input volumes (koaf_mriprep.hip; run/prepare_data_mri_oai.py:185-189, :226, :234-279 and
 * datasets/_mr_t2_mapping.py).  dtype: koaf_widen's codes and on: 2 = uint16, 3 = int16, 4 = float32, 5 = float64; every pointer
 * is aligned to its element size, nothing more (a view into a larger buffer is read in place).  All fp64 arithmetic below is
 * compiled without fused multiply-add and without reassociation; no floating-point atomics: the same bits from run to run.
 *
 * koaf_t2_fit  fit_t2_map: per voxel of vol [S][R][C][E] (echo fastest), with x = tes[s][e] (fp64 [S][E]) and y the intensity
 *   widened to fp64 (int16 keeps its sign), the IEEE-754 evaluation of the reference's source text: the five sums S_x2_y += x*x*y,
 *   S_y_lny += y*log(y), S_x_y += x*y, S_x_y_lny += x*y*log(y), S_y += y in echo order from 0.0; denom = S_y*S_x2_y - S_x_y*S_x_y;
 *   a = (S_x2_y*S_y_lny - S_x_y*S_x_y_lny) / denom; b = (S_y*S_x_y_lny - S_x_y*S_y_lny) / denom; t = -1 / b.  In this order:
 *   denom == 0, a NaN or b NaN -> 0;  t NaN -> nan_to;  t < val_low or t > val_high -> 0;  else t.  (A zero or negative intensity
 *   makes y*log(y) NaN, so background becomes 0.  Only log differs from the host's, by its last bit.)  decimals >= 0: the value
 *   stored is rint(v * 10^decimals) / 10^decimals, numpy's np.round, bit for bit; decimals < 0: v itself.  margin >= 0 voxels
 *   are dropped at both ends of R and of C (2 * margin < R, C).  layout 0: out [S][R-2m][C-2m]; layout 1: out [R-2m][C-2m][S], the
 *   reference's moveaxis(t2, [0,1,2], [2,0,1]).  2 <= E <= 16: with one echo denom is y*((x*x)*y) - (x*y)*(x*y), zero or one
 *   ulp depending on rounding, and the reference's own answer is noise.  Series of several patients concatenate along S.
 * koaf_series_hist  bins[u >> shift] += 1 over the n < 2^31 elements of x, u the uint16 that astype(np.uint16) makes of the
 *   element (uint16 as is, int16 reinterpreted, floats truncated toward zero); bins is int32 [65536 >> shift], zeroed by the caller,
 *   2 <= shift <= 8.  A float that is not finite raises bit 0 of *flag (a device word the caller zeroed), one outside [0, 65535]
 *   bit 1; neither is counted.  Per-block counts in LDS, integer atomics only.
 * koaf_series_quantiles  one block: out[j] = lerp(x_(k[j]), x_(min(k[j] + 1, n - 1)), gamma[j]) over the order statistics of the
 *   counted values, numpy's _lerp: a + (b - a) * gamma, and b - (b - a) * (1 - gamma) where gamma >= 0.5.  k / gamma are HOST
 *   arrays of K <= 8 pairs (they travel as kernel arguments), out fp64 [K] on the device; np.percentile(q) is k = floor(v),
 *   gamma = v - k of v = (n - 1) * (q / 100) in fp64.  An index beyond the counted elements gives the largest counted value.
 * koaf_series_pack  out[r - m][c - m][s] = narrow(min(max(u >> shift, limits[0]), limits[1])) of x [R][C][S]; limits is a DEVICE
 *   fp64 pair (the two values koaf_series_quantiles left: no host round trip); the clip is np.clip's in fp64, narrow truncates
 *   toward zero to uint8 (out16 = 0) or uint16 (out16 = 1).  margin m >= 1 (numpy's [0:-0] is empty), 2 m < R, C. */
int koaf_t2_fit(const void* vol, int32_t dtype, const double* tes, int32_t S, int32_t R, int32_t C, int32_t E, double nan_to,
                double val_low, double val_high, int32_t decimals, int32_t margin, int32_t layout, double* out, void* stream);
int koaf_series_hist(const void* x, int32_t dtype, int64_t n, int32_t shift, int32_t* bins, uint32_t* flag, void* stream);
int koaf_series_quantiles(const int32_t* bins, int32_t shift, int64_t n, const int64_t* k, const double* gamma, int32_t K,
                          double* out, void* stream);
int koaf_series_pack(const void* x, int32_t dtype, int32_t R, int32_t C, int32_t S, int32_t shift, int32_t margin,
                     const double* limits, void* out, int32_t out16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KOAF_H */
