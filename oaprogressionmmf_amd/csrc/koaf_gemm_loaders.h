// koaf_gemm_loaders.h -- the operand access modes of koaf_gemm_kernel and its five operand loaders: TileLoader (fp32 source,
// block-wide, through registers), StreamA (fp32 source, per wave, several k-tiles ahead), and the three LDS-DMA loaders of
// pre-split plane images: PlaneLoader (weights), PlaneGatherLoader (activations, conv gathers), PlaneKLoader (K-major pairs).
#pragma once
#include "koaf_pieces.h"

namespace {

// ---- bf16 ACTIVATION STORAGE (KoafGemm.act16) ------------------------------------------------------------------------------
// The forward activations of a trunk (conv outputs, block outputs) may live in HBM as bf16 instead of fp32: half the bytes on
// every HBM-bound call.  Arithmetic is unchanged: a loader widens the bf16 values to fp32 (exact), applies its transform and
// cuts the fp32 result into the same two fp16 pieces; accumulation, statistics and all gradients stay fp32; only the store of a
// forward output rounds (to nearest even).  Raw 16-bit loads are kept as bits in the loader slot and widened in finish(), so
// that the loads stay in flight under the MFMAs exactly like the fp32 ones.
// 4 consecutive elements at element offset `off` of a tensor stored as fp32 (H = false) or bf16 (H = true: the pointer is typed
// float* all the same); the 16-bit form returns the raw bits in lanes 0 / 1 (widen_bf16x4 later)
template <bool H>
__device__ __forceinline__ v4f load4_raw(const float* p, int64_t off) {
    if constexpr (!H) return *(const v4f*)(p + off);
    else {
        const uint2 u = *(const uint2*)(reinterpret_cast<const unsigned short*>(p) + off);
        return (v4f){__uint_as_float(u.x), __uint_as_float(u.y), 0.f, 0.f};
    }
}
// operand access modes (compile-time: the loaders are straight-line code, so hipcc can schedule their
// address arithmetic into the shadows of the MFMAs)
enum { M_KC = 0,     // K-contiguous rows, dense
       M_KC_G1 = 1,  // K-contiguous, conv forward gather (NHWC source)
       M_KC_G2 = 2,  // K-contiguous, transposed-conv (dgrad) gather
       M_KM = 3,     // K-major, dense
       M_KM_G1 = 4,  // K-major, conv gather on the k index (wgrad activations)
       M_KM_G3 = 5,  // K-major, tapped weights (dgrad)
       M_PS = 6,     // pre-split fp16 plane images, K-contiguous rows, optionally tapped (weights: forward and dgrad)
       M_PA1 = 7,    // pre-split fp16 plane images of an NHWC activation, conv forward gather (A operand)
       M_PA2 = 8,    // the same, transposed-conv (dgrad) gather
       M_PH = 9,     // the same images, 3x3 / stride 1 / pad 1: the tile's pixel rows + halo stay in LDS for all nine taps
       M_PK = 10,    // activation plane images read K-major (weight gradient: k = pixel, rows = channels), dense
       M_PKG = 11,   // the same with the conv gather on the k index and the filter tap in the column (wgrad activations)
       M_PT = 12,    // activation plane images, 3x3 / stride 1 / pad 1, 2-D pixel tiles (8 x 16) with a zero-filled halo in LDS (64 channels
                     // at a time: one filter tap x 64 channels per barrier)
       M_KS = 13     // K-contiguous dense rows (as M_KC), STREAMED: every wave loads, transforms and splits its OWN 32 rows, several
                     // k-tiles ahead in registers (StreamA) -- the 1x1 / stride-1 convolutions and their data gradients
};
__host__ __device__ constexpr bool mode_is_kc(int m) { return m < 3 || m == M_KS; }
__host__ __device__ constexpr bool mode_is_pa(int m) { return m == M_PA1 || m == M_PA2; }

// TF = transform on load (KoafOperand.tf): 0 none; 1 relu(sc[c] * x + sh[c]) -- the producer's BatchNorm + ReLU; 2 the
// BatchNorm-BACKWARD apply dc = sc[c] * dz + sh[c] - sc2[c] * c_raw of TWO source tensors (x = dz at ptr, c_raw at ptr2, same
// layout): the gradient w.r.t. a conv output is formed in the loaders of the dgrad / wgrad GEMMs that consume it and never
// written to HBM.  (TF 2 needs the vector path.)
// F16: the operand feeds the fp16 scheme: finish() also multiplies by the operand's scale `fsc` (folded into the transform
// coefficients where there is a transform) and clamps to the fp16 range (relu and clamp are one v_med3 for TF 1).
// S16 / S2_16: the source tensor at ptr / ptr2 is stored as bf16 (activation storage mode; vector path only)
template <int ROWS, int MODE, int TF, bool VEC, bool F16, bool S16 = false, bool S2_16 = false>
struct TileLoader {
    static_assert(!(S16 || S2_16) || VEC, "bf16 sources need the vector path");
    static constexpr int NU = ROWS / 32;
    static constexpr bool KC = mode_is_kc(MODE);
    static constexpr int NU2 = (TF == 2 || TF == 3) ? NU : 1;
    static_assert(TF != 3 || (MODE == M_KC && VEC && F16), "the bottleneck-tail prologue (tf 3) serves the dense K-contiguous fp16-scheme loader");
    // registers of one k-tile in flight
    struct Slot {
        v4f r[NU];
        v4f r2[NU2];   // TF 2: the second source
        unsigned vm;   // validity bits: VEC 1 bit / unit, else 4 bits / unit
        v4f ts4, th4, tk4;  // transform coefficients of the tile (KC operands: they depend on k)
        v4f tq4;            // TF 3 with the identity's own affine (a downsample branch): its shift (tk4 = its scale)
    };
    Slot sa, sb;
    bool tail2 = false;      // TF 3: the identity is sc2[c] * x2 + sh2[c] (KoafOperand.sc2 / sh2 given)
    v4f kts4, kth4, ktk4;    // transform coefficients of this thread's columns (KM operands: fixed)
    float fsc;               // F16: operand scale (a power of two)
    unsigned satmax;         // F16, TF 1: packed maximum of the fp16 hi pieces stored so far (0x7bff = clamped at 65504)
    // KC state (ext-vector values, not arrays: arrays of per-unit state were left in scratch by hipcc and
    // every scratch reload drained the in-flight global loads through the in-order vmcnt)
    v4l base;          // element offset of each unit's row / image from the operand pointer
    v4i iy0, ix0;
    unsigned rvm;      // row-valid bits
    v4i toff;          // conv gathers: per-image element offset of the CURRENT filter tap (recomputed per tap,
    unsigned tvm;      //   not per k-step: a tap spans C/32 k-steps) and its validity bits
    int tap_cur;
    // KM state
    int col, cc, kh_, kw_;
    unsigned cvm;      // column-valid bits
    // Running decomposition of k.  issue() is called for k0 = kbeg, kbeg + BK, ... in order, so the filter tap of a
    // k-tile (u_*: wave-uniform) and the source pixel of every k row of a gathered K-major tile (g_*: per unit) are
    // carried from one call to the next by adds and single carries instead of being re-derived by integer divisions
    // and 64-bit multiplies -- those were a third of the vector instructions of the weight-gradient kernels.
    int u_tap, u_coff, u_kh, u_kw;
    v4i gsx, gsy;
    v4l goff;
    int g_cs, g_bs, g_pws, g_phs, g_sxlim, g_sylim;
    int64_t g_d0, g_d1, g_d2;

    __device__ __forceinline__ void init(const KoafOperand& op, int r0, int R, int z1, float scale) {
        const int t = threadIdx.x;
        fsc = scale;
        satmax = 0u;
        sa.vm = sb.vm = 0;
        sa.ts4 = sa.th4 = sb.ts4 = sb.th4 = kts4 = kth4 = sa.tk4 = sb.tk4 = ktk4 = sa.tq4 = sb.tq4 = (v4f){0.f, 0.f, 0.f, 0.f};
        if constexpr (TF == 3) tail2 = op.sc2 != nullptr;
        rvm = cvm = 0;
        base = (v4l){0, 0, 0, 0};
        iy0 = ix0 = toff = (v4i){0, 0, 0, 0};
        tvm = 0;
        tap_cur = -1;
        col = cc = kh_ = kw_ = 0;
        if constexpr (KC) {
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int row = r0 + (t >> 3) + 32 * i;
                rvm |= (row < R ? 1u : 0u) << i;
                if constexpr (MODE == M_KC) {
                    base[i] = (int64_t)row * op.ld + 4 * (t & 7);
                } else {
                    const int ppi = op.PH * op.PW;
                    const int n = row / ppi;
                    const int rem = row - n * ppi;
                    const int py = rem / op.PW;
                    const int px = rem - py * op.PW;
                    base[i] = (int64_t)n * op.H * op.W * op.CS + 4 * (t & 7);
                    if constexpr (MODE == M_KC_G1) {
                        iy0[i] = py * op.stride - op.pad;
                        ix0[i] = px * op.stride - op.pad_w;
                    } else {
                        iy0[i] = py + op.pad;
                        ix0[i] = px + op.pad_w;
                    }
                }
            }
        } else {
            constexpr int CV = ROWS / 4;
            col = r0 + 4 * (t % CV);
#pragma unroll
            for (int j = 0; j < 4; ++j) cvm |= ((col + j) < R ? 1u : 0u) << j;
            cc = col;
            if constexpr (MODE == M_KM_G1) {
                // this thread's own filter tap (its 4 columns lie in one tap: C % 4 == 0), so a tile may span taps
                const int tap = col / op.C;
                cc = col - tap * op.C;
                kh_ = tap / op.KW;
                kw_ = tap - kh_ * op.KW;
            }
            if constexpr (TF != 0) {
                const float* sc = op.sc + z1 * op.tf_bs;
                const float* sh = op.sh + z1 * op.tf_bs;
                if (VEC) {
                    if (cvm & 1u) {
                        kts4 = *(const v4f*)(sc + cc);
                        kth4 = *(const v4f*)(sh + cc);
                        if constexpr (TF == 2) ktk4 = *(const v4f*)(op.sc2 + z1 * op.tf_bs + cc);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((cvm >> j) & 1u) { kts4[j] = sc[cc + j]; kth4[j] = sh[cc + j]; }
                }
                if constexpr (F16) { kts4 *= fsc; kth4 *= fsc; ktk4 *= fsc; }
            }
        }
    }

    // Position the running k decomposition at k0 (the only place that divides); call once before the first issue().
    __device__ __forceinline__ void seek(const KoafOperand& op, int k0) {
        u_tap = u_coff = u_kh = u_kw = 0;
        gsx = gsy = (v4i){0, 0, 0, 0};
        goff = (v4l){0, 0, 0, 0};
        g_cs = g_bs = g_pws = g_phs = g_sxlim = g_sylim = 0;
        g_d0 = g_d1 = g_d2 = 0;
        if constexpr (MODE == M_KC_G1 || MODE == M_KC_G2 || MODE == M_KM_G3) {
            u_tap = k0 / op.C;
            u_coff = k0 - u_tap * op.C;
            u_kh = u_tap / op.KW;
            u_kw = u_tap - u_kh * op.KW;
        }
        if constexpr (MODE == M_KM_G1) {
            constexpr int CV = ROWS / 4;
            constexpr int RP = 256 / CV;
            const int ppi = op.PH * op.PW;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int k = k0 + (int)threadIdx.x / CV + RP * i;
                const int n = k / ppi;
                const int rem = k - n * ppi;
                const int py = rem / op.PW;
                const int px = rem - py * op.PW;
                gsy[i] = py * op.stride - op.pad + kh_;
                gsx[i] = px * op.stride - op.pad_w + kw_;
                goff[i] = ((int64_t)(n * op.H + gsy[i]) * op.W + gsx[i]) * op.CS + cc;
            }
            // one k-step = BK rows further: BK = a * ppi + b * PW + c  (c < PW, b < PH: single carries below)
            const int a = BK / ppi, r = BK - a * ppi, b = r / op.PW, c = r - b * op.PW;
            const int64_t wcs = (int64_t)op.W * op.CS, hwcs = (int64_t)op.H * wcs;
            g_cs = c * op.stride;
            g_bs = b * op.stride;
            g_pws = op.PW * op.stride;
            g_phs = op.PH * op.stride;
            g_sxlim = g_pws - op.pad_w + kw_;      // px == PW  <=>  sx == sxlim
            g_sylim = g_phs - op.pad + kh_;
            g_d0 = a * hwcs + g_bs * wcs + (int64_t)g_cs * op.CS;
            g_d1 = (int64_t)op.stride * wcs - (int64_t)g_pws * op.CS;    // px wraps: next pixel row
            g_d2 = hwcs - g_phs * wcs;                                   // py wraps: next image
        }
    }

    // Issue the global loads of the k-tile [k0, k0+32): nothing here consumes a loaded value, so the
    // s_waitcnt lands in finish(), after the MFMAs of the tile currently in LDS.
    __device__ __forceinline__ void issue(Slot& s, const KoafOperand& op, const float* ptr, int k0, int kend, int z1) {
        const int t = threadIdx.x;
        [[maybe_unused]] const float* ptr2 = (TF == 2 || TF == 3) ? op.ptr2 + (ptr - op.ptr) : nullptr;   // (same batch offset; batches of one where the storage types differ)
        s.vm = 0;
        if constexpr (KC) {
            const int kk = k0 + 4 * (t & 7);
            const bool kok = kk < kend;
            int ch = kk, coff = k0;
            if constexpr (MODE != M_KC) {
                // a 32-wide k chunk lies inside one filter tap (C % 32 == 0); (tap, coff, kh, kw) of this k0 are carried
                const int tap = u_tap;
                coff = u_coff;
                ch = coff + 4 * (t & 7);
                const int kh = u_kh, kw = u_kw;
                u_coff += BK;
                if (u_coff >= op.C) {
                    u_coff -= op.C;
                    ++u_tap;
                    if (++u_kw == op.KW) { u_kw = 0; ++u_kh; }
                }
                if (tap != tap_cur) {          // wave-uniform: new tap -> new source pixel / bounds for every unit
                    tap_cur = tap;
                    tvm = 0;
#pragma unroll
                    for (int i = 0; i < NU; ++i) {
                        int sy, sx;
                        bool ok = (rvm >> i) & 1u;
                        if constexpr (MODE == M_KC_G1) {
                            sy = iy0[i] + kh;
                            sx = ix0[i] + kw;
                        } else {
                            const int ny = iy0[i] - kh, nx = ix0[i] - kw;
                            ok = ok && ny >= 0 && nx >= 0;
                            if (op.stride == 1) {
                                sy = ny;
                                sx = nx;
                            } else if (op.stride == 2) {
                                sy = ny >> 1;
                                sx = nx >> 1;
                                ok = ok && (((ny | nx) & 1) == 0);
                            } else {
                                sy = ny / op.stride;
                                sx = nx / op.stride;
                                ok = ok && (sy * op.stride == ny) && (sx * op.stride == nx);
                            }
                        }
                        ok = ok && (unsigned)sy < (unsigned)op.H && (unsigned)sx < (unsigned)op.W;
                        toff[i] = (sy * op.W + sx) * op.CS;   // per-image offset fits 32 bits
                        tvm |= (ok ? 1u : 0u) << i;
                    }
                }
            }
            if constexpr (TF != 0) {
                const float* sc = op.sc + z1 * op.tf_bs;
                const float* sh = op.sh + z1 * op.tf_bs;
                if (VEC) {
                    const int c = kok ? ch : 0;
                    s.ts4 = *(const v4f*)(sc + c);
                    s.th4 = *(const v4f*)(sh + c);
                    if constexpr (TF == 2) s.tk4 = *(const v4f*)(op.sc2 + z1 * op.tf_bs + c);
                    if constexpr (TF == 3) {
                        if (tail2) { s.tk4 = *(const v4f*)(op.sc2 + c); s.tq4 = *(const v4f*)(op.sh2 + c); }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = (kk + j < kend) ? ch + j : 0;
                        s.ts4[j] = sc[c];
                        s.th4[j] = sh[c];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const bool rok = (rvm >> i) & 1u;
                if constexpr (MODE == M_KC) {
                    if (VEC) {
                        const bool ok = rok && kok;
                        s.r[i] = load4_raw<S16>(ptr, ok ? base[i] + k0 : 0);
                        if constexpr (TF == 2 || TF == 3) s.r2[i] = load4_raw<S2_16>(ptr2, ok ? base[i] + k0 : 0);
                        s.vm |= (ok ? 1u : 0u) << i;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool ok = rok && (kk + j) < kend;
                            s.r[i][j] = ptr[ok ? base[i] + k0 + j : 0];
                            s.vm |= (ok ? 1u : 0u) << (4 * i + j);
                        }
                    }
                } else {
                    const bool ok = kok && ((tvm >> i) & 1u);
                    s.r[i] = load4_raw<S16>(ptr, ok ? base[i] + (toff[i] + coff) : 0);
                    if constexpr (TF == 2) s.r2[i] = load4_raw<S2_16>(ptr2, ok ? base[i] + (toff[i] + coff) : 0);
                    s.vm |= (ok ? 1u : 0u) << i;
                }
            }
        } else {
            constexpr int CV = ROWS / 4;
            constexpr int RP = 256 / CV;
            const int kr0 = t / CV;
            int c03 = 0, th3 = 0, tw3 = 0;
            if constexpr (MODE == M_KM_G3) {
                c03 = u_coff; th3 = u_kh; tw3 = u_kw;
                u_coff += BK;
                if (u_coff >= op.C) {
                    u_coff -= op.C;
                    if (++u_kw == op.KW) { u_kw = 0; ++u_kh; }
                }
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const int k = k0 + kr0 + RP * i;
                bool ok = k < kend;
                int64_t off;
                if constexpr (MODE == M_KM) {
                    off = (int64_t)k * op.ld + col;
                } else if constexpr (MODE == M_KM_G3) {
                    // tapped weights: k = (tap, ck), tap = th*KW + tw; element at ck*ld + th*tap_stride_h + tw*tap_stride + col
                    off = (int64_t)(c03 + kr0 + RP * i) * op.ld + th3 * op.tap_stride_h + tw3 * op.tap_stride + col;
                } else {
                    const int sy = gsy[i], sx = gsx[i];
                    ok = ok && (unsigned)sy < (unsigned)op.H && (unsigned)sx < (unsigned)op.W;
                    off = goff[i];
                    // advance this unit's source pixel by BK rows of k
                    int nsx = sx + g_cs;
                    const bool c1 = nsx >= g_sxlim;
                    nsx -= c1 ? g_pws : 0;
                    int nsy = sy + g_bs + (c1 ? op.stride : 0);
                    const bool c2 = nsy >= g_sylim;
                    nsy -= c2 ? g_phs : 0;
                    gsx[i] = nsx;
                    gsy[i] = nsy;
                    goff[i] = off + g_d0 + (c1 ? g_d1 : (int64_t)0) + (c2 ? g_d2 : (int64_t)0);
                }
                if (VEC) {
                    ok = ok && (cvm & 1u);
                    s.r[i] = load4_raw<S16>(ptr, ok ? off : 0);
                    if constexpr (TF == 2) s.r2[i] = load4_raw<S2_16>(ptr2, ok ? off : 0);
                    s.vm |= (ok ? 1u : 0u) << i;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool okj = ok && ((cvm >> j) & 1u);
                        s.r[i][j] = ptr[okj ? off + j : 0];
                        s.vm |= (okj ? 1u : 0u) << (4 * i + j);
                    }
                }
            }
        }
    }

    // transform + zero-fill of the tile issued by issue(); first consumer of the loaded registers
    // TF 3 (the bottleneck tail formed on load): y = relu(sc[c] * x + sh[c] + x2) of the conv output x at ptr and the identity x2
    // at ptr2 -- the arithmetic of koaf_bn_add_relu, bit for bit; y itself is written to `side` (same layout as x) when this
    // block owns the column range (side != nullptr: the first column tile), at element offset base[i] + k0s.
    float* side = nullptr;
    int k0s = 0;
    // FULL: every element of this wave's slot is valid (interior tiles of the dense operands: the usual case) -- no zero-fill selects
    template <bool FULL>
    __device__ __forceinline__ void finish_unit(Slot& s, int i, v4f a, v4f b, v4f k, v4f q = (v4f){0.f, 0.f, 0.f, 0.f}) {
        constexpr float HMAX = 65504.f;
        if constexpr (S16) s.r[i] = widen_bf16x4(__float_as_uint(s.r[i][0]), __float_as_uint(s.r[i][1]));
        if constexpr (S2_16 && (TF == 2 || TF == 3)) s.r2[i < NU2 ? i : 0] = widen_bf16x4(__float_as_uint(s.r2[i < NU2 ? i : 0][0]), __float_as_uint(s.r2[i < NU2 ? i : 0][1]));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = FULL || (VEC ? ((s.vm >> i) & 1u) : ((s.vm >> (4 * i + j)) & 1u));
            float x = s.r[i][j];
            if constexpr (TF == 1) {
                x = fmaf(x, a[j], b[j]);
                x = F16 ? __builtin_amdgcn_fmed3f(x, 0.f, HMAX) : fmaxf(x, 0.f);
            } else if constexpr (TF == 2) {
                x = fmaf(a[j], x, fmaf(-k[j], s.r2[i < NU2 ? i : 0][j], b[j]));
                if constexpr (F16) x = __builtin_amdgcn_fmed3f(x, -HMAX, HMAX);
            } else if constexpr (TF == 3) {
                float idv = s.r2[i < NU2 ? i : 0][j];
                if (tail2) idv = fmaf(idv, k[j], q[j]);                  // (a downsample branch: its BatchNorm, as koaf_bn_add_relu's idsc / idsh)
                x = fmaxf(fmaf(x, a[j], b[j]) + idv, 0.f);      // (a, b unscaled here: y is stored as it is)
                if constexpr (S16) x = widen_bf16x4(round_bf16x4((v4f){x, 0.f, 0.f, 0.f}).x, 0u)[0];   // bf16 storage: everyone reads the ROUNDED y
                s.r2[i < NU2 ? i : 0][j] = x;
                x = fminf(x * fsc, HMAX);
            } else if constexpr (F16) {
                x = __builtin_amdgcn_fmed3f(x * fsc, -HMAX, HMAX);
            }
            s.r[i][j] = ok ? x : 0.f;
        }
        if constexpr (TF == 3) {
            if (side != nullptr && (FULL || ((s.vm >> i) & 1u))) {
                if constexpr (S16) store4<true>(side, base[i] + k0s, s.r2[i < NU2 ? i : 0]);
                else *(v4f*)(side + base[i] + k0s) = s.r2[i < NU2 ? i : 0];
            }
        }
    }
    __device__ __forceinline__ void finish(Slot& s) {
        v4f a = KC ? s.ts4 : kts4, b = KC ? s.th4 : kth4, k = KC ? s.tk4 : ktk4;
        if constexpr (F16 && KC && TF != 0 && TF != 3) { a *= fsc; b *= fsc; k *= fsc; }     // (KM coefficients were scaled once in init)
        // (wave-uniform: one ballot per tile; the ragged last tiles and the padded taps of gathers take the selecting form)
        constexpr unsigned ALLV = VEC ? ((NU >= 32) ? ~0u : ((1u << NU) - 1u)) : ((4 * NU >= 32) ? ~0u : ((1u << (4 * NU)) - 1u));
        if (__builtin_amdgcn_ballot_w64(s.vm != ALLV) == 0ull) {
#pragma unroll
            for (int i = 0; i < NU; ++i) finish_unit<true>(s, i, a, b, k, s.tq4);
        } else {
#pragma unroll
            for (int i = 0; i < NU; ++i) finish_unit<false>(s, i, a, b, k, s.tq4);
        }
    }
    // LDS dword offset (within a plane) of unit i of this thread
    __device__ __forceinline__ int plane_off(int i) const {
        const int t = threadIdx.x;
        if constexpr (KC) {
            return ((t >> 3) + 32 * i) * 20 + 2 * (t & 7);
        } else {
            constexpr int CV = ROWS / 4;
            constexpr int RP = 256 / CV;
            return (t / CV + RP * i) * (ROWS / 2 + 16) + 2 * (t % CV);
        }
    }

    template <int NPL>
    __device__ __forceinline__ void store(const Slot& s, float* Sf) {
        unsigned* S = (unsigned*)Sf;
        constexpr int P = plane_dwords(ROWS, KC);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            unsigned pl[NPL][2];
            if constexpr (F16) split2h(s.r[i], pl);
            else split3v(s.r[i], pl);
            if constexpr (F16 && (TF == 1 || TF == 3) && KC) {
                // saturation watch of the fixed activation scale: behind the ReLU the hi pieces are non-negative fp16, whose
                // bits order like the values -- one packed 16-bit maximum per two elements; a tile that reached 65504 (0x7bff)
                // clamped something (koaf.h koaf_set_status_buffer)
                typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int d = 0; d < 2; ++d)
                    satmax = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, satmax),
                                                                                     __builtin_bit_cast(u16x2, pl[0][d])));
            }
            const int off = plane_off(i);
#pragma unroll
            for (int q = 0; q < NPL; ++q) *(uint2*)&S[q * P + off] = make_uint2(pl[q][0], pl[q][1]);
        }
    }
};


// ---- M_KS: the dense K-contiguous fp32 A operand, streamed per wave ------------------------------------------------------------
// The block-wide loader above keeps ONE k-tile in flight (issued at the top of a k-step, consumed at its end) and meets at two
// barriers per step: on the 1x1 convolutions of layer2-4 -- K = 128 .. 2048, 4 .. 64 steps of 24 MFMAs per wave -- every step
// then costs a memory latency (in-kernel stamps: 1.7 us per step against 0.4 us of matrix work; the same kernel fed from
// pre-split plane images by LDS-DMA, no conversion at all, is only 10 % faster).  Here the waves of a block are 4 x 1: wave w
// owns rows 32 w .. 32 w + 31 of the tile and ALL its columns, so the A image rows it writes are the rows it reads -- no block
// barrier on the A side, only the in-order LDS queue of the wave itself -- and it keeps SD k-tiles of its rows in flight in
// registers (16 per tile and source).  The flattened (tile, k-step) sequence of a persistent block is prefetched across tile
// boundaries: the first SD k-tiles of the next tile land under the epilogue of the current one.  Arithmetic, pieces and MFMA
// order per accumulator are those of TileLoader + the shared k-loop: bit-identical outputs (test_stream_kernel_is_bit_identical).
// Lane l of a wave: unit i (0..3) = row 8 i + l / 8 of the wave's band, k = 4 (l % 8) .. + 3 -- 128-B row segments per 8 lanes.
constexpr int STREAM_TAB_K = 1024;      // longest k range of a TF 1 call on the streamed path (8 KiB of LDS beside the operand images)
template <int TF, int SD>
struct StreamA {
    static constexpr bool TWO = (TF == 2 || TF == 3);
    struct Slot {
        v4f r[4];
        v4f r2[TWO ? 4 : 1];
        v4f ts, th, tk, tq;      // transform coefficients of the k-tile's 4 columns of this lane (sc, sh, sc2, sh2)
    };
    Slot sl[SD];
    const float* ptr;
    const float* ptr2;
    const float* sc;
    const float* sh;
    const float* sc2;
    const float* sh2;
    const float* tab;     // TF 1: LDS table [2][STREAM_TAB_K] of sc * fsc, sh * fsc (the coefficients depend on k only: read when a k-tile
                          // is consumed instead of riding in eight registers per tile in flight)
    int64_t ld;
    float fsc;
    bool tail2;
    bool once;        // the A operand is read by ONE column tile (N <= BN): non-temporal loads (measured, kept on)
    unsigned satmax;
    // issue cursor: the k-tile the next issue() fetches
    v4l ibase;        // element offset of each unit's (clamped) row + 4 (l % 8)
    int ik;
    // consumer side
    v4l cbase;        // TF 3: offsets of the side store (the tile being consumed)
    unsigned rvm;     // row-valid bits of the tile being consumed
    int kbeg, kend;

    __device__ __forceinline__ v4l bases(int m0, int M) const {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        v4l b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = min(m0 + 32 * w + 8 * i + (lane >> 3), M - 1);     // (rows past M re-read the last row: zeroed in consume())
            b[i] = (int64_t)row * ld + 4 * (lane & 7);
        }
        return b;
    }
    __device__ __forceinline__ void init(const KoafOperand& op, const float* p, int m0, int M, int kb, int ke, float scale) {
        ptr = p;
        ptr2 = TWO ? op.ptr2 + (p - op.ptr) : nullptr;
        sc = op.sc; sh = op.sh; sc2 = op.sc2; sh2 = op.sh2;
        ld = op.ld;
        fsc = scale;
        tail2 = (TF == 3) && op.sc2 != nullptr;
        once = false;
        satmax = 0u;
        tab = nullptr;
        kbeg = kb; kend = ke;
        ik = kb;
        ibase = bases(m0, M);
        tile(m0, M);
    }
    // the consumer moves on to the tile at m0
    __device__ __forceinline__ void tile(int m0, int M) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        rvm = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) rvm |= ((m0 + 32 * w + 8 * i + (lane >> 3)) < M ? 1u : 0u) << i;
        if constexpr (TF == 3) cbase = bases(m0, M);
    }
    // loads of the k-tile at the cursor into slot s; the cursor then advances by one k-tile and, at the end of the k range, to
    // the first row next() returns for the block's following tile (the cursor runs SD k-tiles ahead of the consumer, so with as few
    // as SD k-steps per tile it is a whole tile ahead: it keeps its own place in the block's tile sequence); next() < 0: no
    // further tile -- the k-loop issues no more loads then
    template <class NextFn>
    __device__ __forceinline__ void issue(Slot& s, NextFn next, int M) {
        const int lane = threadIdx.x & 63;
        const int c = ik + 4 * (lane & 7);
        if constexpr (TF > 1) {
            s.ts = *(const v4f*)(sc + c);
            s.th = *(const v4f*)(sh + c);
            if constexpr (TF == 2) s.tk = *(const v4f*)(sc2 + c);
            if constexpr (TF == 3) {
                if (tail2) { s.tk = *(const v4f*)(sc2 + c); s.tq = *(const v4f*)(sh2 + c); }
            }
        }
        if (once) {
            // (one column tile: every A byte is read exactly once by the whole grid -- streamed past the caches' replacement order)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s.r[i] = __builtin_nontemporal_load((const v4f*)(ptr + ibase[i] + ik));
                if constexpr (TWO) s.r2[i] = __builtin_nontemporal_load((const v4f*)(ptr2 + ibase[i] + ik));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s.r[i] = *(const v4f*)(ptr + ibase[i] + ik);
                if constexpr (TWO) s.r2[i] = *(const v4f*)(ptr2 + ibase[i] + ik);
            }
        }
        ik += BK;
        if (ik >= kend) {
            ik = kbeg;
            const int nm0 = next();
            if (nm0 >= 0) ibase = bases(nm0, M);
        }
    }
    // transform (TileLoader::finish_unit's arithmetic), split and store of slot s = the k-tile at k0 of the tile being consumed,
    // into this wave's rows of the block's A plane images S (plane_dwords(128, true) dwords per plane)
    template <bool FULL>
    __device__ __forceinline__ void consume_as(Slot& s, unsigned* S, int k0, float* side) {
        constexpr float HMAX = 65504.f;
        constexpr int P = plane_dwords(128, true);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        v4f a = s.ts, b = s.th, k = s.tk;
        if constexpr (TF == 2) { a *= fsc; b *= fsc; k *= fsc; }
        if constexpr (TF == 1) {
            a = *(const v4f*)(tab + (k0 - kbeg) + 4 * (lane & 7));
            b = *(const v4f*)(tab + STREAM_TAB_K + (k0 - kbeg) + 4 * (lane & 7));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = FULL || ((rvm >> i) & 1u);
            v4f x = s.r[i];
            [[maybe_unused]] v4f y = x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = x[j];
                if constexpr (TF == 1) {
                    v = fmaf(v, a[j], b[j]);
                    v = __builtin_amdgcn_fmed3f(v, 0.f, HMAX);
                } else if constexpr (TF == 2) {
                    v = fmaf(a[j], v, fmaf(-k[j], s.r2[i][j], b[j]));
                    v = __builtin_amdgcn_fmed3f(v, -HMAX, HMAX);
                } else if constexpr (TF == 3) {
                    float idv = s.r2[i][j];
                    if (tail2) idv = fmaf(idv, k[j], s.tq[j]);
                    v = fmaxf(fmaf(v, a[j], b[j]) + idv, 0.f);
                    y[j] = v;
                    v = fminf(v * fsc, HMAX);
                } else {
                    v = __builtin_amdgcn_fmed3f(v * fsc, -HMAX, HMAX);
                }
                x[j] = ok ? v : 0.f;
            }
            if constexpr (TF == 3) {
                if (side != nullptr && ok) *(v4f*)(side + cbase[i] + k0) = y;
            }
            unsigned pl[2][2];
            split2h(x, pl);
            if constexpr (TF == 1 || TF == 3) {
                typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int d = 0; d < 2; ++d)
                    satmax = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, satmax),
                                                                                     __builtin_bit_cast(u16x2, pl[0][d])));
            }
            const int off = (32 * w + 8 * i + (lane >> 3)) * 20 + 2 * (lane & 7);
#pragma unroll
            for (int q = 0; q < 2; ++q) *(uint2*)&S[q * P + off] = make_uint2(pl[q][0], pl[q][1]);
        }
    }
    __device__ __forceinline__ void consume(Slot& s, unsigned* S, int k0, float* side) {
        if (__builtin_amdgcn_ballot_w64(rvm != 15u) == 0ull) consume_as<true>(s, S, k0, side);
        else consume_as<false>(s, S, k0, side);
    }
};

// Pre-split operand (M_PS): bf16 plane images [plane][row][K] cut in HBM by koaf_wplanes_build, moved global -> LDS by
// global_load_lds_dwordx4.  One wave instruction fills 1 KiB = 16 rows x 64 B of one plane; the LDS image is linear
// (DMA writes land at wave base + 16 * lane), so its 16-B chunks are XOR-swizzled through the SOURCE address: lane l
// fetches chunk (l & 3) ^ (row / 4 % 4) of row l / 4 of its piece, and frag_load_ps() applies the same XOR.
template <int ROWS>
struct PlaneLoader {
    static constexpr int NPIECE = ROWS / 16;       // 1-KiB pieces per plane
    static constexpr int PPW = NPIECE / 4;         // per wave
    static constexpr int PLANE_BYTES = ROWS * 64;
    int64_t src[PPW];      // element offset (bf16) of this lane's chunk at k = 0, plane 0
    int u_coff, u_kh, u_kw;

    __device__ __forceinline__ void init(const KoafOperand& op, int r0, int R) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            // rows past R re-read the last row: finite values that only reach output columns >= N, which are never stored
            const int row = min(r0 + 16 * (w + 4 * j) + (lane >> 2), R - 1);
            src[j] = (int64_t)row * op.ld + 8 * ((lane & 3) ^ ((lane >> 4) & 3));
        }
        u_coff = u_kh = u_kw = 0;
    }
    __device__ __forceinline__ void seek(const KoafOperand& op, int k0) {
        const int tap = k0 / op.C;
        u_coff = k0 - tap * op.C;
        u_kh = tap / op.KW;
        u_kw = tap - u_kh * op.KW;
    }
    // DMA of the k-tile at the running position into the plane images at `lds` (one buffer = NPL * PLANE_BYTES)
    template <int NPL>
    __device__ __forceinline__ void issue(const KoafOperand& op, const unsigned short* planes, unsigned lds) {
        const int w = threadIdx.x >> 6;
        const int64_t koff = u_kh * op.tap_stride_h + u_kw * op.tap_stride + u_coff;
        u_coff += BK;
        if (u_coff >= op.C) {
            u_coff -= op.C;
            if (++u_kw == op.KW) { u_kw = 0; ++u_kh; }
        }
#pragma unroll
        for (int q = 0; q < NPL; ++q)
#pragma unroll
            for (int j = 0; j < PPW; ++j)
                lds_dma16(planes + q * op.plane_stride + src[j] + koff, lds + q * PLANE_BYTES + (w + 4 * j) * 1024);
    }
};

// Pre-split ACTIVATION operand (M_PA1 / M_PA2): the two fp16 piece planes [plane][pixel][CS] of an NHWC tensor, cut once
// by koaf_act_planes (BatchNorm + ReLU prologue or BatchNorm-backward apply included), gathered global -> LDS by
// global_load_lds_dwordx4 exactly like PlaneLoader: a lane moves the 16 B = 8 channels of ONE source pixel, so the im2col
// gather costs address arithmetic only (once per filter tap) -- no conversion, no split, no VGPR staging in the k-loop,
// where the fp32 loader redoes the split of every element for each of the KH*KW taps that touch it.  Padding taps and
// rows past M fetch the image's zero chunk (KoafOperand.zeros).  G = 1: conv forward gather; 2: transposed (dgrad).
template <int ROWS, int G>
struct PlaneGatherLoader {
    static constexpr int NPIECE = ROWS / 16;
    static constexpr int PPW = NPIECE / 4;
    static_assert(PPW >= 1 && PPW <= 4, "1..4 pieces per wave");
    static constexpr int PLANE_BYTES = ROWS * 64;
    v4l base;          // element offset of the piece row's image + this lane's swizzled chunk
    v4i iy0, ix0;
    v4i toff;          // per-image element offset of the current tap's source pixel
    unsigned rvm, tvm;
    int u_coff, u_kh, u_kw;
    bool fresh;

    __device__ __forceinline__ void init(const KoafOperand& op, int r0, int R) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        base = (v4l){0, 0, 0, 0};
        iy0 = ix0 = toff = (v4i){0, 0, 0, 0};
        rvm = tvm = 0;
        const int ppi = op.PH * op.PW;
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int row = r0 + 16 * (w + 4 * j) + (lane >> 2);
            rvm |= (row < R ? 1u : 0u) << j;
            const int n = row / ppi;
            const int rem = row - n * ppi;
            const int py = rem / op.PW;
            const int px = rem - py * op.PW;
            base[j] = (int64_t)n * op.H * op.W * op.CS + 8 * ((lane & 3) ^ ((lane >> 4) & 3));
            if constexpr (G == 1) {
                iy0[j] = py * op.stride - op.pad;
                ix0[j] = px * op.stride - op.pad_w;
            } else {
                iy0[j] = py + op.pad;
                ix0[j] = px + op.pad_w;
            }
        }
        u_coff = u_kh = u_kw = 0;
        fresh = true;
    }
    __device__ __forceinline__ void seek(const KoafOperand& op, int k0) {
        const int tap = k0 / op.C;
        u_coff = k0 - tap * op.C;
        u_kh = tap / op.KW;
        u_kw = tap - u_kh * op.KW;
        fresh = true;
    }
    __device__ __forceinline__ void issue(const KoafOperand& op, const unsigned short* planes, unsigned lds) {
        const int w = threadIdx.x >> 6;
        if (fresh || u_coff == 0) {        // wave-uniform: a new filter tap -> new source pixel / bounds of every piece row
            fresh = false;
            tvm = 0;
#pragma unroll
            for (int j = 0; j < PPW; ++j) {
                int sy, sx;
                bool ok = (rvm >> j) & 1u;
                if constexpr (G == 1) {
                    sy = iy0[j] + u_kh;
                    sx = ix0[j] + u_kw;
                } else {
                    const int ny = iy0[j] - u_kh, nx = ix0[j] - u_kw;
                    ok = ok && ny >= 0 && nx >= 0;
                    if (op.stride == 1) {
                        sy = ny;
                        sx = nx;
                    } else if (op.stride == 2) {
                        sy = ny >> 1;
                        sx = nx >> 1;
                        ok = ok && (((ny | nx) & 1) == 0);
                    } else {
                        sy = ny / op.stride;
                        sx = nx / op.stride;
                        ok = ok && (sy * op.stride == ny) && (sx * op.stride == nx);
                    }
                }
                ok = ok && (unsigned)sy < (unsigned)op.H && (unsigned)sx < (unsigned)op.W;
                toff[j] = (sy * op.W + sx) * op.CS;
                tvm |= (ok ? 1u : 0u) << j;
            }
        }
        const int coff = u_coff;
        u_coff += BK;
        if (u_coff >= op.C) {
            u_coff = 0;
            if (++u_kw == op.KW) { u_kw = 0; ++u_kh; }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < PPW; ++j) {
                const bool ok = (tvm >> j) & 1u;
                const unsigned short* src = ok ? planes + q * op.plane_stride + base[j] + (toff[j] + coff) : op.zeros;
                lds_dma16(src, lds + q * PLANE_BYTES + (w + 4 * j) * 1024);
            }
    }
};

// K-major operands from activation plane images (M_PK / M_PKG: the weight gradient, k = pixel): one DMA instruction moves
// 1 KiB = KPI whole k-rows (pixels) of ROWS channels; the LDS image is plane[32 k][ROWS] fp16, linear, its 16-B chunks
// XOR-swizzled by k so that the transposing fragment reads (ds_read_b64_tr_b16: 4 k-rows x 32 B per 16-lane group, two
// groups per LDS cycle) hit 64 distinct banks: chunk ^ 4 (k & 3) for 256-B rows, chunk ^ 4 (k / 2 & 1) for 128-B rows.

template <int ROWS, bool GATHER>
struct PlaneKLoader {
    static_assert(ROWS == 128 || ROWS == 64, "tile rows");
    static constexpr int CPR = ROWS / 8;          // 16-B chunks per k-row
    static constexpr int KPI = 64 / CPR;          // k-rows per DMA instruction
    static constexpr int NPIECE = 32 / KPI;       // instructions per plane and k-tile
    static constexpr int PPW = NPIECE / 4;        // per wave
    static constexpr int PLANE_BYTES = ROWS * 64;
    int col, cc, kh_, kw_;      // first column of this lane's chunk; its channel and filter tap (gather)
    bool cok;
    v4i kk;                     // k of each piece of this lane (k-tile origin excluded)
    // running source pixel of each piece (gather), as in TileLoader's M_KM_G1: advanced by adds and single carries
    v4i gsx, gsy;
    v4l goff;
    int g_cs, g_bs, g_pws, g_phs, g_sxlim, g_sylim;
    int64_t g_d0, g_d1, g_d2;

    __device__ __forceinline__ void init(const KoafOperand& op, int r0, int R) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const int kl = lane / CPR, phys = lane % CPR;
        col = r0 + 8 * (phys ^ kmd_swz(ROWS, kl));       // (pieces start on multiples of KPI >= 4 | 8: the swizzle sees kl only)
        cok = col < R;                                   // R % 8 == 0
        cc = col; kh_ = kw_ = 0;
        if constexpr (GATHER) {
            const int tap = col / op.C;
            cc = col - tap * op.C;
            kh_ = tap / op.KW;
            kw_ = tap - kh_ * op.KW;
        }
        kk = (v4i){0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < PPW; ++j) kk[j] = KPI * (w + 4 * j) + kl;
        gsx = gsy = (v4i){0, 0, 0, 0};
        goff = (v4l){0, 0, 0, 0};
        g_cs = g_bs = g_pws = g_phs = g_sxlim = g_sylim = 0;
        g_d0 = g_d1 = g_d2 = 0;
    }
    __device__ __forceinline__ void seek(const KoafOperand& op, int k0) {
        if constexpr (GATHER) {
            const int ppi = op.PH * op.PW;
#pragma unroll
            for (int j = 0; j < PPW; ++j) {
                const int k = k0 + kk[j];
                const int n = k / ppi;
                const int rem = k - n * ppi;
                const int py = rem / op.PW;
                const int px = rem - py * op.PW;
                gsy[j] = py * op.stride - op.pad + kh_;
                gsx[j] = px * op.stride - op.pad_w + kw_;
                goff[j] = ((int64_t)(n * op.H + gsy[j]) * op.W + gsx[j]) * op.CS + cc;
            }
            const int a = BK / ppi, r = BK - a * ppi, b = r / op.PW, c = r - b * op.PW;
            const int64_t wcs = (int64_t)op.W * op.CS, hwcs = (int64_t)op.H * wcs;
            g_cs = c * op.stride;
            g_bs = b * op.stride;
            g_pws = op.PW * op.stride;
            g_phs = op.PH * op.stride;
            g_sxlim = g_pws - op.pad_w + kw_;
            g_sylim = g_phs - op.pad + kh_;
            g_d0 = a * hwcs + g_bs * wcs + (int64_t)g_cs * op.CS;
            g_d1 = (int64_t)op.stride * wcs - (int64_t)g_pws * op.CS;
            g_d2 = hwcs - g_phs * wcs;
        }
    }
    // DMA of the k-tile [k0, k0 + 32) into the two plane images at LDS byte address `lds`
    __device__ __forceinline__ void issue(const KoafOperand& op, const unsigned short* planes, int k0, int kend, unsigned lds) {
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            bool ok = cok && (k0 + kk[j]) < kend;
            int64_t off;
            if constexpr (GATHER) {
                const int sy = gsy[j], sx = gsx[j];
                ok = ok && (unsigned)sy < (unsigned)op.H && (unsigned)sx < (unsigned)op.W;
                off = goff[j];
                int nsx = sx + g_cs;
                const bool c1 = nsx >= g_sxlim;
                nsx -= c1 ? g_pws : 0;
                int nsy = sy + g_bs + (c1 ? op.stride : 0);
                const bool c2 = nsy >= g_sylim;
                nsy -= c2 ? g_phs : 0;
                gsx[j] = nsx;
                gsy[j] = nsy;
                goff[j] = off + g_d0 + (c1 ? g_d1 : (int64_t)0) + (c2 ? g_d2 : (int64_t)0);
            } else {
                off = (int64_t)(k0 + kk[j]) * op.ld + col;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned short* src = ok ? planes + q * op.plane_stride + off : op.zeros;
                lds_dma16(src, lds + q * PLANE_BYTES + (w + 4 * j) * 1024);
            }
        }
    }
};

}  // namespace
