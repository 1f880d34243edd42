// koaf_pieces.h -- what every matrix-pipe kernel of libkoaf shares: the exact 16-bit pieces of fp32 operands, the operand
// scale, the LDS plane-image layouts with their MFMA fragment loads, and the LDS-DMA instruction.
//
// Arithmetic: gfx950 has no TF32-class matrix mode and its fp32 MFMA runs at 1/16 of the bf16 rate, so the fp32 x fp32
// products are formed on the 16-bit matrix pipe from exact pieces of the operands, fp32 accumulate.  Two schemes
// (KoafGemm.fmt), both at fp32 rounding level against float64 (scripts/gemm_accuracy.py, tests/test_kernels_gpu.py):
//   fmt 0 "bf16 x 3": every operand value is cut by truncation into three bf16 pieces hi + mid + lo that together hold
//       all 24 significand bits; of the nine piece products the six of relative weight >= 2^-16 are issued as
//       v_mfma_f32_32x32x16_bf16 (each exact in fp32); the three dropped ones are < 2^-21 of the product.  Works for any
//       fp32 operand (bf16 has fp32's exponent range): linear layers, attention, anything without scale information.
//       Six 8-pass MFMAs replace eight 16-pass fp32 MFMAs per 16 k: matrix-pipe bound 2500 / 6 = 417 TFLOP/s.
//   fmt 1 "fp16 x 2": the operand is multiplied by a power of two that puts its largest magnitude near 2^14 (the
//       producer of the tensor leaves max |x| in device memory: KoafOperand.amax; activations behind BatchNorm use a
//       fixed factor) and cut into hi = fp16(x'), lo = fp16(x' - hi), round-to-nearest: x' = hi + lo to 2^-24 relative
//       (lo is signed: 22 explicit bits + sign) down to |x'| = 2^-2 and to 2^-25 ABSOLUTE below (fp16 subnormals, which
//       the MFMA does not flush), i.e. <= 2^-40 of the tensor's largest magnitude.  Three products hi*hi, hi*lo, lo*hi on
//       v_mfma_f32_32x32x16_f16 (11 x 11 bits: exact in fp32); the dropped lo*lo is <= 2^-24 of the product.  Half the
//       matrix instructions of fmt 0 for the same accuracy -- this is what the convolutions (97 % of the FLOPs) run:
//       the bf16 scheme sits at the chip's power limit (the clock falls under six MFMAs per product), so fewer matrix
//       instructions per product is the lever.  Bound 2500 / 3 = 833 TFLOP/s.
//   Inf operands become NaN (inf - inf in the split); NaN stays NaN.
#pragma once
#include "koaf_common.h"

namespace {

constexpr int BK = 32;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int v2i __attribute__((ext_vector_type(2)));

// The split runs once per element in the loader and LDS holds three packed-bf16 plane images
// per operand:  KC operand  plane[row][32 k + 8 pad]   (80-B rows: ds_read_b128 fragments, conflict-free)
//               KM operand  plane[k][ROWS + 32 pad]    (ds_write_b64 of 4 rows, fragments by the transposing
//                                                       ds_read_b64_tr_b16; k-row stride = 16 (mod 64) dwords)
// Lane (r, h) of a 32x32x16 MFMA holds k = 16g + 8h + e (e = 0..7) of its row in both images.
__host__ __device__ constexpr int plane_dwords(int rows, bool kc) { return kc ? rows * 20 : 32 * (rows / 2 + 16); }

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// four fp32 values -> three (hi, mid, lo) pairs of dwords holding 4 packed bf16 each
__device__ __forceinline__ void split3v(const v4f x, unsigned out[3][2]) {
    float r1[4], r2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r1[e] = x[e] - __uint_as_float(__float_as_uint(x[e]) & 0xffff0000u);
        r2[e] = r1[e] - __uint_as_float(__float_as_uint(r1[e]) & 0xffff0000u);
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        out[0][d] = __builtin_amdgcn_perm(__float_as_uint(x[2 * d + 1]), __float_as_uint(x[2 * d]), 0x07060302u);
        out[1][d] = __builtin_amdgcn_perm(__float_as_uint(r1[2 * d + 1]), __float_as_uint(r1[2 * d]), 0x07060302u);
        out[2][d] = __builtin_amdgcn_perm(__float_as_uint(r2[2 * d + 1]), __float_as_uint(r2[2 * d]), 0x07060302u);
    }
}

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// power of two that brings a tensor whose largest magnitude is amax to [2^14, 2^15) (1 for amax == 0); koaf_wplanes_build
// and the GEMM kernel both derive an operand's scale from the same device scalar with this function
__device__ __forceinline__ float scale_of_amax(float amax) {
    if (!(amax > 0.f)) return 1.f;
    const int e = min(max(__builtin_amdgcn_frexp_expf(amax), -100), 100);   // amax = m * 2^e, m in [0.5, 1)
    return __builtin_ldexpf(1.f, 15 - e);
}
__device__ __forceinline__ float operand_scale(const KoafOperand& o) {
    return o.amax ? scale_of_amax(*o.amax) : (o.fscale != 0.f ? o.fscale : 1.f);
}

// four fp32 values x' (already multiplied by the operand's scale and clamped to the fp16 range by the loader's finish()) ->
// (hi, lo) pairs of dwords holding 4 packed fp16 each: hi = fp16(x'), lo = fp16(x' - hi), both round-to-nearest, so
// x' = hi + lo to 2^-24 relative (lo carries a sign) down to |x'| = 2^-2 and to 2^-25 absolute below that (fp16 subnormal
// spacing 2^-24).  The residual is taken from the PACKED hi, so one v_cvt_pk_f16_f32 serves storage and residual.
__device__ __forceinline__ void split2h(const v4f x, unsigned out[2][2]) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float a = x[2 * d], b = x[2 * d + 1];
        const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector((v2f){a, b}, h16x2));
        out[0][d] = hb;
        // residuals x - float(hi) in ONE instruction each (v_fma_mix_f32 reads the fp16 half of hb directly: the exact difference,
        // rounded once -- the bits of v_cvt_f32_f16 + v_sub_f32, which hipcc emits for the C++ form, at half the vector issue)
        float ra, rb;
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(hb), "v"(a));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(hb), "v"(b));
        out[1][d] = __builtin_bit_cast(unsigned, __builtin_convertvector((v2f){ra, rb}, h16x2));
    }
}

typedef short v4s __attribute__((ext_vector_type(4)));

// bf16x8 MFMA fragment of plane image P: rows row0 .. row0+31, k = 16g + 8h + (0..7); lane = 32h + r
template <int ROWS, bool KC>
__device__ __forceinline__ v4i frag_load(const unsigned* P, int row0, int g, int lane) {
    if constexpr (KC) {
        return *(const v4i*)&P[(row0 + (lane & 31)) * 20 + 8 * g + 4 * (lane >> 5)];
    } else {
        // two transposed 4(k) x 16(rows) block reads; lane 4q+p of a 16-lane group addresses block row q, cols 4p..4p+3
        const int li = lane & 15, q = li >> 2, pp = li & 3;
        const int rb = row0 + 16 * ((lane >> 4) & 1) + 4 * pp;
        const int k0 = 16 * g + 8 * (lane >> 5) + q;
        constexpr int SK = ROWS / 2 + 16;
        typedef __attribute__((address_space(3))) v4s* lds_v4s;
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(P + k0 * SK + rb / 2));
        const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(P + (k0 + 4) * SK + rb / 2));
        const v2i l2 = __builtin_bit_cast(v2i, lo), h2 = __builtin_bit_cast(v2i, hi);
        return (v4i){l2[0], l2[1], h2[0], h2[1]};
    }
}

// One LDS-DMA instruction: 64 lanes x 16 B from per-lane global addresses to the 1 KiB at LDS byte address `lds_addr`
// (wave-uniform), lane-linear.
// Issued as inline assembly, not through __builtin_amdgcn_global_load_lds: the compiler's wait-count pass treats every
// LDS read after a builtin LDS-DMA as possibly aliasing it and puts s_waitcnt vmcnt(0) in front of the ds_reads of the k-loop
// -- which drains the prefetch of the NEXT tiles before the current one is multiplied and was the largest single stall
// of the DMA kernels.  The kernels order DMA against LDS reads themselves (counted s_waitcnt vmcnt + s_barrier); no
// compiler-tracked vector memory operation is in flight while these are (the loops hold only DMA, and they drain it
// before the epilogue).
// (m0 is a reserved register to clang, which warns that it does not preserve it around the statement: nothing else in
// these kernels lives in m0 -- gfx9 LDS instructions do not read it and there is no indirect register indexing.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds_addr) {
    const int la = __builtin_amdgcn_readfirstlane((int)lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(la) : "memory", "m0");
}
// LDS byte address of a __shared__ array (taken ONCE, on the array itself, where the cast folds: converting the
// generic pointers computed later back to LDS addresses left a null check on the aperture register that hipcc could not select)
#define KOAF_LDS_ADDR(arr) ((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(arr))
#pragma clang diagnostic pop

// fragment of a swizzled linear plane image written by PlaneLoader: rows of 16 dwords (32 k)
__device__ __forceinline__ v4i frag_load_ps(const unsigned* P, int row0, int g, int lane) {
    const int row = row0 + (lane & 31);
    return *(const v4i*)&P[row * 16 + 4 * ((2 * g + (lane >> 5)) ^ ((row >> 2) & 3))];
}

// 16-B chunk swizzle of a K-major plane image [32 k][ROWS] fp16 (PlaneKLoader writes it, frag_load_kmd reads it)
__host__ __device__ constexpr int kmd_swz(int rows, int k) { return rows == 128 ? 4 * (k & 3) : 4 * ((k >> 1) & 1); }

// fragment of a k-swizzled K-major plane image written by PlaneKLoader (cf. frag_load's K-major branch)
template <int ROWS>
__device__ __forceinline__ v4i frag_load_kmd(const unsigned* P, int row0, int g, int lane) {
    const int li = lane & 15, q = li >> 2, pp = li & 3;
    const int rb = row0 + 16 * ((lane >> 4) & 1) + 4 * pp;
    const int k0 = 16 * g + 8 * (lane >> 5) + q;         // (k0 + 4 has the same swizzle)
    const int boff = k0 * (ROWS * 2) + (((rb >> 3) ^ kmd_swz(ROWS, k0)) << 4) + ((rb & 7) << 1);
    typedef __attribute__((address_space(3))) v4s* lds_v4s;
    const char* Pb = reinterpret_cast<const char*>(P);
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(Pb + boff));
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(Pb + boff + 4 * (ROWS * 2)));
    const v2i l2 = __builtin_bit_cast(v2i, lo), h2 = __builtin_bit_cast(v2i, hi);
    return (v4i){l2[0], l2[1], h2[0], h2[1]};
}

}  // namespace
