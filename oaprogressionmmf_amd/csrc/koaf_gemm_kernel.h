// koaf_gemm_kernel.h -- koaf_gemm_kernel, the one MFMA GEMM template under every dense contraction of the koafusion train
// step, with its shared epilogue.  The family files (koaf_gemm_*.hip) instantiate it; koaf_gemm.hip decides which.
//
// Block = 256 threads = 4 waves (2x2), block tile BM x BN x 32, wave tile (BM/2) x (BN/2) built from 32x32 MFMA
// tiles; 2 blocks per CU.  Operand tiles are staged global -> registers (fused BN+ReLU prologue, zero fill) ->
// split -> LDS; the next tile's global loads are in flight under the current tile's MFMAs.  LDS holds three
// (fmt 1: two) packed 16-bit plane images per operand (see plane_dwords()):
//   K-contiguous operand ("KC"): plane[row][32 k + 8 pad] -- ds_write_b64, fragments by ds_read_b128
//       (80-B rows: the 16 lanes of a b128 group hit 16 distinct 4-bank slots).
//   K-major operand ("KM"):      plane[k][ROWS + 32 pad]  -- ds_write_b64 of 4 rows, fragments by the transposing
//       ds_read_b64_tr_b16 (k-row stride = 16 mod 64 dwords: conflict-free).
// Both present the same k order to the MFMA (lane (r, h), element e: k = 16g + 8h + e), so any pairing of KC / KM
// operands works.  Accumulators live in VGPRs (built with -mllvm -amdgpu-mfma-vgpr-form, see the Makefile).
//   Pre-split operand ("PS", conv weights, fmt 1): the two planes are cut ONCE per optimizer step by koaf_wplanes_build into
//       fp16 plane images [plane][row][K] in HBM; the kernel moves them global -> LDS with global_load_lds_dwordx4 (no
//       VGPR staging, no split arithmetic in the k-loop) into a linear [row][32 k] image whose 16-B chunks are
//       XOR-swizzled (chunk ^ (row / 4 % 4), applied to the per-lane SOURCE address and to the ds_read_b128 address):
//       LDS-DMA writes are lane-linear, so rows cannot be padded, and the swizzle keeps the fragment reads conflict-free.
//       Double-buffered: the DMA of k-tile t+1 lands while tile t is multiplied.
#pragma once
#include "koaf_gemm_loaders.h"

// In-kernel phase stamps (diagnostic builds only: make stamps -> libkoaf_stamps.so, koaf_gemm_stamps.hip, scripts/stamps_*.py): thread 0 of every
// block adds the 100 MHz real-time counter differences between its phase boundaries to a device table.
#ifdef KOAF_STAMPS
// (64 replicas of the table, indexed by block id: the adds of ~10^5 tiles per launch must not queue on eight addresses; the
// stamps themselves are wave-uniform s_memrealtime reads kept in scalar registers, consumed only at the end of the tile)
__device__ unsigned long long koaf_stamp_tab[64][8];
#define KOAF_STAMP_DECL unsigned long long kst_[6] = {0, 0, 0, 0, 0, 0}
#define KOAF_STAMP(i) do { kst_[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define KOAF_STAMP_ADD(slot, a, b) do { if (threadIdx.x == 0 && kst_[b] >= kst_[a]) atomicAdd(&koaf_stamp_tab[blockIdx.x & 63][slot], kst_[b] - kst_[a]); } while (0)
#define KOAF_STAMP_ACC(slot, v) do { if (threadIdx.x == 0) atomicAdd(&koaf_stamp_tab[blockIdx.x & 63][slot], (unsigned long long)(v)); } while (0)
#define KOAF_STAMP_NOW() __builtin_amdgcn_s_memrealtime()
#else
#define KOAF_STAMP_NOW() 0ull
#define KOAF_STAMP_DECL
#define KOAF_STAMP(i)
#define KOAF_STAMP_ADD(slot, a, b)
#define KOAF_STAMP_ACC(slot, v)
#endif

namespace {

// halo kernel (M_PH): widest image row kept in LDS (BM + 2 W + 2 pixels of 32 channels, two buffers) and the number of
// weight-tile stages, chosen per column-tile width so that everything fits 160 KiB
// Two shapes: 256 pixel rows / 8 waves / one block per CU with the halo double-buffered across channel chunks, and 128 rows /
// 4 waves with ONE halo buffer in under 80 KiB, so that two blocks share a CU and one's prologue, chunk switch and epilogue
// run under the other's MFMAs (the shallow-K layers: 64 channels = two chunks, where those phases outweigh the k-loop).
__host__ __device__ constexpr int halo_max_w(int bn, int bm = 256) { return bm == 256 ? (bn == 64 ? 96 : 64) : (bn == 64 ? 96 : 48); }
__host__ __device__ constexpr int halo_b_stages(int bn, int bm = 256) { return bm == 256 ? 3 : (bn == 64 ? 4 : 3); }

// v & m as four opaque v_and_b32 (written in C++, hipcc turns the masked fragment load into a branch around the ds_read --
// or, with a plain vector AND, fails in instruction selection on this kernel)
__device__ __forceinline__ v4i and_mask(v4i v, int m) {
    v4i r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int x;
        asm("v_and_b32 %0, %1, %2" : "=v"(x) : "v"(v[e]), "v"(m));
        r[e] = x;
    }
    return r;
}

// M_PT: LDS-DMA of the 10 x 18 pixel halo of 2-D tile `tm` (64 channels from channel 64 * chunk, both planes: 2880 granules of 16 B
// = 45 pieces; wave w moves pieces w, w + 4, ...) into the image at LDS byte address halo0.  Granule c of halo pixel (y, x) lands at
// ((18 y + x) * 8 + (c ^ (x / 2 % 8))) * 16; pixels outside the image fetch the operand's zero chunk.
__device__ __forceinline__ void t2d_issue_halo(const KoafOperand& A, const unsigned short* Apl, int tm, int chunk, unsigned halo0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int Wd = A.W, Hd = A.H, CSa = A.CS;
    const int txn = Wd >> 4, tpi = (Hd >> 3) * txn;          // tiles per image row / per image
    const int img = tm / tpi, trem = tm - img * tpi, tyi = trem / txn, txi = trem - tyi * txn;
    // this lane's granule of its wave's first piece; every later piece is 256 granules = 32 halo pixels further on (one halo row and
    // 14 pixels), the second plane 1440 granules = 10 halo rows back: the pixel is carried, not re-derived by divisions
    int Gp = w * 64 + lane, q = 0;
    const int cs = Gp & 7;
    int y = (Gp >> 3) / 18, x = (Gp >> 3) - 18 * y;
    const int iy0 = tyi * 8 - 1, ix0 = txi * 16 - 1;
    const int64_t ibase = (int64_t)img * Hd * Wd;
#pragma unroll 1
    for (int pc = w; pc < 45; pc += 4) {
        const int c16 = cs ^ ((x >> 1) & 7);
        const int iy = iy0 + y, ix = ix0 + x;
        const bool ok = (unsigned)iy < (unsigned)Hd && (unsigned)ix < (unsigned)Wd;
        const unsigned short* src = ok ? Apl + q * A.plane_stride + (ibase + iy * Wd + ix) * CSa + (chunk * 64 + c16 * 8) : A.zeros;
        lds_dma16(src, halo0 + pc * 1024);
        Gp += 256; x += 14; y += 1;
        if (x >= 18) { x -= 18; y += 1; }
        if (q == 0 && Gp >= 1440) { Gp -= 1440; q = 1; y -= 10; }
    }
}

// Row loop of the vector epilogue for a FULL tile without row map, specialised on what is fused (residual, BatchNorm-
// backward mode, second BatchNorm) so that it is branch-free: the loads of four rows go out together before the first
// is consumed (the generic loop below tests every row and ends up with one load in flight at a time, which held the
// HBM-bound 1x1-dgrad epilogues at 2-3 TB/s).
// C16: the output tensor is stored as bf16; E16: the BatchNorm-backward operands (c / y / c2) are (KoafGemm.act16 1 / 2)
// KoafGemm.out_planes: the activation plane images of relu(out_sc * v + out_sh) * KOAF_ACT_SCALE for the four output elements v at
// element offset `off` -- koaf_act_planes' tf-1 arithmetic on the value as STORED (bf16 storage: the rounded one), bit for bit
template <bool C16>
__device__ __forceinline__ void epi_emit_planes(const KoafGemm& p, int64_t off, v4f v, v4f a, v4f b, unsigned& nsat) {
    constexpr float HMAX = 65504.f;
    if constexpr (C16) { const uint2 u = round_bf16x4(v); v = widen_bf16x4(u.x, u.y); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u = fmaf(v[j], a[j], b[j]);
        nsat += !(u <= HMAX) ? 1u : 0u;
        v[j] = __builtin_amdgcn_fmed3f(u, 0.f, HMAX);
    }
    unsigned pl[2][2];
    split2h(v, pl);
    *(uint2*)(p.out_planes + off) = make_uint2(pl[0][0], pl[0][1]);
    *(uint2*)(p.out_planes + p.out_ps + off) = make_uint2(pl[1][0], pl[1][1]);
}

// T2D: the tile's rows are an 8 x 16 pixel rectangle of one image (M_PT): row lr = pixel (lr / 16, lr % 16) of the tile whose first
// pixel is m0, image rows w2d pixels apart
// EMIT: the kernel instantiation that serves KoafGemm.out_planes (separate instantiations: the persistent 1x1 kernels carry the next
// tile's operand slot through this loop at the 256-register limit, and the emission arithmetic inline cost them 55-126 spilled registers)
template <int BM, int BN, int NT, bool HAS_R, int MODE, bool HAS_C2, bool C16, bool E16, bool T2D = false, bool EMIT = false>
__device__ __forceinline__ void epi_rows_full(const KoafGemm& p, const float* Cs, int ldcs, float* Cp, int64_t ldc,
                                              const float* Rp, int m0, int col, int c4, int rr, v4f bv, v4f mu, v4f is,
                                              v4f ms, v4f mh, v4f mu2, v4f is2, v4f& q1, v4f& q2, v4f& q3, v4f& qm, int w2d = 0) {
    constexpr int C4 = BN / 4, RPP = NT / C4, U = 4;
    static_assert((BM / RPP) % U == 0, "rows per thread must be a multiple of the batch");
    [[maybe_unused]] v4f ea = {0.f, 0.f, 0.f, 0.f}, eb = ea;      // KoafGemm.out_planes: this thread's columns of out_sc / out_sh, at the activation scale
    [[maybe_unused]] unsigned nsat = 0;
    if constexpr (EMIT && MODE == 0 && !HAS_R) {
        if (p.out_planes) { ea = *(const v4f*)(p.out_sc + col) * KOAF_ACT_SCALE; eb = *(const v4f*)(p.out_sh + col) * KOAF_ACT_SCALE; }
    }
#pragma unroll 1
    for (int row = rr; row < BM; row += RPP * U) {
        v4f rv[U], cv[U], yv[U], c2v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t orow;
            if constexpr (T2D) { const int lr_ = row + u * RPP; orow = m0 + (lr_ >> 4) * w2d + (lr_ & 15); }
            else orow = m0 + row + u * RPP;
            // (streamed once: non-temporal, like the stores below -- the tile's operands, not these, should stay in L2)
            if constexpr (HAS_R) rv[u] = __builtin_nontemporal_load((const v4f*)(Rp + orow * p.ldr + col));
            if constexpr (MODE != 0) cv[u] = load4_nt<E16>(p.bnb_c, orow * ldc + col);
            if constexpr (MODE == 1) yv[u] = load4_nt<E16>(p.bnb_y, orow * ldc + col);
            if constexpr (HAS_C2) c2v[u] = load4_nt<E16>(p.bnb2_c, orow * ldc + col);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t orow;
            if constexpr (T2D) { const int lr_ = row + u * RPP; orow = m0 + (lr_ >> 4) * w2d + (lr_ & 15); }
            else orow = m0 + row + u * RPP;
            v4f v = *(const v4f*)&Cs[(row + u * RPP) * ldcs + 4 * c4] + bv;
            if constexpr (HAS_R) v += rv[u];
            if constexpr (MODE == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = yv[u][j] > 0.f ? v[j] : 0.f;
            } else if constexpr (MODE == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (cv[u][j] * ms[j] + mh[j]) > 0.f ? v[j] : 0.f;
            }
            if constexpr (MODE != 0) {
                q1 += v;
                q2 += v * ((cv[u] - mu) * is);
                if constexpr (HAS_C2) q3 += v * ((c2v[u] - mu2) * is2);
#pragma unroll
                for (int j = 0; j < 4; ++j) qm[j] = __uint_as_float(max(__float_as_uint(qm[j]), koaf_absbits(v[j])));
            }
            store4_nt<C16>(Cp, orow * ldc + col, v);
            if constexpr (EMIT && MODE == 0 && !HAS_R) {
                if (p.out_planes) epi_emit_planes<C16>(p, orow * ldc + col, v, ea, eb, nsat);
            }
        }
    }
    if constexpr (EMIT && MODE == 0 && !HAS_R) koaf_status_add(p.status, 0, nsat);
}


// F16 = KoafGemm.fmt == 1 (two fp16 planes per operand, three products); else three bf16 planes, six products
// NT = threads per block: 256 (waves 2 x 2) or 512 (waves 4 x 2: the 256-row tiles of the halo kernel)
// PERSIST variants (see the kernel): the one-source A loaders only -- measured on the headline step, the forward 1x1
// convolutions gain 4-11 %, while the two-source (BatchNorm-backward apply) data-gradient kernels, whose second slot and
// fused-reduction epilogue already fill the register file, spill 40-250 B per lane and lose 8-20 %.
__host__ __device__ constexpr bool persist_mode(int am, int bmd, bool f16, int tfa) {
    return f16 && bmd == M_PS && am <= M_KC_G2 && tfa != 2 && tfa != 3;
}
// (the persistent variants carry the next tile's A slot through the epilogue: held to two waves per SIMD = 256 registers)
// ACT = KoafGemm.act16: which tensors of this call are bf16 ACTIVATIONS (0: none; 1 forward: A.ptr and C; 2 data gradient:
// A.ptr2 (the conv output c of a tf-2 apply) and the BatchNorm-backward operands of the epilogue; 3 weight gradient: A.ptr2 and B.ptr)
// SD (M_KS only): k-tiles of its rows a wave keeps in flight; the host picks one that divides the number of k-steps
template <int BM, int BN, int AM, int BMD, int TFA, int TFB, bool VEC, bool F16, int NT = 256, int ACT = 0, bool EMIT = false, int SD = 0>
__global__ void __launch_bounds__(NT, (persist_mode(AM, BMD, F16, TFA) || AM == M_PT || AM == M_KS) ? 2 : 1) koaf_gemm_kernel(const KoafGemm p) {
    static_assert(ACT == 0 || VEC, "bf16 activation storage needs the vector path");
    constexpr bool C16 = (ACT == 1), E16 = (ACT == 2);
    static_assert((TFA < 2 && TFB < 2) || VEC, "the two-source prologues need the vector path");
    constexpr int NPL = F16 ? 2 : 3;
    static_assert(BMD != M_PS || F16, "plane images are fp16");
    constexpr bool AS = (AM == M_KS);                // the streamed dense A operand: waves 4 x 1, each on its own 32 rows (StreamA)
    static_assert(!AS || (BM == 128 && NT == 256 && BMD == M_PS && F16 && VEC && ACT == 0 && (SD == 2 || SD == 4) && TFB == 0),
                  "the streamed A operand's one shape");
    constexpr int WGN = AS ? 1 : 2;
    constexpr int NW = NT / 64, WGM = NW / WGN;                      // waves: WGM along M x WGN along N
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr bool AKC = mode_is_kc(AM), BKC = mode_is_kc(BMD), BPS = (BMD == M_PS), APS = mode_is_pa(AM), AH = (AM == M_PH);
    constexpr bool AT = (AM == M_PT);                // 3x3 over plane images in 8 x 16 pixel tiles: halo in LDS, weight fragments in registers
    static_assert(!AT || (BM == 128 && BN == 64 && NT == 256 && BMD == M_PS && TFA == 0 && F16 && VEC), "the 2-D tile kernel's one shape");
    constexpr bool WPS = (AM == M_PK);               // weight gradient from plane images: both operands K-major by LDS-DMA
    static_assert(WPS == (BMD == M_PKG || BMD == M_PK), "K-major plane images come in pairs");
    static_assert(!(APS || AH || AT) || (BPS && TFA == 0), "a pre-split A pairs with a pre-split B and carries its transform in the image");
    static_assert(NT == 256 || AH, "only the halo kernel runs 512 threads (the fp32 loaders are laid out for 256)");
    static_assert(!AH || (BM == 256) == (NT == 512), "halo shapes: 256 rows x 512 threads, 128 rows x 256 threads");
    constexpr int HP_MAX = (BM + 2 * halo_max_w(BN, BM) + 2 + 15) / 16;  // 16-pixel (1 KiB) pieces of a halo plane
    constexpr bool HDB = (NT == 512);                // halo double-buffered across channel chunks (the 256-row shape)
    constexpr int A_PL = AH ? HP_MAX * 256 : ((APS || WPS) ? BM * 16 : plane_dwords(BM, AKC));
    constexpr int B_PL = (BPS || WPS) ? BN * 16 : plane_dwords(BN, BKC);
    constexpr int A_ELEMS = NPL * A_PL, B_ELEMS = NPL * B_PL;
    constexpr int NBA = (APS || (AH && HDB) || WPS) ? 2 : 1;                                  // LDS buffers per operand
    constexpr int NBB = AH ? halo_b_stages(BN, BM) : (AS ? 3 : ((BPS || WPS) ? 2 : 1));
    constexpr int LDC_S = BN + 4;                                    // epilogue staging row (floats)
    // the 256-row halo kernel multiplies in 16 x 16 x 32 MFMAs (the same FLOPs, LDS bytes and issue cycles as 32 x 32 x 16; the chip
    // clocks them higher under sustained load: scripts/mfma_shapes.hip, 1.12-1.14 x): its accumulators are NRB x NCB tiles of v4f
    constexpr bool M16 = (AM == M_PH) && (NT == 512);
    constexpr int NRB = M16 ? WM / 16 : 1, NCB = M16 ? WN / 16 : 1;
    constexpr int C_ELEMS = VEC ? BM * LDC_S : 0;
    constexpr int OPS = NBA * A_ELEMS + NBB * B_ELEMS;
    // M_PT: the epilogue's staging tile (which the two weight-tile stages of the k-loop share) and the halo image (180 pixels x 64
    // channels x two fp16 planes = 45 KiB) sit side by side: 80 960 B with the 64 B of block_amax_raise_bits -- two blocks per CU
    constexpr int T2D_HALO_BYTES = 2 * 180 * 128;
    constexpr int SMEM = AT ? (C_ELEMS + T2D_HALO_BYTES / 4) : ((OPS > C_ELEMS) ? OPS : C_ELEMS);
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    __shared__ __attribute__((aligned(16))) float s_tab[(AS && TFA == 1) ? 2 * STREAM_TAB_K : 4];     // M_KS, tf 1: see StreamA::tab

    KOAF_STAMP_DECL;
    KOAF_STAMP(0);
    const int ntn = (p.N + BN - 1) / BN;
    // Workgroups are dealt round-robin to the 8 XCDs (each with its own 4 MiB L2): without a remap the ntn blocks that
    // share an A row tile land on ntn different L2s and the tile is fetched from beyond L2 ntn times.  Bijective remap:
    // XCD x works through one contiguous chunk of the tile order, so a row tile's blocks follow each other on one L2.
    // PERSIST (fp32 A loader + weight tiles by DMA: the 1x1 and stride-2 convolutions, whose k-loops are 2-32 steps): the
    // block walks the tiles vt = blockIdx.x, + gridDim.x, ... (the host launches 2 blocks per CU) and issues the NEXT tile's
    // first A loads before the epilogue of the current one, so their HBM latency runs under the staging / stores instead
    // of in front of the next k-loop.  All other variants run their single tile through the same loop.
    constexpr bool PERSIST = persist_mode(AM, BMD, F16, TFA) || (AS && TFA < 2 && SD == 2);      // (M_KS with four k-tiles in flight: one tile per block)
    const unsigned ntx = (unsigned)((p.M - p.m_base + BM - 1) / BM) * (unsigned)ntn;     // tiles of one (split, batch) slice
    auto decode = [&](unsigned v, int& tm_, int& tn_) {
        const unsigned q = ntx >> 3, rem = ntx & 7, x = v & 7, j = v >> 3;
        const unsigned b = x * q + (x < rem ? x : rem) + j;
        tn_ = (int)(b % (unsigned)ntn);
        tm_ = (int)(b / (unsigned)ntn);
    };
    unsigned vt = blockIdx.x;
    unsigned bid = blockIdx.x;
    int split = blockIdx.y;
    if (gridDim.y > 1 && (gridDim.y & 7) == 0) {
        // Split-K (weight gradients): the tiles of ONE k-range read the same pixels of both operands, so they should share an
        // L2 -- left alone, the handful of tiles of a split are dealt to different XCDs and every one of them fetches its
        // operands from HBM again (a 3x3 weight gradient re-read its inputs 5-9 times).  Dispatch order is x-fastest:
        // XCD = linear id % 8; XCD x takes the splits = x (mod 8), all tiles of a split in consecutive slots.
        const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y, x = lin & 7, slot = lin >> 3;
        bid = slot % gridDim.x;
        split = (int)((slot / gridDim.x) * 8 + x);
    }
    int tn = bid % ntn, tm = bid / ntn;
    if (!(gridDim.y > 1 && (gridDim.y & 7) == 0)) decode(vt, tm, tn);
    int m0 = p.m_base + tm * BM, n0 = tn * BN;
    const int z0 = blockIdx.z / p.nb1, z1 = blockIdx.z - z0 * p.nb1;
    const int kchunk = (((p.K + p.splitk - 1) / p.splitk + BK - 1) / BK) * BK;
    const int kbeg = split * kchunk;
    const int kend = min(p.K, kbeg + kchunk);

    // operand scales of the fp16 scheme (powers of two; 1 otherwise): applied on load, divided out in the epilogue
    const float sca = F16 ? operand_scale(p.A) : 1.f;
    const float scb = F16 ? operand_scale(p.B) : 1.f;
    float alpha = F16 ? p.alpha / (sca * scb) : p.alpha;
    if constexpr (F16) {
        // a NaN / Inf anywhere in an operand reaches its amax scalar (the reductions propagate them, koaf_common.h); the pieces
        // themselves are clamped to the fp16 range, so the whole OUTPUT is made NaN here: a diverged run shows as one
        const bool bad = (p.A.amax && !koaf_bits_finite(koaf_absbits(*p.A.amax))) || (p.B.amax && !koaf_bits_finite(koaf_absbits(*p.B.amax)));
        if (bad) {
            alpha = __uint_as_float(0x7fc00000u);
            if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) koaf_status_add(p.status, 1, 1u);
        }
    }

    // (batch offsets count elements: a bf16 tensor behind a float-typed pointer advances by half the bytes)
    auto eoff = [](const float* q, int64_t elems, bool h16) { return h16 ? (const float*)((const unsigned short*)q + elems) : q + elems; };
    const float* Ap = (APS || AH || AT || WPS) ? nullptr : eoff(p.A.ptr, z0 * p.A.bs0 + z1 * p.A.bs1, ACT == 1);
    const unsigned short* Apl = (APS || AH || AT || WPS) ? p.A.planes + z0 * p.A.bs0 + z1 * p.A.bs1 : nullptr;
    const float* Bp = (BPS || WPS) ? nullptr : eoff(p.B.ptr, z0 * p.B.bs0 + z1 * p.B.bs1, ACT == 3);
    const unsigned short* Bpl = (BPS || WPS) ? p.B.planes + z0 * p.B.bs0 + z1 * p.B.bs1 : nullptr;

    // (the unused ones of the loaders are dead code to the compiler)
    TileLoader<(APS || AH || AT) ? 128 : BM, (APS || AH || AT || WPS || AS) ? M_KC : AM, AS ? 0 : TFA, VEC, F16, ACT == 1,
               ((ACT == 2 || ACT == 3) && TFA == 2) || (ACT == 1 && TFA == 3)> la;
    TileLoader<BN, (BPS || WPS) ? M_KC : BMD, TFB, VEC, F16, ACT == 3> lb;
    PlaneKLoader<WPS ? BM : 128, false> wka;
    PlaneKLoader<BN, BMD == M_PKG> wkb;
    PlaneLoader<BN> lp;
    PlaneGatherLoader<AH ? 128 : BM, AM == M_PA2 ? 2 : 1> lpa;
    StreamA<AS ? TFA : 0, AS ? SD : 2> st;
    if constexpr (AS) {
        // (set up below, once the first tile is known)
    } else if constexpr (WPS) {
        wka.init(p.A, m0, p.M);
        wka.seek(p.A, kbeg);
        wkb.init(p.B, n0, p.N);
        wkb.seek(p.B, kbeg);
    } else if constexpr (APS) {
        lpa.init(p.A, m0, p.M);
        lpa.seek(p.A, kbeg);
    } else if constexpr (!AH && !AT) {
        la.init(p.A, m0, p.M, z1, sca);
        la.seek(p.A, kbeg);
    }
    if constexpr (AH || AT || WPS) {
        // (the halo loop below addresses both operands itself; the K-major pair was set up above)
    } else if constexpr (BPS) {
        lp.init(p.B, n0, p.N);
        lp.seek(p.B, kbeg);
    } else {
        lb.init(p.B, n0, p.N, z1, scb);
        lb.seek(p.B, kbeg);
    }

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wm = w / WGN, wn = w % WGN;
    const int r = lane & 31, h = lane >> 5;
    if constexpr (PERSIST && !AS) {
        if (kbeg < kend) la.issue(la.sa, p.A, Ap, kbeg, kend, z1);      // the first tile's A loads
    }
    // M_KS: the tile after this one (the cursor of the A stream crosses into it SD k-steps before this tile's k-loop ends)
    [[maybe_unused]] bool s_has_next = false;
    [[maybe_unused]] int s_tm2 = 0, s_tn2 = 0, s_m0n = -1;
    auto stream_next = [&]() {
        s_has_next = PERSIST && (vt + gridDim.x) < ntx;
        s_m0n = -1;
        if (s_has_next) { decode(vt + gridDim.x, s_tm2, s_tn2); s_m0n = p.m_base + s_tm2 * BM; }
    };
    [[maybe_unused]] unsigned c_vt = blockIdx.x;      // the tile the A stream's cursor is on
    auto cursor_next = [&]() -> int {
        if (!PERSIST || c_vt + gridDim.x >= ntx) return -1;
        c_vt += gridDim.x;
        int a, b;
        decode(c_vt, a, b);
        return p.m_base + a * BM;
    };
    if constexpr (AS) {
        st.init(p.A, Ap, m0, p.M, kbeg, kend, sca);
        st.once = (ntn == 1);
        if constexpr (TFA == 1) {
            for (int k = t; k < kend - kbeg; k += NT) { s_tab[k] = p.A.sc[kbeg + k] * sca; s_tab[STREAM_TAB_K + k] = p.A.sh[kbeg + k] * sca; }
            st.tab = s_tab;
            __syncthreads();
        }
        stream_next();
#pragma unroll
        for (int d = 0; d < SD; ++d) st.issue(st.sl[d], cursor_next, p.M);      // the first SD k-tiles of this block's first tile
    }
    for (;;) {      // the tiles of this block (one, unless PERSIST)
    KOAF_STAMP(0);
    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    [[maybe_unused]] v4f acc16[NRB][NCB];
#pragma unroll
    for (int i = 0; i < NRB; ++i)
#pragma unroll
        for (int j = 0; j < NCB; ++j) acc16[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};

    float* const Bs0 = smem + NBA * A_ELEMS;
    const unsigned sm0 = KOAF_LDS_ADDR(smem), sb0 = sm0 + NBA * A_ELEMS * 4;     // LDS byte addresses of the A / B buffers
    [[maybe_unused]] int t2d_base = 0, t2d_w = 0;                               // M_PT: first pixel of the tile's rectangle, image row pitch
    // the MFMAs of one k-tile whose plane images sit at Au / Bu
    auto mma = [&](const unsigned* Au, const unsigned* Bu) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            v4i ap[TM][NPL], bp[NPL];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    if constexpr (APS) ap[i][q] = frag_load_ps(Au + q * A_PL, wm * WM + 32 * i, g, lane);
                    else if constexpr (WPS) ap[i][q] = frag_load_kmd<BM>(Au + q * A_PL, wm * WM + 32 * i, g, lane);
                    else ap[i][q] = frag_load<BM, AKC>(Au + q * A_PL, wm * WM + 32 * i, g, lane);
                }
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    if constexpr (BPS) bp[q] = frag_load_ps(Bu + q * B_PL, wn * WN + 32 * jn, g, lane);
                    else if constexpr (WPS) bp[q] = frag_load_kmd<BN>(Bu + q * B_PL, wn * WN + 32 * jn, g, lane);
                    else bp[q] = frag_load<BN, BKC>(Bu + q * B_PL, wn * WN + 32 * jn, g, lane);
                }
                // piece products, smallest first.  bf16: the six of weight >= 2^-16.  fp16: lo*hi, hi*lo, hi*hi.
                constexpr int NTERM = F16 ? 3 : 6;
                constexpr int PA3[6] = {2, 0, 1, 1, 0, 0}, PB3[6] = {0, 2, 1, 0, 1, 0};
                constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};
#pragma unroll
                for (int term = 0; term < NTERM; ++term) {
                    const int pa = F16 ? PAH[term] : PA3[term];
                    const int pb = F16 ? PBH[term] : PB3[term];
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        if constexpr (F16)
                            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, ap[i][pa]),
                                                                                __builtin_bit_cast(h16x8, bp[pb]),
                                                                                acc[i][jn], 0, 0, 0);
                        else
                            acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[i][pa]),
                                                                                 __builtin_bit_cast(bf16x8, bp[pb]),
                                                                                 acc[i][jn], 0, 0, 0);
                    }
                }
            }
        }
    };
    if constexpr (AH) {
        // 3x3 / stride 1 / pad 1 over activation plane images, both operands by LDS-DMA.  The tile's BM output pixels are
        // consecutive in raster order, so the source pixels of ALL nine taps lie in the contiguous range
        // [m0 - W - 1, m0 + BM + W + 1): that halo (32 channels of it) is fetched ONCE per channel chunk and tap (dy, dx)
        // is the same LDS image read W*dy + dx pixels further on -- the input tile travels L2 -> LDS 1.8 times instead of
        // nine.  Taps that fall off the image (the raster neighbour is then another row or image) are zeroed in the
        // fragment registers by per-row validity bits.  k runs (chunk, tap, channel); the weight tile of every (chunk, tap)
        // step is double-buffered as in the loops above, the next chunk's halo arrives in ninths under the nine tap steps.
        static_assert(!HDB || 2 * HP_MAX <= 14 * NW, "the next halo is spread over seven tap steps, at most two pieces per wave and step");
        constexpr int NPB = BN / 16;                        // 1-KiB pieces of a weight plane tile
        constexpr int BPW = (2 * NPB + NW - 1) / NW;        // weight pieces per wave and step
        const int Wd = p.A.W, Hd = p.A.H, CSa = p.A.CS, Ca = p.A.C;
        const bool flip = p.A.gather == 2;
        const int np2 = 2 * ((BM + 2 * Wd + 2 + 15) >> 4);  // halo pieces per chunk (two planes)
        const int64_t hbase = (int64_t)m0 - Wd - 1, plast = (int64_t)p.M - 1;
        const int nchunk = Ca / 32;
        const int swz = 8 * ((lane & 3) ^ ((lane >> 4) & 3));
        // validity bits of the nine taps (bit kh*3+kw) and halo pixel of the centre tap for this lane's row of each M tile
        constexpr int NVB = HDB ? WM / 16 : TM;             // row blocks of a wave: 16 rows (256-row shape: 16 x 16 x 32 MFMAs) or 32
        unsigned vb[NVB];
        int i0[NVB];
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int lrow = HDB ? wm * WM + 16 * i + (lane & 15) : wm * WM + 32 * i + r, row = m0 + lrow;
            i0[i] = lrow + Wd + 1;
            vb[i] = 0;
            if (row < p.M) {
                const int rem = row % (Hd * Wd), y = rem / Wd, x = rem - y * Wd;
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const int dy = flip ? 1 - tp / 3 : tp / 3 - 1, dx = flip ? 1 - tp % 3 : tp % 3 - 1;
                    const bool ok = (unsigned)(y + dy) < (unsigned)Hd && (unsigned)(x + dx) < (unsigned)Wd;
                    vb[i] |= (ok ? 1u : 0u) << tp;
                }
            }
        }
        int64_t bsrc[BPW];
#pragma unroll
        for (int j = 0; j < BPW; ++j) {
            const int idx = w + NW * j, piece = idx % NPB;
            const int row = min(n0 + 16 * piece + (lane >> 2), p.N - 1);     // (rows past N: finite values, never stored)
            bsrc[j] = (int64_t)(idx / NPB) * p.B.plane_stride + (int64_t)row * p.B.ld + swz;
        }
        auto issue_halo = [&](int idx, int chunk, unsigned buf) {
            const int piece = idx >> 1, q = idx & 1;
            int64_t gp = hbase + 16 * piece + (lane >> 2);
            gp = gp < 0 ? 0 : (gp > plast ? plast : gp);       // (pixels off the tensor are never valid taps)
            const unsigned short* src = Apl + q * p.A.plane_stride + gp * CSa + (chunk * 32 + swz);
            lds_dma16(src, buf + q * (A_PL * 4) + piece * 1024);
        };
        auto issue_b = [&](int tap, int chunk, unsigned buf) {
            const int koff = tap * Ca + chunk * 32;
#pragma unroll
            for (int j = 0; j < BPW; ++j) {
                const int idx = w + NW * j;
                if (idx < 2 * NPB)
                    lds_dma16(Bpl + bsrc[j] + koff, buf + (idx / NPB) * (B_PL * 4) + (idx % NPB) * 1024);
            }
        };
        if constexpr (HDB) {
        // 256-row shape.  Software pipeline over the steps s = (chunk, tap):
        //   * weight tiles: three LDS stages; tile s + 3 is issued at step s into the stage tile s leaves;
        //   * fragments: the registers of step s + 1 are read from LDS DURING the MFMAs of step s (two register sets,
        //     ping-pong), so the matrix pipe never waits for an LDS read burst -- with one barrier per step all eight waves
        //     used to read, then multiply, in lockstep, and the k-loop ran at half the matrix rate;
        //   * the next chunk's halo arrives under taps 0..6 of the current chunk (its first fragments are read at tap 8);
        //   * waits are counted (loads retire in order): barrier(s) needs tile s + 1, issued two steps earlier, and lets
        //     everything issued since stay in flight -- no drain at chunk boundaries.
        static_assert(NBB == 3, "three weight-tile stages");
        typedef const __attribute__((address_space(3))) v4i* lds_v4i;
        typedef const __attribute__((address_space(3))) unsigned* lds_u;
        constexpr int NST = 7;                              // taps that carry pieces of the next halo
        const int nh = (np2 + NW - 1) / NW;                 // halo pieces per wave and chunk
        const int hq = nh / NST, hr = nh - hq * NST;        // pieces at tap t < NST: hq + (t < hr)   (<= 2: np2 <= 14 NW)
        const int nstep = 9 * nchunk;
        // fragments of one step (32 channels of one tap) for 16 x 16 x 32 MFMAs: lane (r = l % 16, c = l / 16) holds k = 8 c .. 8 c + 7 of
        // row r of its block -- 16-B chunk c of the pixel / weight row, one read per block and plane
        struct Frags { v4i a[NRB][2]; v4i b[NCB][2]; };
        const int q4 = lane >> 4;
        // (shift: the tap's pixel offset in the halo, (kh - 1) W + (kw - 1), negated for the data gradient's flipped filter -- carried
        // by the loop, not derived from the tap)
        auto load_frags = [&](Frags& f, int shift, int hbuf, int stage) {
            const lds_u Ah = (lds_u)smem + hbuf * A_ELEMS;
            const lds_u Bu = (lds_u)smem + NBA * A_ELEMS + stage * B_ELEMS;
#pragma unroll
            for (int i = 0; i < NRB; ++i) {
                const int hp = i0[i] + shift;
                const int off = hp * 16 + 4 * (q4 ^ ((hp >> 2) & 3));
#pragma unroll
                for (int q = 0; q < 2; ++q) f.a[i][q] = *(lds_v4i)&Ah[q * A_PL + off];
            }
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                const int brow = wn * WN + 16 * j + (lane & 15);
#pragma unroll
                for (int q = 0; q < 2; ++q) f.b[j][q] = *(lds_v4i)&Bu[q * B_PL + brow * 16 + 4 * (q4 ^ ((brow >> 2) & 3))];
            }
        };
        for (int idx = w; idx < np2; idx += NW) issue_halo(idx, 0, sm0);
#pragma unroll
        for (int d = 0; d < 3; ++d) issue_b(d, 0, sb0 + d * (B_ELEMS * 4));       // (nstep >= 9)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * BPW) : "memory");             // halo 0 and tile 0 have landed
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        KOAF_STAMP(1);
        Frags F0, F1;
        const int shift0 = flip ? Wd + 1 : -Wd - 1, dshift = flip ? -1 : 1, rshift = flip ? 2 - Wd : Wd - 2;     // tap 0; to the next tap in a row / to the next row
        load_frags(F0, shift0, 0, 0);
        int nshift = shift0, nkw = 0;       // of tap + 1 (advanced below)
        int tap = 0, chunk = 0, sb = 0;     // this step; sb = stage of its weight tile
        int itap = 3, ich = 0;              // (tap, chunk) of tile s + 3
        int hk = 0, hprev = 0;              // halo pieces of the next chunk issued so far / loads per wave at the previous step
        [[maybe_unused]] unsigned long long kst_hw = 0, kst_hv = 0;
        // this wave's halo pieces inside the loop: slot hk of a chunk is piece 4 hk + w / 2 of plane w % 2 (idx = 8 hk + w above), so the
        // plane, the lane's pixel offset and its 64-bit base are per-tile constants and a piece costs a clamp and one multiply-add
        // (slots past the last piece repeat it)
        const int ws = __builtin_amdgcn_readfirstlane(w);
        const int h_npp = np2 >> 1, h_p0 = ws >> 1;
        const int h_px = (int)hbase + (lane >> 2), h_last = (int)plast;
        const unsigned short* const h_src = Apl + (ws & 1) * p.A.plane_stride + swz;
        const unsigned h_dst = (ws & 1) * (A_PL * 4);
        auto issue_halo_w = [&](int k, int chunk, unsigned buf) {
            const int piece = min(4 * k + h_p0, h_npp - 1);
            const int gp = min(max(h_px + 16 * piece, 0), h_last);
            lds_dma16(h_src + ((int64_t)gp * CSa + chunk * 32), buf + h_dst + piece * 1024);
        };
        auto vm_wait = [&](int h) {
            if (h == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BPW) : "memory");
            else if (h == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BPW + 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BPW + 2) : "memory");
        };
        auto lgkm0_barrier = [&]() {
            // (the wait is the BUILTIN: hipcc's wait-count pass does not read inline assembly and would take the fragment registers
            // of step s for still in flight at their MFMAs)
            __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
            asm volatile("s_barrier" ::: "memory");
        };
        // One step = four (two: 64 columns) groups of twelve MFMAs (one 16-column block), each followed by a piece of everything else (the
        // fragment reads of step s + 1, the two halo pieces, the weight tile), pinned by scheduling barriers: a wave issues in
        // order, and the address arithmetic in one block in front of 24 back-to-back MFMAs ran with the matrix pipe idle in both
        // waves of the SIMD (the step barrier keeps them in lockstep).
        auto mask_all = [&](Frags& f) {       // (in place: the set is dead after its step)
#pragma unroll
            for (int i = 0; i < NRB; ++i) {
                const int okm = -(int)((vb[i] >> tap) & 1u);       // all ones / zero: the tap's validity as an AND mask
#pragma unroll
                for (int q = 0; q < 2; ++q) f.a[i][q] = and_mask(f.a[i][q], okm);
            }
        };
        auto mma_col = [&](Frags& f, int j) {      // column block j: 3 NRB MFMAs
            constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < NRB; ++i)
                    acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, f.a[i][PAH[term]]),
                                                                          __builtin_bit_cast(h16x8, f.b[j][PBH[term]]), acc16[i][j], 0, 0, 0);
        };
        constexpr int NQ = NCB;             // MFMA groups of a step
        static_assert(NQ == 4 || NQ == 2, "the four pieces follow the MFMA groups in ones or twos");
        auto body = [&](Frags& cur, Frags& nxt) {
            [[maybe_unused]] const unsigned long long tw0 = KOAF_STAMP_NOW();
            // tile s + 1 (issued at step s - 2, the last loads of that step) has landed; what step s - 1 issued stays in flight
            vm_wait(hprev);
            lgkm0_barrier();
            [[maybe_unused]] const unsigned long long tw1 = KOAF_STAMP_NOW();
            const bool more_chunks = chunk + 1 < nchunk;
            const int hc = (more_chunks && tap < NST) ? hq + (tap < hr ? 1 : 0) : 0;
            const unsigned Anext = sm0 + ((chunk + 1) & 1) * (A_ELEMS * 4);
            hprev = hc;
            int ntap = tap + 1, nch2 = chunk;
            if (++nkw == 3) { nkw = 0; nshift += rshift; } else nshift += dshift;
            if (ntap == 9) { ntap = 0; ++nch2; nshift = shift0; }
            int sbn = sb + 1;
            if (sbn == 3) sbn = 0;
            auto piece = [&](int f) {
                __builtin_amdgcn_sched_barrier(0);
                // (past the last step the reads fetch a stage / halo nobody uses: unconditional, so that the two register sets stay two)
                if (f == 0) load_frags(nxt, nshift, nch2 & 1, sbn);
                if (f == 1 && hc > 0) { issue_halo_w(hk, chunk + 1, Anext); ++hk; }
                if (f == 2 && hc > 1) { issue_halo_w(hk, chunk + 1, Anext); ++hk; }
                // tile s + 3 into the stage tile s leaves (past the end: re-fetch the last tile there -- nobody reads it, the counts stay uniform)
                if (f == 3) issue_b(ich < nchunk ? itap : 8, ich < nchunk ? ich : nchunk - 1, sb0 + sb * (B_ELEMS * 4));
                __builtin_amdgcn_sched_barrier(0);
            };
#pragma unroll
            for (int m = 0; m < NQ; ++m) {
                if (m == 0) mask_all(cur);
                mma_col(cur, m);
#pragma unroll
                for (int f = m * (4 / NQ); f < (m + 1) * (4 / NQ); ++f) piece(f);
            }
            if (++itap == 9) { itap = 0; ++ich; }
            if (ntap == 0) hk = 0;
            sb = sbn;
            [[maybe_unused]] const unsigned long long tw2 = KOAF_STAMP_NOW();
            kst_hv += tw1 - tw0;
            kst_hw += tw2 - tw1;
            tap = ntap; chunk = nch2;
        };
#pragma unroll 1
        for (int s2 = 0; s2 + 1 < nstep; s2 += 2) {
            body(F0, F1);
            body(F1, F0);
        }
        if (nstep & 1) body(F0, F1);
        KOAF_STAMP_ACC(5, kst_hv);
        KOAF_STAMP_ACC(6, kst_hw);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the surplus fetches behind the last step)
        __syncthreads();       // the epilogue reuses the operand buffers
        } else {
        // Pipeline: the weight tile of step s + D (D = NBB - 1 steps ahead) and one halo piece of the NEXT chunk are issued
        // at step s; loads retire in order, so "the tile of step s has landed" is a counted wait that leaves the younger
        // loads in flight.  Only the first tap of a chunk drains everything (its halo was completed by the previous step).
        constexpr int D = NBB - 1;
        auto step_of = [&](int sidx, int& tp, int& ch) { ch = sidx / 9; tp = sidx - 9 * ch; };
        const int nstep = 9 * nchunk;
        for (int idx = w; idx < np2; idx += NW) issue_halo(idx, 0, sm0);
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d < nstep) { int tp, ch; step_of(d, tp, ch); issue_b(tp, ch, sb0 + d * (B_ELEMS * 4)); }
        int sb = 0;                 // stage holding the current step's weight tile
        int ntap = D % 9, nch = D / 9;     // (tap, chunk) of step s + D
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            // (LDS pointers typed as such: left generic, hipcc could not always prove the address space of these reads)
            typedef const __attribute__((address_space(3))) v4i* lds_v4i;
            typedef const __attribute__((address_space(3))) unsigned* lds_u;
            const lds_u Ah = (lds_u)smem + (HDB ? (chunk & 1) : 0) * A_ELEMS;
            const unsigned Anext = sm0 + (HDB ? ((chunk + 1) & 1) : 0) * (A_ELEMS * 4);
            const bool more_chunks = chunk + 1 < nchunk;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                // in flight behind this step's tile: D - 1 younger tiles (BPW loads each) and, inside a chunk, D halo pieces
                if (tap == 0) {
                    KOAF_STAMP(4);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                else if (HDB && more_chunks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * BPW + (D < 9 ? D : 9)) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * BPW) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (tap == 0) {
                    KOAF_STAMP(5);
                    KOAF_STAMP_ADD(5, 4, 5);          // exposed wait for a chunk's halo (+ barrier skew)
                    if (chunk == 0) KOAF_STAMP(1);
                }
                {
                    int sd = sb + D;
                    if (sd >= NBB) sd -= NBB;
                    // (past the last step: re-fetch the last tile into a stage nobody reads, which keeps the counts uniform)
                    issue_b(nch < nchunk ? ntap : 8, nch < nchunk ? nch : nchunk - 1, sb0 + sd * (B_ELEMS * 4));
                    if (++ntap == 9) { ntap = 0; ++nch; }
                }
                if (HDB && more_chunks) {
                    const int idx = tap * NW + w;
                    issue_halo(idx < np2 ? idx : np2 - 1, chunk + 1, Anext);    // (surplus slots repeat the last piece)
                }
                const int kh = tap / 3, kw = tap - 3 * kh;
                const int shift = flip ? (1 - kh) * Wd + (1 - kw) : (kh - 1) * Wd + (kw - 1);
                const lds_u Bu = (lds_u)smem + NBA * A_ELEMS + sb * B_ELEMS;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    v4i ap[TM][2], bp[2];
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int hp = i0[i] + shift;
                        const int okm = -(int)((vb[i] >> tap) & 1u);       // all ones / zero: the tap's validity as an AND mask
                        const int off = hp * 16 + 4 * ((2 * g + h) ^ ((hp >> 2) & 3));
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const v4i v = *(lds_v4i)&Ah[q * A_PL + off];
                            ap[i][q] = and_mask(v, okm);
                        }
                    }
#pragma unroll
                    for (int jn = 0; jn < TN; ++jn) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int brow = wn * WN + 32 * jn + (lane & 31);
                            bp[q] = *(lds_v4i)&Bu[q * B_PL + brow * 16 + 4 * ((2 * g + h) ^ ((brow >> 2) & 3))];   // = frag_load_ps
                        }
                        constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};
#pragma unroll
                        for (int term = 0; term < 3; ++term)
#pragma unroll
                            for (int i = 0; i < TM; ++i)
                                acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, ap[i][PAH[term]]),
                                                                                    __builtin_bit_cast(h16x8, bp[PBH[term]]),
                                                                                    acc[i][jn], 0, 0, 0);
                    }
                }
                if (++sb == NBB) sb = 0;
            }
            if (!HDB && more_chunks) {
                // one halo buffer: every wave is done with this chunk, then the next one is fetched whole (the first tap of
                // the next chunk waits for it; the CU's other block computes meanwhile)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                for (int idx = w; idx < np2; idx += NW) issue_halo(idx, chunk + 1, Anext);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the surplus fetches behind the last step)
        __syncthreads();       // the epilogue reuses the operand buffers
        }
    } else if constexpr (AT) {
        // 3x3 / stride 1 / pad 1 over activation plane images, 8 x 16 pixel tiles of ONE image (H % 8 == 0, W % 16 == 0).
        //   * Halo: the 10 x 18 source pixels of the tile, 64 channels at a time, both fp16 planes, are fetched ONCE by LDS-DMA;
        //     pixels outside the image fetch the zero chunk, so the k-loop needs no validity masks.  A raster tile of 128 pixels
        //     (M_PH) needs 128 + 2 W + 2 halo pixels -- 2.5 tiles' worth at W = 96; the rectangle needs 1.4 -- and that is what
        //     lets a 64-channel halo AND two blocks share a CU: one step = one filter tap over all 64 channels = 24 MFMAs per
        //     wave (M_PH, 128 rows: 12 per barrier).
        //   * LDS image: granule (16 B = 8 channels) c of halo pixel (y, x) at ((18 y + x) * 8 + (c ^ (x / 2 % 8))) * 16: the 16 lanes
        //     of a ds_read_b128 group hold x = x0 + {0..3, 12..15} of one tile row and x0 + {4..11} of the next, i.e. every
        //     residue mod 16 once -- (x % 2, x / 2 % 8) are 16 distinct (bank half, 16-B slot) pairs: conflict-free.  The DMA
        //     writes lane-linear, so the permutation is applied to the per-lane SOURCE address.
        //   * Weights: the 64 x 64 tile of one (tap, chunk) step by LDS-DMA, double-buffered INSIDE the epilogue's staging region
        //     (the two never live at the same time), one barrier per step.  (Loading the fragments straight into registers --
        //     no barrier at all -- was measured first: 64 KB per step and CU through the vector memory path in 32-B segments
        //     was the limiter, 245 TFLOP/s.)
        //   * k runs (chunk of 64 channels, tap, channel); C = 128 reloads the halo once (two barriers).
        typedef const __attribute__((address_space(3))) v4i* lds_v4i;
        typedef const __attribute__((address_space(3))) char* lds_c;
        const int Wd = p.A.W, Hd = p.A.H, CSa = p.A.CS, Ca = p.A.C;
        const bool flip = p.A.gather == 2;
        const int txn = Wd >> 4, tpi = (Hd >> 3) * txn;          // tiles per image row / per image
        const int img = tm / tpi, trem = tm - img * tpi, tyi = trem / txn, txi = trem - tyi * txn;
        const int nchunk = Ca >> 6;
        const unsigned halo0 = KOAF_LDS_ADDR(smem) + C_ELEMS * 4;
        t2d_base = (img * Hd + tyi * 8) * Wd + txi * 16;
        t2d_w = Wd;
        // this lane's rows of the two M tiles: pixel (ly, lx) of the tile; halo pixel of tap (ky, kx) = (ly + ky, lx + kx)
        const int lx = r & 15;
        int hp0[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) hp0[i] = (4 * wm + 2 * i + (r >> 4)) * 18 + lx;
        // weight tile of one step: 64 output channels x 64 k x two planes = 16 KiB = 16 DMA pieces, four per wave; granule c of row
        // `row` at (row * 8 + (c ^ (row / 2 % 8))) * 16 (the halo image's conflict-free pattern); two stages in the staging region
        const unsigned bst0 = KOAF_LDS_ADDR(smem);
        int64_t bsrc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int G = (w + 4 * j) * 64 + lane, q = G >> 9, Gp = G & 511, row = Gp >> 3, cs = Gp & 7;
            const int brow = min(n0 + row, p.N - 1);                // (rows past N: finite values, never stored)
            bsrc[j] = (int64_t)q * p.B.plane_stride + (int64_t)brow * p.B.ld + 8 * (cs ^ ((row >> 1) & 7));
        }
        auto issue_b = [&](int tap, int chunk, int stage) {
            const int koff = tap * Ca + chunk * 64;
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_dma16(Bpl + bsrc[j] + koff, bst0 + stage * 16384 + (w + 4 * j) * 1024);
        };
        // fragments of k-group g of filter tap `tap`: A of both M tiles, B of this wave's 32 columns, both planes
        struct FR { v4i a[TM][2]; v4i b[2]; };
        const int browl = wn * WN + r, bsw = (browl >> 1) & 7;
        auto read_f = [&](FR& f, int tap, int g, int stage) {
            const int kh = tap / 3, kw = tap - 3 * kh;
            const int ky = flip ? 2 - kh : kh, kx = flip ? 2 - kw : kw;
            const int sw = ((lx + kx) >> 1) & 7;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const unsigned off = (unsigned)((hp0[i] + ky * 18 + kx) * 128 + (((2 * g + h) ^ sw) << 4));
#pragma unroll
                for (int q = 0; q < 2; ++q) f.a[i][q] = *(lds_v4i)((lds_c)smem + (C_ELEMS * 4 + q * 23040) + off);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
                f.b[q] = *(lds_v4i)((lds_c)smem + (stage * 16384 + q * 8192 + browl * 128 + (((2 * g + h) ^ bsw) << 4)));
        };
        auto mma_g = [&](const FR& f) {
            constexpr int PAH[3] = {1, 0, 0}, PBH[3] = {0, 1, 0};
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, f.a[i][PAH[term]]),
                                                                        __builtin_bit_cast(h16x8, f.b[PBH[term]]),
                                                                        acc[i][0], 0, 0, 0);
        };
        static_assert(TM == 2 && TN == 1 && C_ELEMS * 4 >= 2 * 16384, "2 x 2 waves of 64 x 32; two weight stages inside the staging region");
        FR R0, R1;
        t2d_issue_halo(p.A, Apl, tm, 0, halo0);
        issue_b(0, 0, 0);
        const int nstep = 9 * nchunk;
        int tap = 0, chunk = 0;
        // One step = one filter tap over 64 channels = four k-groups of 6 MFMAs per wave, one barrier.  Pinned with scheduling
        // barriers (left alone, hipcc sinks every LDS read to just in front of its first use): the fragments of k-group g + 1
        // are read while group g is multiplied; the next step's weight tile lands under this step's MFMAs.
#pragma unroll 1
        for (int s_ = 0; s_ < nstep; ++s_) {
            const int stage = s_ & 1;
            int ntap = tap + 1, nch = chunk;
            if (ntap == 9) { ntap = 0; ++nch; }
            const bool has_next = s_ + 1 < nstep;
            // this step's weight tile (and, at s = 0, the halo) has landed; every wave is done with the other stage
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (s_ == 0) KOAF_STAMP(1);
            if (has_next && ntap != 0) issue_b(ntap, nch, stage ^ 1);
            read_f(R0, tap, 0, stage);
            __builtin_amdgcn_sched_barrier(0);
            read_f(R1, tap, 1, stage);
            __builtin_amdgcn_sched_barrier(0);
            mma_g(R0);
            __builtin_amdgcn_sched_barrier(0);
            read_f(R0, tap, 2, stage);
            __builtin_amdgcn_sched_barrier(0);
            mma_g(R1);
            __builtin_amdgcn_sched_barrier(0);
            read_f(R1, tap, 3, stage);
            __builtin_amdgcn_sched_barrier(0);
            mma_g(R0);
            __builtin_amdgcn_sched_barrier(0);
            mma_g(R1);
            __builtin_amdgcn_sched_barrier(0);
            if (has_next && ntap == 0) {
                // next 64 channels: every wave is done with this halo, then it is replaced together with the first weight tile
                // (the CU's other block computes meanwhile)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                t2d_issue_halo(p.A, Apl, tm, nch, halo0);
                issue_b(0, nch, stage ^ 1);
            }
            tap = ntap; chunk = nch;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();       // the epilogue's staging tile covers the weight stages
    } else if constexpr (AS) {
        // Streamed A (StreamA) x weight plane images by LDS-DMA through a three-stage ring.  Step s of the tile, per wave:
        //   consume A(s) -- the registers issued SD steps ago: transform, split, this wave's rows of the A image; wait for this
        //   wave's pieces of B(s) (issued at step s - 2: counted, what was issued since stays in flight) and meet the other waves:
        //   B(s) is complete and nobody still reads the stage of step s - 1, which B(s + 2) now overwrites; issue B(s + 2), then
        //   A(s + SD) into the registers A(s) left; fragments + MFMAs.
        // The A loads are ordinary loads (the compiler keeps their registers and waits for them itself); the LDS-DMA is inline
        // assembly it does not see, so its wait for A(s) also retires the (SD - 1) NB oldest operations issued after A(s) -- in this
        // order those are B(s - SD + 3), A(s + 1), B(s - SD + 4) ...: tiles already needed or needed next.  The manual waits
        // count only loads that are certainly issued (NLA data loads per A tile: coefficient loads and side stores make the true
        // count larger, which errs towards waiting longer).
        // (Measured and dropped: the transform + split of A(s + 1) cut into quarters between the MFMAs of step s -- pinned with
        // scheduling barriers, since hipcc otherwise puts every vector instruction behind the last MFMA -- was slower than this
        // order on every layer, 2002 against 1977 ms per step.)
        constexpr int NLA = (TFA == 2 || TFA == 3) ? 8 : 4;
        constexpr int NB = 2 * (BN / 64);                   // LDS-DMA instructions per wave and weight tile (two planes)
        const int nstep = (kend - kbeg) / BK;               // host: a multiple of SD
        unsigned* const Aim = (unsigned*)smem;
        float* const side = (TFA == 3 && n0 == 0) ? p.A.side : nullptr;
        lp.template issue<NPL>(p.B, Bpl, sb0);
        if (nstep > 1) lp.template issue<NPL>(p.B, Bpl, sb0 + (B_ELEMS * 4));
        // "at most n vector-memory operations of this wave still in flight", rounded down to an immediate of the ladder, + barrier
        auto wait_barrier = [&](int n) {
            if (n >= 2 * NLA + NB) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * NLA + NB) : "memory");
            else if (n >= 2 * NLA) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * NLA) : "memory");
            else if (n >= NLA + NB) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NLA + NB) : "memory");
            else if (n >= NLA) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NLA) : "memory");
            else if (n >= NB) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NB) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        };
        // does step j issue an A tile?  (its target k-tile exists: later in this tile, or in the next tile of a persistent block)
        auto issues = [&](int j) { return j >= 0 && (j + SD < nstep || s_m0n >= 0); };
        int bst = 0;
        KOAF_STAMP(1);
        [[maybe_unused]] unsigned long long kst_c = 0, kst_w = 0;      // (stamps build: time in consume() incl. the wait for A; in the B wait + barrier)
        // one step; ISSUE: it fetches an A tile (compile-time: the steps that do and the steps that do not sit in two loops, because a
        // load issued on one path only makes hipcc count its waits for the path WITHOUT it -- every wait for A then retires nearly
        // everything in flight)
        auto sstep = [&](auto D, auto ISSUE, int ss) {
            constexpr int d = decltype(D)::value;
            [[maybe_unused]] const unsigned long long ta0 = KOAF_STAMP_NOW();
            st.consume(st.sl[d], Aim, kbeg + ss * BK, side);
            [[maybe_unused]] const unsigned long long ta1 = KOAF_STAMP_NOW();
            // younger than B(ss): the A tiles of steps ss - 2 and ss - 1, B(ss + 1)
            wait_barrier((issues(ss - 2) ? NLA : 0) + (issues(ss - 1) ? NLA : 0) + ((ss + 1 < nstep) ? NB : 0));
            kst_c += ta1 - ta0;
            kst_w += KOAF_STAMP_NOW() - ta1;
            if (ss + 2 < nstep) {
                int b2 = bst + 2;
                if (b2 >= 3) b2 -= 3;
                lp.template issue<NPL>(p.B, Bpl, sb0 + b2 * (B_ELEMS * 4));
            }
            if constexpr (decltype(ISSUE)::value) st.issue(st.sl[d], cursor_next, p.M);
            mma(Aim, (const unsigned*)(Bs0 + bst * B_ELEMS));
            if (++bst == 3) bst = 0;
        };
        static_assert(SD == 0 || SD == 2, "two steps per group");
        const int nmain = (s_m0n >= 0) ? nstep : nstep - SD;        // the steps that issue (all of them when a next tile follows)
        int s0 = 0;
#pragma unroll 1
        for (; s0 < nmain; s0 += SD) {
            sstep(std::integral_constant<int, 0>{}, std::true_type{}, s0);
            sstep(std::integral_constant<int, 1>{}, std::true_type{}, s0 + 1);
        }
        if (s0 < nstep) {
            sstep(std::integral_constant<int, 0>{}, std::false_type{}, s0);
            sstep(std::integral_constant<int, 1>{}, std::false_type{}, s0 + 1);
        }
        // every wave is done with the operand images (the epilogue's staging tile covers them); the next tile's A stays in flight
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        KOAF_STAMP_ACC(5, kst_w);
        KOAF_STAMP_ACC(6, kst_c);
        if constexpr (TFA == 1 || TFA == 3) {
            if (((st.satmax & 0xffffu) >= 0x7bffu) | ((st.satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
            st.satmax = 0u;
        }
    } else if constexpr (WPS) {
        // weight gradient: both K-major operands by LDS-DMA, double-buffered, one barrier per k-tile (as below)
        if (kbeg < kend) {
            wka.issue(p.A, Apl, kbeg, kend, sm0);
            wkb.issue(p.B, Bpl, kbeg, kend, sb0);
        }
        int cur = 0;
        KOAF_STAMP(1);
        for (int k0 = kbeg; k0 < kend; k0 += BK) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if ((k0 + BK) < kend) {
                wka.issue(p.A, Apl, k0 + BK, kend, sm0 + (cur ^ 1) * (A_ELEMS * 4));
                wkb.issue(p.B, Bpl, k0 + BK, kend, sb0 + (cur ^ 1) * (B_ELEMS * 4));
            }
            mma((const unsigned*)(smem + cur * A_ELEMS), (const unsigned*)(Bs0 + cur * B_ELEMS));
            cur ^= 1;
        }
        __syncthreads();       // the epilogue reuses the operand buffers
    } else if constexpr (APS) {
        // both operands by LDS-DMA, double-buffered: one barrier per k-tile.  At the top of iteration t every wave waits for
        // its own pieces of tile t (issued one iteration ago, under the MFMAs of tile t-1) and meets the others: tile t is
        // complete and nobody still reads the buffers of tile t-1, which the DMA of tile t+1 now overwrites.
        if (kbeg < kend) {
            lpa.issue(p.A, Apl, sm0);
            lp.template issue<NPL>(p.B, Bpl, sb0);
        }
        int cur = 0;
        KOAF_STAMP(1);
        for (int k0 = kbeg; k0 < kend; k0 += BK) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if ((k0 + BK) < kend) {
                lpa.issue(p.A, Apl, sm0 + (cur ^ 1) * (A_ELEMS * 4));
                lp.template issue<NPL>(p.B, Bpl, sb0 + (cur ^ 1) * (B_ELEMS * 4));
            }
            mma((const unsigned*)(smem + cur * A_ELEMS), (const unsigned*)(Bs0 + cur * B_ELEMS));
            cur ^= 1;
        }
        __syncthreads();       // the epilogue reuses the operand buffers
    } else {
    if (kbeg < kend) {
        if constexpr (BPS) lp.template issue<NPL>(p.B, Bpl, sb0);
        if constexpr (!PERSIST) la.issue(la.sa, p.A, Ap, kbeg, kend, z1);       // (PERSIST: in flight since the last tile's epilogue)
        if constexpr (!BPS) lb.issue(lb.sa, p.B, Bp, kbeg, kend, z1);
        if constexpr (TFA == 3) { la.side = (n0 == 0) ? p.A.side : nullptr; la.k0s = kbeg; }
        la.finish(la.sa);
        la.template store<NPL>(la.sa, smem);
        if constexpr (!BPS) {
            lb.finish(lb.sa);
            lb.template store<NPL>(lb.sa, Bs0);
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's DMA pieces have landed
        }
    }
    __syncthreads();
    int cur = 0;
    KOAF_STAMP(1);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        const bool more = (k0 + BK) < kend;
        // the next tile's global loads go out first: in flight under this tile's MFMAs (the DMA into the other B buffer,
        // which every wave stopped reading at the last barrier)
        if (more) {
            if constexpr (BPS) lp.template issue<NPL>(p.B, Bpl, sb0 + (cur ^ 1) * (B_ELEMS * 4));
            la.issue(la.sa, p.A, Ap, k0 + BK, kend, z1);
            if constexpr (!BPS) lb.issue(lb.sa, p.B, Bp, k0 + BK, kend, z1);
        }
        mma((const unsigned*)smem, (const unsigned*)(Bs0 + cur * B_ELEMS));
        // every wave is done reading the A image (and this B buffer).  With LDS-DMA in flight __syncthreads() would
        // drain vmcnt here, in the middle of the MFMA stream: a raw barrier behind the LDS-read wait keeps the next
        // tile's loads in flight until finish() needs them.
        if constexpr (BPS) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else __syncthreads();
        if (more) {
            if constexpr (TFA == 3) la.k0s = k0 + BK;
            la.finish(la.sa);
            la.template store<NPL>(la.sa, smem);
            if constexpr (!BPS) {
                lb.finish(lb.sa);
                lb.template store<NPL>(lb.sa, Bs0);
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                cur ^= 1;
            }
            __syncthreads();
        }
    }
    }

    // the next tile of this block: ids, A loader state and its first loads -- before the epilogue, whose staging, loads
    // and stores they run under (the A slot registers are free here; the LDS is not: the staging tile covers the operand
    // buffers, so the weight tile's DMA has to wait for the end of the epilogue)
    bool has_next = false;
    int tm2 = 0, tn2 = 0;
    // (M_PT blocks are NOT persistent: requesting the next tile's halo under this tile's epilogue was measured -- the prologue
    // fell from 3.9 to 0.7 us per tile and the k-loops grew by as much: with two blocks per CU one block's prologue already runs
    // under the other's MFMAs)
    if constexpr (AS) {
        has_next = s_has_next; tm2 = s_tm2; tn2 = s_tn2;       // (its first SD k-tiles are already in flight)
    } else if constexpr (PERSIST) {
        has_next = (vt + gridDim.x) < ntx;
        if (has_next) {
            decode(vt + gridDim.x, tm2, tn2);
            la.init(p.A, p.m_base + tm2 * BM, p.M, z1, sca);
            la.seek(p.A, kbeg);
            if (kbeg < kend) la.issue(la.sa, p.A, Ap, kbeg, kend, z1);
        }
    }

    if constexpr (F16 && (TFA == 1 || TFA == 3) && AKC && !APS && !AH && !WPS && !AS) {
        if (((la.satmax & 0xffffu) >= 0x7bffu) | ((la.satmax >> 16) >= 0x7bffu)) koaf_status_add(p.status, 0, 1u);
        la.satmax = 0u;
    }
    // ---- epilogue ----
    KOAF_STAMP(2);
    float* Cp;
    int64_t ldc;
    const bool slab = p.splitk > 1;
    if (slab) {
        Cp = p.C + (int64_t)(blockIdx.z * p.splitk + split) * p.M * p.N;
        ldc = p.N;
    } else {
        Cp = const_cast<float*>(eoff(p.C, z0 * p.cbs0 + z1 * p.cbs1, C16));
        ldc = p.ldc;
    }
    const float* Rp = (p.residual && !slab) ? p.residual + z0 * p.rbs0 + z1 * p.rbs1 : nullptr;
    const float* bias = slab ? nullptr : p.bias;
    const bool do_stats = (p.stats != nullptr) && !slab;
    // (per 32-row band i of the wave's rows: the tile's sums are then the same tree whether its four bands sit in two waves or,
    // on the streamed kernels, in four -- band sums, lane halves, band pairs, pair of pairs)
    float s1[TM][TN], s2[TM][TN], kshift[TN];
    [[maybe_unused]] float t1[NCB], t2[NCB], kshift16[NCB];      // (M16: per 16-column block)
    if constexpr (M16) {
#pragma unroll
        for (int j = 0; j < NCB; ++j) {
            t1[j] = t2[j] = 0.f;
            const int scol = n0 + wn * WN + 16 * j + (lane & 15);
            kshift16[j] = (do_stats && p.stats_shift && scol < p.N) ? p.stats_shift[(int64_t)blockIdx.z * p.stats_bs + scol] : 0.f;
        }
    }
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
#pragma unroll
        for (int i = 0; i < TM; ++i) s1[i][jn] = s2[i][jn] = 0.f;
        // statistics are summed about a per-column shift (the BatchNorm's running mean): sum (v - k), sum (v - k)^2
        // lose nothing to cancellation when |mean| >> std, which sum v^2 - (sum v)^2 / n does
        const int scol = n0 + wn * WN + 32 * jn + r;
        kshift[jn] = (do_stats && p.stats_shift && scol < p.N) ? p.stats_shift[(int64_t)blockIdx.z * p.stats_bs + scol] : 0.f;
    }
    // Rows of a ragged last tile past M were accumulated as zeros.  Under a shift each puts (0 - k) and k^2 into the sums above;
    // taking n k and n k^2 out again afterwards leaves the rounding of sums as large as n k^2 in a tile whose own rows may sum to
    // far less (4 real rows of 128: 3.5e-5 of the sum of squares, 3e-4 of the sum).  Such a tile sums its real rows from the
    // staged tile instead.  Block-uniform; full tiles and unshifted statistics run what they always ran.
    const int mreal = p.M - m0;                  // real rows of this tile (>= BM: all of them)
    const bool ragged_shift = do_stats && p.stats_shift != nullptr && mreal < BM;
    [[maybe_unused]] float rg1 = 0.f, rg2 = 0.f;

    if constexpr (VEC) {
        // stage the accumulator tile through LDS so global stores (and residual / bias loads) are
        // 16 B per lane on full 512-B row segments instead of 4 B per lane.  (Measured alternatives: 4-B stores straight
        // from the accumulator registers -- two 128-B segments per wave store -- are 25-30 % slower on the output-bound 1x1
        // convolutions; staging in two 64-row halves to fit a third block per CU needs <= 168 VGPRs, which spills ~130
        // dwords per lane here and halves the speed.)
        float* Cs = smem;   // all waves passed the k-loop's last barrier: operand tiles are dead
        if constexpr (M16) {
            // 16 x 16 tiles: lane (c = l % 16, q = l / 16) holds column c, rows 4 q + e of its tile
#pragma unroll
            for (int i = 0; i < NRB; ++i)
#pragma unroll
                for (int j = 0; j < NCB; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = alpha * acc16[i][j][e];
                        t1[j] += v - kshift16[j];
                        t2[j] = fmaf(v - kshift16[j], v - kshift16[j], t2[j]);
                        Cs[(wm * WM + 16 * i + 4 * (lane >> 4) + e) * LDC_S + wn * WN + 16 * j + (lane & 15)] = v;
                    }
        } else
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = alpha * acc[i][jn][e];
                    s1[i][jn] += v - kshift[jn];
                    s2[i][jn] = fmaf(v - kshift[jn], v - kshift[jn], s2[i][jn]);     // (explicit: every instantiation rounds alike)
                    Cs[(wm * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) * LDC_S + wn * WN + 32 * jn + r] = v;
                }
        __syncthreads();
        KOAF_STAMP(3);
        constexpr int C4 = BN / 4;
        constexpr int RPP = NT / C4;           // rows per pass
        const int c4 = t % C4, rr = t / C4;
        const int col = n0 + 4 * c4;
        const bool bnb = (p.bnb_mode != 0) && !slab;
        v4f q1 = {0.f, 0.f, 0.f, 0.f}, q2 = q1, q3 = q1;   // fused BN-backward column sums of this thread's rows
        v4f qm = q1;                                       // and the largest |dz| it stored (KoafGemm.bnb_amax), as magnitude bits
        if (col < p.N) {                         // N % 4 == 0 on this path
            v4f bv = {0.f, 0.f, 0.f, 0.f};
            if (bias) bv = *(const v4f*)(bias + col);
            v4f mu = bv, is = bv, ms = bv, mh = bv, mu2 = bv, is2 = bv;
            if (bnb) {
                mu = *(const v4f*)(p.bnb_mean + col);
                is = *(const v4f*)(p.bnb_invstd + col);
                if (p.bnb_mode == 2) { ms = *(const v4f*)(p.bnb_sc + col); mh = *(const v4f*)(p.bnb_sh + col); }
                if (p.bnb2_c) { mu2 = *(const v4f*)(p.bnb2_mean + col); is2 = *(const v4f*)(p.bnb2_invstd + col); }
            }
            const bool full = (m0 + BM <= p.M) && !p.cmap;
            if (full) {
                const bool hr = Rp != nullptr, h2 = bnb && p.bnb2_c != nullptr;
                const int mode = bnb ? p.bnb_mode : 0;
#define KOAF_EPI(R_, M_, C2_) epi_rows_full<BM, BN, NT, R_, M_, C2_, C16, E16, AT, EMIT>(p, Cs, LDC_S, Cp, ldc, Rp, AT ? t2d_base : m0, col, c4, rr, bv, mu, is, \
                                                                 ms, mh, mu2, is2, q1, q2, q3, qm, t2d_w)
                if (mode == 0) { if (hr) KOAF_EPI(true, 0, false); else KOAF_EPI(false, 0, false); }
                else if (mode == 1) {
                    if (hr) { if (h2) KOAF_EPI(true, 1, true); else KOAF_EPI(true, 1, false); }
                    else { if (h2) KOAF_EPI(false, 1, true); else KOAF_EPI(false, 1, false); }
                } else {
                    if (hr) { if (h2) KOAF_EPI(true, 2, true); else KOAF_EPI(true, 2, false); }
                    else { if (h2) KOAF_EPI(false, 2, true); else KOAF_EPI(false, 2, false); }
                }
#undef KOAF_EPI
            } else
#pragma unroll 4
            for (int row = rr; row < BM; row += RPP) {
                const int grow = m0 + row;
                if (grow < p.M) {
                    int64_t orow = grow;
                    if (p.cmap) {
                        const int ppi = p.cm_PH * p.cm_PW;
                        const int n = grow / ppi;
                        const int rem = grow - n * ppi;
                        const int yy = rem / p.cm_PW;
                        const int xx = rem - yy * p.cm_PW;
                        orow = ((int64_t)n * p.cm_H + 2 * yy + p.cm_py) * p.cm_W + 2 * xx + p.cm_px;
                    }
                    v4f v = *(const v4f*)&Cs[row * LDC_S + 4 * c4] + bv;
                    if (Rp) v += *(const v4f*)(Rp + orow * p.ldr + col);
                    if (bnb) {
                        const v4f cv = load4_nt<E16>(p.bnb_c, orow * ldc + col);
                        if (p.bnb_mode == 1) {
                            const v4f yv = load4_nt<E16>(p.bnb_y, orow * ldc + col);
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = yv[j] > 0.f ? v[j] : 0.f;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = (cv[j] * ms[j] + mh[j]) > 0.f ? v[j] : 0.f;
                        }
                        q1 += v;
                        q2 += v * ((cv - mu) * is);
#pragma unroll
                        for (int j = 0; j < 4; ++j) qm[j] = __uint_as_float(max(__float_as_uint(qm[j]), koaf_absbits(v[j])));
                        if (p.bnb2_c) {
                            const v4f c2 = load4_nt<E16>(p.bnb2_c, orow * ldc + col);
                            q3 += v * ((c2 - mu2) * is2);
                        }
                    }
                    store4_nt<C16>(Cp, orow * ldc + col, v);
                    if (EMIT && p.out_planes && !bnb && !Rp) {
                        unsigned ns = 0;
                        epi_emit_planes<C16>(p, orow * ldc + col, v, *(const v4f*)(p.out_sc + col) * KOAF_ACT_SCALE,
                                             *(const v4f*)(p.out_sh + col) * KOAF_ACT_SCALE, ns);
                        koaf_status_add(p.status, 0, ns);
                    }
                }
            }
        }
        if (EMIT && p.out_planes && tm == 0 && tn == 0 && t == 0 && blockIdx.z == 0) *(uint4*)(p.out_planes + 2 * p.out_ps) = make_uint4(0u, 0u, 0u, 0u);   // the zero chunk
        if (bnb) {
            if (p.bnb_amax) block_amax_raise_bits(max(max(__float_as_uint(qm[0]), __float_as_uint(qm[1])), max(__float_as_uint(qm[2]), __float_as_uint(qm[3]))), p.bnb_amax);
            // column sums over the block's rows: RPP row-threads per column vector -> LDS -> one partial row
            __syncthreads();                     // Cs fully consumed
            v4f* red4 = reinterpret_cast<v4f*>(smem);   // [3][RPP][C4]
            red4[(0 * RPP + rr) * C4 + c4] = q1;
            red4[(1 * RPP + rr) * C4 + c4] = q2;
            red4[(2 * RPP + rr) * C4 + c4] = q3;
            __syncthreads();
            const int nsum = p.bnb2_c ? 3 : 2;
            if (rr < nsum && col < p.N) {
                v4f a = red4[(rr * RPP) * C4 + c4];
                for (int j = 1; j < RPP; ++j) a += red4[(rr * RPP + j) * C4 + c4];
                *(v4f*)(p.bnb_part + ((int64_t)(p.part_row0 + tm) * nsum + rr) * p.N + col) = a;
            }
        }
        if (do_stats) __syncthreads();           // Cs is about to be reused by the statistics reduction
        if (ragged_shift) {
            // the staged tile still holds every accumulator: this column's sums over the tile's real rows only
            if (t < BN && (n0 + t) < p.N) {
                const float k = p.stats_shift[(int64_t)blockIdx.z * p.stats_bs + n0 + t];
                for (int row = 0; row < mreal; ++row) {
                    const float d = Cs[row * LDC_S + t] - k;
                    rg1 += d;
                    rg2 = fmaf(d, d, rg2);
                }
            }
            __syncthreads();
        }
    } else {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int col = n0 + wn * WN + 32 * jn + r;
            const bool cok = col < p.N;
            const float bv = (bias && cok) ? bias[col] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = alpha * acc[i][jn][e];
                const float k = row < p.M ? kshift[jn] : 0.f;       // (rows past M hold zeros: summed about 0, they add nothing)
                s1[i][jn] += v - k;
                s2[i][jn] = fmaf(v - k, v - k, s2[i][jn]);     // (explicit: every instantiation rounds alike)
                if (cok && row < p.M) {
                    v += bv;
                    if (Rp) v += Rp[(int64_t)row * p.ldr + col];
                    Cp[(int64_t)row * ldc + col] = v;
                }
            }
        }
    }
    }
    if (do_stats) {
        // column sums over this block's BM rows: lanes (r,0)+(r,1), then the WGM M-waves via LDS
        float* red = smem;  // [WGM][2][BN]
        if constexpr (M16) {
            // the four lane quarters hold rows 4 q .. 4 q + 3 of every tile of the column
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                float a1 = t1[j] + __shfl_xor(t1[j], 16, 64), a2 = t2[j] + __shfl_xor(t2[j], 16, 64);
                a1 += __shfl_xor(a1, 32, 64);
                a2 += __shfl_xor(a2, 32, 64);
                if (lane < 16) {
                    red[(wm * 2 + 0) * BN + wn * WN + 16 * j + lane] = a1;
                    red[(wm * 2 + 1) * BN + wn * WN + 16 * j + lane] = a2;
                }
            }
        } else
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            float a1 = s1[0][jn] + __shfl_xor(s1[0][jn], 32, 64);
            float a2 = s2[0][jn] + __shfl_xor(s2[0][jn], 32, 64);
#pragma unroll
            for (int i = 1; i < TM; ++i) {
                a1 += s1[i][jn] + __shfl_xor(s1[i][jn], 32, 64);
                a2 += s2[i][jn] + __shfl_xor(s2[i][jn], 32, 64);
            }
            if (h == 0) {
                red[(wm * 2 + 0) * BN + wn * WN + 32 * jn + r] = a1;
                red[(wm * 2 + 1) * BN + wn * WN + 32 * jn + r] = a2;
            }
        }
        __syncthreads();
        if (t < BN && (n0 + t) < p.N) {
            float* st = p.stats + (int64_t)(p.part_row0 + tm) * 2 * p.stats_ld + (int64_t)blockIdx.z * p.stats_bs;
            float a1 = red[0 * BN + t], a2 = red[1 * BN + t];
            if constexpr (WGM == 4 && TM == 1) {      // (the streamed kernels' four one-band waves: pairs first, as two two-band waves add up)
                a1 = (a1 + red[2 * BN + t]) + (red[4 * BN + t] + red[6 * BN + t]);
                a2 = (a2 + red[3 * BN + t]) + (red[5 * BN + t] + red[7 * BN + t]);
            } else {
#pragma unroll
                for (int m = 1; m < WGM; ++m) { a1 += red[(2 * m) * BN + t]; a2 += red[(2 * m + 1) * BN + t]; }
            }
            if constexpr (VEC) {
                if (ragged_shift) { a1 = rg1; a2 = rg2; }
            }
            st[n0 + t] = a1;
            st[p.stats_ld + n0 + t] = a2;
        }
    }
    KOAF_STAMP(4);
    KOAF_STAMP_ADD(0, 0, 1);      // prologue (entry -> first k-step ready); only the halo loop sets stamp 1
    KOAF_STAMP_ADD(1, 1, 2);      // k-loop
    KOAF_STAMP_ADD(2, 2, 3);      // accumulators -> LDS staging
    KOAF_STAMP_ADD(3, 3, 4);      // stores / fused reductions / statistics
    KOAF_STAMP_ADD(4, 0, 4);      // whole tile
    KOAF_STAMP_ACC(7, 1);         // tiles
    if (!has_next) break;
    // on to this block's next tile (PERSIST only): its A loads are in flight; the LDS is free once every wave is here
    __syncthreads();
    vt += gridDim.x;
    tm = tm2; tn = tn2;
    m0 = p.m_base + tm * BM; n0 = tn * BN;
    if constexpr (PERSIST) {
        lp.init(p.B, n0, p.N);
        lp.seek(p.B, kbeg);
    }
    if constexpr (AS) {
        st.tile(m0, p.M);
        stream_next();
    }
    }
}

}  // namespace
