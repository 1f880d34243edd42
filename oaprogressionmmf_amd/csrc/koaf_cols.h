// koaf_cols.h -- column reductions over a [rows][C] tensor, shared by the BatchNorm unit (koaf_bn.hip) and LayerNorm's parameter
// gradients (koaf_rows.hip): the block geometry, the in-block LDS tree and the final pass over the partial rows.  Every
// colfinal_kernel<NS> instantiation belongs to ONE unit (<1>: koaf_bn.hip, <2>: koaf_rows.hip).
#pragma once
#include "koaf_common.h"

namespace {
// ------------------------------------------------------------------------------------------------
// column partial sums over a [rows][C] tensor.  Block (256 thr) owns a chunk of <= 1024 columns and
// `rpb` rows; thread (cvx, ry) walks rows ry, ry+RP, ...; LDS tree over ry; writes part[blk][k][C].
// ------------------------------------------------------------------------------------------------
struct ColGeom {
    int CW;      // columns per chunk
    int nchunk;  // column chunks
    int CV;      // column vectors per chunk (CW/4)
    int RP;      // rows per pass (256/CV)
    int rpb;     // rows per block
    int nblk;    // row blocks
};
inline bool col_geom(int64_t rows, int C, int max_blk, ColGeom* g) {
    if (C % 4) return false;
    int CW = C > 1024 ? 1024 : C;
    if (C % CW) return false;
    int CV = CW / 4;
    if (256 % CV) return false;
    g->CW = CW;
    g->nchunk = C / CW;
    g->CV = CV;
    g->RP = 256 / CV;
    int64_t rpb = cdiv64(rows, max_blk);
    rpb = cdiv64(rpb, g->RP) * g->RP;
    if (rpb < g->RP * 4) rpb = g->RP * 4;
    g->rpb = (int)rpb;
    g->nblk = (int)cdiv64(rows, rpb);
    return true;
}

template <int NS>
__device__ __forceinline__ void col_block_reduce(v4f (&s)[NS], float* part, int blk, int C, int c0, int CV,
                                                 int RP) {
    __shared__ v4f red[256];
    const int t = threadIdx.x;
    const int cvx = t % CV, ry = t / CV;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        __syncthreads();
        red[t] = s[k];
        __syncthreads();
        if (ry == 0) {
            v4f a = red[cvx];
            for (int j = 1; j < RP; ++j) a += red[j * CV + cvx];
            *(v4f*)&part[((int64_t)blk * NS + k) * C + c0 + 4 * cvx] = a;
        }
    }
}

// partial [rows][NS][C] -> out [NS][C]; block = 64 columns x 16 row groups
template <int NS>
__global__ void __launch_bounds__(1024) colfinal_kernel(const float* __restrict__ part, int rows, int C,
                                                        float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ double red[NS][16][64];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    if (c < C)
        for (int r = gy; r < rows; r += 16)
#pragma unroll
            for (int k = 0; k < NS; ++k) a[k] += (double)part[((int64_t)r * NS + k) * C + c];
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][gy][cx] = a[k];
    __syncthreads();
    if (gy == 0 && c < C) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double s = 0.0;
            for (int j = 0; j < 16; ++j) s += red[k][j][cx];
            (k == 0 ? out0 : out1)[c] = (float)s;
        }
    }
}
}  // namespace
