// koaf_occl.hip -- occlusion sensitivity maps (captum's Occlusion; not in the reference's driver, named in its recipe): the copies
// of an input with a sliding window replaced by the baseline, the slice images of such a copy gathered straight from the stored
// volume (only the slices a window touches are ever encoded again), the splice of their fresh feature rows into the cached ones,
// and the map from the score differences.  Every kernel is element-wise or row-wise: no atomics, no cross-thread reduction, no
// arithmetic but the map's fixed-order sum and its one division -- the bits do not depend on the grid (koaf.h).
#include "koaf_common.h"

namespace {

constexpr int OC_BLOCK = 256;
constexpr int OC_CHUNK = 4096;          // elements per block of the streaming kernels: 4 dwordx4 accesses per lane
constexpr int OC_MAX_J = KOAF_ATTR_MAX_J;
constexpr int OC_G = 16;                // table rows per block of the staged slice gather
constexpr int OC_P = 64;                // pixels per block of the staged slice gather
constexpr int OC_LD = OC_P + 4;         // its LDS row pitch: bank = 4 q + p, distinct over a wave's 16 rows x 4 pixels

// an input row as a box of four extents (padded in front with ones), the window, the strides and the window counts
struct OcBox { int d[4], w[4], s[4], cnt[4]; };
struct OcWin { int lo[4], hi[4]; };

// window k (flat, row-major over cnt, last dimension fastest) covers [j s, min(j s + w, d)) along every dimension
__device__ __forceinline__ OcWin oc_window(const OcBox& bx, int k) {
    OcWin wn;
#pragma unroll
    for (int a = 3; a >= 0; --a) {
        const int j = k % bx.cnt[a];
        k /= bx.cnt[a];
        wn.lo[a] = j * bx.s[a];
        wn.hi[a] = min(wn.lo[a] + bx.w[a], bx.d[a]);
    }
    return wn;
}
struct OcPos { int c[4]; };
__device__ __forceinline__ OcPos oc_coords(const OcBox& bx, int e) {
    OcPos p;
#pragma unroll
    for (int a = 3; a > 0; --a) { p.c[a] = e % bx.d[a]; e /= bx.d[a]; }
    p.c[0] = e;
    return p;
}
__device__ __forceinline__ void oc_next(const OcBox& bx, OcPos& p) {     // the next element of the row
#pragma unroll
    for (int a = 3; a > 0; --a) {
        if (++p.c[a] < bx.d[a]) return;
        p.c[a] = 0;
    }
    ++p.c[0];
}
__device__ __forceinline__ bool oc_inside(const OcPos& p, const int* lo, const int* hi) {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) in = in && p.c[a] >= lo[a] && p.c[a] < hi[a];
    return in;
}

// out[j][b][i] = (i in window k0 + j) ? bs : x[b][i].  Block (c, b) owns elements [c * OC_CHUNK, ...) of row b; the J windows sit
// in LDS.  VEC: rows are 16-byte aligned (n % 4 == 0 and aligned pointers) -- a lane takes 4 elements; else one element per lane.
template <bool VEC, bool BASE>
__global__ void __launch_bounds__(OC_BLOCK) occl_points_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                               float base_value, float* __restrict__ out, int J, int B, int n,
                                                               OcBox bx, int k0) {
    __shared__ int wlo[OC_MAX_J][4], whi[OC_MAX_J][4];
    if ((int)threadIdx.x < J) {
        const OcWin wn = oc_window(bx, k0 + threadIdx.x);
#pragma unroll
        for (int a = 0; a < 4; ++a) { wlo[threadIdx.x][a] = wn.lo[a]; whi[threadIdx.x][a] = wn.hi[a]; }
    }
    __syncthreads();
    const int b = blockIdx.y;
    const int e0 = blockIdx.x * OC_CHUNK, e1 = min(e0 + OC_CHUNK, n);
    const int64_t row = (int64_t)b * n, plane = (int64_t)B * n;
    const float* __restrict__ xr = x + row;
    const float* __restrict__ br = BASE ? base + row : nullptr;
    float* __restrict__ orow = out + row;
    if constexpr (VEC) {
        for (int v = e0 / 4 + threadIdx.x; v < e1 / 4; v += OC_BLOCK) {
            const v4f xv = *(const v4f*)&xr[v * 4];
            v4f bv = {base_value, base_value, base_value, base_value};
            if constexpr (BASE) bv = *(const v4f*)&br[v * 4];
            OcPos p[4];
            p[0] = oc_coords(bx, v * 4);
#pragma unroll
            for (int u = 1; u < 4; ++u) { p[u] = p[u - 1]; oc_next(bx, p[u]); }
            for (int j = 0; j < J; ++j) {
                v4f r;
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = oc_inside(p[u], wlo[j], whi[j]) ? bv[u] : xv[u];
                __builtin_nontemporal_store(r, (v4f*)&orow[j * plane + v * 4]);      // (written once, read by the model much later)
            }
        }
    } else {
        for (int i = e0 + threadIdx.x; i < e1; i += OC_BLOCK) {
            const float xv = xr[i], bv = BASE ? br[i] : base_value;
            const OcPos p = oc_coords(bx, i);
            for (int j = 0; j < J; ++j) orow[j * plane + i] = oc_inside(p, wlo[j], whi[j]) ? bv : xv;
        }
    }
}

// one table row: (k, n) -> window, sample and slice; a row outside the table's ranges is marked with b = -1 and written as zeros
struct OcRow { int b, kk; };
__device__ __forceinline__ OcRow oc_row(const int* __restrict__ rows, int r, int K, int B, int K_img, int& k) {
    k = rows[2 * r];
    const int n = rows[2 * r + 1];
    if (k < 0 || k >= K || n < 0 || n >= B * K_img) { k = 0; return {-1, 0}; }
    return {n / K_img, n % K_img};
}

// Columns are the unit-stride axis of the source (sj == 1: radiographs and the src / cs / rs views), or no axis is (V == 1, any
// strides).  Block (r, c) writes pixels [c * 256 * V, ...) of table row r; a thread takes V consecutive columns of one image row.
template <int V, bool BASE>
__global__ void __launch_bounds__(OC_BLOCK) occl_slices_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                               float base_value, float* __restrict__ out,
                                                               const int* __restrict__ rows, int B, OcBox bx, int K, int K_img, int H,
                                                               int W, int64_t sb, int64_t sk, int64_t si, int64_t sj) {
    const int r = blockIdx.x, HW = H * W;
    const int pix = (blockIdx.y * OC_BLOCK + threadIdx.x) * V;
    if (pix >= HW) return;
    int k;
    const OcRow rw = oc_row(rows, r, K, B, K_img, k);
    float* o = out + (int64_t)r * HW + pix;
    if (rw.b < 0) {
#pragma unroll
        for (int u = 0; u < V; ++u) o[u] = 0.f;
        return;
    }
    const OcWin wn = oc_window(bx, k);
    const int i = pix / W, j = pix % W;
    const int e = (int)(rw.kk * sk + i * si + j * sj);
    const int64_t off = rw.b * sb + e;
    if constexpr (V == 4) {
        const v4f xv = *(const v4f*)&x[off];
        v4f bv = {base_value, base_value, base_value, base_value}, res;
        if constexpr (BASE) bv = *(const v4f*)&base[off];
        OcPos p = oc_coords(bx, e);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            res[u] = oc_inside(p, wn.lo, wn.hi) ? bv[u] : xv[u];
            oc_next(bx, p);
        }
        *(v4f*)o = res;
    } else {
        const float bv = BASE ? base[off] : base_value;
        o[0] = oc_inside(oc_coords(bx, e), wn.lo, wn.hi) ? bv : x[off];
    }
}

// Slices are the unit-stride axis of the source (sk == 1: the (B,1,R,C,S) volumes under the rc view).  One image's pixels lie S
// elements apart there, so a lane per pixel would touch a cache line per lane.  Block (g, c) instead takes OC_G consecutive table
// rows and OC_P pixels: on the read, 16 consecutive lanes take one pixel of the 16 rows -- consecutive slices of one sample where
// the table lists them so, as run.occlusion's does: 64 contiguous bytes -- and lay it into LDS; on the write, a wave takes 64
// consecutive pixels of one row.  Both sides are coalesced and the LDS pitch keeps both free of bank conflicts.
template <bool BASE>
__global__ void __launch_bounds__(OC_BLOCK) occl_slices_staged_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                      float base_value, float* __restrict__ out,
                                                                      const int* __restrict__ rows, int nrows, int B, OcBox bx, int K,
                                                                      int K_img, int H, int W, int64_t sb, int64_t si, int64_t sj) {
    __shared__ float tile[OC_G][OC_LD];
    __shared__ int wlo[OC_G][4], whi[OC_G][4], rb[OC_G], rkk[OC_G];
    const int r0 = blockIdx.x * OC_G, p0 = blockIdx.y * OC_P, HW = H * W;
    if (threadIdx.x < OC_G) {
        const int q = threadIdx.x;
        OcRow rw = {-1, 0};
        int k = 0;
        if (r0 + q < nrows) rw = oc_row(rows, r0 + q, K, B, K_img, k);
        const OcWin wn = oc_window(bx, k);
#pragma unroll
        for (int a = 0; a < 4; ++a) { wlo[q][a] = wn.lo[a]; whi[q][a] = wn.hi[a]; }
        rb[q] = rw.b;
        rkk[q] = rw.kk;
    }
    __syncthreads();
    const int q = threadIdx.x % OC_G;
#pragma unroll
    for (int ps = 0; ps < OC_P; ps += OC_BLOCK / OC_G) {
        const int p = ps + threadIdx.x / OC_G, pix = p0 + p;
        float val = 0.f;
        if (rb[q] >= 0 && pix < HW) {
            const int i = pix / W, j = pix % W;
            const int e = (int)(rkk[q] + i * si + j * sj);
            const int64_t off = rb[q] * sb + e;
            val = oc_inside(oc_coords(bx, e), wlo[q], whi[q]) ? (BASE ? base[off] : base_value) : x[off];
        }
        tile[q][p] = val;
    }
    __syncthreads();
    const int p = threadIdx.x % OC_P;
#pragma unroll
    for (int qs = 0; qs < OC_G; qs += OC_BLOCK / OC_P) {
        const int qq = qs + threadIdx.x / OC_P;
        if (r0 + qq < nrows && p0 + p < HW) out[(int64_t)(r0 + qq) * HW + p0 + p] = tile[qq][p];
    }
}

// out[row][u] = (src[row] < 0 ? cache[row % N] : fresh[src[row]])[u] over rows of upr units of T (16 or 4 bytes); a src outside
// [0, F) takes the cached row.  Grid-stride over the J * N * upr units: consecutive lanes, consecutive units.
template <typename T>
__global__ void __launch_bounds__(OC_BLOCK) occl_rows_kernel(const T* __restrict__ cache, const T* __restrict__ fresh,
                                                             const int* __restrict__ src, T* __restrict__ out, int64_t total, int N,
                                                             int F, int upr) {
    for (int64_t t = (int64_t)blockIdx.x * OC_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * OC_BLOCK) {
        const int64_t row = t / upr;
        const int u = (int)(t - row * upr);
        const int s = src[row];
        const T* from = (s >= 0 && s < F) ? fresh + (int64_t)s * upr : cache + (row % N) * upr;
        out[t] = from[u];
    }
}

// map[b][i] = (sum of delta[k][b] over the windows k that cover i, ascending k) / their number.  Along dimension a the covering
// windows are j in [max(0, ceil((c - w + 1) / s)), min(cnt - 1, floor(c / s))]; four nested loops walk them in ascending flat k.
__global__ void __launch_bounds__(OC_BLOCK) occl_fold_kernel(const float* __restrict__ delta, float* __restrict__ out, int B, int n,
                                                             OcBox bx) {
    const int b = blockIdx.y;
    const int e0 = blockIdx.x * OC_CHUNK, e1 = min(e0 + OC_CHUNK, n);
    for (int i = e0 + threadIdx.x; i < e1; i += OC_BLOCK) {
        const OcPos p = oc_coords(bx, i);
        int jl[4], jh[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int t = p.c[a] - bx.w[a] + 1;
            jl[a] = t <= 0 ? 0 : (t + bx.s[a] - 1) / bx.s[a];
            jh[a] = min(bx.cnt[a] - 1, p.c[a] / bx.s[a]);
        }
        float s = 0.f;
        int cnt = 0;
        for (int j0 = jl[0]; j0 <= jh[0]; ++j0)
            for (int j1 = jl[1]; j1 <= jh[1]; ++j1)
                for (int j2 = jl[2]; j2 <= jh[2]; ++j2)
                    for (int j3 = jl[3]; j3 <= jh[3]; ++j3) {
                        const int k = ((j0 * bx.cnt[1] + j1) * bx.cnt[2] + j2) * bx.cnt[3] + j3;
                        s += delta[(int64_t)k * B + b];
                        ++cnt;
                    }
        out[(int64_t)b * n + i] = s / (float)cnt;
    }
}

// the box of an entry point's dims / win / str (host arrays of four); 0 when they break 1 <= s <= w <= d or the sizes overflow
bool oc_box(const int32_t* dims, const int32_t* win, const int32_t* str, OcBox* bx, int64_t* n, int64_t* K) {
    if (!dims || !win || !str) return false;
    *n = 1;
    *K = 1;
    for (int a = 0; a < 4; ++a) {
        if (!(1 <= str[a] && str[a] <= win[a] && win[a] <= dims[a])) return false;
        bx->d[a] = dims[a];
        bx->w[a] = win[a];
        bx->s[a] = str[a];
        bx->cnt[a] = 1 + (dims[a] - win[a] + str[a] - 1) / str[a];
        *n *= dims[a];
        *K *= bx->cnt[a];
        if (*n >= (1ll << 31) || *K >= (1ll << 31)) return false;
    }
    return true;
}

}  // namespace

#define KOAF_OC_BOX(what)                                                                                              \
    OcBox bx;                                                                                                          \
    int64_t n, K;                                                                                                      \
    KOAF_REQUIRE(oc_box(dims, win, str, &bx, &n, &K),                                                                  \
                 what ": dims, win, str hold four extents with 1 <= str <= win <= dims, a row and a window count below 2^31")

extern "C" int koaf_occl_points(const float* x, const float* base, float base_value, float* out, int32_t J, int32_t B,
                                const int32_t* dims, const int32_t* win, const int32_t* str, int32_t k0, void* stream) {
    KOAF_OC_BOX("koaf_occl_points");
    KOAF_REQUIRE(J >= 1 && J <= OC_MAX_J, "koaf_occl_points: 1 <= J <= %d (J = %d)", OC_MAX_J, J);
    KOAF_REQUIRE(B >= 1 && B <= 65535, "koaf_occl_points: 1 <= B <= 65535 (B = %d)", B);
    KOAF_REQUIRE(x && out, "koaf_occl_points: x and out are required");
    KOAF_REQUIRE(k0 >= 0 && (int64_t)k0 + J <= K, "koaf_occl_points: windows [%d, %d + %d) leave the %lld of the box", k0, k0, J, (long long)K);
    const bool vec = n % 4 == 0 && aligned16(x) && aligned16(out) && (!base || aligned16(base));
    const dim3 grid((unsigned)cdiv64(n, OC_CHUNK), (unsigned)B), block(OC_BLOCK);
#define KOAF_OP(V, T) hipLaunchKernelGGL((occl_points_kernel<V, T>), grid, block, 0, STREAM, x, base, base_value, out, J, B, (int)n, bx, k0)
    if (vec) { if (base) KOAF_OP(true, true); else KOAF_OP(true, false); }
    else { if (base) KOAF_OP(false, true); else KOAF_OP(false, false); }
#undef KOAF_OP
    return koaf_check_launch("koaf_occl_points");
}

extern "C" int koaf_occl_slices(const float* x, const float* base, float base_value, float* out, const int32_t* rows, int32_t nrows,
                                int32_t B, const int32_t* dims, const int32_t* win, const int32_t* str, int32_t K_img, int32_t H,
                                int32_t W, int64_t sb, int64_t sk, int64_t si, int64_t sj, void* stream) {
    KOAF_OC_BOX("koaf_occl_slices");
    KOAF_REQUIRE(x && out && rows && nrows >= 1 && B >= 1 && K_img >= 1 && H >= 1 && W >= 1, "koaf_occl_slices: bad args");
    KOAF_REQUIRE(sb > 0 && sk > 0 && si > 0 && sj > 0, "koaf_occl_slices: strides are positive element counts");
    // the images tile the sample: K_img * H * W of its n elements, the farthest one inside it
    KOAF_REQUIRE((int64_t)K_img * H * W == n && sb == n && (K_img - 1) * sk + (H - 1) * si + (W - 1) * sj < n,
                 "koaf_occl_slices: %d images of %d x %d with strides (%lld, %lld, %lld, %lld) are not a sample of %lld elements", K_img,
                 H, W, (long long)sb, (long long)sk, (long long)si, (long long)sj, (long long)n);
    KOAF_REQUIRE((int64_t)B * K_img < (1ll << 31), "koaf_occl_slices: too many images");
    const int HW = H * W;
    const dim3 block(OC_BLOCK);
    if (sk == 1 && sj != 1 && K_img > 1) {
        const int64_t gy = cdiv64(HW, OC_P);
        KOAF_REQUIRE(gy <= 65535, "koaf_occl_slices: image too large (%d x %d)", H, W);
        const dim3 grid((unsigned)cdiv64(nrows, OC_G), (unsigned)gy);
#define KOAF_OS(T) hipLaunchKernelGGL(occl_slices_staged_kernel<T>, grid, block, 0, STREAM, x, base, base_value, out, rows, nrows, B, bx, (int)K, K_img, H, W, sb, si, sj)
        if (base) KOAF_OS(true); else KOAF_OS(false);
#undef KOAF_OS
    } else {
        const bool v4 = sj == 1 && W % 4 == 0 && sb % 4 == 0 && sk % 4 == 0 && si % 4 == 0 && aligned16(x) && aligned16(out) &&
                        (!base || aligned16(base));
        const int64_t gy = cdiv64(HW / (v4 ? 4 : 1), OC_BLOCK);
        KOAF_REQUIRE(gy <= 65535, "koaf_occl_slices: image too large (%d x %d)", H, W);
        const dim3 grid((unsigned)nrows, (unsigned)gy);
#define KOAF_OS(V, T) hipLaunchKernelGGL((occl_slices_kernel<V, T>), grid, block, 0, STREAM, x, base, base_value, out, rows, B, bx, (int)K, K_img, H, W, sb, sk, si, sj)
        if (v4) { if (base) KOAF_OS(4, true); else KOAF_OS(4, false); }
        else { if (base) KOAF_OS(1, true); else KOAF_OS(1, false); }
#undef KOAF_OS
    }
    return koaf_check_launch("koaf_occl_slices");
}

extern "C" int koaf_occl_rows(const void* cache, const void* fresh, const int32_t* src, void* out, int32_t J, int32_t N, int32_t F,
                              int64_t row_bytes, void* stream) {
    KOAF_REQUIRE(cache && src && out && J >= 1 && N >= 1 && F >= 0 && (fresh || F == 0), "koaf_occl_rows: bad args");
    KOAF_REQUIRE(row_bytes >= 4 && row_bytes % 4 == 0 && row_bytes < (1ll << 31), "koaf_occl_rows: row_bytes is a positive multiple of 4 below 2^31 (%lld)", (long long)row_bytes);
    const bool v16 = row_bytes % 16 == 0 && aligned16(cache) && aligned16(out) && (!fresh || aligned16(fresh));
    const int upr = (int)(row_bytes / (v16 ? 16 : 4));
    const int64_t total = (int64_t)J * N * upr;
    const dim3 grid(ew_grid(total)), block(OC_BLOCK);
    if (v16) hipLaunchKernelGGL(occl_rows_kernel<v4i>, grid, block, 0, STREAM, (const v4i*)cache, (const v4i*)fresh, src, (v4i*)out, total, N, F, upr);
    else hipLaunchKernelGGL(occl_rows_kernel<int>, grid, block, 0, STREAM, (const int*)cache, (const int*)fresh, src, (int*)out, total, N, F, upr);
    return koaf_check_launch("koaf_occl_rows");
}

extern "C" int koaf_occl_fold(const float* delta, float* out, int32_t K_given, int32_t B, const int32_t* dims, const int32_t* win,
                              const int32_t* str, void* stream) {
    KOAF_OC_BOX("koaf_occl_fold");
    KOAF_REQUIRE(delta && out && B >= 1 && B <= 65535, "koaf_occl_fold: delta, out and 1 <= B <= 65535");
    KOAF_REQUIRE(K_given == K, "koaf_occl_fold: delta holds %d windows, the box has %lld", K_given, (long long)K);
    const dim3 grid((unsigned)cdiv64(n, OC_CHUNK), (unsigned)B), block(OC_BLOCK);
    hipLaunchKernelGGL(occl_fold_kernel, grid, block, 0, STREAM, delta, out, B, (int)n, bx);
    return koaf_check_launch("koaf_occl_fold");
}
