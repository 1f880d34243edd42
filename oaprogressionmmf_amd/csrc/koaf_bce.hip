// koaf_bce.hip -- binary cross-entropy on probabilities (nn.BCELoss) and on logits (nn.BCEWithLogitsLoss), the registry's
// "bce_loss" / "bce_wlogits_loss" (koafusion/various/_losses.py:111-117): loss and input gradient in one launch, like the focal
// kernel (koaf_loss.hip), and with its reduction design -- one block up to its single-block reach, beyond that a grid of
// fixed-size chunks whose partial sums one block adds in index order.
#include "koaf_common.h"

namespace {

constexpr int64_t BCE_ONE_BLOCK = 8192;   // elements one block covers in a few passes
constexpr int64_t BCE_CHUNK = 4096;       // elements per block of the grid form

// One element: returns the loss term and writes d loss / d x (both without the reduction's 1 / n).
//   LOGITS 0 (nn.BCELoss):  l = -w * (t * max(log x, -100) + (1 - t) * max(log(1 - x), -100)) -- torch's clamp of the logs --,
//     dl/dx = w * (x - t) / max((1 - x) * x, 1e-12) -- torch's backward of it.  A probability outside [0, 1] (NaN included) is
//     where torch raises a device assert: the element gets zero loss and zero gradient and is counted in `bad`, the policy the
//     softmax losses have for out-of-range labels.
//   LOGITS 1 (nn.BCEWithLogitsLoss), stable form:  l = w * ((1 - t) * x + lw * (log1p(exp(-|x|)) + max(-x, 0))) with
//     lw = 1 + (pw - 1) * t;  dl/dx = w * (lw * sigmoid(x) - pw * t)
template <bool LOGITS>
__device__ __forceinline__ float bce_one(float x, float t, float w, float pw, float* dx, unsigned* bad) {
    if constexpr (LOGITS) {
        const float e = expf(-fabsf(x));
        const float sig = (x >= 0.f ? 1.f : e) / (1.f + e);
        const float lw = 1.f + (pw - 1.f) * t;
        *dx = w * (lw * sig - pw * t);
        return w * ((1.f - t) * x + lw * (log1pf(e) + fmaxf(-x, 0.f)));
    } else {
        if (!(x >= 0.f && x <= 1.f)) {
            *bad += 1u;
            *dx = 0.f;
            return 0.f;
        }
        const float lx = fmaxf(logf(x), -100.f), l1x = fmaxf(log1pf(-x), -100.f);
        *dx = w * (x - t) / fmaxf((1.f - x) * x, 1e-12f);
        return -w * (t * lx + (1.f - t) * l1x);
    }
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// Block k owns the elements [k * chunk, (k + 1) * chunk); its 256 lanes stride through them.  reduction 0 (none): loss[i] is
// the element's term and dx its derivative.  Otherwise dx carries the reduction's scale (1 / n for the mean) and the block's
// sum goes through one LDS tree to part[k] -- or, when the grid is one block (part == NULL), scaled straight to *loss.
template <bool LOGITS>
__global__ void __launch_bounds__(256) bce_kernel(const float* __restrict__ x, const float* __restrict__ target,
                                                  const float* __restrict__ weight, const float* __restrict__ pos_weight,
                                                  float* __restrict__ loss, float* __restrict__ dx, float* __restrict__ part,
                                                  int64_t n, int C, int64_t chunk, int reduction, uint32_t* status) {
    __shared__ float red[256];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    const float scale = (reduction == 1) ? 1.f / (float)n : 1.f;
    float acc = 0.f;
    unsigned nbad = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float w = weight ? weight[i] : 1.f;
        const float pw = (LOGITS && pos_weight) ? pos_weight[i % C] : 1.f;
        float d;
        const float l = bce_one<LOGITS>(x[i], target[i], w, pw, &d, &nbad);
        dx[i] = d * scale;
        if (reduction == 0) loss[i] = l;
        else acc += l;
    }
    koaf_status_add(status, 1, nbad);
    if (reduction == 0) return;
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        if (part) part[blockIdx.x] = s;
        else *loss = s * scale;
    }
}

// *loss = (sum_k part[k]) * scale, k in index order (lane l takes k = l, l + 256, ...; one LDS tree)
__global__ void __launch_bounds__(256) bce_sum_kernel(const float* __restrict__ part, int nblk, float* __restrict__ loss, float scale) {
    __shared__ float red[256];
    float a = 0.f;
    for (int k = threadIdx.x; k < nblk; k += 256) a += part[k];
    const float s = block_sum_256(a, red);
    if (threadIdx.x == 0) *loss = s * scale;
}

}  // namespace

extern "C" int64_t koaf_bce_ws(int64_t n) { return n > BCE_ONE_BLOCK ? (n + BCE_CHUNK - 1) / BCE_CHUNK : 0; }

extern "C" int koaf_bce_loss(const float* x, const float* target, const float* weight, const float* pos_weight, float* loss,
                             float* dx, int64_t n, int32_t C, int32_t from_logits, int32_t reduction, float* ws, void* stream) {
    KOAF_REQUIRE(x && target && loss && dx && n > 0 && C > 0, "koaf_bce_loss: bad args");
    KOAF_REQUIRE(reduction >= 0 && reduction <= 2, "koaf_bce_loss: reduction is 0 (none), 1 (mean) or 2 (sum)");
    KOAF_REQUIRE(!pos_weight || (from_logits && n % C == 0), "koaf_bce_loss: pos_weight [C] belongs to the logits form, C the last dimension");
    // reduction none needs no sum: always the grid.  A sum beyond one block's reach takes the grid when the caller brought the
    // workspace for its partials; without one the single block walks everything.
    const bool grid = n > BCE_ONE_BLOCK && (reduction == 0 || ws);
    const int nblk = grid ? (int)((n + BCE_CHUNK - 1) / BCE_CHUNK) : 1;
    const int64_t chunk = grid ? BCE_CHUNK : n;
    float* part = (grid && reduction != 0) ? ws : nullptr;
    if (from_logits)
        hipLaunchKernelGGL((bce_kernel<true>), dim3(nblk), dim3(256), 0, STREAM, x, target, weight, pos_weight, loss, dx, part, n, C, chunk,
                           reduction, koaf_status_ptr());
    else
        hipLaunchKernelGGL((bce_kernel<false>), dim3(nblk), dim3(256), 0, STREAM, x, target, weight, pos_weight, loss, dx, part, n, C, chunk,
                           reduction, koaf_status_ptr());
    if (part)
        hipLaunchKernelGGL(bce_sum_kernel, dim3(1), dim3(256), 0, STREAM, part, nblk, loss, reduction == 1 ? 1.f / (float)n : 1.f);
    return koaf_check_launch("koaf_bce_loss");
}
