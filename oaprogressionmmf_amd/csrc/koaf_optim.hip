// koaf_optim.hip -- the registry's optimizers (koafusion/various/_optimizers.py:47-52: "SGD", "RMSprop", "Adam" / "AdamW") as
// one-pass streams over the flat parameter arena: 16-byte loads and stores, a grid-stride loop, a scalar tail; every operand is
// read once and every updated one written once.  SGD's and RMSprop's options that do not change from launch to launch (momentum /
// Nesterov / centered / ...) are template parameters, so each variant carries only its own loads and stores; Adam's two (adamw,
// amsgrad) are run-time arguments of its one kernel.
// Below them: what sits between backward and the optimizer step -- the gradient fold of micro-batched steps and global-norm clipping.
#include "koaf_common.h"

namespace {

// ++step; hyper = {lr, first}: first = 1 on the very first update (SGD starts its momentum buffer with the gradient there), from
// the device scalars, so that a captured (HIP-graph) optimizer step advances from replay to replay like koaf_adam_hyper's
__global__ void optim_hyper_kernel(int32_t* step, const float* lr, float* hyper) {
    const int st = *step + 1;
    *step = st;
    hyper[0] = *lr;
    hyper[1] = (st == 1) ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------
// SGD (torch.optim.SGD single-tensor rule): g' = +-g + wd * p;  buf = first ? g' : mu * buf + (1 - damp) * g';
// step = nesterov ? g' + mu * buf : buf (g' without momentum);  p -= lr * step
// ------------------------------------------------------------------------------------------------
template <bool MOM, bool NEST>
__device__ __forceinline__ void sgd_one(float& p, float g, float& b, float lr, float mu, float omd, float wd, float sign, bool first) {
    g = sign * g + wd * p;
    float st = g;
    if constexpr (MOM) {
        b = first ? g : mu * b + omd * g;
        st = NEST ? g + mu * b : b;
    }
    p -= lr * st;
}

template <bool MOM, bool NEST>
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  int64_t n, float lr, float mu, float omd, float wd, float sign, int first,
                                                  const float* __restrict__ hyper) {
    if (hyper) { lr = hyper[0]; first = hyper[1] != 0.f; }     // device-resident step state (koaf_optim_hyper)
    const int64_t nvec = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        v4f pv = *(const v4f*)&p[i * 4];
        const v4f gv = *(const v4f*)&g[i * 4];
        v4f bv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MOM) {
            if (!first) bv = *(const v4f*)&buf[i * 4];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], bj = bv[j];
            sgd_one<MOM, NEST>(pj, gv[j], bj, lr, mu, omd, wd, sign, first);
            pv[j] = pj;
            bv[j] = bj;
        }
        *(v4f*)&p[i * 4] = pv;
        if constexpr (MOM) *(v4f*)&buf[i * 4] = bv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = nvec * 4 + threadIdx.x;
        float pj = p[i], bj = 0.f;
        if constexpr (MOM) {
            if (!first) bj = buf[i];
        }
        sgd_one<MOM, NEST>(pj, g[i], bj, lr, mu, omd, wd, sign, first);
        p[i] = pj;
        if constexpr (MOM) buf[i] = bj;
    }
}

// ------------------------------------------------------------------------------------------------
// RMSprop (torch.optim.RMSprop single-tensor rule): sq = alpha * sq + (1 - alpha) * g'^2;  centered: gavg = lerp(gavg, g',
// 1 - alpha), avg = sqrt(sq - gavg^2) + eps, else avg = sqrt(sq) + eps;  momentum: buf = mu * buf + g' / avg, p -= lr * buf,
// else p -= lr * g' / avg
// ------------------------------------------------------------------------------------------------
template <bool CEN, bool MOM>
__device__ __forceinline__ void rms_one(float& p, float g, float& sq, float& ga, float& b, float lr, float alpha, float oma,
                                        float eps, float wd, float mu, float sign) {
    g = sign * g + wd * p;
    sq = alpha * sq + oma * g * g;
    float avg;
    if constexpr (CEN) {
        // Tensor.lerp_'s two forms: the weight decides which end the rounding error stays close to
        ga = (oma < 0.5f) ? ga + oma * (g - ga) : g - (g - ga) * (1.f - oma);
        avg = sqrtf(sq - ga * ga) + eps;
    } else {
        avg = sqrtf(sq) + eps;
    }
    if constexpr (MOM) {
        b = mu * b + g / avg;
        p -= lr * b;
    } else {
        p -= lr * (g / avg);
    }
}

template <bool CEN, bool MOM>
__global__ void __launch_bounds__(256) rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                      float* __restrict__ gavg, float* __restrict__ buf, int64_t n, float lr,
                                                      float alpha, float oma, float eps, float wd, float mu, float sign,
                                                      const float* __restrict__ hyper) {
    if (hyper) lr = hyper[0];
    const int64_t nvec = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        v4f pv = *(const v4f*)&p[i * 4], sv = *(const v4f*)&sq[i * 4];
        const v4f gv = *(const v4f*)&g[i * 4];
        v4f av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (CEN) av = *(const v4f*)&gavg[i * 4];
        if constexpr (MOM) bv = *(const v4f*)&buf[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], sj = sv[j], aj = av[j], bj = bv[j];
            rms_one<CEN, MOM>(pj, gv[j], sj, aj, bj, lr, alpha, oma, eps, wd, mu, sign);
            pv[j] = pj;
            sv[j] = sj;
            av[j] = aj;
            bv[j] = bj;
        }
        *(v4f*)&p[i * 4] = pv;
        *(v4f*)&sq[i * 4] = sv;
        if constexpr (CEN) *(v4f*)&gavg[i * 4] = av;
        if constexpr (MOM) *(v4f*)&buf[i * 4] = bv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = nvec * 4 + threadIdx.x;
        float pj = p[i], sj = sq[i], aj = 0.f, bj = 0.f;
        if constexpr (CEN) aj = gavg[i];
        if constexpr (MOM) bj = buf[i];
        rms_one<CEN, MOM>(pj, g[i], sj, aj, bj, lr, alpha, oma, eps, wd, mu, sign);
        p[i] = pj;
        sq[i] = sj;
        if constexpr (CEN) gavg[i] = aj;
        if constexpr (MOM) buf[i] = bj;
    }
}

// ------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam single-tensor update rule, coupled L2; adamw: decoupled)
// ------------------------------------------------------------------------------------------------
// ++step; hyper = {lr, lr / (1 - b1^step), sqrt(1 - b2^step)}: what koaf_adam_step derives on the host from (lr, step), derived
// on the device so that a captured (HIP-graph) optimizer step advances from replay to replay
__global__ void adam_hyper_kernel(int32_t* step, const float* lr, double b1, double b2, float* hyper) {
    const int st = *step + 1;
    *step = st;
    const double bc1 = 1.0 - pow(b1, (double)st), bc2 = 1.0 - pow(b2, (double)st);
    hyper[0] = *lr;
    hyper[1] = (float)((double)*lr / bc1);
    hyper[2] = (float)sqrt(bc2);
}

// torch.maximum: the larger one, and a NaN on either side stays (fmaxf would drop it, and amsgrad's maximum would come out finite
// beside a NaN second moment)
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float omb1, float b2, float omb2, float eps, float wd, float step_size,
                                                   float bc2_sqrt, int adamw, const float* __restrict__ hyper,
                                                   float* __restrict__ vmax) {
    // (omb1 = 1 - beta1 and omb2 = 1 - beta2 arrive rounded from the DOUBLE differences, as torch forms them: 1.f - 0.999f is
    // 1.3e-5 away from float(1 - 0.999), which showed in the second moments)
    if (hyper) { lr = hyper[0]; step_size = hyper[1]; bc2_sqrt = hyper[2]; }   // device-resident step state (koaf_adam_hyper)
    const int64_t nvec = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EB) {
        v4f pv = *(const v4f*)&p[i * 4], gv = *(const v4f*)&g[i * 4];
        v4f mv = *(const v4f*)&m[i * 4], vv = *(const v4f*)&v[i * 4];
        v4f xv = {0.f, 0.f, 0.f, 0.f};
        if (vmax) xv = *(const v4f*)&vmax[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gj = gv[j], pj = pv[j];
            if (adamw) pj *= (1.f - lr * wd);
            else gj += wd * pj;
            const float mj = mv[j] + (gj - mv[j]) * omb1;
            const float vj = vv[j] * b2 + omb2 * gj * gj;
            float vd = vj;
            if (vmax) { vd = max_nan(xv[j], vj); xv[j] = vd; }   // amsgrad: the running maximum of the second moment
            const float denom = sqrtf(vd) / bc2_sqrt + eps;
            pv[j] = pj - step_size * (mj / denom);
            mv[j] = mj;
            vv[j] = vj;
        }
        *(v4f*)&p[i * 4] = pv;
        *(v4f*)&m[i * 4] = mv;
        *(v4f*)&v[i * 4] = vv;
        if (vmax) *(v4f*)&vmax[i * 4] = xv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = nvec * 4 + threadIdx.x;
        float gj = g[i], pj = p[i];
        if (adamw) pj *= (1.f - lr * wd);
        else gj += wd * pj;
        const float mj = m[i] + (gj - m[i]) * omb1;
        const float vj = v[i] * b2 + omb2 * gj * gj;
        float vd = vj;
        if (vmax) { vd = max_nan(vmax[i], vj); vmax[i] = vd; }
        p[i] = pj - step_size * (mj / (sqrtf(vd) / bc2_sqrt + eps));
        m[i] = mj;
        v[i] = vj;
    }
}

// ------------------------------------------------------------------------------------------------
// Gradient accumulation over micro-batches and global-norm clipping, on flat fp32 ranges of the arena.  Streaming kernels
// shaped like the ones above (16-byte accesses, a scalar tail), but every block owns one FIXED chunk of GN_CHUNK elements:
// the norm is a two-stage reduction whose partials (one per chunk, slot = chunk index) must not depend on the grid, so that
// the bits repeat from run to run.  No atomics anywhere.
//   fold     mode 0: acc = w * g;  1: acc = acc + w * g;  2: g = acc + w * g (the last micro-batch, written back into G, and
//            optionally the norm partials of what it writes).  Product and sum are rounded separately (contraction off: no fused multiply-add),
//            so that numpy restates them: np.float32(w) * g, then +.
//   norm     2-norm: squares and sums in fp64 (the square of an fp32 value is exact there and cannot overflow);
//            inf-norm: an integer maximum over the magnitude bits (koaf_absbits: a NaN compares above +Inf and survives).
//   final    one block adds / maximises all partials in index order -> norm[0], coef[0] = min(1, max_norm / (norm + 1e-6f))
//   scale    g *= coef[0] read from the device; a block whose coef is exactly 1 leaves without touching memory.
// ------------------------------------------------------------------------------------------------
constexpr int GN_CHUNK = 16384;         // elements per block (64 KiB per operand: 16 dwordx4 accesses per lane)
constexpr int GN_NONE = -1, GN_L2 = 0, GN_INF = 1;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one norm term: KIND GN_L2 adds x^2 to sq, GN_INF raises mx to |x|'s bits
template <int KIND>
__device__ __forceinline__ void gn_term(float x, double& sq, unsigned& mx) {
    if constexpr (KIND == GN_L2) sq += (double)x * (double)x;
    if constexpr (KIND == GN_INF) { const unsigned b = koaf_absbits(x); mx = mx > b ? mx : b; }
}

// the block's partial -> its 8-byte workspace slot (an fp64 sum, or the magnitude bits widened to 64): fixed lane / wave order
template <int KIND>
__device__ __forceinline__ void gn_block_partial(double sq, unsigned mx, void* __restrict__ ws) {
    if constexpr (KIND == GN_L2) {
        __shared__ double red[4];
        sq = wave_sum_f64(sq);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) ((double*)ws)[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
    if constexpr (KIND == GN_INF) {
        __shared__ unsigned redu[4];
        mx = wave_max_u(mx);
        if ((threadIdx.x & 63) == 0) redu[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = redu[0];
            for (int i = 1; i < 4; ++i) m = m > redu[i] ? m : redu[i];
            ((unsigned long long*)ws)[blockIdx.x] = m;
        }
    }
}

template <int MODE>
__device__ __forceinline__ float fold_one(float a, float g, float w) {
#pragma clang fp contract(off)          // the product rounds first: no fma (hipcc contracts __fmul_rn + __fadd_rn like any a * b + c)
    const float wg = w * g;
    return MODE == 0 ? wg : a + wg;
}

template <int MODE, int KIND>
__global__ void __launch_bounds__(256) grad_fold_kernel(float* __restrict__ acc, float* __restrict__ g, int64_t n, float w,
                                                        void* __restrict__ ws) {
    const int64_t e0 = (int64_t)blockIdx.x * GN_CHUNK, e1 = e0 + GN_CHUNK < n ? e0 + GN_CHUNK : n;
    const int64_t v1 = e1 / 4;          // (e0 is a multiple of 4: only the last block has a scalar tail)
    float* __restrict__ dst = MODE == 2 ? g : acc;
    double sq = 0.0;
    unsigned mx = 0u;
#pragma unroll 4
    for (int64_t i = e0 / 4 + threadIdx.x; i < v1; i += EB) {
        const v4f gv = *(const v4f*)&g[i * 4];
        v4f av = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE != 0) av = *(const v4f*)&acc[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            av[j] = fold_one<MODE>(av[j], gv[j], w);
            gn_term<KIND>(av[j], sq, mx);
        }
        *(v4f*)&dst[i * 4] = av;
    }
    const int64_t i = v1 * 4 + threadIdx.x;
    if (i < e1) {
        const float r = fold_one<MODE>(MODE != 0 ? acc[i] : 0.f, g[i], w);
        gn_term<KIND>(r, sq, mx);
        dst[i] = r;
    }
    gn_block_partial<KIND>(sq, mx, ws);
}

template <int KIND>
__global__ void __launch_bounds__(256) grad_norm_part_kernel(const float* __restrict__ g, int64_t n, void* __restrict__ ws) {
    const int64_t e0 = (int64_t)blockIdx.x * GN_CHUNK, e1 = e0 + GN_CHUNK < n ? e0 + GN_CHUNK : n;
    const int64_t v1 = e1 / 4;
    double sq = 0.0;
    unsigned mx = 0u;
#pragma unroll 4
    for (int64_t i = e0 / 4 + threadIdx.x; i < v1; i += EB) {
        const v4f gv = *(const v4f*)&g[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gn_term<KIND>(gv[j], sq, mx);
    }
    const int64_t i = v1 * 4 + threadIdx.x;
    if (i < e1) gn_term<KIND>(g[i], sq, mx);
    gn_block_partial<KIND>(sq, mx, ws);
}

// all partials (of every range, laid end to end) -> norm, coef.  Lane t takes slots t, t + 256, ... in rising order, then the
// fixed wave / block order: the same bits whatever the scheduling.  c > 1 ? 1 : c keeps a NaN (fminf would drop it).
template <int KIND>
__global__ void __launch_bounds__(256) grad_norm_final_kernel(const void* __restrict__ ws, int64_t nparts, float max_norm,
                                                              float* __restrict__ norm, float* __restrict__ coef) {
    double sq = 0.0;
    unsigned mx = 0u;
    for (int64_t i = threadIdx.x; i < nparts; i += EB) {
        if constexpr (KIND == GN_L2) sq += ((const double*)ws)[i];
        if constexpr (KIND == GN_INF) { const unsigned b = (unsigned)((const unsigned long long*)ws)[i]; mx = mx > b ? mx : b; }
    }
    float nv;
    if constexpr (KIND == GN_L2) {
        __shared__ double red[4];
        sq = wave_sum_f64(sq);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        nv = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
    } else {
        __shared__ unsigned redu[4];
        mx = wave_max_u(mx);
        if ((threadIdx.x & 63) == 0) redu[threadIdx.x >> 6] = mx;
        __syncthreads();
        unsigned m = redu[0];
        for (int i = 1; i < 4; ++i) m = m > redu[i] ? m : redu[i];
        nv = __uint_as_float(m);
    }
    if (threadIdx.x == 0) {
        norm[0] = nv;
        if (coef) {
            const float c = __fdiv_rn(max_norm, __fadd_rn(nv, 1e-6f));
            coef[0] = c > 1.f ? 1.f : c;
        }
    }
}

__global__ void __launch_bounds__(256) grad_scale_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ coef) {
    const float c = coef[0];
    if (c == 1.f) return;               // not clipped: one scalar read per block, no traffic
    const int64_t e0 = (int64_t)blockIdx.x * GN_CHUNK, e1 = e0 + GN_CHUNK < n ? e0 + GN_CHUNK : n;
    const int64_t v1 = e1 / 4;
#pragma unroll 4
    for (int64_t i = e0 / 4 + threadIdx.x; i < v1; i += EB) {
        v4f gv = *(const v4f*)&g[i * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = __fmul_rn(gv[j], c);
        *(v4f*)&g[i * 4] = gv;
    }
    const int64_t i = v1 * 4 + threadIdx.x;
    if (i < e1) g[i] = __fmul_rn(g[i], c);
}

inline int64_t gn_blocks(int64_t n) { return cdiv64(n, GN_CHUNK); }

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" int koaf_optim_hyper(int32_t* step, const float* lr, float* hyper, void* stream) {
    KOAF_REQUIRE(step && lr && hyper, "koaf_optim_hyper: bad args");
    hipLaunchKernelGGL(optim_hyper_kernel, dim3(1), dim3(1), 0, STREAM, step, lr, hyper);
    return koaf_check_launch("koaf_optim_hyper");
}

extern "C" int koaf_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, double momentum, double dampening,
                             float weight_decay, int32_t nesterov, int32_t maximize, int32_t first, const float* hyper,
                             void* stream) {
    KOAF_REQUIRE(p && g && n > 0, "koaf_sgd_step: bad args");
    KOAF_REQUIRE(momentum == 0.0 || buf, "koaf_sgd_step: momentum needs its buffer");
    KOAF_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "koaf_sgd_step: Nesterov needs a momentum and no dampening");
    KOAF_REQUIRE(aligned16(p) && aligned16(g) && (!buf || aligned16(buf)), "koaf_sgd_step: unaligned");
    const dim3 grid(ew_grid(n / 4 + 1)), block(EB);
    const float mu = (float)momentum, omd = (float)(1.0 - dampening), sign = maximize ? -1.f : 1.f;
    const int fi = first ? 1 : 0;
    if (momentum == 0.0)
        hipLaunchKernelGGL((sgd_kernel<false, false>), grid, block, 0, STREAM, p, g, (float*)nullptr, n, lr, mu, omd, weight_decay, sign, fi, hyper);
    else if (nesterov)
        hipLaunchKernelGGL((sgd_kernel<true, true>), grid, block, 0, STREAM, p, g, buf, n, lr, mu, omd, weight_decay, sign, fi, hyper);
    else
        hipLaunchKernelGGL((sgd_kernel<true, false>), grid, block, 0, STREAM, p, g, buf, n, lr, mu, omd, weight_decay, sign, fi, hyper);
    return koaf_check_launch("koaf_sgd_step");
}

extern "C" int koaf_rmsprop_step(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, float lr, double alpha,
                                 float eps, float weight_decay, double momentum, int32_t maximize, const float* hyper,
                                 void* stream) {
    KOAF_REQUIRE(p && g && sq && n > 0, "koaf_rmsprop_step: bad args");
    KOAF_REQUIRE((momentum > 0.0) == (buf != nullptr), "koaf_rmsprop_step: a momentum and its buffer come together");
    KOAF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(sq) && (!gavg || aligned16(gavg)) && (!buf || aligned16(buf)),
                 "koaf_rmsprop_step: unaligned");
    const dim3 grid(ew_grid(n / 4 + 1)), block(EB);
    const float al = (float)alpha, oma = (float)(1.0 - alpha), mu = (float)momentum, sign = maximize ? -1.f : 1.f;
#define KOAF_RMS(CEN, MOM)                                                                                                  \
    hipLaunchKernelGGL((rmsprop_kernel<CEN, MOM>), grid, block, 0, STREAM, p, g, sq, gavg, buf, n, lr, al, oma, eps, weight_decay, \
                       mu, sign, hyper)
    if (gavg && buf) KOAF_RMS(true, true);
    else if (gavg) KOAF_RMS(true, false);
    else if (buf) KOAF_RMS(false, true);
    else KOAF_RMS(false, false);
#undef KOAF_RMS
    return koaf_check_launch("koaf_rmsprop_step");
}

extern "C" int koaf_adam_hyper(int32_t* step, const float* lr, double beta1, double beta2, float* hyper, void* stream) {
    KOAF_REQUIRE(step && lr && hyper, "koaf_adam_hyper: bad args");
    hipLaunchKernelGGL(adam_hyper_kernel, dim3(1), dim3(1), 0, STREAM, step, lr, beta1, beta2, hyper);
    return koaf_check_launch("koaf_adam_hyper");
}
extern "C" int koaf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1,
                              double beta2, float eps, float weight_decay, int32_t step, int32_t adamw,
                              const float* hyper, float* vmax, void* stream) {
    if (hyper) step = 1;      // (lr / step come from the device; the host values are ignored)
    KOAF_REQUIRE(p && g && m && v && n > 0 && step >= 1, "koaf_adam_step: bad args");
    KOAF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!vmax || aligned16(vmax)),
                 "koaf_adam_step: unaligned");
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n / 4 + 1)), dim3(EB), 0, STREAM, p, g, m, v, n, lr, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), eps, weight_decay, step_size, bc2_sqrt, adamw, hyper, vmax);
    return koaf_check_launch("koaf_adam_step");
}

extern "C" int64_t koaf_grad_norm_ws(int64_t n) { return n > 0 ? 2 * gn_blocks(n) : 0; }      // (one 8-byte partial per block)

extern "C" int koaf_grad_fold(float* acc, float* g, int64_t n, float w, int32_t mode, int32_t norm_kind, float* ws, void* stream) {
    KOAF_REQUIRE(acc && g && n > 0, "koaf_grad_fold: bad args");
    KOAF_REQUIRE(mode >= 0 && mode <= 2, "koaf_grad_fold: mode is 0 (acc = w g), 1 (acc += w g) or 2 (g = acc + w g)");
    KOAF_REQUIRE(!ws || (mode == 2 && (norm_kind == GN_L2 || norm_kind == GN_INF)),
                 "koaf_grad_fold: norm partials come with mode 2 and a norm kind of 0 (2-norm) or 1 (inf-norm)");
    KOAF_REQUIRE(aligned16(acc) && aligned16(g), "koaf_grad_fold: unaligned");
    KOAF_REQUIRE((((uintptr_t)ws) & 7) == 0, "koaf_grad_fold: the workspace is 8-byte aligned");
    KOAF_REQUIRE(gn_blocks(n) < (1ll << 31), "koaf_grad_fold: range too long");
    const dim3 grid((unsigned)gn_blocks(n)), block(EB);
#define KOAF_FOLD(MODE, KIND) hipLaunchKernelGGL((grad_fold_kernel<MODE, KIND>), grid, block, 0, STREAM, acc, g, n, w, (void*)ws)
    if (mode == 0) KOAF_FOLD(0, GN_NONE);
    else if (mode == 1) KOAF_FOLD(1, GN_NONE);
    else if (!ws) KOAF_FOLD(2, GN_NONE);
    else if (norm_kind == GN_L2) KOAF_FOLD(2, GN_L2);
    else KOAF_FOLD(2, GN_INF);
#undef KOAF_FOLD
    return koaf_check_launch("koaf_grad_fold");
}

extern "C" int koaf_grad_norm_part(const float* g, int64_t n, int32_t norm_kind, float* ws, void* stream) {
    KOAF_REQUIRE(g && ws && n > 0, "koaf_grad_norm_part: bad args");
    KOAF_REQUIRE(norm_kind == GN_L2 || norm_kind == GN_INF, "koaf_grad_norm_part: the norm kind is 0 (2-norm) or 1 (inf-norm)");
    KOAF_REQUIRE(aligned16(g), "koaf_grad_norm_part: unaligned");
    KOAF_REQUIRE((((uintptr_t)ws) & 7) == 0, "koaf_grad_norm_part: the workspace is 8-byte aligned");
    KOAF_REQUIRE(gn_blocks(n) < (1ll << 31), "koaf_grad_norm_part: range too long");
    const dim3 grid((unsigned)gn_blocks(n)), block(EB);
    if (norm_kind == GN_L2) hipLaunchKernelGGL(grad_norm_part_kernel<GN_L2>, grid, block, 0, STREAM, g, n, (void*)ws);
    else hipLaunchKernelGGL(grad_norm_part_kernel<GN_INF>, grid, block, 0, STREAM, g, n, (void*)ws);
    return koaf_check_launch("koaf_grad_norm_part");
}

extern "C" int koaf_grad_norm_final(const float* ws, int64_t nws, int32_t norm_kind, float max_norm, float* norm, float* coef,
                                    void* stream) {
    KOAF_REQUIRE(ws && norm && nws > 0 && (nws & 1) == 0, "koaf_grad_norm_final: bad args");
    KOAF_REQUIRE(norm_kind == GN_L2 || norm_kind == GN_INF, "koaf_grad_norm_final: the norm kind is 0 (2-norm) or 1 (inf-norm)");
    KOAF_REQUIRE((((uintptr_t)ws) & 7) == 0, "koaf_grad_norm_final: the workspace is 8-byte aligned");
    if (norm_kind == GN_L2)
        hipLaunchKernelGGL(grad_norm_final_kernel<GN_L2>, dim3(1), dim3(EB), 0, STREAM, (const void*)ws, nws / 2, max_norm, norm, coef);
    else
        hipLaunchKernelGGL(grad_norm_final_kernel<GN_INF>, dim3(1), dim3(EB), 0, STREAM, (const void*)ws, nws / 2, max_norm, norm, coef);
    return koaf_check_launch("koaf_grad_norm_final");
}

extern "C" int koaf_grad_scale(float* g, int64_t n, const float* coef, void* stream) {
    KOAF_REQUIRE(g && coef && n > 0, "koaf_grad_scale: bad args");
    KOAF_REQUIRE(aligned16(g), "koaf_grad_scale: unaligned");
    KOAF_REQUIRE(gn_blocks(n) < (1ll << 31), "koaf_grad_scale: range too long");
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)gn_blocks(n)), dim3(EB), 0, STREAM, g, n, coef);
    return koaf_check_launch("koaf_grad_scale");
}
