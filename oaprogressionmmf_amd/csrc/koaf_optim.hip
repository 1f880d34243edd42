// koaf_optim.hip -- the registry's other two optimizers (koafusion/various/_optimizers.py:47-52: "SGD", "RMSprop") as one-pass
// streams over the flat parameter arena, shaped like adam_kernel (koaf_elem.hip): 16-byte loads and stores, a grid-stride loop,
// a scalar tail; every operand is read once and every updated one written once.  The options that do not change from launch to
// launch (momentum / Nesterov / centered / ...) are template parameters, so each variant carries only its own loads and stores.
#include "koaf_common.h"

namespace {

constexpr int EB = 256;  // elementwise block

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

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
#define STREAM ((hipStream_t)stream)

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
