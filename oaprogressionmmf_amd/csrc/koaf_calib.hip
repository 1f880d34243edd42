// koaf_calib.hip -- calibration of a binary model's predicted probabilities on the device: Brier score, log-loss, the reliability
// table with ECE / MCE, net benefit over a threshold list (decision curves), the quantile bin edges, and logistic recalibration
// (calibration intercept / slope, temperature scaling, calibration-in-the-large) -- for the sample itself and for R bootstrap
// resamples, one block per row, as koaf_metrics.hip does it for the discrimination metrics.  The reference has no such code: the
// definitions are scikit-learn's (brier_score_loss, log_loss, calibration_curve) and numpy's (percentile).
// Everything is fp64.  Counts are integers (LDS integer atomics, per-thread counters); every fp64 sum has one owner and a fixed
// order: thread t adds the draws [t L, (t + 1) L) of its row, L = ceil(m / 256), in row order, then a fixed tree runs over the 256
// threads.  No floating-point atomics, no contraction into FMA: the same bits from run to run.  Every loop bound is a constant or
// an argument.
#include "koaf_common.h"

namespace {

constexpr int CB_BLOCK = 256;
constexpr int CB_MAX_N = KOAF_METRICS_MAX_N;
constexpr int CB_MAX_BINS = KOAF_CALIB_MAX_BINS;
constexpr int CB_MAX_THR = KOAF_CALIB_MAX_THR;
constexpr int CB_TILE = 2048;            // scores per LDS tile of the edges kernel
constexpr int CB_GROUP = 8;              // bins whose score sums one pass over the row forms
constexpr double CB_DBL_MAX = 1.7976931348623157e308;
// "L does not increase" up to the rounding of L itself: a sum 64 + 8 additions deep over terms that carry a few ulp each is good to
// about 128 * 2^-52 of its value, and near the optimum a Newton step changes L by less than that
constexpr double CB_L_SLACK = 0x1p-45;

__device__ __forceinline__ double cb_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool cb_finite(double v) { return fabs(v) <= CB_DBL_MAX; }
__device__ __forceinline__ double cb_clip(double p, double eps) {
#pragma clang fp contract(off)
    const double hi = 1.0 - eps;
    return p < eps ? eps : (p > hi ? hi : p);
}

// the row of block r: its draws (idx row, or nullptr for the identity) and how many they are
__device__ __forceinline__ const int32_t* cb_row(const int32_t* idx, int r, int n, int m, int with_identity, int& draws) {
    draws = n;
    if (idx == nullptr || (with_identity && r == 0)) return nullptr;
    draws = m;
    return idx + (int64_t)(r - (with_identity ? 1 : 0)) * m;
}

// the run of draws thread t owns: [d0, d1) = [t L, min(draws, (t + 1) L))
__device__ __forceinline__ void cb_run(int draws, int& d0, int& d1) {
    const int L = (draws + CB_BLOCK - 1) / CB_BLOCK;
    d0 = (int)threadIdx.x * L < draws ? (int)threadIdx.x * L : draws;
    d1 = d0 + L < draws ? d0 + L : draws;
}

// the fixed tree over the 256 threads of K sums held as red[k * 256 + t]; the totals land in red[k * 256]
template <int K>
__device__ __forceinline__ void cb_tree(double* red) {
#pragma clang fp contract(off)
    __syncthreads();
    for (int o = CB_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k * CB_BLOCK + threadIdx.x] += red[k * CB_BLOCK + threadIdx.x + o];
        }
        __syncthreads();
    }
}

// ---- quantile bin edges ------------------------------------------------------------------------------------------------------
// np.percentile(scores, 100 q) with the default linear method, without a sort: element i is the order statistic of every position
// k with less_i <= k < leq_i (less_i / leq_i: how many scores lie below it / at or below it, all-pairs counting through LDS
// tiles as koaf_score_ranks counts); the two neighbours of each virtual index h = q (n - 1) are picked by those counts (tied
// elements write the same value) and joined by numpy's two-sided lerp.  One block.
template <typename T>
__global__ void __launch_bounds__(CB_BLOCK) calib_edges_kernel(const T* __restrict__ s, int64_t stride, int n,
                                                               const double* __restrict__ q, int nq, double* __restrict__ edges,
                                                               uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ T tile[CB_TILE];
    __shared__ double s_h[CB_MAX_BINS + 1], s_a[CB_MAX_BINS + 1], s_b[CB_MAX_BINS + 1];
    __shared__ int s_lo[CB_MAX_BINS + 1], s_hi[CB_MAX_BINS + 1];
    if ((int)threadIdx.x < nq) {
        const double h = q[threadIdx.x] * (double)(n - 1);
        int lo = n - 1, hi = n - 1;                     // (h >= n - 1, or a NaN fraction: numpy takes the last element twice)
        if (h < 0.0) lo = hi = 0;
        else if (h < (double)(n - 1)) { lo = (int)floor(h); hi = lo + 1; }
        s_h[threadIdx.x] = h;
        s_lo[threadIdx.x] = lo;
        s_hi[threadIdx.x] = hi;
        s_a[threadIdx.x] = s_b[threadIdx.x] = cb_nan();
    }
    unsigned bad = 0;
    const int E = (n + CB_BLOCK - 1) / CB_BLOCK;
    for (int e = 0; e < E; ++e) {
        const int i = e * CB_BLOCK + threadIdx.x;
        const T mine = i < n ? s[(int64_t)i * stride] : (T)0;
        int less = 0, leq = 0;
        for (int t0 = 0; t0 < n; t0 += CB_TILE) {
            const int len = n - t0 < CB_TILE ? n - t0 : CB_TILE;
            __syncthreads();
            for (int j = threadIdx.x; j < len; j += CB_BLOCK) tile[j] = s[(int64_t)(t0 + j) * stride];
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < len; ++j) {
                const T v = tile[j];
                less += v < mine ? 1 : 0;
                leq += v <= mine ? 1 : 0;
            }
        }
        if (i < n) {
            if (!cb_finite((double)mine)) bad |= 1u;
            for (int k = 0; k < nq; ++k) {
                if (less <= s_lo[k] && s_lo[k] < leq) s_a[k] = (double)mine;
                if (less <= s_hi[k] && s_hi[k] < leq) s_b[k] = (double)mine;
            }
        }
    }
    if (bad) atomicOr(flag, bad);
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        const double a = s_a[threadIdx.x], b = s_b[threadIdx.x];
        const double t = s_h[threadIdx.x] - (double)s_lo[threadIdx.x];      // (a == b at and beyond the ends: t then weighs 0)
        const double d = b - a;
        double v = a + d * t;
        if (t >= 0.5) v = b - d * (1.0 - t);
        edges[threadIdx.x] = v;
    }
}

// ---- calibration metrics of R resamples ----------------------------------------------------------------------------------
// Block r: one pass over the row's draws for the scalar sums, the bin of every draw (kept in LDS) with the bins' integer counts,
// and the threshold histogram; then one pass per group of 8 bins for the bins' score sums.  See koaf.h for the outputs.
// Net benefit of the prediction p >= t: with c(p) = #{k : thr[k] <= p} and r_k = #{j : thr[j] <= thr[k]}, p >= thr[k] exactly
// when c(p) >= r_k, so one integer histogram over c per class serves every threshold, sorted or not.
__device__ __forceinline__ double cb_net_benefit(double tp, double fp, double dm, double t) {
#pragma clang fp contract(off)
    const double a = tp / dm, b = fp / dm, w = t / (1.0 - t);
    return a - b * w;
}

template <typename T>
__global__ void __launch_bounds__(CB_BLOCK) calib_metrics_kernel(const T* __restrict__ s, int64_t stride,
                                                                 const int32_t* __restrict__ labels, int n,
                                                                 const double* __restrict__ edges, int nbins,
                                                                 const double* __restrict__ thr, int nthr,
                                                                 const int32_t* __restrict__ idx, int m, int with_identity,
                                                                 double eps, double* __restrict__ out, double* __restrict__ bins,
                                                                 double* __restrict__ nb, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ double red[CB_GROUP * CB_BLOCK];
    __shared__ uint8_t s_bin[CB_MAX_N];
    __shared__ double s_edge[CB_MAX_BINS + 1], s_thr[CB_MAX_THR], s_sp[CB_MAX_BINS];
    __shared__ int s_cnt[CB_MAX_BINS], s_pos[CB_MAX_BINS];
    __shared__ int s_hist[2][CB_MAX_THR + 1];
    __shared__ int s_P, s_N;
    const int r = blockIdx.x;
    int draws;
    const int32_t* row = cb_row(idx, r, n, m, with_identity, draws);
    for (int k = threadIdx.x; k <= nbins; k += CB_BLOCK) s_edge[k] = edges[k];
    for (int k = threadIdx.x; k < nbins; k += CB_BLOCK) { s_cnt[k] = 0; s_pos[k] = 0; }
    for (int k = threadIdx.x; k < nthr; k += CB_BLOCK) s_thr[k] = thr[k];
    for (int k = threadIdx.x; k <= nthr; k += CB_BLOCK) { s_hist[0][k] = 0; s_hist[1][k] = 0; }
    if (threadIdx.x == 0) { s_P = 0; s_N = 0; }
    __syncthreads();
    int d0, d1;
    cb_run(draws, d0, d1);
    double brier = 0.0, ll = 0.0, sp = 0.0;
    int P = 0, N = 0;
    unsigned bad = 0;
    for (int d = d0; d < d1; ++d) {
        const int i = row ? row[d] : d;
        if ((unsigned)i >= (unsigned)n) { bad |= 4u; s_bin[d] = 0xffu; continue; }
        const double p = (double)s[(int64_t)i * stride];
        const int32_t l = labels[i];
        if (!cb_finite(p)) bad |= 1u;
        if (l != 0 && l != 1) bad |= 2u;
        const int y = l == 1 ? 1 : 0;
        const double e = p - (double)y;
        brier += e * e;
        ll += -log(cb_clip(y ? p : 1.0 - p, eps));
        sp += p;
        P += y;
        N += 1 - y;
        int b = 0;
        for (int k = 1; k < nbins; ++k) b += s_edge[k] < p ? 1 : 0;
        s_bin[d] = (uint8_t)b;
        atomicAdd(&s_cnt[b], 1);
        if (y) atomicAdd(&s_pos[b], 1);
        if (nthr > 0) {
            int c = 0;
            for (int k = 0; k < nthr; ++k) c += s_thr[k] <= p ? 1 : 0;
            atomicAdd(&s_hist[y][c], 1);
        }
    }
    if (bad) atomicOr(flag, bad);
    if (P) atomicAdd(&s_P, P);
    if (N) atomicAdd(&s_N, N);
    red[threadIdx.x] = brier;
    red[CB_BLOCK + threadIdx.x] = ll;
    red[2 * CB_BLOCK + threadIdx.x] = sp;
    cb_tree<3>(red);
    const double dm = (double)draws;
    const double t_brier = red[0], t_ll = red[CB_BLOCK], t_sp = red[2 * CB_BLOCK];
    // the bins' score sums, 8 bins per pass: the draw's bin comes from LDS, its score is read again
    for (int b0 = 0; b0 < nbins; b0 += CB_GROUP) {
        double acc[CB_GROUP];
#pragma unroll
        for (int g = 0; g < CB_GROUP; ++g) acc[g] = 0.0;
        for (int d = d0; d < d1; ++d) {
            const int b = (int)s_bin[d] - b0;
            if ((unsigned)b >= (unsigned)CB_GROUP) continue;            // (another group's bin, or a skipped draw)
            const double p = (double)s[(int64_t)(row ? row[d] : d) * stride];
#pragma unroll
            for (int g = 0; g < CB_GROUP; ++g)
                if (b == g) acc[g] += p;
        }
        __syncthreads();                       // (the previous group's totals have been read)
#pragma unroll
        for (int g = 0; g < CB_GROUP; ++g) red[g * CB_BLOCK + threadIdx.x] = acc[g];
        cb_tree<CB_GROUP>(red);
        if ((int)threadIdx.x < CB_GROUP && b0 + (int)threadIdx.x < nbins) s_sp[b0 + threadIdx.x] = red[threadIdx.x * CB_BLOCK];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ece = 0.0, mce = 0.0;
        int used = 0;
        for (int b = 0; b < nbins; ++b) {
            if (s_cnt[b] == 0) continue;
            const double gap = fabs((double)s_pos[b] - s_sp[b]);
            ece += gap;
            const double g = gap / (double)s_cnt[b];
            if (g > mce) mce = g;
            ++used;
        }
        double* o = out + (int64_t)r * 8;
        o[0] = (double)s_P;
        o[1] = (double)s_N;
        o[2] = t_brier / dm;
        o[3] = t_ll / dm;
        o[4] = t_sp / dm;
        o[5] = ece / dm;
        o[6] = mce;
        o[7] = (double)used;
    }
    if (bins != nullptr)
        for (int b = threadIdx.x; b < nbins; b += CB_BLOCK) {
            double* o = bins + ((int64_t)r * nbins + b) * 3;
            o[0] = (double)s_cnt[b];
            o[1] = (double)s_pos[b];
            o[2] = s_sp[b];
        }
    if (nb != nullptr)
        for (int k = threadIdx.x; k < nthr; k += CB_BLOCK) {
            const double t = s_thr[k];
            int rk = 0;
            for (int j = 0; j < nthr; ++j) rk += s_thr[j] <= t ? 1 : 0;
            int tp = 0, fp = 0;
            for (int c = rk; c <= nthr; ++c) { tp += s_hist[1][c]; fp += s_hist[0][c]; }
            double* o = nb + ((int64_t)r * nthr + k) * 4;
            o[0] = (double)tp;
            o[1] = (double)fp;
            o[2] = cb_net_benefit((double)tp, (double)fp, dm, t);
            o[3] = cb_net_benefit((double)s_P, (double)s_N, dm, t);       // treat all: the same expression at tp = P, fp = N
        }
}

// ---- logistic recalibration ------------------------------------------------------------------------------------------------
// x of one sample: the logit of the clipped probability (kind 0), or the score itself minus the optional second column (kind 1)
template <typename T>
__device__ __forceinline__ double cb_x(const T* __restrict__ s, int64_t stride, const T* __restrict__ s0, int64_t stride0,
                                       int64_t i, int kind, double eps, unsigned& bad) {
#pragma clang fp contract(off)
    const double v = (double)s[i * stride];
    if (!cb_finite(v)) bad |= 1u;
    if (kind == 0) {
        const double p = cb_clip(v, eps);
        return log(p) - log1p(-p);
    }
    if (s0 == nullptr) return v;
    const double v0 = (double)s0[i * stride0];
    if (!cb_finite(v0)) bad |= 1u;
    return v - v0;
}

// sigma(eta) and softplus(eta) without overflow: both from e = exp(-|eta|)
__device__ __forceinline__ void cb_sigmoid(double eta, double& sig, double& softplus) {
#pragma clang fp contract(off)
    const double e = exp(-fabs(eta));
    const double den = 1.0 + e;
    sig = eta >= 0.0 ? 1.0 / den : e / den;
    softplus = (eta > 0.0 ? eta : 0.0) + log1p(e);
}

// Block r: Newton on L(a, b) = sum softplus(a + b x) - y (a + b x) over the row's draws.  Every evaluation is one pass over the
// row (x is formed again from the scores: nothing is kept per draw) and one tree over six sums; `sep` counts the draws the line
// does NOT put strictly on their class's side -- 0 means complete separation: no finite optimum in modes 0 and 1.
template <typename T>
__global__ void __launch_bounds__(CB_BLOCK) recalib_fit_kernel(const T* __restrict__ s, int64_t stride, const T* __restrict__ s0,
                                                               int64_t stride0, const int32_t* __restrict__ labels, int n,
                                                               int kind, int mode, const int32_t* __restrict__ idx, int m,
                                                               int with_identity, double eps, double tol, int max_iter,
                                                               double* __restrict__ report, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ double red[6 * CB_BLOCK];
    __shared__ int s_int[3];                  // P, N, sep
    const int r = blockIdx.x;
    int draws;
    const int32_t* row = cb_row(idx, r, n, m, with_identity, draws);
    int d0, d1;
    cb_run(draws, d0, d1);
    const double dm = (double)draws;
    unsigned bad = 0;
    double a = 0.0, b = 1.0, L = 0.0, ga = 0.0, gb = 0.0, haa = 0.0, hab = 0.0, hbb = 0.0, gmax = 0.0;
    int status = 1, it = 0, P = 0, N = 0, sep = 0;

    // one evaluation at (ea, eb): full = the gradient and the Hessian too.  All threads call it and all hold the totals after it.
    auto eval = [&](double ea, double eb, bool full, double& tL, double& tga, double& tgb, double& thaa, double& thab,
                    double& thbb) {
        double vL = 0.0, vga = 0.0, vgb = 0.0, vhaa = 0.0, vhab = 0.0, vhbb = 0.0;
        int cP = 0, cN = 0, cS = 0;
        for (int d = d0; d < d1; ++d) {
            const int i = row ? row[d] : d;
            if ((unsigned)i >= (unsigned)n) { bad |= 4u; continue; }
            const int32_t l = labels[i];
            if (l != 0 && l != 1) bad |= 2u;
            const int y = l == 1 ? 1 : 0;
            const double x = cb_x(s, stride, s0, stride0, (int64_t)i, kind, eps, bad);
            const double eta = ea + eb * x;
            double sig, spl;
            cb_sigmoid(eta, sig, spl);
            vL += y ? spl - eta : spl;
            cP += y;
            cN += 1 - y;
            cS += (y ? eta > 0.0 : eta < 0.0) ? 0 : 1;
            if (full) {
                const double res = sig - (double)y, w = sig * (1.0 - sig), wx = w * x;
                vga += res;
                vgb += res * x;
                vhaa += w;
                vhab += wx;
                vhbb += wx * x;
            }
        }
        __syncthreads();                       // (the totals of the previous evaluation have been read)
        if (threadIdx.x < 3) s_int[threadIdx.x] = 0;
        red[threadIdx.x] = vL;
        red[CB_BLOCK + threadIdx.x] = vga;
        red[2 * CB_BLOCK + threadIdx.x] = vgb;
        red[3 * CB_BLOCK + threadIdx.x] = vhaa;
        red[4 * CB_BLOCK + threadIdx.x] = vhab;
        red[5 * CB_BLOCK + threadIdx.x] = vhbb;
        __syncthreads();
        if (cP) atomicAdd(&s_int[0], cP);
        if (cN) atomicAdd(&s_int[1], cN);
        if (cS) atomicAdd(&s_int[2], cS);
        cb_tree<6>(red);
        tL = red[0];
        if (full) { tga = red[CB_BLOCK]; tgb = red[2 * CB_BLOCK]; thaa = red[3 * CB_BLOCK]; thab = red[4 * CB_BLOCK]; thbb = red[5 * CB_BLOCK]; }
        P = s_int[0];
        N = s_int[1];
        sep = s_int[2];
    };

    eval(a, b, true, L, ga, gb, haa, hab, hbb);
    if (P == 0 || N == 0) status = 3;
    else {
        for (it = 0; it <= max_iter; ++it) {                              // (uniform: every thread holds the same totals)
            const double fa = mode == 1 ? 0.0 : fabs(ga), fb = mode == 2 ? 0.0 : fabs(gb);
            gmax = (fa > fb ? fa : fb) / dm;
            if (!cb_finite(L) || !cb_finite(gmax)) { status = 2; break; }
            if (mode != 2 && sep == 0) { status = 2; break; }             // complete separation: L has no finite minimum
            if (gmax <= tol) { status = 0; break; }
            if (it == max_iter) { status = 1; break; }
            double da = 0.0, db = 0.0;
            if (mode == 0) {
                const double det = haa * hbb - hab * hab;
                if (!(haa > 0.0) || !(det > 0.0)) { status = 2; break; }
                da = (hbb * ga - hab * gb) / det;
                db = (haa * gb - hab * ga) / det;
            } else if (mode == 1) {
                if (!(hbb > 0.0)) { status = 2; break; }
                db = gb / hbb;
            } else {
                if (!(haa > 0.0)) { status = 2; break; }
                da = ga / haa;
            }
            double step = 1.0, na = a, nb_ = b, nL = L, u0, u1, u2, u3, u4;
            const double slack = CB_L_SLACK * fabs(L);                    // what the sum's own rounding may add to an equal L
            bool took = false;
            for (int h = 0; h <= 30; ++h) {                               // the full step, then at most 30 halvings
                na = a - step * da;
                nb_ = b - step * db;
                eval(na, nb_, false, nL, u0, u1, u2, u3, u4);
                if (nL <= L + slack) { took = true; break; }
                step *= 0.5;
            }
            if (!took) { status = 1; break; }                             // no step lowers L: the rounding floor of L is reached
            if (!cb_finite(na) || !cb_finite(nb_)) { status = 2; break; }
            a = na;
            b = nb_;
            eval(a, b, true, L, ga, gb, haa, hab, hbb);
        }
    }
    if (bad) atomicOr(flag, bad);
    if (threadIdx.x == 0) {
        if (status != 0) atomicOr(flag, 8u);
        double* o = report + (int64_t)r * 8;
        o[0] = status >= 2 ? cb_nan() : a;
        o[1] = status >= 2 ? cb_nan() : b;
        o[2] = (double)(it > max_iter ? max_iter : it);
        o[3] = status == 3 ? cb_nan() : gmax;
        o[4] = status == 3 ? cb_nan() : L / dm;
        o[5] = (double)status;
        o[6] = (double)P;
        o[7] = (double)N;
    }
}

template <typename T>
__global__ void __launch_bounds__(CB_BLOCK) recalib_apply_kernel(const T* __restrict__ s, int64_t stride, const T* __restrict__ s0,
                                                                 int64_t stride0, int64_t n, int kind, double a, double b, double eps,
                                                                 double* __restrict__ out, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    unsigned bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * CB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB_BLOCK) {
        const double x = cb_x(s, stride, s0, stride0, i, kind, eps, bad);
        double sig, spl;
        cb_sigmoid(a + b * x, sig, spl);
        out[i] = sig;
    }
    if (bad) atomicOr(flag, bad);
}

}  // namespace

#define KOAF_CALIB_STRIDE(what, stride) \
    KOAF_REQUIRE((stride) >= 1 && (stride) < (1ll << 32), what ": 1 <= stride < 2^32 (stride = %lld)", (long long)(stride))

// the rows of a launch over resamples, checked as koaf_curve_metrics checks them
#define KOAF_CALIB_ROWS(what)                                                                                             \
    KOAF_REQUIRE(n >= 1 && n <= CB_MAX_N, what ": 1 <= n <= %d (n = %d)", CB_MAX_N, n);                                    \
    KOAF_REQUIRE(R >= 0 && R <= (1 << 20), what ": 0 <= R <= 2^20 (R = %d)", R);                                           \
    KOAF_REQUIRE(idx != nullptr || R == 0, what ": R = %d resamples need an index matrix", R);                            \
    KOAF_REQUIRE(idx == nullptr || (m >= 1 && m <= CB_MAX_N), what ": 1 <= m <= %d (m = %d)", CB_MAX_N, m);                \
    const int rows = R + (with_identity ? 1 : 0);                                                                         \
    KOAF_REQUIRE(rows >= 1, what ": nothing to do (R = 0 and no identity row)");                                          \
    const dim3 grid((unsigned)rows), block(CB_BLOCK);                                                                     \
    const int32_t* ix = R > 0 ? idx : nullptr

extern "C" int koaf_calib_edges(const void* scores, int32_t f64, int64_t stride, int32_t n, const double* q, int32_t nbins,
                                double* edges, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= CB_MAX_N, "koaf_calib_edges: 1 <= n <= %d (n = %d)", CB_MAX_N, n);
    KOAF_CALIB_STRIDE("koaf_calib_edges", stride);
    KOAF_REQUIRE(nbins >= 1 && nbins <= CB_MAX_BINS, "koaf_calib_edges: 1 <= nbins <= %d (nbins = %d)", CB_MAX_BINS, nbins);
    KOAF_REQUIRE(scores && q && edges && flag, "koaf_calib_edges: scores, q, edges and flag are required");
    const dim3 grid(1), block(CB_BLOCK);
    if (f64)
        hipLaunchKernelGGL(calib_edges_kernel<double>, grid, block, 0, STREAM, (const double*)scores, stride, n, q, nbins + 1, edges, flag);
    else
        hipLaunchKernelGGL(calib_edges_kernel<float>, grid, block, 0, STREAM, (const float*)scores, stride, n, q, nbins + 1, edges, flag);
    return koaf_check_launch("koaf_calib_edges");
}

extern "C" int koaf_calib_metrics(const void* scores, int32_t f64, int64_t stride, const int32_t* labels, int32_t n,
                                  const double* edges, int32_t nbins, const double* thr, int32_t T, const int32_t* idx, int32_t R,
                                  int32_t m, int32_t with_identity, double eps, double* out, double* bins, double* nb,
                                  uint32_t* flag, void* stream) {
    KOAF_CALIB_ROWS("koaf_calib_metrics");
    KOAF_CALIB_STRIDE("koaf_calib_metrics", stride);
    KOAF_REQUIRE(nbins >= 1 && nbins <= CB_MAX_BINS, "koaf_calib_metrics: 1 <= nbins <= %d (nbins = %d)", CB_MAX_BINS, nbins);
    KOAF_REQUIRE(T >= 0 && T <= CB_MAX_THR, "koaf_calib_metrics: 0 <= T <= %d (T = %d)", CB_MAX_THR, T);
    KOAF_REQUIRE((thr != nullptr || T == 0) && (nb == nullptr || T > 0), "koaf_calib_metrics: T = %d thresholds need thr, and nb needs thresholds", T);
    KOAF_REQUIRE(eps >= 0.0 && eps < 0.5, "koaf_calib_metrics: 0 <= eps < 0.5 (eps = %g)", eps);
    KOAF_REQUIRE(scores && labels && edges && out && flag, "koaf_calib_metrics: scores, labels, edges, out and flag are required");
    const int nthr = nb != nullptr ? T : 0;
    if (f64)
        hipLaunchKernelGGL(calib_metrics_kernel<double>, grid, block, 0, STREAM, (const double*)scores, stride, labels, n, edges, nbins,
                           thr, nthr, ix, m, with_identity, eps, out, bins, nb, flag);
    else
        hipLaunchKernelGGL(calib_metrics_kernel<float>, grid, block, 0, STREAM, (const float*)scores, stride, labels, n, edges, nbins,
                           thr, nthr, ix, m, with_identity, eps, out, bins, nb, flag);
    return koaf_check_launch("koaf_calib_metrics");
}

extern "C" int koaf_recalib_fit(const void* scores, int32_t f64, int64_t stride, const void* scores0, int64_t stride0,
                                const int32_t* labels, int32_t n, int32_t kind, int32_t mode, const int32_t* idx, int32_t R,
                                int32_t m, int32_t with_identity, double eps, double tol, int32_t max_iter, double* report,
                                uint32_t* flag, void* stream) {
    KOAF_CALIB_ROWS("koaf_recalib_fit");
    KOAF_CALIB_STRIDE("koaf_recalib_fit", stride);
    KOAF_REQUIRE(kind == 0 || kind == 1, "koaf_recalib_fit: kind is 0 (probabilities) or 1 (logits) (kind = %d)", kind);
    KOAF_REQUIRE(mode >= 0 && mode <= 2, "koaf_recalib_fit: mode is 0, 1 or 2 (mode = %d)", mode);
    KOAF_REQUIRE(scores0 == nullptr || kind == 1, "koaf_recalib_fit: a second column goes with kind 1 only");
    if (scores0 != nullptr) KOAF_CALIB_STRIDE("koaf_recalib_fit", stride0);
    KOAF_REQUIRE(eps >= 0.0 && eps < 0.5, "koaf_recalib_fit: 0 <= eps < 0.5 (eps = %g)", eps);
    KOAF_REQUIRE(tol >= 0.0, "koaf_recalib_fit: tol >= 0 (tol = %g)", tol);
    KOAF_REQUIRE(max_iter >= 1 && max_iter <= KOAF_RECALIB_MAX_ITER, "koaf_recalib_fit: 1 <= max_iter <= %d (max_iter = %d)",
                 KOAF_RECALIB_MAX_ITER, max_iter);
    KOAF_REQUIRE(scores && labels && report && flag, "koaf_recalib_fit: scores, labels, report and flag are required");
    if (f64)
        hipLaunchKernelGGL(recalib_fit_kernel<double>, grid, block, 0, STREAM, (const double*)scores, stride, (const double*)scores0,
                           stride0, labels, n, kind, mode, ix, m, with_identity, eps, tol, max_iter, report, flag);
    else
        hipLaunchKernelGGL(recalib_fit_kernel<float>, grid, block, 0, STREAM, (const float*)scores, stride, (const float*)scores0,
                           stride0, labels, n, kind, mode, ix, m, with_identity, eps, tol, max_iter, report, flag);
    return koaf_check_launch("koaf_recalib_fit");
}

extern "C" int koaf_recalib_apply(const void* scores, int32_t f64, int64_t stride, const void* scores0, int64_t stride0, int64_t n,
                                  int32_t kind, double a, double b, double eps, double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n < (1ll << 31), "koaf_recalib_apply: 1 <= n < 2^31 (n = %lld)", (long long)n);
    KOAF_CALIB_STRIDE("koaf_recalib_apply", stride);
    KOAF_REQUIRE(kind == 0 || kind == 1, "koaf_recalib_apply: kind is 0 (probabilities) or 1 (logits) (kind = %d)", kind);
    KOAF_REQUIRE(scores0 == nullptr || kind == 1, "koaf_recalib_apply: a second column goes with kind 1 only");
    if (scores0 != nullptr) KOAF_CALIB_STRIDE("koaf_recalib_apply", stride0);
    KOAF_REQUIRE(eps >= 0.0 && eps < 0.5, "koaf_recalib_apply: 0 <= eps < 0.5 (eps = %g)", eps);
    KOAF_REQUIRE(scores && out && flag, "koaf_recalib_apply: scores, out and flag are required");
    const dim3 grid(ew_grid(n)), block(CB_BLOCK);
    if (f64)
        hipLaunchKernelGGL(recalib_apply_kernel<double>, grid, block, 0, STREAM, (const double*)scores, stride, (const double*)scores0,
                           stride0, n, kind, a, b, eps, out, flag);
    else
        hipLaunchKernelGGL(recalib_apply_kernel<float>, grid, block, 0, STREAM, (const float*)scores, stride, (const float*)scores0, stride0,
                           n, kind, a, b, eps, out, flag);
    return koaf_check_launch("koaf_recalib_apply");
}
