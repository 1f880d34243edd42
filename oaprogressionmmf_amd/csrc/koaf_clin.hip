// koaf_clin.hip -- the clinical logistic-regression baseline (run/train_prog_clin.py): the design matrix of StandardScaler /
// OneHotEncoder per variable, the L2-penalised logistic regression of every (fold, class weight) problem in ONE launch, and the
// predictions, fold ensemble and held-out log-loss.  Everything is fp64; the job is milliseconds of work, so the layout aims at
// one launch for all fits and at identical bits from run to run (every sum has one owner and a fixed order; no floating-point
// atomics), not at a fast single fit.
#include "koaf_common.h"

namespace {
constexpr int CL_MAXV = 32;                      // raw variables of a table
constexpr int LR_MAXP = KOAF_LOGREG_MAX_P;       // D + 1
constexpr int LR_ROWS = 128;                     // rows of one LDS tile
constexpr int LR_ST = LR_MAXP + 1;               // tile row stride in doubles: odd, so the row-per-lane dot product meets no conflict
constexpr int LR_EPT = (LR_MAXP * (LR_MAXP + 1) / 2 + LR_MAXP + 255) / 256;      // Hessian + gradient entries per thread (3)
constexpr double LR_ARMIJO = 1e-4, LR_MIN_STEP = 1.0 / 1073741824.0, LR_EPS = 2.220446049250313e-16;

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// ------------------------------------------------------------------------------------------------
// design: StandardScaler (mean, population standard deviation over the fitting rows) and OneHotEncoder
// ------------------------------------------------------------------------------------------------
struct DesignArgs {
    int V, D;
    int ncat[CL_MAXV], off[CL_MAXV], cat0[CL_MAXV];      // categories (0: continuous), first output column, first entry of cats
    double cats[LR_MAXP];                                // sorted categories of all categorical variables, concatenated
};

// the 256 per-thread partial sums of a block, added by thread 0 in thread order: one fixed order, whatever the timing
__device__ __forceinline__ double block_sum_ordered(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += red[i];
        red[256] = s;
    }
    __syncthreads();
    return red[256];
}

// one block per variable: stats[v] = (mean, sqrt(mean((x - mean)^2))) over the fitting rows; (0, 0) for a categorical variable
__global__ void __launch_bounds__(256) clin_stats_kernel(const double* __restrict__ raw, int64_t n, DesignArgs a,
                                                         const int32_t* __restrict__ fit_idx, int64_t nfit, double* __restrict__ stats,
                                                         uint32_t* __restrict__ flag) {
    __shared__ double red[257];
    const int v = blockIdx.x;
    if (a.ncat[v] != 0) {
        if (threadIdx.x < 2) stats[2 * v + threadIdx.x] = 0.0;
        return;
    }
    const double* x = raw + (int64_t)v * n;
    unsigned bad = 0u;
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double acc = 0.0;
        for (int64_t j = threadIdx.x; j < nfit; j += 256) {
            const int64_t i = fit_idx ? (int64_t)fit_idx[j] : j;
            if (i < 0 || i >= n) { bad |= 8u; continue; }
            const double d = x[i] - mean;                      // pass 0: mean is 0.0
            acc += pass ? d * d : d;
        }
        const double s = block_sum_ordered(acc, red) / (double)nfit;
        if (pass == 0) mean = s;
        else if (threadIdx.x == 0) stats[2 * v] = mean, stats[2 * v + 1] = sqrt(s);
    }
    if (bad) atomicOr(flag, bad);
}

// X[i][off_v ...] of every (variable, row): a standardised value, or the 0 / 1 columns of its category
__global__ void __launch_bounds__(256) clin_design_kernel(const double* __restrict__ raw, int64_t n, DesignArgs a,
                                                          const double* __restrict__ stats, double* __restrict__ X,
                                                          uint32_t* __restrict__ flag) {
    unsigned bad = 0u;
    const int64_t total = n * a.V;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int v = (int)(it / n);
        const int64_t i = it - (int64_t)v * n;
        const double x = raw[it];
        double* o = X + i * a.D + a.off[v];
        if (!finite64(x)) bad |= 1u;
        if (a.ncat[v] == 0) {
            const double sd = stats[2 * v + 1];
            o[0] = (x - stats[2 * v]) / (sd != 0.0 ? sd : 1.0);
        } else {
            bool found = false;
            for (int c = 0; c < a.ncat[v]; ++c) {
                const bool hit = x == a.cats[a.cat0[v] + c];
                o[c] = hit ? 1.0 : 0.0;
                found |= hit;
            }
            if (!found && finite64(x)) bad |= 2u;
        }
    }
    if (bad) atomicOr(flag, bad);
}

// ------------------------------------------------------------------------------------------------
// fit: one block per problem, damped Newton on the scaled objective
//   f(w) = (1/S) sum_i s_i [log(1 + e^{r_i}) - y_i r_i] + |w[:D]|^2 / (2 C S),   r_i = z_i . w,  z_i = (x_i, 1),  S = sum_i s_i
// ------------------------------------------------------------------------------------------------
struct LrShared {
    double z[LR_ROWS * LR_ST];        // the row tile, the ones column included
    double coef[2][LR_ROWS];          // per tile row: s p (1 - p) and s (p - y)
    double H[LR_MAXP * LR_MAXP];      // Hessian, then its Cholesky factor in the lower triangle
    double w[LR_MAXP], wt[LR_MAXP], g[LR_MAXP], d[LR_MAXP];
    double red[257];
    double f, slope, gnorm, S;
    int ok;
};

struct LrProblem {
    const double* X;
    const int32_t* y;
    const double* s;                  // this problem's weight row
    int n, D, P;
    double C;
};

// One walk over the rows in tiles.  Leaves the objective at `w` in sh.f; HESS: also sh.g and sh.H.  Entry e of the P (P + 1) / 2
// lower-triangle Hessian entries and P gradient entries belongs to thread e % 256, which adds its rows in row order.
template <bool HESS>
__device__ void lr_pass(LrShared& sh, const LrProblem& pr, const double* w) {
    const int tid = threadIdx.x, P = pr.P, D = pr.D, NH = P * (P + 1) / 2;
    int ea[LR_EPT], eb[LR_EPT], ew[LR_EPT];
    bool own[LR_EPT];
    double acc[LR_EPT];
#pragma unroll
    for (int q = 0; q < LR_EPT; ++q) {
        const int e = tid + 256 * q;
        acc[q] = 0.0, ea[q] = 0, eb[q] = 0, ew[q] = 0, own[q] = false;
        if (HESS && e < NH) {
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= e) ++a;
            ea[q] = a, eb[q] = e - a * (a + 1) / 2, own[q] = true;
        } else if (HESS && e < NH + P) {
            ea[q] = e - NH, eb[q] = D, ew[q] = 1, own[q] = true;      // gradient: the ones column as the second factor
        }
    }
    double loss = 0.0;
    for (int r0 = 0; r0 < pr.n; r0 += LR_ROWS) {
        const int rows = min(LR_ROWS, pr.n - r0);
        __syncthreads();                                       // the previous tile, and the caller's writes of w, are done with
        const double* src = pr.X + (int64_t)r0 * D;
        for (int idx = tid; idx < rows * D; idx += 256) {
            const int r = idx / D;
            sh.z[r * LR_ST + idx - r * D] = src[idx];
        }
        if (tid < rows) sh.z[tid * LR_ST + D] = 1.0;
        __syncthreads();
        if (tid < rows) {
            const double s = pr.s[r0 + tid];
            double hh = 0.0, rr = 0.0;
            if (s != 0.0) {                                    // a row of weight 0 is not in this problem: its values are never used
                double r = 0.0;
                for (int a = 0; a < P; ++a) r += sh.z[tid * LR_ST + a] * w[a];
                const double yy = (double)pr.y[r0 + tid];
                const double e = exp(-fabs(r));
                const double p = r >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                loss += s * (fmax(r, 0.0) + log1p(e) - yy * r);
                hh = s * p * (1.0 - p), rr = s * (p - yy);
            } else {
                for (int a = 0; a < P; ++a) sh.z[tid * LR_ST + a] = 0.0;      // whatever the row holds, it adds 0 * 0 * 0 below
            }
            sh.coef[0][tid] = hh, sh.coef[1][tid] = rr;
        }
        if (HESS) {
            __syncthreads();
            // no branch in this loop, so that the LDS reads of several rows are in flight together (a thread without an entry
            // adds entry (0, 0) into a sum nobody reads)
#pragma unroll 8
            for (int i = 0; i < rows; ++i) {
#pragma unroll
                for (int q = 0; q < LR_EPT; ++q) acc[q] += sh.coef[ew[q]][i] * sh.z[i * LR_ST + ea[q]] * sh.z[i * LR_ST + eb[q]];
            }
        }
    }
    const double S = sh.S, pen = 1.0 / (pr.C * S);
    const double total = block_sum_ordered(loss, sh.red);
    if (HESS) {
#pragma unroll
        for (int q = 0; q < LR_EPT; ++q) {
            if (!own[q]) continue;
            const int a = ea[q], b = eb[q];
            if (ew[q]) sh.g[a] = acc[q] / S + (a < D ? w[a] * pen : 0.0);
            else sh.H[a * LR_MAXP + b] = sh.H[b * LR_MAXP + a] = acc[q] / S + (a == b && a < D ? pen : 0.0);
        }
    }
    if (tid == 0) {
        double q = 0.0;
        for (int a = 0; a < D; ++a) q += w[a] * w[a];
        sh.f = total / S + 0.5 * q * pen;
    }
    __syncthreads();
}

// H = L L^T in place (lower triangle), then d = -H^-1 g and slope = g . d; sh.ok = 0 when a pivot is not positive
__device__ void lr_newton_step(LrShared& sh, int P) {
    const int tid = threadIdx.x;
    for (int j = 0; j < P; ++j) {
        if (tid == 0) {
            const double pv = sh.H[j * LR_MAXP + j];
            if (!(pv > 0.0) || !finite64(pv)) sh.ok = 0;
            sh.H[j * LR_MAXP + j] = sqrt(pv);
        }
        __syncthreads();
        if (!sh.ok) return;                                    // uniform: read after the barrier
        if (tid > j && tid < P) sh.H[tid * LR_MAXP + j] /= sh.H[j * LR_MAXP + j];
        __syncthreads();
        for (int idx = tid; idx < LR_MAXP * LR_MAXP; idx += 256) {
            const int i = idx / LR_MAXP, k = idx - i * LR_MAXP;
            if (k > j && i >= k && i < P) sh.H[idx] -= sh.H[i * LR_MAXP + j] * sh.H[k * LR_MAXP + j];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = 0; i < P; ++i) {
            double v = -sh.g[i];
            for (int k = 0; k < i; ++k) v -= sh.H[i * LR_MAXP + k] * sh.d[k];
            sh.d[i] = v / sh.H[i * LR_MAXP + i];
        }
        for (int i = P - 1; i >= 0; --i) {
            double v = sh.d[i];
            for (int k = i + 1; k < P; ++k) v -= sh.H[k * LR_MAXP + i] * sh.d[k];
            sh.d[i] = v / sh.H[i * LR_MAXP + i];
        }
        double sl = 0.0;
        for (int i = 0; i < P; ++i) sl += sh.g[i] * sh.d[i];
        sh.slope = sl;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) logreg_fit_kernel(const double* __restrict__ X, const int32_t* __restrict__ y,
                                                         const double* __restrict__ sw, int n, int D, double C, int max_iter, double tol,
                                                         double* __restrict__ W, double* __restrict__ report,
                                                         uint32_t* __restrict__ flag) {
    __shared__ LrShared sh;
    __shared__ int cnt[3];
    const int tid = threadIdx.x, k = blockIdx.x, P = D + 1;
    LrProblem pr{X, y, sw + (int64_t)k * n, n, D, P, C};
    // the problem's rows: S, the two class counts, and what a row may not hold
    if (tid < 3) cnt[tid] = 0;
    if (tid == 0) sh.ok = 1;
    __syncthreads();
    double ssum = 0.0;
    int c0 = 0, c1 = 0, bad = 0;
    for (int i = tid; i < n; i += 256) {
        const double s = pr.s[i];
        if (!finite64(s)) bad |= 1;
        else if (s < 0.0) bad |= 8;
        if (s != 0.0) {
            const int yy = y[i];
            if (yy == 0) ++c0;
            else if (yy == 1) ++c1;
            else bad |= 8;
            ssum += s;
        }
    }
    if (c0) atomicAdd(&cnt[0], c0);                            // integer counts: any order
    if (c1) atomicAdd(&cnt[1], c1);
    if (bad) atomicOr(&cnt[2], bad);
    const double S = block_sum_ordered(ssum, sh.red);
    if (tid == 0) sh.S = S;
    if (tid < P) sh.w[tid] = 0.0;
    __syncthreads();
    unsigned raise = (unsigned)cnt[2];
    if (cnt[0] == 0 || cnt[1] == 0) raise |= 4u;               // scikit-learn: "needs samples of at least 2 classes"
    double* Wk = W + (int64_t)k * P;
    double* rep = report + (int64_t)k * 4;
    if (raise) {
        if (tid < P) Wk[tid] = nan64();
        if (tid < 4) rep[tid] = nan64();
        if (tid == 0) atomicOr(flag, raise);
        return;
    }
    lr_pass<true>(sh, pr, sh.w);
    int it = 0, halvings = 0;
    while (true) {
        if (tid == 0) {
            double m = 0.0;
            bool isnan = false;
            for (int a = 0; a < P; ++a) { const double v = fabs(sh.g[a]); isnan |= v != v; m = fmax(m, v); }
            sh.gnorm = isnan ? nan64() : m;
        }
        __syncthreads();
        if (it >= max_iter || sh.gnorm <= tol) break;
        lr_newton_step(sh, P);
        if (!sh.ok) break;
        const double f0 = sh.f, slope = sh.slope;
        double t = 1.0;
        bool accepted = false;
        while (t >= LR_MIN_STEP) {
            if (tid < P) sh.wt[tid] = sh.w[tid] + t * sh.d[tid];
            // (the pass's first barrier orders the writes of wt.)  The full step is nearly always taken, so its trial already
            // forms gradient and Hessian there: one walk over the rows per Newton step; d and the slope are all that is
            // still needed of the old point
            if (t == 1.0) lr_pass<true>(sh, pr, sh.wt);
            else lr_pass<false>(sh, pr, sh.wt);
            if (sh.f <= f0 + LR_ARMIJO * t * slope + 4.0 * LR_EPS * fabs(f0)) { accepted = true; break; }
            t *= 0.5, ++halvings;
        }
        if (!accepted) {
            if (tid == 0) sh.f = f0;
            break;
        }
        __syncthreads();
        if (tid < P) sh.w[tid] = sh.wt[tid];
        if (t != 1.0) lr_pass<true>(sh, pr, sh.w);
        ++it;
    }
    __syncthreads();
    if (tid < P) Wk[tid] = sh.w[tid];
    if (tid == 0) {
        rep[0] = (double)it, rep[1] = sh.gnorm, rep[2] = sh.f, rep[3] = (double)halvings;
        if (!finite64(sh.f) || !finite64(sh.gnorm)) atomicOr(flag, 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// predict: one block per problem; then the mean over the problems per test row
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) logreg_predict_kernel(const double* __restrict__ W, const double* __restrict__ Xt, int m, int D,
                                                             const int32_t* __restrict__ y, const int32_t* __restrict__ mask,
                                                             double* __restrict__ decision, double* __restrict__ proba,
                                                             double* __restrict__ logloss) {
    __shared__ double w[LR_MAXP];
    __shared__ double red[257];
    __shared__ int cnt;
    const int tid = threadIdx.x, k = blockIdx.x, P = D + 1;
    if (tid < P) w[tid] = W[(int64_t)k * P + tid];
    if (tid == 0) cnt = 0;
    __syncthreads();
    double acc = 0.0;
    int mine = 0;
    for (int i = tid; i < m; i += 256) {
        const double* x = Xt + (int64_t)i * D;
        double r = 0.0;
        for (int a = 0; a < D; ++a) r += x[a] * w[a];
        r += w[D];
        const double e = exp(-fabs(r));
        const double p = r >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        const int64_t o = (int64_t)k * m + i;
        decision[o] = r, proba[2 * o] = 1.0 - p, proba[2 * o + 1] = p;
        if (logloss && mask[o] != 0) {
            const double pt = y[i] == 1 ? p : 1.0 - p;
            acc -= log(fmin(fmax(pt, LR_EPS), 1.0 - LR_EPS));      // sklearn.metrics.log_loss clips at eps
            ++mine;
        }
    }
    if (!logloss) return;
    if (mine) atomicAdd(&cnt, mine);
    const double total = block_sum_ordered(acc, red);
    if (tid == 0) logloss[k] = cnt ? total / (double)cnt : nan64();
}

__global__ void __launch_bounds__(256) logreg_ensemble_kernel(const double* __restrict__ proba, int m, int K, double* __restrict__ ens,
                                                              int32_t* __restrict__ pred) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double s0 = 0.0, s1 = 0.0;                                 // np.mean(axis=0): added in problem order, then divided
    for (int k = 0; k < K; ++k) {
        s0 += proba[2 * ((int64_t)k * m + i)];
        s1 += proba[2 * ((int64_t)k * m + i) + 1];
    }
    s0 /= (double)K, s1 /= (double)K;
    ens[2 * i] = s0, ens[2 * i + 1] = s1;
    pred[i] = s1 > s0 ? 1 : 0;                                 // np.argmax: the first index wins a tie
}
}  // namespace

extern "C" int koaf_clin_design(const double* raw, int64_t n, int32_t V, const int32_t* ncat, const double* cats,
                                const int32_t* fit_idx, int64_t nfit, int32_t fit, double* stats, double* X, uint32_t* flag,
                                void* stream) {
    KOAF_REQUIRE(raw && ncat && stats && X && flag, "koaf_clin_design: null pointer");
    KOAF_REQUIRE(V >= 1 && V <= CL_MAXV, "koaf_clin_design: 1..%d variables, got %d", CL_MAXV, V);
    KOAF_REQUIRE(n >= 1 && n < (1ll << 31) / LR_MAXP, "koaf_clin_design: 1 <= n < 2^31 / %d", LR_MAXP);
    KOAF_REQUIRE(fit == 0 || fit == 1, "koaf_clin_design: fit is 0 or 1");
    KOAF_REQUIRE(!fit || (nfit >= 1 && (fit_idx ? nfit < (1ll << 31) : nfit == n)),
                 "koaf_clin_design: fit needs 1 <= nfit fitting rows (nfit = n without an index list)");
    DesignArgs a;
    a.V = V, a.D = 0;
    int nc = 0;
    for (int v = 0; v < CL_MAXV; ++v) a.ncat[v] = a.off[v] = a.cat0[v] = 0;
    for (int v = 0; v < V; ++v) {
        KOAF_REQUIRE(ncat[v] >= 0 && ncat[v] < LR_MAXP, "koaf_clin_design: variable %d has %d categories", v, ncat[v]);
        a.ncat[v] = ncat[v], a.off[v] = a.D, a.cat0[v] = nc;
        a.D += ncat[v] ? ncat[v] : 1;
        nc += ncat[v];
        KOAF_REQUIRE(a.D + 1 <= LR_MAXP, "koaf_clin_design: D + 1 <= %d columns, the intercept included", LR_MAXP);
    }
    KOAF_REQUIRE(nc == 0 || cats, "koaf_clin_design: null pointer");
    for (int v = 0; v < V; ++v)
        for (int c = 0; c < a.ncat[v]; ++c) {
            const double x = cats[a.cat0[v] + c];
            KOAF_REQUIRE(x == x && (c == 0 || cats[a.cat0[v] + c - 1] < x), "koaf_clin_design: the categories of variable %d are not sorted", v);
            a.cats[a.cat0[v] + c] = x;
        }
    if (fit) hipLaunchKernelGGL(clin_stats_kernel, dim3(V), dim3(256), 0, STREAM, raw, n, a, fit_idx, nfit, stats, flag);
    hipLaunchKernelGGL(clin_design_kernel, dim3(ew_grid(n * V)), dim3(256), 0, STREAM, raw, n, a, stats, X, flag);
    return koaf_check_launch("koaf_clin_design");
}

extern "C" int koaf_logreg_fit(const double* X, const int32_t* y, const double* sw, int64_t n, int32_t D, int32_t K, double C,
                               int32_t max_iter, double tol, double* W, double* report, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(X && y && sw && W && report && flag, "koaf_logreg_fit: null pointer");
    KOAF_REQUIRE(D >= 1 && D + 1 <= LR_MAXP, "koaf_logreg_fit: 1 <= D and D + 1 <= %d, got D = %d", LR_MAXP, D);
    KOAF_REQUIRE(n >= 2 && n < (1ll << 31) / LR_MAXP, "koaf_logreg_fit: 2 <= n < 2^31 / %d", LR_MAXP);
    KOAF_REQUIRE(K >= 1 && K <= 65535, "koaf_logreg_fit: 1..65535 problems, got %d", K);
    KOAF_REQUIRE(C > 0.0 && C <= 1.7976931348623157e308 && max_iter >= 0 && tol >= 0.0, "koaf_logreg_fit: C > 0, max_iter >= 0, tol >= 0");
    hipLaunchKernelGGL(logreg_fit_kernel, dim3(K), dim3(256), 0, STREAM, X, y, sw, (int)n, D, C, max_iter, tol, W, report, flag);
    return koaf_check_launch("koaf_logreg_fit");
}

extern "C" int koaf_logreg_predict(const double* W, const double* Xt, int64_t m, int32_t D, int32_t K, const int32_t* y,
                                   const int32_t* mask, int32_t ensemble, double* decision, double* proba, double* logloss,
                                   double* ens_proba, int32_t* ens_pred, void* stream) {
    KOAF_REQUIRE(W && Xt && decision && proba, "koaf_logreg_predict: null pointer");
    KOAF_REQUIRE(D >= 1 && D + 1 <= LR_MAXP, "koaf_logreg_predict: 1 <= D and D + 1 <= %d, got D = %d", LR_MAXP, D);
    KOAF_REQUIRE(m >= 1 && m < (1ll << 31) / LR_MAXP, "koaf_logreg_predict: 1 <= m < 2^31 / %d", LR_MAXP);
    KOAF_REQUIRE(K >= 1 && K <= 65535 && K * m < (1ll << 30), "koaf_logreg_predict: 1..65535 problems and K m < 2^30, got K = %d", K);
    KOAF_REQUIRE(ensemble == 0 || ensemble == 1, "koaf_logreg_predict: ensemble is 0 or 1");
    KOAF_REQUIRE(!logloss || (y && mask), "koaf_logreg_predict: the log-loss needs y and mask");
    KOAF_REQUIRE(!ensemble || (ens_proba && ens_pred), "koaf_logreg_predict: the ensemble needs ens_proba and ens_pred");
    hipLaunchKernelGGL(logreg_predict_kernel, dim3(K), dim3(256), 0, STREAM, W, Xt, (int)m, D, y, mask, decision, proba, logloss);
    if (ensemble)
        hipLaunchKernelGGL(logreg_ensemble_kernel, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, STREAM, proba, (int)m, K, ens_proba, ens_pred);
    return koaf_check_launch("koaf_logreg_predict");
}
