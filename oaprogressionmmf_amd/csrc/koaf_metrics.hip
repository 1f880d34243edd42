// koaf_metrics.hip -- the validation / evaluation metrics of calc_metrics_v2 (various/_metrics_stat_anlys.py:28-216,
// _metrics_wissam.py:113-172) on the device, bootstrap included.  The scores are ranked once (all-pairs counting, no sort); a
// resample then only changes how often each sample counts, so each resample is an integer histogram over the rank bins and one
// ordered pass over it.  Everything that decides a result is integer arithmetic (LDS integer atomics, integer prefix sums, the
// Mann-Whitney sum in int64); the fp64 sums run in a fixed order.  No floating-point atomics: run-to-run identical bits.
// The paired permutation test of two models (scipy.stats.permutation_test(permutation_type="samples") around roc_auc_score /
// average_precision_score differences) runs on the same pieces: swapping a sample's two predictions leaves the order of the
// union of the 2n scores alone, so the union is ranked once and each permutation is a histogram over its 2n rank bins.
// The curves themselves (roc_curve, precision_recall_curve, precision_recall_curve_calib of _metrics_wissam.py:113-165) are the
// same walk with its points written out at counted offsets; avg_precision_at_recall_range (_metrics_stat_anlys.py:11-25) and
// bestf1score_calib (_metrics_wissam.py:215-231) fold it into other scalars per resample; a small kernel counts confusion pairs.
#include "koaf_common.h"

namespace {

constexpr int MT_BLOCK = 256;
constexpr int MT_MAX_N = KOAF_METRICS_MAX_N;
constexpr int MT_TILE = 2048;            // scores per LDS tile of the rank kernel

// ---- ranks -----------------------------------------------------------------------------------------------------------------
// rank[i] = #{ j : s[j] > s[i] }: thread i keeps its own score and counts over all scores, tiled through LDS (every lane reads
// the same LDS word: a broadcast).  The count of one sample does not depend on the grid.  packed[i] = rank << 1 | (label == pos).
template <typename T>
__global__ void __launch_bounds__(MT_BLOCK) score_ranks_kernel(const T* __restrict__ s, int64_t stride, int n,
                                                               const int32_t* __restrict__ labels, int pos_label,
                                                               int32_t* __restrict__ rank, int32_t* __restrict__ packed,
                                                               uint32_t* __restrict__ flag) {
    __shared__ T tile[MT_TILE];
    const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
    const T mine = i < n ? s[(int64_t)i * stride] : (T)0;
    int cnt = 0;
    for (int t0 = 0; t0 < n; t0 += MT_TILE) {
        const int len = n - t0 < MT_TILE ? n - t0 : MT_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += MT_BLOCK) tile[j] = s[(int64_t)(t0 + j) * stride];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < len; ++j) cnt += tile[j] > mine ? 1 : 0;
    }
    if (i >= n) return;
    unsigned bad = 0;
    if (!(fabs((double)mine) <= 1.7976931348623157e308)) bad |= 1u;          // NaN / Inf
    if (rank) rank[i] = cnt;
    if (labels) {
        const int32_t l = labels[i];
        if (l != 0 && l != 1) bad |= 2u;
        packed[i] = (cnt << 1) | (l == pos_label ? 1 : 0);
    }
    if (bad) atomicOr(flag, bad);
}

// the same over the union of two score columns: element j < n is a[j], element n + j is b[j]; both halves carry the labels of
// the n samples.  A score of one model that equals a score of the other shares its rank bin.
template <typename T>
__global__ void __launch_bounds__(MT_BLOCK) pair_ranks_kernel(const T* __restrict__ a, int64_t stride_a, const T* __restrict__ b,
                                                              int64_t stride_b, int n, const int32_t* __restrict__ labels,
                                                              int pos_label, int32_t* __restrict__ rank,
                                                              int32_t* __restrict__ packed, uint32_t* __restrict__ flag) {
    __shared__ T tile[MT_TILE];
    const int n2 = 2 * n;
    const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
    const T mine = i < n ? a[(int64_t)i * stride_a] : i < n2 ? b[(int64_t)(i - n) * stride_b] : (T)0;
    int cnt = 0;
    for (int t0 = 0; t0 < n2; t0 += MT_TILE) {
        const int len = n2 - t0 < MT_TILE ? n2 - t0 : MT_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += MT_BLOCK) {
            const int k = t0 + j;
            tile[j] = k < n ? a[(int64_t)k * stride_a] : b[(int64_t)(k - n) * stride_b];
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < len; ++j) cnt += tile[j] > mine ? 1 : 0;
    }
    if (i >= n2) return;
    unsigned bad = 0;
    if (!(fabs((double)mine) <= 1.7976931348623157e308)) bad |= 1u;          // NaN / Inf
    if (rank) rank[i] = cnt;
    if (labels) {
        const int32_t l = labels[i < n ? i : i - n];
        if (l != 0 && l != 1) bad |= 2u;
        packed[i] = (cnt << 1) | (l == pos_label ? 1 : 0);
    }
    if (bad) atomicOr(flag, bad);
}

// ---- shared pieces of the curve kernels ----------------------------------------------------------------------------------
// A histogram word holds the bin's positives in its upper and its negatives in its lower 16 bits: at most m <= 16384 draws per
// resample, so neither half can carry.
__device__ __forceinline__ int h_tp(uint32_t w) { return (int)(w >> 16); }
__device__ __forceinline__ int h_fp(uint32_t w) { return (int)(w & 0xffffu); }

// one draw into its bin.  A rank outside [0, bins) is not followed: it raises flag bit 2.
__device__ __forceinline__ void hist_add(uint32_t* hist, int32_t w, int bins, uint32_t* flag) {
    if ((unsigned)(w >> 1) >= (unsigned)bins) { atomicOr(flag, 4u); return; }         // (not a word the rank kernels wrote for this n)
    atomicAdd(&hist[w >> 1], (w & 1) ? 0x10000u : 1u);
}

// zero the n bins, then add the m draws of this resample (idx row, or the identity when idx is NULL).  An index or a rank
// outside [0, n) is not followed: it raises flag bit 2.
__device__ __forceinline__ void fill_hist(uint32_t* hist, const int32_t* __restrict__ packed, int n,
                                          const int32_t* __restrict__ idx, int m, uint32_t* flag) {
    for (int g = threadIdx.x; g < n; g += MT_BLOCK) hist[g] = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += MT_BLOCK) {
        const int i = idx ? idx[k] : k;
        if ((unsigned)i >= (unsigned)n) { atomicOr(flag, 4u); continue; }
        hist_add(hist, packed[i], n, flag);
    }
    __syncthreads();
}

// the same for one side of a paired permutation: sample i counts with its own word (packed[i] on side 0, packed[n + i] on side
// 1) unless bit i of the mask row is set, then with the other model's.  row == NULL: nothing is swapped.  2n bins.
__device__ __forceinline__ void fill_hist_swapped(uint32_t* hist, const int32_t* __restrict__ packed, int n,
                                                  const uint32_t* __restrict__ row, int side, uint32_t* flag) {
    for (int g = threadIdx.x; g < 2 * n; g += MT_BLOCK) hist[g] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MT_BLOCK) {
        const int swapped = row ? (int)((row[i >> 5] >> (i & 31)) & 1u) : 0;
        hist_add(hist, packed[(side ^ swapped) ? n + i : i], 2 * n, flag);
    }
    __syncthreads();
}

// thread t owns bins [t * L, min(n, (t + 1) * L)), L = ceil(n / 256): its (tp, fp) totals, then the exclusive prefix over the
// threads before it and the block totals -- integer sums, any order gives the same value
__device__ __forceinline__ void run_prefix(const uint32_t* hist, int n, int* s_tp, int* s_fp, int& g0, int& g1, int& tp_before,
                                           int& fp_before, int& P, int& N) {
    const int L = (n + MT_BLOCK - 1) / MT_BLOCK;
    g0 = threadIdx.x * L < n ? threadIdx.x * L : n;
    g1 = g0 + L < n ? g0 + L : n;
    int tp = 0, fp = 0;
    for (int g = g0; g < g1; ++g) { const uint32_t w = hist[g]; tp += h_tp(w); fp += h_fp(w); }
    s_tp[threadIdx.x] = tp;
    s_fp[threadIdx.x] = fp;
    __syncthreads();
    tp_before = fp_before = P = N = 0;
    for (int t = 0; t < MT_BLOCK; ++t) {
        const int a = s_tp[t], b = s_fp[t];
        if (t < (int)threadIdx.x) { tp_before += a; fp_before += b; }
        P += a;
        N += b;
    }
}

// the ordered walk of one thread over the non-empty bins of its run [g0, g1) (descending score = ascending rank); tp / fp come in
// as the counts ahead of the run.  auc: the Mann-Whitney sum sum_g fp_g (2 tp_before_g + tp_g); ap: sum_g (tp_g / P) tp / (tp + fp);
// cal (CAL only): the same with the negatives weighted by `ratio`.
template <bool CAL>
__device__ __forceinline__ void walk_run(const uint32_t* hist, int g0, int g1, int tp, int fp, double dP, double ratio,
                                         long long& auc, double& ap, double& cal) {
#pragma clang fp contract(off)
    for (int g = g0; g < g1; ++g) {
        const uint32_t w = hist[g];
        if (w == 0u) continue;
        const int tg = h_tp(w), fg = h_fp(w);
        auc += (long long)fg * (long long)(2 * tp + tg);
        tp += tg;
        fp += fg;
        if (tg != 0) {
            const double dr = (double)tg / dP, dtp = (double)tp;
            ap += dr * (dtp / (double)(tp + fp));
            if (CAL) {
                const double den = dtp + ratio * (double)fp;
                cal += dr * (den == 0.0 ? 0.0 : dtp / den);
            }
        }
    }
}

// ---- curve metrics of R resamples ------------------------------------------------------------------------------------------
// Block r: the histogram of resample r, then per thread one ordered walk over the non-empty bins of its run (descending score =
// ascending rank), then a fixed-order tree over the 256 partial sums.  out[r][0..8): n_pos, n_neg, roc_auc, avg_precision,
// calibrated avg_precision, 0, 0, 0.
template <int BINS>
__global__ void __launch_bounds__(MT_BLOCK) curve_metrics_kernel(const int32_t* __restrict__ packed, int n,
                                                                 const int32_t* __restrict__ idx, int m, int with_identity,
                                                                 double pi0, double* __restrict__ out, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[BINS];
    __shared__ int s_tp[MT_BLOCK], s_fp[MT_BLOCK];
    __shared__ long long r_auc[MT_BLOCK];
    __shared__ double r_ap[MT_BLOCK], r_cal[MT_BLOCK];
    const int r = blockIdx.x;
    const int32_t* row = nullptr;
    int draws = n;
    if (idx != nullptr && !(with_identity && r == 0)) {
        row = idx + (int64_t)(r - (with_identity ? 1 : 0)) * m;
        draws = m;
    }
    fill_hist(hist, packed, n, row, draws, flag);
    int g0, g1, tp, fp, P, N;
    run_prefix(hist, n, s_tp, s_fp, g0, g1, tp, fp, P, N);
    const double dP = (double)P, dN = (double)N;
    const double pi = dP / (double)(P + N);
    const double ratio = pi * (1.0 - pi0) / (pi0 * (1.0 - pi));           // (_metrics_wissam.py:151-152, in its order)
    long long auc = 0;
    double ap = 0.0, cal = 0.0;
    if (P > 0 && N > 0) walk_run<true>(hist, g0, g1, tp, fp, dP, ratio, auc, ap, cal);
    r_auc[threadIdx.x] = auc;
    r_ap[threadIdx.x] = ap;
    r_cal[threadIdx.x] = cal;
    __syncthreads();
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            r_auc[threadIdx.x] += r_auc[threadIdx.x + o];
            r_ap[threadIdx.x] += r_ap[threadIdx.x + o];
            r_cal[threadIdx.x] += r_cal[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)r * 8;
        const bool ok = P > 0 && N > 0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        o[0] = dP;
        o[1] = dN;
        o[2] = ok ? (double)r_auc[0] / (2.0 * dP * dN) : nan;
        o[3] = ok ? r_ap[0] : nan;
        o[4] = ok ? r_cal[0] : nan;
        o[5] = o[6] = o[7] = 0.0;
    }
}

// ---- paired permutation test of two models ----------------------------------------------------------------------------------
// Block (r, side): the histogram over the 2n union bins of what permutation r leaves on that side (0: "ref", 1: "cmp"), the same
// walk and tree.  The labels do not move, so both sides of every row hold the same P and N.  out[r][0..8): P, N, U of side 0,
// U of side 1, avg_precision of side 0, of side 1, 0, 0 -- U the Mann-Whitney sum itself (2 P N roc_auc), an integer < 2^27.
template <int BINS>
__global__ void __launch_bounds__(MT_BLOCK) perm_metrics_kernel(const int32_t* __restrict__ packed, int n,
                                                                const uint32_t* __restrict__ masks, int W, int with_identity,
                                                                double* __restrict__ out, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[BINS];
    __shared__ int s_tp[MT_BLOCK], s_fp[MT_BLOCK];
    __shared__ long long r_auc[MT_BLOCK];
    __shared__ double r_ap[MT_BLOCK];
    const int r = blockIdx.x, side = blockIdx.y;
    const uint32_t* row = nullptr;
    if (masks != nullptr && !(with_identity && r == 0)) row = masks + (int64_t)(r - (with_identity ? 1 : 0)) * W;
    fill_hist_swapped(hist, packed, n, row, side, flag);
    int g0, g1, tp, fp, P, N;
    run_prefix(hist, 2 * n, s_tp, s_fp, g0, g1, tp, fp, P, N);
    const double dP = (double)P, dN = (double)N;
    long long auc = 0;
    double ap = 0.0, cal = 0.0;
    if (P > 0 && N > 0) walk_run<false>(hist, g0, g1, tp, fp, dP, 0.0, auc, ap, cal);
    r_auc[threadIdx.x] = auc;
    r_ap[threadIdx.x] = ap;
    __syncthreads();
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            r_auc[threadIdx.x] += r_auc[threadIdx.x + o];
            r_ap[threadIdx.x] += r_ap[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)r * 8;
        const bool ok = P > 0 && N > 0;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (side == 0) {
            o[0] = dP;
            o[1] = dN;
            o[6] = o[7] = 0.0;
        }
        o[2 + side] = ok ? (double)r_auc[0] : nan;
        o[4 + side] = ok ? r_ap[0] : nan;
    }
}

// ---- point estimates ---------------------------------------------------------------------------------------------------------
// One block, the identity resample.  The Youden cutoff of sensitivity_specificity_cutoff (:224-254): the first maximum of
// tps / P - fps / N over the points roc_curve(drop_intermediate=True) keeps -- the first threshold, the last one and every one
// whose (tp, fp) increment differs from the NEXT threshold's (a non-zero second difference of tps or fps) -- behind the leading
// (0, 0, inf) point, whose value is 0.  Then the confusion counts at `s > thr` and at `s >= cutoff`.
// out[0] = cutoff (a score value, or +inf), out[1..5) = tn, fp, fn, tp at s > thr, out[5..9) = the same at s >= cutoff.
template <typename T, int BINS>
__global__ void __launch_bounds__(MT_BLOCK) point_metrics_kernel(const T* __restrict__ s, int64_t stride,
                                                                 const int32_t* __restrict__ packed, int n, double thr,
                                                                 double* __restrict__ out, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[BINS];
    __shared__ int s_tp[MT_BLOCK], s_fp[MT_BLOCK];
    __shared__ double r_j[MT_BLOCK];
    __shared__ int r_g[MT_BLOCK];
    __shared__ int s_first, s_cnt[8];
    fill_hist(hist, packed, n, nullptr, n, flag);
    int g0, g1, tp, fp, P, N;
    run_prefix(hist, n, s_tp, s_fp, g0, g1, tp, fp, P, N);
    const double dP = (double)P, dN = (double)N;
    double best = 0.0;                 // the (0, 0, inf) point
    int best_g = -1;
    for (int g = g0; g < g1; ++g) {
        const uint32_t w = hist[g];
        if (w == 0u) continue;
        const bool first = tp + fp == 0;
        tp += h_tp(w);
        fp += h_fp(w);
        bool keep = first || tp + fp == P + N;
        if (!keep) {
            int q = g + 1;
            while (q < n && hist[q] == 0u) ++q;    // the next non-empty bin (one exists: this is not the last)
            keep = q >= n || hist[q] != w;
        }
        if (keep) {
            const double j = (double)tp / dP - (double)fp / dN;
            if (j > best) { best = j; best_g = g; }
        }
    }
    r_j[threadIdx.x] = best;
    r_g[threadIdx.x] = best_g;
    if (threadIdx.x == 0) s_first = n;
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    // first maximum: the larger value, and of two equal ones the earlier position (the lower bin; -1 is the leading point)
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && (r_j[threadIdx.x + o] > r_j[threadIdx.x] ||
                                     (r_j[threadIdx.x + o] == r_j[threadIdx.x] && r_g[threadIdx.x + o] < r_g[threadIdx.x]))) {
            r_j[threadIdx.x] = r_j[threadIdx.x + o];
            r_g[threadIdx.x] = r_g[threadIdx.x + o];
        }
        __syncthreads();
    }
    const int cut_g = r_g[0];
    if (cut_g >= 0) {                   // the score of that rank: the first sample that carries it (all of them are equal)
        int mine = n;
        for (int i = threadIdx.x; i < n; i += MT_BLOCK)
            if ((packed[i] >> 1) == cut_g && i < mine) mine = i;
        if (mine < n) atomicMin(&s_first, mine);
    }
    __syncthreads();
    const bool inf_cut = cut_g < 0 || s_first >= n;
    const T cut = inf_cut ? (T)0 : s[(int64_t)s_first * stride];
    int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += MT_BLOCK) {
        const T v = s[(int64_t)i * stride];
        const int pos = packed[i] & 1;
        c[2 * pos + ((double)v > thr ? 1 : 0)] += 1;
        c[4 + 2 * pos + ((!inf_cut && v >= cut) ? 1 : 0)] += 1;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (c[k]) atomicAdd(&s_cnt[k], c[k]);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = inf_cut ? __longlong_as_double(0x7ff0000000000000ll) : (double)cut;
    if (threadIdx.x < 8) out[1 + threadIdx.x] = (double)s_cnt[threadIdx.x];
}

// ---- the curves themselves ---------------------------------------------------------------------------------------------------
// the exclusive prefix of two per-thread counts over the 256 threads and their block totals (integer sums through s_a / s_b)
__device__ __forceinline__ void count_prefix(int a, int b, int* s_a, int* s_b, int& a_before, int& b_before, int& a_all, int& b_all) {
    __syncthreads();                   // (s_a / s_b may still be read by run_prefix)
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    a_before = b_before = a_all = b_all = 0;
    for (int t = 0; t < MT_BLOCK; ++t) {
        const int x = s_a[t], y = s_b[t];
        if (t < (int)threadIdx.x) { a_before += x; b_before += y; }
        a_all += x;
        b_all += y;
    }
}

// roc_curve(drop_intermediate=True)'s rule for the non-empty bin g with word w: the first threshold, the last one, and every one
// whose (tp_g, fp_g) differs from the next non-empty bin's (which may lie in another thread's run).  seen: tp + fp before g.
__device__ __forceinline__ bool roc_keeps(const uint32_t* hist, int n, int g, uint32_t w, int seen, int total) {
    if (seen == 0 || seen + h_tp(w) + h_fp(w) == total) return true;
    int q = g + 1;
    while (q < n && hist[q] == 0u) ++q;
    return q >= n || hist[q] != w;
}

constexpr int CP_HEAD = 8;             // P, N, T, K, last_ind, 0, 0, 0
constexpr int CP_ARRAYS = 8;           // thr, rec, prec, prec_cal, roc fpr, roc tpr, roc thr, scratch: each n + 1 slots

// One block, the identity sample: the histogram walk of curve_metrics_kernel with its points written out.  See koaf.h for the
// layout.  Positions come from counting: each thread counts the thresholds and kept ROC points of its run, an exclusive prefix
// over the threads gives its offsets, and it writes there -- no atomic decides where a point goes.
template <typename T, int BINS>
__global__ void __launch_bounds__(MT_BLOCK) curve_points_kernel(const T* __restrict__ s, int64_t stride,
                                                                const int32_t* __restrict__ packed, int n, double pi0,
                                                                int pi_of_negatives, double* __restrict__ out,
                                                                uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[BINS];
    __shared__ int s_tp[MT_BLOCK], s_fp[MT_BLOCK];
    __shared__ int s_last;
    const int64_t A = (int64_t)n + 1;
    double* a_thr = out + CP_HEAD;
    double* a_rec = a_thr + A;
    double* a_prec = a_rec + A;
    double* a_cal = a_prec + A;
    double* a_fpr = a_cal + A;
    double* a_tpr = a_fpr + A;
    double* a_rthr = a_tpr + A;
    double* by_bin = a_rthr + A;       // the score of each rank bin: every sample of a bin stores the same value
    fill_hist(hist, packed, n, nullptr, n, flag);
    for (int i = threadIdx.x; i < n; i += MT_BLOCK) {
        const int g = packed[i] >> 1;
        if ((unsigned)g < (unsigned)n) by_bin[g] = (double)s[(int64_t)i * stride];
    }
    if (threadIdx.x == 0) s_last = n;
    int g0, g1, tp0, fp0, P, N;
    run_prefix(hist, n, s_tp, s_fp, g0, g1, tp0, fp0, P, N);
    const double dP = (double)P, dN = (double)N;
    const double pi = (pi_of_negatives ? dN : dP) / (double)(P + N);      // (np.sum(y_true) / n: the share of label 1)
    const double ratio = pi * (1.0 - pi0) / (pi0 * (1.0 - pi));           // (_metrics_wissam.py:151-152, in its order)
    // pass 1: how many thresholds and kept ROC points this run holds, and where (if here) full recall is reached
    int cntT = 0, cntK = 0, full = -1, tp = tp0, fp = fp0;
    for (int g = g0; g < g1; ++g) {
        const uint32_t w = hist[g];
        if (w == 0u) continue;
        if (roc_keeps(hist, n, g, w, tp + fp, P + N)) ++cntK;
        tp += h_tp(w);
        fp += h_fp(w);
        if (full < 0 && tp == P) full = cntT;
        ++cntT;
    }
    int offT, offK, allT, allK;
    count_prefix(cntT, cntK, s_tp, s_fp, offT, offK, allT, allK);
    if (full >= 0) atomicMin(&s_last, offT + full);                       // (an integer minimum: a value, not a position)
    // pass 2: the points, at their offsets.  Slot 0 of rec / prec / prec_cal is the closing (0, 1) point of the PR curves,
    // slot 0 of the ROC arrays the leading (0, 0, +inf) point.
    if (threadIdx.x == 0) {
        a_rec[0] = 0.0;
        a_prec[0] = 1.0;
        a_cal[0] = 1.0;
        a_fpr[0] = 0.0;
        a_tpr[0] = 0.0;
        a_rthr[0] = __longlong_as_double(0x7ff0000000000000ll);
    }
    __syncthreads();                   // by_bin is complete (and s_last)
    tp = tp0;
    fp = fp0;
    int64_t jt = offT, jk = (int64_t)offK + 1;
    for (int g = g0; g < g1; ++g) {
        const uint32_t w = hist[g];
        if (w == 0u) continue;
        const bool keep = roc_keeps(hist, n, g, w, tp + fp, P + N);
        tp += h_tp(w);
        fp += h_fp(w);
        const double dtp = (double)tp, dfp = (double)fp, thr = by_bin[g];
        const double rec = dtp / dP;
        const double cal = dtp / (dtp + ratio * dfp);
        a_thr[jt] = thr;
        a_rec[jt + 1] = rec;
        a_prec[jt + 1] = dtp / (double)(tp + fp);
        a_cal[jt + 1] = cal != cal ? 0.0 : cal;                           // (precision[np.isnan(precision)] = 0)
        ++jt;
        if (keep) {
            a_fpr[jk] = dfp / dN;
            a_tpr[jk] = rec;
            a_rthr[jk] = thr;
            ++jk;
        }
    }
    if (threadIdx.x == 0) {
        out[0] = dP;
        out[1] = dN;
        out[2] = (double)allT;
        out[3] = (double)allK;
        out[4] = (double)s_last;
        out[5] = out[6] = out[7] = 0.0;
    }
}

// ---- recall-range average precision and best calibrated F1 of R resamples ----------------------------------------------------
// Block r: the histogram of resample r and one ordered walk per thread along the PR curve, leading (rec 0, prec 1) point first.
// out[r][0..8): P, N, ap_range, best_f1_calib, rec_at_low, rec_at_high, 0, 0 (koaf.h).
template <int BINS>
__global__ void __launch_bounds__(MT_BLOCK) range_metrics_kernel(const int32_t* __restrict__ packed, int n,
                                                                 const int32_t* __restrict__ idx, int m, int with_identity,
                                                                 double pi0, double lo, double hi, double* __restrict__ out,
                                                                 uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[BINS];
    __shared__ int s_tp[MT_BLOCK], s_fp[MT_BLOCK];
    __shared__ double r_ap[MT_BLOCK], r_f1[MT_BLOCK], r_lo[MT_BLOCK], r_hi[MT_BLOCK];
    const int r = blockIdx.x;
    const int32_t* row = nullptr;
    int draws = n;
    if (idx != nullptr && !(with_identity && r == 0)) {
        row = idx + (int64_t)(r - (with_identity ? 1 : 0)) * m;
        draws = m;
    }
    fill_hist(hist, packed, n, row, draws, flag);
    int g0, g1, tp, fp, P, N;
    run_prefix(hist, n, s_tp, s_fp, g0, g1, tp, fp, P, N);
    const double dP = (double)P;
    const double pi = dP / (double)(P + N);
    const double ratio = pi0 > 0.0 ? pi * (1.0 - pi0) / (pi0 * (1.0 - pi)) : 1.0;      // pi0 == 0: not calibrated (tp + 1.0 * fp is exact)
    const bool ok = P > 0 && N > 0;
    double ap = 0.0, f1 = 0.0;                                            // (the closing (1, 0) point of the calibrated curve is worth 0)
    double rlo = 0.0, rhi = __longlong_as_double(0x7ff0000000000000ll);   // (the leading point has rec 0 <= lo)
    if (ok) {
        // the point ahead of the run: the counts ahead of it, or the leading point when nothing is ahead
        double rec_p = 0.0, prec_p = 1.0;
        if (tp + fp != 0) { rec_p = (double)tp / dP; prec_p = (double)tp / (double)(tp + fp); }
        for (int g = g0; g < g1; ++g) {
            const uint32_t w = hist[g];
            if (w == 0u) continue;
            const bool before_full = tp < P;                              // (tps.searchsorted(tps[-1]): the calibrated curve stops at full recall)
            tp += h_tp(w);
            fp += h_fp(w);
            const double dtp = (double)tp, dfp = (double)fp;
            const double rec = dtp / dP, prec = dtp / (double)(tp + fp);
            if (rec > lo && rec_p < hi) ap += (rec - rec_p) * (prec + prec_p) / 2.0;
            if (rec <= lo && rec > rlo) rlo = rec;
            if (rec >= hi && rec < rhi) rhi = rec;
            if (before_full) {
                double cal = dtp / (dtp + ratio * dfp);
                if (cal != cal) cal = 0.0;
                const double f = (2.0 * cal * rec) / (cal + rec);
                if (f == f && f <= 1.7976931348623157e308 && f > f1) f1 = f;   // (nan_to_num: NaN / Inf count 0)
            }
            rec_p = rec;
            prec_p = prec;
        }
    }
    r_ap[threadIdx.x] = ap;
    r_f1[threadIdx.x] = f1;
    r_lo[threadIdx.x] = rlo;
    r_hi[threadIdx.x] = rhi;
    __syncthreads();
    for (int o = MT_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            r_ap[threadIdx.x] += r_ap[threadIdx.x + o];
            if (r_f1[threadIdx.x + o] > r_f1[threadIdx.x]) r_f1[threadIdx.x] = r_f1[threadIdx.x + o];
            if (r_lo[threadIdx.x + o] > r_lo[threadIdx.x]) r_lo[threadIdx.x] = r_lo[threadIdx.x + o];
            if (r_hi[threadIdx.x + o] < r_hi[threadIdx.x]) r_hi[threadIdx.x] = r_hi[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)r * 8;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        o[0] = dP;
        o[1] = (double)N;
        o[2] = ok ? r_ap[0] / (r_hi[0] - r_lo[0]) : nan;
        o[3] = ok ? r_f1[0] : nan;
        o[4] = ok ? r_lo[0] : nan;
        o[5] = ok ? r_hi[0] : nan;
        o[6] = o[7] = 0.0;
    }
}

// ---- confusion counts ----------------------------------------------------------------------------------------------------------
// counts[t][p] += 1 per sample: per-block counts in LDS, then one global integer atomic per non-zero cell
constexpr int CF_MAX_K = 32;
__global__ void __launch_bounds__(MT_BLOCK) confusion_kernel(const int32_t* __restrict__ y_true, const int32_t* __restrict__ y_pred,
                                                             int64_t n, int K, unsigned long long* __restrict__ counts,
                                                             uint32_t* __restrict__ flag) {
    __shared__ uint32_t cell[CF_MAX_K * CF_MAX_K];
    for (int c = threadIdx.x; c < K * K; c += MT_BLOCK) cell[c] = 0u;
    __syncthreads();
    unsigned bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_BLOCK) {
        const int32_t t = y_true[i], p = y_pred[i];
        if ((unsigned)t >= (unsigned)K || (unsigned)p >= (unsigned)K) { bad = 2u; continue; }
        atomicAdd(&cell[t * K + p], 1u);
    }
    if (bad) atomicOr(flag, bad);
    __syncthreads();
    for (int c = threadIdx.x; c < K * K; c += MT_BLOCK)
        if (cell[c]) atomicAdd(&counts[c], (unsigned long long)cell[c]);
}

}  // namespace

extern "C" int64_t koaf_curve_points_len(int32_t n) { return n >= 1 ? CP_HEAD + (int64_t)CP_ARRAYS * ((int64_t)n + 1) : 0; }

extern "C" int koaf_curve_points(const void* scores, int32_t f64, int64_t stride, const int32_t* packed, int32_t n, double pi0,
                                 int32_t pi_of_negatives, double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N, "koaf_curve_points: 1 <= n <= %d (n = %d)", MT_MAX_N, n);
    KOAF_REQUIRE(stride >= 1 && stride < (1ll << 32), "koaf_curve_points: 1 <= stride < 2^32 (stride = %lld)", (long long)stride);
    KOAF_REQUIRE(scores && packed && out && flag, "koaf_curve_points: scores, packed, out and flag are required");
    KOAF_REQUIRE(pi0 > 0.0 && pi0 < 1.0, "koaf_curve_points: 0 < pi0 < 1 (pi0 = %g)", pi0);
    const dim3 grid(1), block(MT_BLOCK);
#define KOAF_CP(T, BINS) hipLaunchKernelGGL((curve_points_kernel<T, BINS>), grid, block, 0, STREAM, (const T*)scores, stride, packed, n, pi0, pi_of_negatives, out, flag)
    if (f64) { if (n <= 4096) KOAF_CP(double, 4096); else KOAF_CP(double, MT_MAX_N); }
    else { if (n <= 4096) KOAF_CP(float, 4096); else KOAF_CP(float, MT_MAX_N); }
#undef KOAF_CP
    return koaf_check_launch("koaf_curve_points");
}

extern "C" int koaf_range_metrics(const int32_t* packed, int32_t n, const int32_t* idx, int32_t R, int32_t m, int32_t with_identity,
                                  double pi0, double lo, double hi, double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N, "koaf_range_metrics: 1 <= n <= %d (n = %d)", MT_MAX_N, n);
    KOAF_REQUIRE(packed && out && flag, "koaf_range_metrics: packed, out and flag are required");
    KOAF_REQUIRE(R >= 0 && R <= (1 << 20), "koaf_range_metrics: 0 <= R <= 2^20 (R = %d)", R);
    KOAF_REQUIRE(idx != nullptr || R == 0, "koaf_range_metrics: R = %d resamples need an index matrix", R);
    KOAF_REQUIRE(idx == nullptr || (m >= 1 && m <= MT_MAX_N), "koaf_range_metrics: 1 <= m <= %d (m = %d)", MT_MAX_N, m);
    KOAF_REQUIRE(pi0 >= 0.0 && pi0 < 1.0, "koaf_range_metrics: 0 <= pi0 < 1, 0 for no calibration (pi0 = %g)", pi0);
    KOAF_REQUIRE(0.0 <= lo && lo <= hi && hi <= 1.0, "koaf_range_metrics: 0 <= lo <= hi <= 1 (lo = %g, hi = %g)", lo, hi);
    const int rows = R + (with_identity ? 1 : 0);
    KOAF_REQUIRE(rows >= 1, "koaf_range_metrics: nothing to do (R = 0 and no identity row)");
    const dim3 grid((unsigned)rows), block(MT_BLOCK);
    const int32_t* ix = R > 0 ? idx : nullptr;
    if (n <= 4096)
        hipLaunchKernelGGL(range_metrics_kernel<4096>, grid, block, 0, STREAM, packed, n, ix, m, with_identity, pi0, lo, hi, out, flag);
    else
        hipLaunchKernelGGL(range_metrics_kernel<MT_MAX_N>, grid, block, 0, STREAM, packed, n, ix, m, with_identity, pi0, lo, hi, out,
                           flag);
    return koaf_check_launch("koaf_range_metrics");
}

extern "C" int koaf_confusion(const int32_t* y_true, const int32_t* y_pred, int64_t n, int32_t K, int64_t* counts, uint32_t* flag,
                              void* stream) {
    KOAF_REQUIRE(n >= 1 && n < (1ll << 31), "koaf_confusion: 1 <= n < 2^31 (n = %lld)", (long long)n);
    KOAF_REQUIRE(K >= 1 && K <= CF_MAX_K, "koaf_confusion: 1 <= K <= %d (K = %d)", CF_MAX_K, K);
    KOAF_REQUIRE(y_true && y_pred && counts && flag, "koaf_confusion: y_true, y_pred, counts and flag are required");
    const int64_t blocks = cdiv64(n, MT_BLOCK * 8);
    const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024)), block(MT_BLOCK);
    hipLaunchKernelGGL(confusion_kernel, grid, block, 0, STREAM, y_true, y_pred, n, K, (unsigned long long*)counts, flag);
    return koaf_check_launch("koaf_confusion");
}

extern "C" int koaf_score_ranks(const void* scores, int32_t f64, int64_t stride, int32_t n, const int32_t* labels,
                                int32_t pos_label, int32_t* rank, int32_t* packed, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N, "koaf_score_ranks: 1 <= n <= %d (n = %d)", MT_MAX_N, n);
    KOAF_REQUIRE(stride >= 1 && stride < (1ll << 32), "koaf_score_ranks: 1 <= stride < 2^32 (stride = %lld)", (long long)stride);
    KOAF_REQUIRE(scores && flag && (rank || packed), "koaf_score_ranks: scores, flag and one of rank / packed are required");
    KOAF_REQUIRE((labels != nullptr) == (packed != nullptr), "koaf_score_ranks: labels and packed go together");
    const dim3 grid((unsigned)cdiv64(n, MT_BLOCK)), block(MT_BLOCK);
    if (f64)
        hipLaunchKernelGGL(score_ranks_kernel<double>, grid, block, 0, STREAM, (const double*)scores, stride, n, labels, pos_label,
                           rank, packed, flag);
    else
        hipLaunchKernelGGL(score_ranks_kernel<float>, grid, block, 0, STREAM, (const float*)scores, stride, n, labels, pos_label,
                           rank, packed, flag);
    return koaf_check_launch("koaf_score_ranks");
}

extern "C" int koaf_curve_metrics(const int32_t* packed, int32_t n, const int32_t* idx, int32_t R, int32_t m,
                                  int32_t with_identity, double pi0, double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N, "koaf_curve_metrics: 1 <= n <= %d (n = %d)", MT_MAX_N, n);
    KOAF_REQUIRE(packed && out && flag, "koaf_curve_metrics: packed, out and flag are required");
    KOAF_REQUIRE(R >= 0 && R <= (1 << 20), "koaf_curve_metrics: 0 <= R <= 2^20 (R = %d)", R);
    KOAF_REQUIRE(idx != nullptr || R == 0, "koaf_curve_metrics: R = %d resamples need an index matrix", R);
    KOAF_REQUIRE(idx == nullptr || (m >= 1 && m <= MT_MAX_N), "koaf_curve_metrics: 1 <= m <= %d (m = %d)", MT_MAX_N, m);
    KOAF_REQUIRE(pi0 > 0.0 && pi0 < 1.0, "koaf_curve_metrics: 0 < pi0 < 1 (pi0 = %g)", pi0);
    const int rows = R + (with_identity ? 1 : 0);
    KOAF_REQUIRE(rows >= 1, "koaf_curve_metrics: nothing to do (R = 0 and no identity row)");
    const dim3 grid((unsigned)rows), block(MT_BLOCK);
    const int32_t* ix = R > 0 ? idx : nullptr;
    if (n <= 4096)
        hipLaunchKernelGGL(curve_metrics_kernel<4096>, grid, block, 0, STREAM, packed, n, ix, m, with_identity, pi0, out, flag);
    else
        hipLaunchKernelGGL(curve_metrics_kernel<MT_MAX_N>, grid, block, 0, STREAM, packed, n, ix, m, with_identity, pi0, out, flag);
    return koaf_check_launch("koaf_curve_metrics");
}

extern "C" int koaf_pair_ranks(const void* a, int64_t stride_a, const void* b, int64_t stride_b, int32_t f64, int32_t n,
                               const int32_t* labels, int32_t pos_label, int32_t* rank, int32_t* packed, uint32_t* flag,
                               void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N / 2, "koaf_pair_ranks: 1 <= n <= %d (n = %d)", MT_MAX_N / 2, n);
    KOAF_REQUIRE(stride_a >= 1 && stride_a < (1ll << 32) && stride_b >= 1 && stride_b < (1ll << 32),
                 "koaf_pair_ranks: 1 <= stride < 2^32 (strides = %lld, %lld)", (long long)stride_a, (long long)stride_b);
    KOAF_REQUIRE(a && b && flag && (rank || packed), "koaf_pair_ranks: both score columns, flag and one of rank / packed are required");
    KOAF_REQUIRE((labels != nullptr) == (packed != nullptr), "koaf_pair_ranks: labels and packed go together");
    const dim3 grid((unsigned)cdiv64(2 * n, MT_BLOCK)), block(MT_BLOCK);
    if (f64)
        hipLaunchKernelGGL(pair_ranks_kernel<double>, grid, block, 0, STREAM, (const double*)a, stride_a, (const double*)b, stride_b,
                           n, labels, pos_label, rank, packed, flag);
    else
        hipLaunchKernelGGL(pair_ranks_kernel<float>, grid, block, 0, STREAM, (const float*)a, stride_a, (const float*)b, stride_b, n,
                           labels, pos_label, rank, packed, flag);
    return koaf_check_launch("koaf_pair_ranks");
}

extern "C" int koaf_perm_metrics(const int32_t* packed, int32_t n, const uint32_t* masks, int32_t R, int32_t with_identity,
                                 double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N / 2, "koaf_perm_metrics: 1 <= n <= %d (n = %d)", MT_MAX_N / 2, n);
    KOAF_REQUIRE(packed && out && flag, "koaf_perm_metrics: packed, out and flag are required");
    KOAF_REQUIRE(R >= 0 && R <= (1 << 20), "koaf_perm_metrics: 0 <= R <= 2^20 (R = %d)", R);
    KOAF_REQUIRE(masks != nullptr || R == 0, "koaf_perm_metrics: R = %d permutations need a mask matrix", R);
    const int rows = R + (with_identity ? 1 : 0);
    KOAF_REQUIRE(rows >= 1, "koaf_perm_metrics: nothing to do (R = 0 and no identity row)");
    const dim3 grid((unsigned)rows, 2), block(MT_BLOCK);
    const uint32_t* mk = R > 0 ? masks : nullptr;
    const int W = (n + 31) / 32;
    if (2 * n <= 4096)
        hipLaunchKernelGGL(perm_metrics_kernel<4096>, grid, block, 0, STREAM, packed, n, mk, W, with_identity, out, flag);
    else
        hipLaunchKernelGGL(perm_metrics_kernel<MT_MAX_N>, grid, block, 0, STREAM, packed, n, mk, W, with_identity, out, flag);
    return koaf_check_launch("koaf_perm_metrics");
}

extern "C" int koaf_point_metrics(const void* scores, int32_t f64, int64_t stride, const int32_t* packed, int32_t n, double thr,
                                  double* out, uint32_t* flag, void* stream) {
    KOAF_REQUIRE(n >= 1 && n <= MT_MAX_N, "koaf_point_metrics: 1 <= n <= %d (n = %d)", MT_MAX_N, n);
    KOAF_REQUIRE(stride >= 1 && stride < (1ll << 32), "koaf_point_metrics: 1 <= stride < 2^32 (stride = %lld)", (long long)stride);
    KOAF_REQUIRE(scores && packed && out && flag, "koaf_point_metrics: scores, packed, out and flag are required");
    const dim3 grid(1), block(MT_BLOCK);
#define KOAF_PM(T, BINS) hipLaunchKernelGGL((point_metrics_kernel<T, BINS>), grid, block, 0, STREAM, (const T*)scores, stride, packed, n, thr, out, flag)
    if (f64) { if (n <= 4096) KOAF_PM(double, 4096); else KOAF_PM(double, MT_MAX_N); }
    else { if (n <= 4096) KOAF_PM(float, 4096); else KOAF_PM(float, MT_MAX_N); }
#undef KOAF_PM
    return koaf_check_launch("koaf_point_metrics");
}
