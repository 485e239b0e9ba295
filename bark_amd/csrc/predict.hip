// Predictions from a fitted posterior (contract in include/bark_hip.h, bark_leaf_posterior_predict_hip): the moments of the
// weighted mixture of the forests' posteriors at C points, its quantiles, the per-forest posteriors themselves and the
// predictive scores of targets under the weighted mixture.  The scan of acquire.hip returns an acquisition value and the score
// scan of scores.hip sums of log densities; this unit returns what both of them form on the way, mu_b and var_b, reduced over
// the forests per point.
//
// Per forest b and point x, mu_b = c s1 and var_b = (scale / m)(dg + 2 off) from the leaf-space sums of acq_point.h, exactly as
// acq_scan_kernel and score_scan_kernel form them; with `observation` var_b + s2_b.  The kernels:
//   predict_scan_kernel      one thread per point; the forests of the chunk in order.  Per point West's weighted one-pass
//                            recurrence over the forests of non-zero weight (W, mean, S, V), kept in a (4, C) buffer between
//                            chunks; optionally mu_b / var_b stored per (forest, point), and the score terms of
//                            score_scan_kernel: per-forest tile partials and the online log-sum-exp, with l + log w_b under weights
//   predict_quantile_kernel  one thread per (point, probability): the root of the mixture's distribution function by a Newton
//                            step on its density inside a bracket that every evaluation tightens; it reads only the stored
//                            mu_b, var_b and the weights, in forest order
//   predict_flag_kernel      one word: does a forest of non-zero weight report a non-zero status?
//   predict_mask_kernel      NaN into the rows of forest_out whose forest reports a non-zero status
//   predict_finish_kernel    mean and (V + S) / W per point, NaN under the flag; predict_poison_kernel the same for the quantiles
//   predict_points_kernel / predict_final_kernel   the mixture's scores per point and their sums, as in scores.hip
// No float atomics; the order of every sum is fixed (leaves in code-bit order, forests 0 .. B-1, lanes and waves of a tile by
// tile_sum2's tree, tiles in index order), so no result depends on the chunk or on the variant.
#include "acq_point.h"

namespace bark {
namespace {

constexpr double PRED_TWO_PI = 6.28318530717958647693;
constexpr double PRED_SQRT2 = 1.41421356237309504880;
constexpr int PRED_MAX_ITER = 256;  // a bracket of doubles is exhausted by bisection alone long before

// Arguments as score_scan_kernel's (LDS_TABLE, ccodes, n, first, info, yp, fpart / tiles / tile0), and: weights the chunk's rows of
// the normalised weights or null (every forest then weighs wq = 1 / B), acc the slab's part of the (4, C) recurrence state
// (rows W, mean, S, V; row stride astride), sacc that of the (3, C) score state (score_scan_kernel's rows), fmu / fvar the
// chunk's first rows of the per-forest output (row stride fstride) or null.
// SCORES: yp, sacc and fpart are used, and every thread of the workgroup meets the barriers of the tile sums.
template <bool LDS_TABLE, bool SCORES>
__global__ __launch_bounds__(ACQ_TILE) void predict_scan_kernel(const uint32_t *__restrict__ ccodes, int W, int cpad, int n,
                                                                const double *__restrict__ wvec, const double *__restrict__ Minv,
                                                                const double *__restrict__ tab, int R,
                                                                const double *__restrict__ noise, const double *__restrict__ scale,
                                                                int m, int bc, const int32_t *__restrict__ info,
                                                                const double *__restrict__ weights, double wq, int observation,
                                                                const double *__restrict__ yp, int first, double *__restrict__ acc,
                                                                size_t astride, double *__restrict__ sacc, double *__restrict__ fmu,
                                                                double *__restrict__ fvar, size_t fstride,
                                                                double *__restrict__ fpart, int tiles, int tile0) {
    extern __shared__ double smem[];  // all of it may be taken (the plan admits tables up to a CU's LDS): no static LDS beside it
    const int tid = threadIdx.x;
    const int c = blockIdx.x * ACQ_TILE + tid;
    const bool active = c < n;
    const int tri = R * (R + 1) / 2;
    unsigned short *idx = reinterpret_cast<unsigned short *>(smem + (LDS_TABLE ? tri + R : 0)) + tid;
    const double y = SCORES && active ? yp[c] : 0.0;
    double Ws = 0.0, mean = 0.0, S = 0.0, V = 0.0;
    double mx = -INFINITY, se = 0.0, sm = 0.0;
    if (active && !first) {
        Ws = acc[c];
        mean = acc[astride + c];
        S = acc[2 * astride + c];
        V = acc[3 * astride + c];
        if (SCORES) {
            mx = sacc[c];
            se = sacc[astride + c];
            sm = sacc[2 * astride + c];
        }
    }
    for (int b = 0; b < bc; ++b) {
        // b and weights[b] are uniform over the workgroup: every thread takes this branch together, so the barriers below are
        // skipped by all of them or by none
        const double wt = weights ? weights[b] : wq;
        if (wt == 0.0) {
            if (active && fmu) {
                fmu[(size_t)b * fstride + c] = NAN;
                fvar[(size_t)b * fstride + c] = NAN;
            }
            continue;
        }
        if (LDS_TABLE || SCORES) __syncthreads();  // the previous forest's reads are done, those of its tile sums included
        if (LDS_TABLE) stage_table(tab, b, tri, R, smem);
        int cnt = active ? point_leaves(ccodes, W, cpad, b, c, m, R, idx) : 0;
        if (cnt > m) cnt = m;
        if (LDS_TABLE) __syncthreads();
        double l = 0.0, sq = 0.0;
        if (active) {
            double s1, dg, off;
            point_sums<LDS_TABLE>(idx, cnt, smem, LDS_TABLE ? smem + tri : wvec + (size_t)b * R, Minv + (size_t)b * R * R, R, s1, dg,
                                  off);
            const double sigma2 = 1e-6 + noise[b];
            const double sc = scale[b];
            double mu = sc / ((double)m * sigma2) * s1;
            double var = sc / (double)m * (dg + 2.0 * off);
            if (observation) var += sigma2;
            if (info[b] != 0) mu = var = NAN;
            if (fmu) {
                fmu[(size_t)b * fstride + c] = mu;
                fvar[(size_t)b * fstride + c] = var;
            }
            Ws += wt;
            const double delta = mu - mean;
            mean += wt / Ws * delta;
            S += wt * delta * (mu - mean);
            V += wt * var;
            if (SCORES) {
                const double r = y - mu;
                sq = r * r;
                l = -0.5 * log(PRED_TWO_PI * var) - 0.5 * sq / var;
                const double lw = weights ? l + log(wt) : l;
                // score_scan_kernel's online log-sum-exp, over l + log w under weights
                const double top = lw > mx ? lw : mx;
                if (!(lw == -INFINITY && mx == -INFINITY)) se = se * exp(mx - top) + exp(lw - top);
                mx = top;
                sm += mu;
            }
        }
        if (SCORES) {
            __syncthreads();  // table and lists are read: the tile sums go through the front of the LDS (at least 512 bytes of lists)
            tile_sum2(l, sq, smem);
            if (tid == 0) {
                double *dst = fpart + ((size_t)b * tiles + tile0 + blockIdx.x) * 2;
                dst[0] = l;
                dst[1] = sq;
            }
        }
    }
    if (active) {
        acc[c] = Ws;
        acc[astride + c] = mean;
        acc[2 * astride + c] = S;
        acc[3 * astride + c] = V;
        if (SCORES) {
            sacc[c] = mx;
            sacc[astride + c] = se;
            sacc[2 * astride + c] = sm;
        }
    }
}

// F(t) = sum_b w_b Phi((t - mu_b) / sd_b) and its density at point c, forests in order from 0.0, weight 0 skipped; a forest
// with sd = 0 is a step at mu (F counts it from t = mu on, the density does not see it)
__device__ __forceinline__ void mixture_cdf(const double *__restrict__ fmu, const double *__restrict__ fvar, size_t fstride, int c,
                                            int B, const double *__restrict__ weights, double wq, double t, double &F, double &f) {
    F = 0.0, f = 0.0;
    for (int b = 0; b < B; ++b) {
        const double w = weights ? weights[b] : wq;
        if (w == 0.0) continue;
        const double mu = fmu[(size_t)b * fstride + c];
        const double var = fvar[(size_t)b * fstride + c];
        const double sd = sqrt(var > 0.0 ? var : 0.0);
        if (sd > 0.0) {
            const double x = (t - mu) / (sd * PRED_SQRT2);
            F += w * (0.5 * erfc(-x));
            f += w * (exp(-(x * x)) * ACQ_INV_SQRT_2PI / sd);
        } else {
            F += w * (t >= mu ? 1.0 : (t < mu ? 0.0 : NAN));
        }
    }
}

struct PredictProbs {
    double p[16], z[16];
};

// thread (c, q = blockIdx.y): out[q ostride + c] = the t with F(t) = p_q.  Bracket: the smallest and the largest component
// quantile mu_b + z_q sd_b; F(lo) >= p gives lo, F(hi) < p gives hi.  Inside, every evaluated t becomes an end of the bracket
// (lo while F(t) < p, else hi) and the next t is the Newton step t - (F(t) - p) / f(t) when that lies strictly inside the
// bracket, else its midpoint; the first t is the secant point of the two ends.  It stops when the step no longer moves t or the
// bracket has no interior point (then hi, the smallest t seen with F(t) >= p).  NaN where the flag is set or F is NaN.
__global__ __launch_bounds__(256) void predict_quantile_kernel(const double *__restrict__ fmu, const double *__restrict__ fvar,
                                                               size_t fstride, int n, int B, const double *__restrict__ weights,
                                                               double wq, PredictProbs pr, const int32_t *__restrict__ flag,
                                                               double *__restrict__ out, size_t ostride) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int q = blockIdx.y;
    double *dst = out + (size_t)q * ostride + c;
    if (*flag) {
        *dst = NAN;
        return;
    }
    double p = 0.0, z = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)  // a select per entry: indexing the by-value argument would put it into scratch
        if (k == q) p = pr.p[k], z = pr.z[k];
    double lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < B; ++b) {
        const double w = weights ? weights[b] : wq;
        if (w == 0.0) continue;
        const double var = fvar[(size_t)b * fstride + c];
        const double cq = fmu[(size_t)b * fstride + c] + z * sqrt(var > 0.0 ? var : 0.0);
        if (cq < lo) lo = cq;
        if (cq > hi) hi = cq;
    }
    double Flo, Fhi, f;
    mixture_cdf(fmu, fvar, fstride, c, B, weights, wq, lo, Flo, f);
    if (!(Flo < p)) {  // F(lo) >= p, or NaN
        *dst = Flo >= p ? lo : NAN;
        return;
    }
    mixture_cdf(fmu, fvar, fstride, c, B, weights, wq, hi, Fhi, f);
    if (!(Fhi >= p)) {
        *dst = Fhi < p ? hi : NAN;
        return;
    }
    double t = lo + (p - Flo) / (Fhi - Flo) * (hi - lo);
    if (!(t > lo && t < hi)) t = 0.5 * (lo + hi);
    double res = hi;
    if (t > lo && t < hi) {
        for (int it = 0; it < PRED_MAX_ITER; ++it) {
            double F;
            mixture_cdf(fmu, fvar, fstride, c, B, weights, wq, t, F, f);
            if (F != F) {
                res = NAN;
                break;
            }
            if (F < p)
                lo = t;
            else
                hi = t;
            double tn = t - (F - p) / f;
            res = t;
            if (tn == t) break;
            if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
            if (!(tn > lo && tn < hi)) {  // no double strictly between the ends
                res = hi;
                break;
            }
            t = tn;
        }
    }
    *dst = res;
}

// one workgroup: *flag = a forest of non-zero weight has a non-zero status
__global__ __launch_bounds__(256) void predict_flag_kernel(const int32_t *__restrict__ info, const double *__restrict__ weights, int B,
                                                           int32_t *__restrict__ flag) {
    int mine = 0;
    for (int b = threadIdx.x; b < B; b += 256) mine |= info[b] != 0 && (!weights || weights[b] != 0.0);
    const int any = __syncthreads_or(mine);
    if (threadIdx.x == 0) *flag = any ? 1 : 0;
}

// rows b of fo (2, B, C) to NaN where info[b] != 0; grid (tiles, up to 65535): row blockIdx.y and every gridDim.y-th after it
__global__ __launch_bounds__(256) void predict_mask_kernel(const int32_t *__restrict__ info, long long B, long long C,
                                                           double *__restrict__ fo) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        if (info[b] == 0) continue;
        fo[b * C + c] = NAN;
        fo[(B + b) * C + c] = NAN;
    }
}

// moments_out (2, C): the recurrence's mean and (V + S) / W
__global__ __launch_bounds__(256) void predict_finish_kernel(const double *__restrict__ acc, long long C, const int32_t *__restrict__ flag,
                                                             double *__restrict__ moments) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const bool bad = *flag != 0;
    moments[c] = bad ? NAN : acc[C + c];
    moments[C + c] = bad ? NAN : (acc[3 * C + c] + acc[2 * C + c]) / acc[c];
}

__global__ __launch_bounds__(256) void predict_poison_kernel(double *__restrict__ out, long long n, const int32_t *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && *flag) out[i] = NAN;
}

// score_points_kernel for the weighted mixture: mx + log(se) and the squared error against the recurrence's mean with weights,
// mx + log(se / B) and the squared error against (sum_b mu_b) / B without (that kernel's own arithmetic)
__global__ __launch_bounds__(ACQ_TILE) void predict_points_kernel(const double *__restrict__ acc, const double *__restrict__ sacc,
                                                                  long long C, int B, int weighted, const double *__restrict__ yp,
                                                                  double *__restrict__ values_out, double *__restrict__ mpart) {
    __shared__ double red[8];
    const long long c = (long long)blockIdx.x * ACQ_TILE + threadIdx.x;
    double l = 0.0, sq = 0.0;
    if (c < C) {
        l = weighted ? sacc[c] + log(sacc[C + c]) : sacc[c] + log(sacc[C + c] / (double)B);
        const double r = yp[c] - (weighted ? acc[C + c] : sacc[2 * C + c] / (double)B);
        sq = r * r;
        if (values_out) {
            values_out[c] = l;
            values_out[C + c] = sq;
        }
    }
    tile_sum2(l, sq, red);
    if (threadIdx.x == 0) {
        mpart[(size_t)blockIdx.x * 2] = l;
        mpart[(size_t)blockIdx.x * 2 + 1] = sq;
    }
}

// one workgroup: mixture_out from the tiles in index order, NaN under the flag; NaN rows of per_forest_out for the forests
// with a non-zero status and for those of weight 0 (which the scan skipped)
__global__ __launch_bounds__(64) void predict_final_kernel(const double *__restrict__ mpart, int tiles, const int32_t *__restrict__ info,
                                                           const double *__restrict__ weights, int B, const int32_t *__restrict__ flag,
                                                           double *__restrict__ per_forest_out, double *__restrict__ mixture_out) {
    for (int b = threadIdx.x; b < B; b += 64)
        if (info[b] != 0 || (weights && weights[b] == 0.0)) {
            per_forest_out[2 * b] = NAN;
            per_forest_out[2 * b + 1] = NAN;
        }
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int k = 0; k < tiles; ++k) s += mpart[(size_t)k * 2 + threadIdx.x];
        mixture_out[threadIdx.x] = *flag ? NAN : s;
    }
}

using PredictKernel = decltype(&predict_scan_kernel<true, true>);
PredictKernel predict_kernel(bool lds, bool scores) {
    if (scores) return lds ? predict_scan_kernel<true, true> : predict_scan_kernel<false, true>;
    return lds ? predict_scan_kernel<true, false> : predict_scan_kernel<false, false>;
}

// the LDS variant of predict_scan_kernel can use a whole CU's LDS; predict_scan calls this before it launches
int raise_predict_lds_limits() {
    static const LdsLimit limits[] = {{reinterpret_cast<const void *>(predict_kernel(true, false)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(predict_kernel(true, true)), ACQ_LDS_MAX}};
    static LdsLimitsOnce once;
    return raise_lds_limits(once, limits);
}

}  // namespace

int predict_scan(int variant, bool scores, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
                 const double *tab, int R, const double *noise, const double *scale, int m, int bc, const int32_t *info,
                 const double *weights, double wq, int observation, const double *yp, int first, double *acc, size_t astride,
                 double *sacc, double *fmu, double *fvar, size_t fstride, double *fpart, int tiles, int tile0, hipStream_t s) {
    const dim3 g((unsigned)((n + ACQ_TILE - 1) / ACQ_TILE));
    const int rc = raise_predict_lds_limits();
    if (rc) return rc;
    const bool lds = variant == 1;
    hipLaunchKernelGGL(predict_kernel(lds, scores), g, dim3(ACQ_TILE), scan_lds_bytes(R, m, lds), s, ccodes, W, cpad, n, wvec, Minv, tab,
                       R, noise, scale, m, bc, info, weights, wq, observation, yp, first, acc, astride, sacc, fmu, fvar, fstride, fpart,
                       tiles, tile0);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int predict_quantiles(const double *fmu, const double *fvar, size_t fstride, int n, int B, const double *weights, double wq,
                      const double *probs, const double *zscores, int Q, const int32_t *flag, double *out, size_t ostride,
                      hipStream_t s) {
    PredictProbs pr{};
    for (int q = 0; q < Q; ++q) pr.p[q] = probs[q], pr.z[q] = zscores[q];
    hipLaunchKernelGGL(predict_quantile_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)Q), dim3(256), 0, s, fmu, fvar, fstride, n, B,
                       weights, wq, pr, flag, out, ostride);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int predict_flag(const int32_t *info, const double *weights, int B, int32_t *flag, hipStream_t s) {
    hipLaunchKernelGGL(predict_flag_kernel, dim3(1), dim3(256), 0, s, info, weights, B, flag);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int predict_finish(const double *acc, int64_t C, int B, const int32_t *info, const int32_t *flag, double *moments_out,
                   double *forest_out, double *quantiles_out, int Q, hipStream_t s) {
    const unsigned tiles = (unsigned)((C + 255) / 256);
    hipLaunchKernelGGL(predict_finish_kernel, dim3(tiles), dim3(256), 0, s, acc, (long long)C, flag, moments_out);
    BARK_LAUNCH_CHECK();
    if (forest_out) {
        hipLaunchKernelGGL(predict_mask_kernel, dim3(tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, s, info, (long long)B,
                           (long long)C, forest_out);
        BARK_LAUNCH_CHECK();
    }
    if (Q > 0) {
        const long long n = (long long)Q * C;
        hipLaunchKernelGGL(predict_poison_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, quantiles_out, n, flag);
        BARK_LAUNCH_CHECK();
    }
    return BARK_OK;
}

int predict_score_finish(const double *acc, const double *sacc, int64_t C, int B, const double *weights, const double *yp,
                         double *values_out, double *mpart, const int32_t *info, const int32_t *flag, double *per_forest_out,
                         double *mixture_out, hipStream_t s) {
    const int tiles = (int)acq_partials(C);
    hipLaunchKernelGGL(predict_points_kernel, dim3((unsigned)tiles), dim3(ACQ_TILE), 0, s, acc, sacc, (long long)C, B, weights ? 1 : 0, yp,
                       values_out, mpart);
    BARK_LAUNCH_CHECK();
    hipLaunchKernelGGL(predict_final_kernel, dim3(1), dim3(64), 0, s, mpart, tiles, info, weights, B, flag, per_forest_out, mixture_out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace bark
