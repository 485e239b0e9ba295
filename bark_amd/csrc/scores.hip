// Predictive scores in leaf space (contract in include/bark_hip.h): log densities and squared errors of targets under the forest
// samples' posteriors at held-out points, or under their leave-one-out predictives at the training points, reduced over the
// points per forest and over the forests per point without a (B, C) intermediate.  The scan of acquire.hip sums over forests
// and takes a minimum over candidates; this unit sums over points per forest and takes a log-mean-exp over forests per point.
//
// Per forest b and point x (leaves a_0 < a_1 < ..., acq_point.h) the two leaf-space sums s1 = sum_i w[a_i] and
// q = z'M^-1 z = dg + 2 off give, with c = scale / (m s2):
//     held out:        mu = c s1,                         var = (scale / m) q              (the scan's mu_b and var_b)
//     leave one out:   mu = y - (y - c s1) / (1 - c q),   var = s2 / (1 - c q)             (x = x_i, y = y_i; derivation in the header)
// and l = -0.5 log(2 pi var) - 0.5 (y - mu)^2 / var.  The kernels:
//   score_scan_kernel     one thread per point; the forests of the chunk in order.  Per point the running maximum and the rescaled
//                         sum of the log-sum-exp over forests and the sum of mu, kept in a (3, C) buffer between chunks; per forest
//                         the tile's sums of l and (y - mu)^2 by a fixed tree (wave butterfly, then the four waves in order), one
//                         partial pair per (forest, tile)
//   score_forests_kernel  per forest of the chunk the tiles' partials in index order -> per_forest_out
//   score_points_kernel   the mixture's log density and squared error per point, their tile sums by the same tree
//   score_final_kernel    the tiles in index order -> mixture_out; NaN wherever info says a forest failed
// No float atomics; the order of every sum is fixed (leaves in code-bit order, forests 0 .. B-1, lanes and waves of a tile by the
// tree, tiles in index order), so the result depends neither on the chunk nor on the variant: both variants of score_scan_kernel
// run the same arithmetic on the same values.
#include "acq_point.h"

namespace bark {
namespace {

constexpr double SCORE_TWO_PI = 6.28318530717958647693;

// Arguments as acq_scan_kernel's (LDS_TABLE, ccodes, n, acc / astride, first), and: info (bc) the sweep's status of the chunk's
// forests (a failed forest counts as mu = var = NaN), yp the targets of the slab's points, fpart (bc, tiles, 2) with this
// workgroup's tile at tile0 + blockIdx.x.  Rows of acc: running maximum of l over the forests so far, sum of exp(l - maximum),
// sum of mu.  Points past n add +0 to the tile sums.
template <bool LDS_TABLE, int MODE>
__global__ __launch_bounds__(ACQ_TILE) void score_scan_kernel(const uint32_t *__restrict__ ccodes, int W, int cpad, int n,
                                                              const double *__restrict__ wvec, const double *__restrict__ Minv,
                                                              const double *__restrict__ tab, int R,
                                                              const double *__restrict__ noise, const double *__restrict__ scale,
                                                              int m, int bc, const int32_t *__restrict__ info,
                                                              const double *__restrict__ yp, int first, double *__restrict__ acc,
                                                              size_t astride, double *__restrict__ fpart, int tiles, int tile0) {
    extern __shared__ double smem[];  // all of it may be taken (the plan admits tables up to a CU's LDS): no static LDS beside it
    const int tid = threadIdx.x;
    const int c = blockIdx.x * ACQ_TILE + tid;
    const bool active = c < n;
    const int tri = R * (R + 1) / 2;
    unsigned short *idx = reinterpret_cast<unsigned short *>(smem + (LDS_TABLE ? tri + R : 0)) + tid;
    const double y = active ? yp[c] : 0.0;
    double mx = -INFINITY, se = 0.0, sm = 0.0;
    if (active && !first) {
        mx = acc[c];
        se = acc[astride + c];
        sm = acc[2 * astride + c];
    }
    for (int b = 0; b < bc; ++b) {
        __syncthreads();  // the previous forest's reads are done, those of its tile sums included
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
            if (MODE == BARK_SCORE_LOO) {
                const double den = 1.0 - sc / ((double)m * sigma2) * (dg + 2.0 * off);  // s2 [K_s^-1]_ii
                mu = y - (y - mu) / den;
                var = sigma2 / den;
            }
            if (info[b] != 0) mu = var = NAN;
            const double r = y - mu;
            sq = r * r;
            l = -0.5 * log(SCORE_TWO_PI * var) - 0.5 * sq / var;
            // log-sum-exp over the forests so far as (mx, se): sum_b exp(l_b) = exp(mx) se.  A NaN l makes se NaN; l = -inf
            // while mx = -inf adds nothing.
            const double top = l > mx ? l : mx;
            if (!(l == -INFINITY && mx == -INFINITY)) se = se * exp(mx - top) + exp(l - top);
            mx = top;
            sm += mu;
        }
        __syncthreads();  // table and lists are read: the tile sums go through the front of the LDS (at least 512 bytes of lists)
        tile_sum2(l, sq, smem);
        if (tid == 0) {
            double *dst = fpart + ((size_t)b * tiles + tile0 + blockIdx.x) * 2;
            dst[0] = l;
            dst[1] = sq;
        }
    }
    if (active) {
        acc[c] = mx;
        acc[astride + c] = se;
        acc[2 * astride + c] = sm;
    }
}

// thread (b, k): rows[b][k] = the tiles' partials of forest b in index order
__global__ __launch_bounds__(64) void score_forests_kernel(const double *__restrict__ fpart, int tiles, int bc,
                                                           double *__restrict__ rows) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * bc) return;
    const double *src = fpart + (size_t)(t >> 1) * tiles * 2 + (t & 1);
    double s = 0.0;
    for (int k = 0; k < tiles; ++k) s += src[(size_t)k * 2];
    rows[t] = s;
}

// per point: log((1/B) sum_b N(y; mu_b, var_b)) = mx + log(se / B) and (y - (1/B) sum_b mu_b)^2; mpart (tiles, 2)
__global__ __launch_bounds__(ACQ_TILE) void score_points_kernel(const double *__restrict__ acc, long long C, int B,
                                                                const double *__restrict__ yp, double *__restrict__ values_out,
                                                                double *__restrict__ mpart) {
    __shared__ double red[8];
    const long long c = (long long)blockIdx.x * ACQ_TILE + threadIdx.x;
    double l = 0.0, sq = 0.0;
    if (c < C) {
        l = acc[c] + log(acc[C + c] / (double)B);
        const double r = yp[c] - acc[2 * C + c] / (double)B;
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

// one workgroup: mixture_out from the tiles in index order; with a forest whose info != 0 (sweep failed, or an invalid categorical
// value met by one of its walks) its row of per_forest_out and mixture_out are NaN
__global__ __launch_bounds__(64) void score_final_kernel(const double *__restrict__ mpart, int tiles,
                                                         const int32_t *__restrict__ info, int B,
                                                         double *__restrict__ per_forest_out, double *__restrict__ mixture_out) {
    int bad = 0;
    for (int b = threadIdx.x; b < B; b += 64)
        if (info[b] != 0) {
            bad = 1;
            per_forest_out[2 * b] = NAN;
            per_forest_out[2 * b + 1] = NAN;
        }
    bad = __any(bad);
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int k = 0; k < tiles; ++k) s += mpart[(size_t)k * 2 + threadIdx.x];
        mixture_out[threadIdx.x] = bad ? NAN : s;
    }
}

using ScoreKernel = decltype(&score_scan_kernel<true, BARK_SCORE_HELDOUT>);
ScoreKernel score_kernel(bool lds, int mode) {
    if (mode == BARK_SCORE_LOO) return lds ? score_scan_kernel<true, BARK_SCORE_LOO> : score_scan_kernel<false, BARK_SCORE_LOO>;
    return lds ? score_scan_kernel<true, BARK_SCORE_HELDOUT> : score_scan_kernel<false, BARK_SCORE_HELDOUT>;
}

// the LDS variant of score_scan_kernel can use a whole CU's LDS; score_scan calls this before it launches
int raise_score_lds_limits() {
    static const LdsLimit limits[] = {{reinterpret_cast<const void *>(score_kernel(true, BARK_SCORE_HELDOUT)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(score_kernel(true, BARK_SCORE_LOO)), ACQ_LDS_MAX}};
    static LdsLimitsOnce once;
    return raise_lds_limits(once, limits);
}

}  // namespace

int score_scan(int variant, int mode, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
               const double *tab, int R, const double *noise, const double *scale, int m, int bc, const int32_t *info,
               const double *yp, int first, double *acc, size_t astride, double *fpart, int tiles, int tile0, hipStream_t s) {
    const dim3 g((unsigned)((n + ACQ_TILE - 1) / ACQ_TILE));
    const int rc = raise_score_lds_limits();
    if (rc) return rc;
    const bool lds = variant == 1;
    hipLaunchKernelGGL(score_kernel(lds, mode), g, dim3(ACQ_TILE), scan_lds_bytes(R, m, lds), s, ccodes, W, cpad, n, wvec, Minv, tab, R,
                       noise, scale, m, bc, info, yp, first, acc, astride, fpart, tiles, tile0);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int score_forests(const double *fpart, int tiles, int bc, double *rows, hipStream_t s) {
    hipLaunchKernelGGL(score_forests_kernel, dim3((unsigned)((2 * bc + 63) / 64)), dim3(64), 0, s, fpart, tiles, bc, rows);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int score_finish(const double *acc, int64_t C, int B, const double *yp, double *values_out, double *mpart, const int32_t *info,
                 double *per_forest_out, double *mixture_out, hipStream_t s) {
    const int tiles = (int)acq_partials(C);
    hipLaunchKernelGGL(score_points_kernel, dim3((unsigned)tiles), dim3(ACQ_TILE), 0, s, acc, (long long)C, B, yp, values_out, mpart);
    BARK_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_final_kernel, dim3(1), dim3(64), 0, s, mpart, tiles, info, B, per_forest_out, mixture_out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace bark
