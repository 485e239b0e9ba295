// Acquisition scan over candidates in leaf space (contract in include/bark_hip.h): the lower confidence bound of the forest
// samples' posteriors, reduced over the forests and minimised over the candidates without a (B, C) intermediate.
//
// Per forest b (leaf-space quantities of leafspace.hip: w = M^-1 Z'y, M^-1, c = scale / (m s2)) and candidate x with the
// leaves L(x) = a_0 < a_1 < ... (bits of its one-hot code, i.e. tree order):
//     mu_b(x)  = c_b * sum_i w_b[a_i]
//     var_b(x) = (scale_b / m) * ( sum_i Minv[a_i][a_i] + 2 * sum_i ( sum_{j < i} Minv[a_j][a_i] ) )
// Only the upper triangle of M^-1 is read, m (m + 1) / 2 entries instead of leaf_predict_kernel's m^2.  The kernels:
//   acq_condition_kernel  optional: M^-1 conditioned on the pending points (rank-one downdates), before anything reads it
//   acq_condition_from_kernel  the same out of place, for the scan from a fitted state (the state is only read)
//   acq_observe_kernel    a fitted state's M^-1 and w conditioned in place on points with observed or fantasised values
//   acq_pack_kernel     upper triangle of M^-1, rows packed, followed by w: the image acq_scan_kernel stages in LDS
//   acq_scan_kernel     one thread per candidate; the forests of the chunk in order, three running sums per candidate in
//                       registers (sum of mu - kappa sd, of mu, of var + mu^2), kept in a (3, C) buffer between chunks
//                       the target kinds (EI, PI, MES) instead keep one sum, of -(1/S) sum_s g(mu, sd, t_{b,s}), the
//                       S targets of the forest read through wave-uniform addresses
//                       with importance weights (the scan from a fitted state only) each forest's terms are multiplied by
//                       its normalised weight and a forest of weight 0 is skipped: instantiations of their own
//   acq_finish_kernel   the acquisition value per candidate and per-workgroup (value, lowest index) minima;
//   acq_best_kernel     reduces those (no float atomics: ties go to the lowest candidate index)
// The order of every sum is fixed (leaves in code-bit order, targets 0 .. S-1, forests 0 .. B-1), so the result depends neither on the chunk
// nor on the variant: the LDS and the global variant of acq_scan_kernel run the same arithmetic on the same values.
#include "acq_point.h"
#include "philox.h"

namespace bark {
namespace {

constexpr int ACQ_COND_THREADS = 1024;         // acq_condition_kernel: one workgroup per forest
constexpr uint32_t OBSERVE_KEY = 0x66616E74u;  // "fant": keeps the fantasies apart from every other stream of the same seed

// Image (bc, tri + R): row a of the upper triangle of M^-1 at a (2R - a - 1) / 2 + a, i.e. entry (a, b >= a) at
// a (2R - a - 1) / 2 + b; then w.
__global__ __launch_bounds__(256) void acq_pack_kernel(const double *__restrict__ Minv, const double *__restrict__ w, int R,
                                                       double *__restrict__ tab) {
    const int a = blockIdx.x, b = blockIdx.y;
    const size_t tri = (size_t)R * (R + 1) / 2;
    double *dst = tab + (size_t)b * (tri + R);
    const double *row = Minv + ((size_t)b * R + a) * R;
    const int base = a * (2 * R - a - 1) / 2;
    for (int c = a + threadIdx.x; c < R; c += 256) dst[base + c] = row[c];
    if (a == 0)
        for (int c = threadIdx.x; c < R; c += 256) dst[tri + c] = w[(size_t)b * R + c];
}

// Conditioning on P pending points ("kriging believer": the fantasised observation at a pending point x* is the forest's own
// posterior mean there, so w does not change and only M^-1 does).  With z the one-hot row of x* (leaves a_0 < a_1 < ... in
// code-bit order) and c = scale / (m s2), per point, in the order given, each update seeing the previous one:
//     t = M^-1 z   (t_i = sum_k Minv[i][a_k], k in code-bit order),   q = z't = sum_k t[a_k]   (one wave, a fixed butterfly)
//     Minv[i][j] -= g (t_i t_j),   g = c / (1 + c q)
// over the full matrix; (i, j) and (j, i) subtract the same product, so a symmetric M^-1 stays symmetric in bits.  One
// workgroup per forest of the chunk: nothing crosses workgroups, every hand-over is a workgroup barrier (which also orders the
// workgroup's global stores before its later loads).  Forests whose sweep failed (info != 0) are left alone.
// LDS (8-byte items only): t [R], q, then the point's leaf list [ACQ_MAX_TREES] and its length.
__global__ __launch_bounds__(ACQ_COND_THREADS) void acq_condition_kernel(const uint32_t *__restrict__ pcodes, int W, int ppad,
                                                                         int P, double *Minv, int R,
                                                                         const double *__restrict__ noise,
                                                                         const double *__restrict__ scale, int m,
                                                                         const int32_t *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    if (info[b] != 0) return;  // the whole workgroup: no barrier is left waiting
    double *t = smem;
    double *qs = smem + R;
    int *leaves = reinterpret_cast<int *>(smem + R + 1);
    int *count = leaves + ACQ_MAX_TREES;
    double *Mb = Minv + (size_t)b * R * R;
    const double c = scale[b] / ((double)m * (1e-6 + noise[b]));
    for (int p = 0; p < P; ++p) {
        if (tid == 0) {
            int cnt = 0;
            for (int w0 = 0; w0 < W; ++w0) {
                uint32_t bits = pcodes[((size_t)b * W + w0) * ppad + p];
                while (bits) {  // bits in increasing order: tree order
                    const int a = 32 * w0 + __builtin_ctz(bits);
                    if (cnt < ACQ_MAX_TREES && a < R) leaves[cnt++] = a;
                    bits &= bits - 1;
                }
            }
            *count = cnt;
        }
        __syncthreads();
        const int cnt = *count;
        for (int i = tid; i < R; i += ACQ_COND_THREADS) {
            const double *row = Mb + (size_t)i * R;
            double s = 0.0;
            for (int k = 0; k < cnt; ++k) s += row[leaves[k]];
            t[i] = s;
        }
        __syncthreads();
        if (wave == 0) {
            double v = lane < cnt ? t[leaves[lane]] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) *qs = v;
        }
        __syncthreads();
        const double g = c / (1.0 + c * *qs);
        for (int i = wave; i < R; i += ACQ_COND_THREADS / 64) {
            const double ti = t[i];
            double *row = Mb + (size_t)i * R;
            for (int j = lane; j < R; j += 64) row[j] -= g * (ti * t[j]);
        }
        __syncthreads();  // the next point reads the updated matrix and reuses t and the leaf list
    }
}

// The same conditioning out of place, for a scan that starts from a fitted state it must not modify (fitted.hip,
// bark_acquisition_scan_fitted_hip): the first point reads `src` (the state's M^-1) and writes `dst` (scratch of the call),
// the later points run in place on `dst`.  P >= 1.  Every product, sum and their order are acq_condition_kernel's, so `dst`
// ends with the bits that kernel leaves in a matrix that started as `src`.  A forest whose sweep failed is copied as it is:
// the scan still reads it (its result is NaN / -1 through acq_best_kernel).  Same LDS layout; src and dst do not overlap.
__global__ __launch_bounds__(ACQ_COND_THREADS) void acq_condition_from_kernel(const uint32_t *__restrict__ pcodes, int W, int ppad,
                                                                              int P, const double *src, double *dst, int R,
                                                                              const double *__restrict__ noise,
                                                                              const double *__restrict__ scale, int m,
                                                                              const int32_t *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const double *Sb = src + (size_t)b * R * R;
    double *Db = dst + (size_t)b * R * R;
    if (info[b] != 0) {  // the whole workgroup: no barrier is left waiting
        for (size_t e = tid; e < (size_t)R * R; e += ACQ_COND_THREADS) Db[e] = Sb[e];
        return;
    }
    double *t = smem;
    double *qs = smem + R;
    int *leaves = reinterpret_cast<int *>(smem + R + 1);
    int *count = leaves + ACQ_MAX_TREES;
    const double c = scale[b] / ((double)m * (1e-6 + noise[b]));
    for (int p = 0; p < P; ++p) {
        const double *Mb = p == 0 ? Sb : Db;  // what this point reads; it writes Db
        if (tid == 0) {
            int cnt = 0;
            for (int w0 = 0; w0 < W; ++w0) {
                uint32_t bits = pcodes[((size_t)b * W + w0) * ppad + p];
                while (bits) {  // bits in increasing order: tree order
                    const int a = 32 * w0 + __builtin_ctz(bits);
                    if (cnt < ACQ_MAX_TREES && a < R) leaves[cnt++] = a;
                    bits &= bits - 1;
                }
            }
            *count = cnt;
        }
        __syncthreads();
        const int cnt = *count;
        for (int i = tid; i < R; i += ACQ_COND_THREADS) {
            const double *row = Mb + (size_t)i * R;
            double s = 0.0;
            for (int k = 0; k < cnt; ++k) s += row[leaves[k]];
            t[i] = s;
        }
        __syncthreads();
        if (wave == 0) {
            double v = lane < cnt ? t[leaves[lane]] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) *qs = v;
        }
        __syncthreads();
        const double g = c / (1.0 + c * *qs);
        for (int i = wave; i < R; i += ACQ_COND_THREADS / 64) {
            const double ti = t[i];
            const double *in = Mb + (size_t)i * R;
            double *out = Db + (size_t)i * R;
            for (int j = lane; j < R; j += 64) out[j] = in[j] - g * (ti * t[j]);
        }
        __syncthreads();  // the next point reads the updated matrix and reuses t and the leaf list
    }
}

// Conditioning on P points with values: the state's M^-1 AND w, in place (include/bark_hip.h, bark_leaf_posterior_observe_hip).
// Per point, in the order given, with t, q, g and the rewrite of M^-1 exactly as in acq_condition_kernel (the same products
// and sums in the same order, so M^-1 ends with the bits that kernel leaves), and on top of them, by lane 0 of wave 0 in the
// phase of the butterfly:
//     s = sum_k w[a_k]  (k in code-bit order from 0.0: acq_scan_kernel's order),   mu = c s,   v = (scale / m) q + s2
//     y* = values[b value_stride + p]   or   mu + sqrt(v) eps,   eps = eps[b P + p] or a Philox normal (below)
//     logpred += -1/2 ( log v + (y* - mu)^2 / v ),     d = (y* - mu) / (1 + c q)
// and by the whole workgroup, in the phase that rewrites M^-1:  w[i] += t[i] d.
// Hand-overs: s is read from w between the barrier that publishes t and the one that publishes q and d, i.e. before this
// point's rewrite of w and after the barrier that closes the previous point's; w and M^-1 are rewritten from t (LDS), which
// nobody writes in that phase.  Every hand-over is a workgroup barrier, as in acq_condition_kernel, and nothing crosses
// workgroups.  The Philox normal of (forest, draw, p): key (k0, k1) = (seed low word, seed high word ^ "fant"), counter
// (b0 + b, draw, p / 2, 0), Box-Muller as paths_normals_kernel (paths.hip): even p takes r cos th, odd p takes r sin th.
// Forests whose sweep failed (info != 0) are left alone; their rows of values_out / logpred_out are NaN.
// LDS (8-byte items only): t [R], q, s, d, logpred, then the point's leaf list [ACQ_MAX_TREES] and its length.
__global__ __launch_bounds__(ACQ_COND_THREADS) void acq_observe_kernel(const uint32_t *__restrict__ pcodes, int W, int ppad, int P,
                                                                       double *Minv, double *wvec, int R,
                                                                       const double *__restrict__ noise,
                                                                       const double *__restrict__ scale, int m,
                                                                       const int32_t *__restrict__ info, int mode,
                                                                       const double *__restrict__ values, int value_stride,
                                                                       const double *__restrict__ eps, uint32_t k0, uint32_t k1,
                                                                       uint32_t b0, uint32_t draw, double *__restrict__ values_out,
                                                                       double *__restrict__ logpred_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    if (info[b] != 0) {  // the whole workgroup: no barrier is left waiting
        if (values_out)
            for (int p = tid; p < P; p += ACQ_COND_THREADS) values_out[(size_t)b * P + p] = NAN;
        if (logpred_out && tid == 0) logpred_out[b] = NAN;
        return;
    }
    double *t = smem;
    double *qs = smem + R;
    double *obs = smem + R + 1;  // s, d, logpred
    int *leaves = reinterpret_cast<int *>(smem + R + 4);
    int *count = leaves + ACQ_MAX_TREES;
    double *Mb = Minv + (size_t)b * R * R;
    double *wb = wvec + (size_t)b * R;
    const double s2 = 1e-6 + noise[b];
    const double c = scale[b] / ((double)m * s2);
    if (tid == 0) obs[2] = 0.0;  // read and written by this thread only
    for (int p = 0; p < P; ++p) {
        if (tid == 0) {
            int cnt = 0;
            for (int w0 = 0; w0 < W; ++w0) {
                uint32_t bits = pcodes[((size_t)b * W + w0) * ppad + p];
                while (bits) {  // bits in increasing order: tree order
                    const int a = 32 * w0 + __builtin_ctz(bits);
                    if (cnt < ACQ_MAX_TREES && a < R) leaves[cnt++] = a;
                    bits &= bits - 1;
                }
            }
            *count = cnt;
        }
        __syncthreads();
        const int cnt = *count;
        for (int i = tid; i < R; i += ACQ_COND_THREADS) {
            const double *row = Mb + (size_t)i * R;
            double s = 0.0;
            for (int k = 0; k < cnt; ++k) s += row[leaves[k]];
            t[i] = s;
        }
        __syncthreads();
        if (wave == 0) {
            double v = lane < cnt ? t[leaves[lane]] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) {
                *qs = v;
                double s = 0.0;
                for (int k = 0; k < cnt; ++k) s += wb[leaves[k]];  // w as the previous point left it
                const double mu = c * s;
                const double var = scale[b] / (double)m * v + s2;
                double ys;
                if (mode == BARK_OBSERVE_VALUES) {
                    ys = values[(size_t)b * value_stride + p];
                } else {
                    double e;
                    if (eps) {
                        e = eps[(size_t)b * P + p];
                    } else {
                        uint32_t x[4];
                        philox(k0, k1, b0 + (uint32_t)b, draw, (uint32_t)(p >> 1), 0u, x);
                        const double u1 = uniform53(x[0], x[1]), u2 = uniform53(x[2], x[3]);
                        const double r = sqrt(-2.0 * log(1.0 - u1)), th = 6.283185307179586 * u2;
                        e = (p & 1) ? r * sin(th) : r * cos(th);
                    }
                    ys = mu + sqrt(var) * e;
                }
                const double dy = ys - mu;
                obs[0] = s;
                obs[1] = dy / (1.0 + c * v);
                obs[2] += -0.5 * (log(var) + dy * dy / var);
                if (values_out) values_out[(size_t)b * P + p] = ys;
            }
        }
        __syncthreads();
        const double g = c / (1.0 + c * *qs);
        const double dw = obs[1];
        for (int i = tid; i < R; i += ACQ_COND_THREADS) wb[i] += t[i] * dw;
        for (int i = wave; i < R; i += ACQ_COND_THREADS / 64) {
            const double ti = t[i];
            double *row = Mb + (size_t)i * R;
            for (int j = lane; j < R; j += 64) row[j] -= g * (ti * t[j]);
        }
        __syncthreads();  // the next point reads the updated matrix and w, and reuses t, the leaf list and q, s, d
    }
    if (tid == 0 && logpred_out) logpred_out[b] = obs[2];
}

// LDS_TABLE: the forest's image sits in LDS in front of the tile's leaf lists; otherwise only the lists do and M^-1 / w are
// read from global memory (acq_point.h has the layout and the per-candidate steps).
// n: candidates of this slab (ccodes (bc, W, cpad) holds their codes), acc: the slab's part of the (3, C) sums, row stride
// `astride`; first: this is the first chunk of forests (the sums start at zero).
// KIND: BARK_ACQ_LCB_MEAN for both confidence bounds (three sums; kappa), or a target kind (row 0 of acc only; targets (bc, S)).
// WEIGHTED: every term of forest b enters its sum multiplied by weights[b] (the chunk's rows of the caller's normalised
// importance weights; one address per forest, the same in all lanes, so it loads like noise[b]), and a forest whose weight is
// exactly 0 is skipped whole.  Without it `weights` is not read and the code is the equal-weight scan, unchanged.
template <bool LDS_TABLE, int KIND, bool WEIGHTED>
__global__ __launch_bounds__(ACQ_TILE) void acq_scan_kernel(const uint32_t *__restrict__ ccodes, int W, int cpad, int n,
                                                            const double *__restrict__ wvec, const double *__restrict__ Minv,
                                                            const double *__restrict__ tab, int R,
                                                            const double *__restrict__ noise, const double *__restrict__ scale,
                                                            int m, int bc, double kappa, const double *__restrict__ targets,
                                                            int S, int first, double *__restrict__ acc, size_t astride,
                                                            const double *__restrict__ weights) {
    constexpr bool LCB = KIND == BARK_ACQ_LCB_MEAN;
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * ACQ_TILE + tid;
    const bool active = c < n;
    const int tri = R * (R + 1) / 2;
    unsigned short *idx = reinterpret_cast<unsigned short *>(smem + (LDS_TABLE ? tri + R : 0)) + tid;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (active && !first) {
        a0 = acc[c];
        if (LCB) {
            a1 = acc[astride + c];
            a2 = acc[2 * astride + c];
        }
    }
    for (int b = 0; b < bc; ++b) {
        double wt = 1.0;
        if (WEIGHTED) {
            // b and weights[b] are uniform over the workgroup: every thread takes this branch together, so the two barriers
            // below are skipped by all of them or by none.  No table staging, no leaf lists, no arithmetic for the forest.
            wt = weights[b];
            if (wt == 0.0) continue;
        }
        if (LDS_TABLE) {
            __syncthreads();  // the previous forest's reads are done
            stage_table(tab, b, tri, R, smem);
        }
        int cnt = active ? point_leaves(ccodes, W, cpad, b, c, m, R, idx) : 0;
        if (cnt > m) cnt = m;
        if (LDS_TABLE) __syncthreads();
        if (!active) continue;  // no barrier depends on what follows
        double s1, dg, off;
        point_sums<LDS_TABLE>(idx, cnt, smem, LDS_TABLE ? smem + tri : wvec + (size_t)b * R, Minv + (size_t)b * R * R, R, s1, dg, off);
        const double sigma2 = 1e-6 + noise[b];
        const double sc = scale[b];
        const double mu = sc / ((double)m * sigma2) * s1;
        const double var = sc / (double)m * (dg + 2.0 * off);
        if (LCB) {
            const double t0 = mu - kappa * sqrt(var > 0.0 ? var : 0.0);
            const double t2 = var + mu * mu;
            a0 += WEIGHTED ? wt * t0 : t0;
            a1 += WEIGHTED ? wt * mu : mu;
            a2 += WEIGHTED ? wt * t2 : t2;
        } else {
            const double t0 = acq_target_term<KIND>(mu, var, targets + (size_t)b * S, S);
            a0 += WEIGHTED ? wt * t0 : t0;
        }
    }
    if (active) {
        acc[c] = a0;
        if (LCB) {
            acc[astride + c] = a1;
            acc[2 * astride + c] = a2;
        }
    }
}

// (value, index) minimum with ties to the lower index: associative and commutative, so any reduction tree gives the
// result of a scan in candidate order.  NaN never wins.
__device__ __forceinline__ void take_min(double &v, long long &i, double ov, long long oi) {
    if (ov < v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ void block_min(double &v, long long &i, double *rv, long long *ri) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(i, o);
        take_min(v, i, ov, oi);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        rv[wave] = v;
        ri[wave] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < 4; ++k) take_min(v, i, rv[k], ri[k]);
}

constexpr long long ACQ_NO_INDEX = 0x7fffffffffffffffLL;

// kind 0: mean over the forests of mu - kappa sd (the reference's calculate_acqf, tests/optimization/test_optimality.py);
// kind 1: the lower confidence bound of the moment-matched mixture (tree_gps.py:116-131);
// the target kinds: mean over the forests of the scan's one sum, like kind 0
// skip (n_skip entries): candidates that keep their value in acq_out but never win the minimum
// weighted: the sums already carry normalised weights (acq_scan_kernel<.., .., true>), so nothing is divided by B
__global__ __launch_bounds__(256) void acq_finish_kernel(const double *__restrict__ acc, long long C, int B, int weighted, double kappa,
                                                         int kind, const long long *__restrict__ skip, int n_skip,
                                                         double *__restrict__ acq_out, double *__restrict__ part_v,
                                                         long long *__restrict__ part_i) {
    __shared__ double rv[4];
    __shared__ long long ri[4];
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    double v = INFINITY;
    long long i = ACQ_NO_INDEX;
    if (c < C) {
        if (kind != BARK_ACQ_LCB_MIXTURE) {
            v = weighted ? acc[c] : acc[c] / (double)B;
        } else {
            const double mu = weighted ? acc[C + c] : acc[C + c] / (double)B;
            const double var = (weighted ? acc[2 * C + c] : acc[2 * C + c] / (double)B) - mu * mu;
            v = mu - kappa * sqrt(var > 0.0 ? var : 0.0);
        }
        if (acq_out) acq_out[c] = v;
        i = c;
        for (int k = 0; k < n_skip; ++k)
            if (skip[k] == c) {
                v = INFINITY;
                i = ACQ_NO_INDEX;
            }
    }
    block_min(v, i, rv, ri);
    if (threadIdx.x == 0) {
        part_v[blockIdx.x] = v;
        part_i[blockIdx.x] = i;
    }
}

// one workgroup: the minimum over the partials; NaN / -1 when a forest of the call failed (info != 0), no value is finite or
// every candidate was skipped.  weights (B,) or null: a forest of weight exactly 0 took no part in the scan, so its status is ignored
__global__ __launch_bounds__(256) void acq_best_kernel(const double *__restrict__ part_v, const long long *__restrict__ part_i,
                                                       int nblk, const int32_t *__restrict__ info, int B,
                                                       const double *__restrict__ weights, double *__restrict__ best,
                                                       long long *__restrict__ best_i) {
    __shared__ double rv[4];
    __shared__ long long ri[4];
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    double v = INFINITY;
    long long i = ACQ_NO_INDEX;
    for (int k = threadIdx.x; k < nblk; k += 256) take_min(v, i, part_v[k], part_i[k]);
    int mine = 0;
    for (int b = threadIdx.x; b < B; b += 256) mine |= info[b] != 0 && (!weights || weights[b] != 0.0);
    if (mine) bad = 1;  // every writer stores the same value
    block_min(v, i, rv, ri);
    if (threadIdx.x == 0) {
        const bool none = bad || i == ACQ_NO_INDEX;
        *best = none ? NAN : v;
        *best_i = none ? -1 : i;
    }
}

size_t acq_condition_lds_bytes(int64_t R) { return ((size_t)R + 1) * sizeof(double) + (ACQ_MAX_TREES + 2) * sizeof(int); }
size_t acq_observe_lds_bytes(int64_t R) { return acq_condition_lds_bytes(R) + 3 * sizeof(double); }

// the instantiation of a variant and kind; both confidence bounds share one (they differ in the finish only)
using ScanKernel = decltype(&acq_scan_kernel<true, BARK_ACQ_LCB_MEAN, false>);
template <bool WEIGHTED> ScanKernel scan_kernel_of(bool lds, int kind) {
    switch (kind) {
        case BARK_ACQ_EI: return lds ? acq_scan_kernel<true, BARK_ACQ_EI, WEIGHTED> : acq_scan_kernel<false, BARK_ACQ_EI, WEIGHTED>;
        case BARK_ACQ_PI: return lds ? acq_scan_kernel<true, BARK_ACQ_PI, WEIGHTED> : acq_scan_kernel<false, BARK_ACQ_PI, WEIGHTED>;
        case BARK_ACQ_MES: return lds ? acq_scan_kernel<true, BARK_ACQ_MES, WEIGHTED> : acq_scan_kernel<false, BARK_ACQ_MES, WEIGHTED>;
        default: return lds ? acq_scan_kernel<true, BARK_ACQ_LCB_MEAN, WEIGHTED> : acq_scan_kernel<false, BARK_ACQ_LCB_MEAN, WEIGHTED>;
    }
}
// the weighted scan has instantiations of its own, so the equal-weight ones keep their code
ScanKernel scan_kernel(bool lds, int kind, bool weighted = false) {
    return weighted ? scan_kernel_of<true>(lds, kind) : scan_kernel_of<false>(lds, kind);
}

// The kernels of this unit that can use more than 64 KiB of dynamic LDS: the LDS variant of the scan, every kind (up to a whole CU's),
// and acq_condition_kernel / acq_observe_kernel at the largest R the leaf-space path admits (8192: 264 / 288 bytes past
// 64 KiB).  acq_condition, acq_observe and acq_scan call this before they launch.
int raise_acq_lds_limits() {
    static const LdsLimit limits[] = {{reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_LCB_MEAN)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_EI)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_PI)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_MES)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_LCB_MEAN, true)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_EI, true)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_PI, true)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(scan_kernel(true, BARK_ACQ_MES, true)), ACQ_LDS_MAX},
                                      {reinterpret_cast<const void *>(acq_condition_kernel), acq_condition_lds_bytes(8192)},
                                      {reinterpret_cast<const void *>(acq_condition_from_kernel), acq_condition_lds_bytes(8192)},
                                      {reinterpret_cast<const void *>(acq_observe_kernel), acq_observe_lds_bytes(8192)}};
    static LdsLimitsOnce once;
    return raise_lds_limits(once, limits);
}

}  // namespace

int64_t acq_partials(int64_t C) { return (C + 255) / 256; }
size_t scan_lds_bytes(int64_t R, int64_t m, bool lds_table) {
    const size_t lists = (size_t)m * ACQ_TILE * sizeof(unsigned short);
    return (lds_table ? ((size_t)R * (R + 1) / 2 + R) * sizeof(double) : 0) + lists;
}
size_t acq_table_doubles(int64_t R) { return (size_t)R * (R + 1) / 2 + R; }

// M^-1 of the chunk's forests conditioned on the P pending points whose codes are pcodes (bc, W, ppad)
int acq_condition(const uint32_t *pcodes, int W, int ppad, int P, double *Minv, int R, const double *noise, const double *scale,
                  int m, int bc, const int32_t *info, hipStream_t s) {
    const int rc = raise_acq_lds_limits();
    if (rc) return rc;
    hipLaunchKernelGGL(acq_condition_kernel, dim3((unsigned)bc), dim3(ACQ_COND_THREADS), acq_condition_lds_bytes(R), s, pcodes, W,
                       ppad, P, Minv, R, noise, scale, m, info);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// ... out of place: dst = src conditioned on the P >= 1 points; src is only read
int acq_condition_from(const uint32_t *pcodes, int W, int ppad, int P, const double *src, double *dst, int R, const double *noise,
                       const double *scale, int m, int bc, const int32_t *info, hipStream_t s) {
    const int rc = raise_acq_lds_limits();
    if (rc) return rc;
    hipLaunchKernelGGL(acq_condition_from_kernel, dim3((unsigned)bc), dim3(ACQ_COND_THREADS), acq_condition_lds_bytes(R), s, pcodes,
                       W, ppad, P, src, dst, R, noise, scale, m, info);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// M^-1 and w of the chunk's forests conditioned on the P points with values (acq_observe_kernel); b0: the chunk's first forest
int acq_observe(const uint32_t *pcodes, int W, int ppad, int P, double *Minv, double *w, int R, const double *noise,
                const double *scale, int m, int bc, const int32_t *info, int mode, const double *values, int value_stride,
                const double *eps, uint64_t seed, int64_t b0, int64_t draw, double *values_out, double *logpred_out, hipStream_t s) {
    const int rc = raise_acq_lds_limits();
    if (rc) return rc;
    hipLaunchKernelGGL(acq_observe_kernel, dim3((unsigned)bc), dim3(ACQ_COND_THREADS), acq_observe_lds_bytes(R), s, pcodes, W, ppad, P,
                       Minv, w, R, noise, scale, m, info, mode, values, value_stride, eps, (uint32_t)seed,
                       (uint32_t)(seed >> 32) ^ OBSERVE_KEY, (uint32_t)b0, (uint32_t)draw, values_out, logpred_out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// image of the chunk for the LDS variant
int acq_pack(const double *Minv, const double *w, int R, int bc, double *tab, hipStream_t s) {
    hipLaunchKernelGGL(acq_pack_kernel, dim3((unsigned)R, (unsigned)bc), dim3(256), 0, s, Minv, w, R, tab);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// variant: 1 LDS, 2 global (resolved by bark_acquisition_plan); n candidates of one slab against the bc forests of the chunk.
// kind: BARK_ACQ_*; both confidence bounds run the same kernel, the target kinds read targets (bc, S).
// weights: the chunk's rows of the normalised forest weights (the weighted instantiation), or null (the equal-weight one).
int acq_scan(int variant, int kind, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
             const double *tab, int R, const double *noise, const double *scale, int m, int bc, double kappa, const double *targets,
             int S, int first, double *acc, size_t astride, const double *weights, hipStream_t s) {
    const dim3 g((unsigned)((n + ACQ_TILE - 1) / ACQ_TILE));
    const int rc = raise_acq_lds_limits();
    if (rc) return rc;
    const bool lds = variant == 1;
    const size_t bytes = scan_lds_bytes(R, m, lds);
    hipLaunchKernelGGL(scan_kernel(lds, kind, weights != nullptr), g, dim3(ACQ_TILE), bytes, s, ccodes, W, cpad, n, wvec, Minv, tab, R,
                       noise, scale, m, bc, kappa, targets, S, first, acc, astride, weights);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int acq_finish(const double *acc, int64_t C, int B, double kappa, int kind, const int64_t *skip, int n_skip, double *acq_out,
               double *part_v, int64_t *part_i, const int32_t *info, const double *weights, double *best, int64_t *best_i,
               hipStream_t s) {
    const int nblk = (int)acq_partials(C);
    hipLaunchKernelGGL(acq_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, s, acc, (long long)C, B, weights ? 1 : 0, kappa, kind,
                       reinterpret_cast<const long long *>(skip), n_skip, acq_out, part_v, reinterpret_cast<long long *>(part_i));
    BARK_LAUNCH_CHECK();
    hipLaunchKernelGGL(acq_best_kernel, dim3(1), dim3(256), 0, s, part_v, reinterpret_cast<const long long *>(part_i), nblk, info, B,
                       weights, best, reinterpret_cast<long long *>(best_i));
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace bark

extern "C" int bark_acquisition_plan(int64_t max_bits, int64_t m, int variant, int *variant_out, int64_t *lds_bytes_out) {
    using namespace bark;
    error_buffer()[0] = 0;
    if (variant_out) *variant_out = 0;
    if (lds_bytes_out) *lds_bytes_out = 0;
    if (max_bits < 1 || max_bits > 8192 || m < 1 || m > ACQ_MAX_TREES)
        return fail(BARK_ERR_ARG, "acquisition scan supports at most %d trees and 8192 leaves per forest (got m = %lld, R = %lld)",
                    ACQ_MAX_TREES, (long long)m, (long long)max_bits);
    if (variant < 0 || variant > 2) return fail(BARK_ERR_ARG, "acquisition scan: unknown variant %d", variant);
    const size_t need = scan_lds_bytes(max_bits, m, true);
    const bool fits = need <= ACQ_LDS_MAX;
    if (variant == 1 && !fits) {
        if (lds_bytes_out) *lds_bytes_out = (int64_t)need;
        return fail(BARK_ERR_ARG, "acquisition scan: the LDS variant needs %zu bytes for R = %lld, m = %lld (limit %zu)", need,
                    (long long)max_bits, (long long)m, ACQ_LDS_MAX);
    }
    const int v = variant ? variant : (fits ? 1 : 2);
    if (variant_out) *variant_out = v;
    if (lds_bytes_out) *lds_bytes_out = (int64_t)scan_lds_bytes(max_bits, m, v == 1);
    return BARK_OK;
}
