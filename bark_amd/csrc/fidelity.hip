// Information gain about the minimum of the target function from evaluating another point (contract and formulas in
// include/bark_hip.h, bark_fidelity_gain_fitted_hip): the reference's information_based_fidelity.py:90-167 in leaf space.
// The fidelity is an input column like any other, so the two points of a pair, query[c] (what would be evaluated) and
// target[c] (whose function's minimum the targets describe), differ in leaves only under the forests that split on it.
//
// Per chunk of forests, four launches:
//   fid_moments_kernel     one thread per candidate, the forests of the chunk in order: the leaf lists of both points, their
//                          means and variances with the scan's arithmetic (acq_point.h), the cross-covariance from the
//                          leaves(query) x leaves(target) block of M^-1 (global memory), and the two closed cases: sd_m == 0
//                          (-inf) and equal leaf lists (the scan's MES term, acq_target_term).  Everything else is a
//                          "separated" pair: its five moments go to `mom` for the quadrature.
//   fid_quadrature_kernel  one wave per (candidate, forest), the separated pairs only: Z_s into LDS, the support search over
//                          the n_a grid points and the G-point trapezoid, a grid point per lane and the S targets in the
//                          lane's loop.  phi and u(f) are formed once per grid point, the reciprocals once per pair; the
//                          targets are read through wave-uniform addresses, Z_s by LDS broadcast.
//   fid_accumulate_kernel  one thread per candidate: the chunk's values added in forest order to the running sum
//   fid_finish_kernel      after the last chunk: the division by B (equal weights), NaN where a forest failed
// Order (part of the contract): cov sums i outer, j inner into one accumulator; the sum over the targets runs s = 0 .. S-1
// for every grid point; lane l takes the grid points l, l + 64, ... in that order; the 64 partial sums meet in a xor
// butterfly (offsets 32 .. 1), which gives every lane the same bits.  Nothing depends on the chunk: a pair's value is
// formed by one thread or one wave from the state alone, and the forests are added one by one.
// Neither kernel asks for more than 64 KiB of dynamic LDS (two leaf lists at 64 trees are exactly 64 KiB; S <= 1024 targets
// are 8 KiB), so this unit registers nothing with raise_lds_limits (common.h).
#include "acq_point.h"

namespace bark {
namespace {

constexpr int FID_WAVE = 64;

__device__ __forceinline__ double fid_Phi(double z) { return 0.5 * erfc(-z * ACQ_SQRT1_2); }

// mom (bc, FID_MOMENTS, n): mu_m, var_m, mu_0, var_0, cov, then 1.0 for a separated pair and 0.0 for one that is done.
// g (bc, n): the pair's value when it is done (NaN for a forest of weight 0: it takes no part).
// weights: the chunk's rows, or null.  No barrier: a thread past n leaves at once.
__global__ __launch_bounds__(ACQ_TILE) void fid_moments_kernel(const uint32_t *__restrict__ qcodes, const uint32_t *__restrict__ tcodes,
                                                               int W, int cpad, int n, const double *__restrict__ wvec,
                                                               const double *__restrict__ Minv, int R,
                                                               const double *__restrict__ noise, const double *__restrict__ scale,
                                                               int m, int bc, const double *__restrict__ targets, int S,
                                                               const double *__restrict__ weights, double *__restrict__ mom,
                                                               double *__restrict__ g) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * ACQ_TILE + tid;
    if (c >= n) return;
    unsigned short *qi = reinterpret_cast<unsigned short *>(smem) + tid;
    unsigned short *ti = qi + (size_t)m * ACQ_TILE;
    for (int b = 0; b < bc; ++b) {
        double *mb = mom + (size_t)b * FID_MOMENTS * n;
        double *gb = g + (size_t)b * n;
        if (weights && weights[b] == 0.0) {  // uniform over the grid
            gb[c] = NAN;
            mb[(size_t)5 * n + c] = 0.0;
            continue;
        }
        int cq = point_leaves(qcodes, W, cpad, b, c, m, R, qi);
        if (cq > m) cq = m;
        int ct = point_leaves(tcodes, W, cpad, b, c, m, R, ti);
        if (ct > m) ct = m;
        const double *wb = wvec + (size_t)b * R;
        const double *Mb = Minv + (size_t)b * R * R;
        const double sigma2 = 1e-6 + noise[b];
        const double sc = scale[b];
        double s1, dg, off;
        point_sums<false>(qi, cq, smem, wb, Mb, R, s1, dg, off);
        const double mu_m = sc / ((double)m * sigma2) * s1;
        const double var_m = sc / (double)m * (dg + 2.0 * off);
        bool same = cq == ct;
        for (int i = 0; same && i < cq; ++i) same = qi[i * ACQ_TILE] == ti[i * ACQ_TILE];
        double flag = 0.0, val;
        if (!(var_m > 0.0)) {
            val = -INFINITY;
        } else if (same) {
            val = -acq_target_term<BARK_ACQ_MES>(mu_m, var_m, targets + (size_t)b * S, S);
        } else {
            point_sums<false>(ti, ct, smem, wb, Mb, R, s1, dg, off);
            double cs = 0.0;
            for (int i = 0; i < cq; ++i) {
                const double *row = Mb + (size_t)qi[i * ACQ_TILE] * R;
                for (int j = 0; j < ct; ++j) cs += row[ti[j * ACQ_TILE]];
            }
            mb[c] = mu_m;
            mb[(size_t)n + c] = var_m;
            mb[(size_t)2 * n + c] = sc / ((double)m * sigma2) * s1;
            mb[(size_t)3 * n + c] = sc / (double)m * (dg + 2.0 * off);
            mb[(size_t)4 * n + c] = sc / (double)m * cs;
            flag = 1.0;
            val = NAN;  // the quadrature writes it
        }
        mb[(size_t)5 * n + c] = flag;
        gb[c] = val;
    }
}

// what a grid point f contributes beside the targets: u(f) and phi((f - mu_m) / (sd_m + 1e-9))
struct FidPair {
    double mu_m, mu_0, cov, vden, inv_m, inv_s;
    __device__ __forceinline__ void at(double f, double &u, double &p) const {
        const double d = f - mu_m;
        u = mu_0 + cov * d / vden;
        const double z = d * inv_m;
        p = exp(-0.5 * (z * z)) * ACQ_INV_SQRT_2PI;
    }
};

// grid (n, bc), one wave each; dynamic LDS: S doubles (Z_s).  targets: the chunk's rows (bc, S).
__global__ __launch_bounds__(FID_WAVE) void fid_quadrature_kernel(const double *__restrict__ mom, int n,
                                                                  const double *__restrict__ targets, int S, double lo, double hi,
                                                                  int n_a, double pad, int G, double *__restrict__ g) {
    extern __shared__ double zs[];
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const double *mb = mom + (size_t)b * FID_MOMENTS * n;
    if (mb[(size_t)5 * n + c] == 0.0) return;  // the whole wave
    const double var_m = mb[(size_t)n + c], var_0 = mb[(size_t)3 * n + c];
    FidPair q;
    q.mu_m = mb[c], q.mu_0 = mb[(size_t)2 * n + c], q.cov = mb[(size_t)4 * n + c];
    const double *__restrict__ t = targets + (size_t)b * S;
    const double sd_m = sqrt(var_m > 0.0 ? var_m : 0.0), sd_0 = sqrt(var_0 > 0.0 ? var_0 : 0.0);
    q.vden = var_m + 1e-9;
    const double s2 = var_0 - q.cov * q.cov / q.vden;
    q.inv_s = 1.0 / (sqrt(s2 > 0.0 ? s2 : 0.0) + 1e-9);
    q.inv_m = 1.0 / (sd_m + 1e-9);
    const double inv_0 = 1.0 / (sd_0 + 1e-9);
    for (int s = lane; s < S; s += FID_WAVE) zs[s] = 1.0 / (fid_Phi((t[s] - q.mu_0) * inv_0) * sd_m + 1e-10);
    __syncthreads();

    // support: the live points of the n_a grid
    const double step = (hi - lo) / (double)(n_a - 1);
    int kmin = 0x7fffffff, kmax = -1;
    for (int k = lane; k < n_a; k += FID_WAVE) {
        double u, p;
        q.at(lo + (double)k * step, u, p);
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += fabs(fid_Phi((t[s] - u) * q.inv_s) * p);
        if (sum > 1e-8) {
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(kmin, o), z = __shfl_xor(kmax, o);
        kmin = a < kmin ? a : kmin;
        kmax = z > kmax ? z : kmax;
    }
    double *out = g + (size_t)b * n + c;
    if (kmax < 0) {  // no live point: the reference would raise
        if (lane == 0) *out = NAN;
        return;
    }
    const double fmin = (lo + (double)kmin * step) - pad, fmax = (lo + (double)kmax * step) + pad;

    // trapezoid of sum_s xlogy(Z_s Psi_s, Z_s Psi_s) over the G points
    const double h = (fmax - fmin) / (double)(G - 1);
    double acc = 0.0;
    for (int j = lane; j < G; j += FID_WAVE) {
        double u, p;
        q.at(fmin + (double)j * h, u, p);
        double col = 0.0;
        for (int s = 0; s < S; ++s) {
            const double z = zs[s] * (fid_Phi((t[s] - u) * q.inv_s) * p);
            col += z == 0.0 ? 0.0 : z * log(z);
        }
        acc += (j == 0 || j == G - 1) ? 0.5 * col : col;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        const double h2 = -(acc * h / (double)S);
        *out = log(sd_m * ACQ_SQRT_2PI_E) - h2;
    }
}

// acc[c] (+)= sum over the chunk's forests, in order, of g[b][c] (times weights[b]; weight 0 skipped)
__global__ __launch_bounds__(256) void fid_accumulate_kernel(const double *__restrict__ g, int n, int bc,
                                                             const double *__restrict__ weights, int first, double *__restrict__ acc) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double a = first ? 0.0 : acc[c];
    for (int b = 0; b < bc; ++b) {
        const double v = g[(size_t)b * n + c];
        if (weights) {
            const double wt = weights[b];
            if (wt == 0.0) continue;
            a += wt * v;
        } else {
            a += v;
        }
    }
    acc[c] = a;
}

// gain_out from the sums; a failed forest (info != 0) of non-zero weight makes every gain NaN, and the rows of failed
// forests in per_forest_out (B, C) NaN
__global__ __launch_bounds__(256) void fid_finish_kernel(const double *__restrict__ acc, int C, int B, const double *__restrict__ weights,
                                                         const int32_t *__restrict__ info, double *__restrict__ gain_out,
                                                         double *__restrict__ per_forest_out) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int b = threadIdx.x; b < B; b += 256) mine |= info[b] != 0 && (!weights || weights[b] != 0.0);
    if (mine) bad = 1;  // every writer stores the same value
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    gain_out[c] = bad ? NAN : (weights ? acc[c] : acc[c] / (double)B);
    if (per_forest_out)
        for (int b = 0; b < B; ++b)
            if (info[b] != 0) per_forest_out[(size_t)b * C + c] = NAN;
}

}  // namespace

size_t fidelity_moments_lds_bytes(int64_t m) { return (size_t)2 * m * ACQ_TILE * sizeof(unsigned short); }

int fidelity_moments(const uint32_t *qcodes, const uint32_t *tcodes, int W, int cpad, int n, const double *wvec, const double *Minv,
                     int R, const double *noise, const double *scale, int m, int bc, const double *targets, int S,
                     const double *weights, double *mom, double *g, hipStream_t s) {
    hipLaunchKernelGGL(fid_moments_kernel, dim3((unsigned)((n + ACQ_TILE - 1) / ACQ_TILE)), dim3(ACQ_TILE), fidelity_moments_lds_bytes(m),
                       s, qcodes, tcodes, W, cpad, n, wvec, Minv, R, noise, scale, m, bc, targets, S, weights, mom, g);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int fidelity_quadrature(const double *mom, int n, int bc, const double *targets, int S, double lo, double hi, int n_a, double pad,
                        int G, double *g, hipStream_t s) {
    hipLaunchKernelGGL(fid_quadrature_kernel, dim3((unsigned)n, (unsigned)bc), dim3(FID_WAVE), (size_t)S * sizeof(double), s, mom, n,
                       targets, S, lo, hi, n_a, pad, G, g);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int fidelity_accumulate(const double *g, int n, int bc, const double *weights, int first, double *acc, hipStream_t s) {
    hipLaunchKernelGGL(fid_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, n, bc, weights, first, acc);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int fidelity_finish(const double *acc, int C, int B, const double *weights, const int32_t *info, double *gain_out,
                    double *per_forest_out, hipStream_t s) {
    hipLaunchKernelGGL(fid_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, acc, C, B, weights, info, gain_out,
                       per_forest_out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace bark
