// Joint posterior covariance between points from a fitted posterior (contract in include/bark_hip.h,
// bark_leaf_posterior_covariance_hip): per forest the C1 x C2 block cov_b = (scale_b / m) Z_1 M_b^-1 Z_2', and the
// covariance of the weighted mixture of the forests by the law of total covariance.  predict.hip returns the diagonal of this
// block; the off-diagonal entries are one more bilinear form in the M^-1 of the state, formed here in two stages:
//   T_b[i][r]    = sum_k M_b^-1[a_k][r]   over the leaves a_k of x1[i]: m rows of M^-1 summed once per x1 point
//   cov_b[i][j]  = (scale_b / m) sum_l T_b[i][b_l]   over the leaves b_l of x2[j]: m gathers per entry
// The kernels:
//   cov_tile_kernel        one workgroup per (group of column tiles, row tile of COV_TI points, forest of the chunk).  LDS_T: the
//                          row tile's T (COV_TI x R doubles) is built once in LDS, from coalesced rows of M^-1, and every
//                          column tile of the group gathers from it; otherwise no T is kept and every T[i][b_l] an entry needs
//                          is summed from M^-1 in global memory, k in the same order, so both give the same bits.
//                          Lane = column j, wave = rows: a wave's 64 gathers of one step read one row of T at the leaves of
//                          one tree (lock step in l), neighbouring columns, so the banks differ whatever R is, and a tree of
//                          few leaves is a broadcast.  The symmetric call runs only the tiles that hold an entry with
//                          i >= j, and the thread of such an entry stores it at (i, j) and at (j, i).
//   cov_accumulate_kernel  one thread per entry: the chunk's forests of non-zero weight in order onto the running sum of the
//                          mixture, which lives in mixture_out between the chunks
//   cov_finish_kernel      the division by W; NaN under the flag
//   cov_mask_kernel        NaN into the blocks of forest_out whose forest has weight 0 or a non-zero status
// The means of the mixture and mu_b are predict_scan_kernel's (predict.hip), by its launcher: predict's bits.
// No float atomics; the order of every sum is fixed, so no result depends on the chunk, on the variant or on the grid.
#include "acq_point.h"

namespace bark {
namespace {

constexpr int COV_TI = 32, COV_TJ = 64;   // rows (x1) and columns (x2) of a workgroup's tile; 256 threads, 8 rows per thread
constexpr int COV_THREADS = 256;
constexpr int COV_LISTS = COV_TI + COV_TJ;  // leaf lists side by side: [m][COV_LISTS] 16-bit ids, the rows' first
constexpr int COV_GROUP = 8;               // column tiles that share a workgroup, and with it one T
constexpr size_t COV_LDS_DEFAULT = 64 * 1024;  // dynamic LDS a kernel may use without a raised limit

// dynamic LDS: with LDS_T the tile's T in front of the lists
size_t cov_lds_bytes(int64_t R, int64_t m, bool lds_t) {
    return (lds_t ? (size_t)COV_TI * R * sizeof(double) : 0) + (size_t)m * COV_LISTS * sizeof(unsigned short);
}

// codes1 (bc, W, cpad1) of the C1 row points, codes2 (bc, W, cpad2) of the C2 column points (symmetric: the same array);
// Minv (bc, R, R), noise / scale / weights (or null) the chunk's rows; out (bc, C1, C2).  grid (column groups, row tiles, bc).
template <bool LDS_T>
__global__ __launch_bounds__(COV_THREADS) void cov_tile_kernel(const uint32_t *__restrict__ codes1, int cpad1, int C1,
                                                               const uint32_t *__restrict__ codes2, int cpad2, int C2, int W,
                                                               const double *__restrict__ Minv, int R,
                                                               const double *__restrict__ noise, const double *__restrict__ scale,
                                                               int m, const double *__restrict__ weights, int symmetric,
                                                               int observation, double *__restrict__ out) {
    extern __shared__ double smem[];
    __shared__ int cnt_s[COV_LISTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z;
    if (weights && weights[b] == 0.0) return;  // uniform over the workgroup; cov_mask_kernel fills the block
    const int i0 = blockIdx.y * COV_TI;
    const int tiles_j = (C2 + COV_TJ - 1) / COV_TJ;
    // symmetric: the column tiles up to the one that holds the diagonal entry of the tile's last row
    const int last_j = symmetric ? (i0 + COV_TI - 1) / COV_TJ : tiles_j - 1;
    if ((int)blockIdx.x > last_j) return;
    double *T = smem;
    unsigned short *lists = reinterpret_cast<unsigned short *>(smem + (LDS_T ? (size_t)COV_TI * R : 0));
    const double *Mb = Minv + (size_t)b * R * R;

    if (tid < COV_TI) {
        const int i = i0 + tid;
        int cnt = i < C1 ? point_leaves<COV_LISTS>(codes1, W, cpad1, b, i, m, R, lists + tid) : 0;
        cnt_s[tid] = cnt > m ? m : cnt;
    }
    __syncthreads();
    if (LDS_T) {
        // wave w sums rows w, w + 4, ...: the leaf ids are uniform over the wave, the reads of M^-1 run along its rows
        for (int ii = wave; ii < COV_TI; ii += 4) {
            const int cnt = cnt_s[ii];
            for (int r = lane; r < R; r += 64) {
                double t = 0.0;
                for (int k = 0; k < cnt; ++k) t += Mb[(size_t)lists[k * COV_LISTS + ii] * R + r];
                T[(size_t)ii * R + r] = t;
            }
        }
    }
    const double sm = scale[b] / (double)m;
    const double s2 = 1e-6 + noise[b];
    double *ob = out + (size_t)b * C1 * C2;
    for (int tj = blockIdx.x; tj <= last_j && tj < tiles_j; tj += gridDim.x) {
        __syncthreads();  // T is written; the previous tile's column lists are read
        const int j0 = tj * COV_TJ;
        if (tid < COV_TJ) {
            const int j = j0 + tid;
            int cnt = j < C2 ? point_leaves<COV_LISTS>(codes2, W, cpad2, b, j, m, R, lists + COV_TI + tid) : 0;
            cnt_s[COV_TI + tid] = cnt > m ? m : cnt;
        }
        __syncthreads();
        const int cj = cnt_s[COV_TI + lane];
        double acc[COV_TI / 4];
#pragma unroll
        for (int q = 0; q < COV_TI / 4; ++q) acc[q] = 0.0;
        for (int l = 0; l < cj; ++l) {
            const int col = lists[l * COV_LISTS + COV_TI + lane];
#pragma unroll
            for (int q = 0; q < COV_TI / 4; ++q) {
                const int ii = wave + 4 * q;
                double t;
                if (LDS_T) {
                    t = T[(size_t)ii * R + col];
                } else {
                    const int cnt = cnt_s[ii];
                    t = 0.0;
                    for (int k = 0; k < cnt; ++k) t += Mb[(size_t)lists[k * COV_LISTS + ii] * R + col];
                }
                acc[q] += t;
            }
        }
        const int j = j0 + lane;
#pragma unroll
        for (int q = 0; q < COV_TI / 4; ++q) {
            const int i = i0 + wave + 4 * q;
            if (i >= C1 || j >= C2 || (symmetric && i < j)) continue;
            double v = sm * acc[q];
            if (observation && i == j) v += s2;
            ob[(size_t)i * C2 + j] = v;
            if (symmetric && i != j) ob[(size_t)j * C2 + i] = v;
        }
    }
}

// mix[e] (+)= sum over the chunk's forests b of non-zero weight, in order, of w_b (cov_b[e] + (mu1_b[i] - mean1[i]) (mu2_b[j] -
// mean2[j])), e = i C2 + j.  cov (bc, C1 C2), mu1 (bc, C1) / mu2 (bc, C2) the chunk's rows, mean1 / mean2 the recurrence's means.
__global__ __launch_bounds__(256) void cov_accumulate_kernel(const double *__restrict__ cov, long long C1, long long C2,
                                                             const double *__restrict__ mu1, const double *__restrict__ mean1,
                                                             const double *__restrict__ mu2, const double *__restrict__ mean2,
                                                             const double *__restrict__ weights, double wq, int bc, int first,
                                                             double *__restrict__ mix) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= C1 * C2) return;
    const long long i = e / C2, j = e - i * C2;
    const double mi = mean1[i], mj = mean2[j];
    double acc = first ? 0.0 : mix[e];
    for (int b = 0; b < bc; ++b) {
        const double wt = weights ? weights[b] : wq;
        if (wt == 0.0) continue;
        const double di = mu1[(size_t)b * C1 + i] - mi;
        const double dj = mu2[(size_t)b * C2 + j] - mj;
        acc += wt * (cov[(size_t)b * C1 * C2 + e] + di * dj);
    }
    mix[e] = acc;
}

// mix[e] / W, W the recurrence's sum of the weights (the same at every point); NaN under the flag
__global__ __launch_bounds__(256) void cov_finish_kernel(double *__restrict__ mix, long long n, const double *__restrict__ Wsum,
                                                         const int32_t *__restrict__ flag) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    mix[e] = *flag ? NAN : mix[e] / *Wsum;
}

// block b of fo (B, n) to NaN where the forest has weight 0 or a non-zero status; grid (tiles, up to 65535): block
// blockIdx.y and every gridDim.y-th after it
__global__ __launch_bounds__(256) void cov_mask_kernel(const int32_t *__restrict__ info, const double *__restrict__ weights, long long B,
                                                       long long n, double *__restrict__ fo) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    for (long long b = blockIdx.y; b < B; b += gridDim.y)
        if (info[b] != 0 || (weights && weights[b] == 0.0)) fo[b * n + e] = NAN;
}

}  // namespace

int cov_tiles(int variant, const uint32_t *codes1, int cpad1, int C1, const uint32_t *codes2, int cpad2, int C2, int W, const double *Minv,
              int R, const double *noise, const double *scale, int m, int bc, const double *weights, int symmetric, int observation,
              double *out, hipStream_t s) {
    const bool lds = variant == 1;
    const size_t bytes = cov_lds_bytes(R, m, lds);
    if (bytes > COV_LDS_DEFAULT) return fail(BARK_ERR_ARG, "covariance: the tile needs %zu bytes of LDS (limit %zu)", bytes, COV_LDS_DEFAULT);
    const int tiles_j = (C2 + COV_TJ - 1) / COV_TJ;
    const dim3 g((unsigned)((tiles_j + COV_GROUP - 1) / COV_GROUP), (unsigned)((C1 + COV_TI - 1) / COV_TI), (unsigned)bc);
    hipLaunchKernelGGL(lds ? cov_tile_kernel<true> : cov_tile_kernel<false>, g, dim3(COV_THREADS), bytes, s, codes1, cpad1, C1, codes2,
                       cpad2, C2, W, Minv, R, noise, scale, m, weights, symmetric, observation, out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int cov_accumulate(const double *cov, int64_t C1, int64_t C2, const double *mu1, const double *mean1, const double *mu2,
                   const double *mean2, const double *weights, double wq, int bc, int first, double *mix, hipStream_t s) {
    const long long n = (long long)C1 * C2;
    hipLaunchKernelGGL(cov_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cov, (long long)C1, (long long)C2, mu1,
                       mean1, mu2, mean2, weights, wq, bc, first, mix);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int cov_finish(double *mix, int64_t C1, int64_t C2, const double *Wsum, const int32_t *flag, const int32_t *info, const double *weights,
               int B, double *forest_out, hipStream_t s) {
    const long long n = (long long)C1 * C2;
    const unsigned tiles = (unsigned)((n + 255) / 256);
    if (mix) {
        hipLaunchKernelGGL(cov_finish_kernel, dim3(tiles), dim3(256), 0, s, mix, n, Wsum, flag);
        BARK_LAUNCH_CHECK();
    }
    if (forest_out) {
        hipLaunchKernelGGL(cov_mask_kernel, dim3(tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, s, info, weights, (long long)B, n,
                           forest_out);
        BARK_LAUNCH_CHECK();
    }
    return BARK_OK;
}

}  // namespace bark
