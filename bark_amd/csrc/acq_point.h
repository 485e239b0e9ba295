// The per-point part of the leaf-space kernels that run one thread per point over the forests of a chunk (acq_scan_kernel
// in acquire.hip, score_scan_kernel in scores.hip): the forest's table image into LDS, the point's leaf list, and the two
// leaf-space sums.  Both kernels form mu_b and var_b from these in the same order, so they agree bit for bit.
// LDS layout (dynamic, ACQ_TILE threads): with LDS_TABLE the forest's image ([tri + R] doubles: packed upper triangle of
// M^-1, then w; acq_pack) in front of the tile's leaf lists ([m][ACQ_TILE] 16-bit ids, lane fastest: conflict-free);
// otherwise only the lists, and M^-1 / w are read from global memory.
// acq_target_term, the utility of the target kinds, is here too: the scan (acquire.hip) and the fidelity gain (fidelity.hip)
// call the one function, so a forest that sees query and target as one point gives the scan's MES bits.
#pragma once
#include "common.h"

namespace bark {

// the image of forest b of the chunk into LDS; the caller's barriers separate it from the reads before and after
__device__ __forceinline__ void stage_table(const double *__restrict__ tab, int b, int tri, int R, double *smem) {
    const double *src = tab + (size_t)b * (tri + R);
    for (int e = threadIdx.x; e < tri + R; e += ACQ_TILE) smem[e] = src[e];
}

// Leaves of point c under forest b from its one-hot code (ccodes (bc, W, cpad)), in code-bit order (tree order), into
// idx[k * STRIDE]; returns their number, which the caller clamps to m (only the first m are stored).  STRIDE: the lists of
// the workgroup side by side, ACQ_TILE for the one-thread-per-point kernels; covariance.hip holds two shorter sets of lists.
template <int STRIDE = ACQ_TILE>
__device__ __forceinline__ int point_leaves(const uint32_t *__restrict__ ccodes, int W, int cpad, int b, int c, int m, int R,
                                            unsigned short *idx) {
    int cnt = 0;
    for (int w0 = 0; w0 < W; w0 += 8) {
        uint32_t word[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) word[u] = w0 + u < W ? ccodes[((size_t)b * W + w0 + u) * cpad + c] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            uint32_t bits = word[u];
            while (bits) {  // bits in increasing order: tree order
                const int a = 32 * (w0 + u) + __builtin_ctz(bits);
                if (cnt < m) idx[cnt * STRIDE] = (unsigned short)(a < R ? a : R - 1);
                bits &= bits - 1;
                ++cnt;
            }
        }
    }
    return cnt;
}

// s1 = sum_i w[a_i], dg = sum_i Minv[a_i][a_i], off = sum_i ( sum_{j < i} Minv[a_j][a_i] ) over the point's cnt leaves.  A
// wave's 64 points walk the tree pairs (j, i) in lock step, so their table reads fall into the leaves(tree j) x leaves(tree i)
// block of M^-1: for prior-sized trees a handful of distinct addresses, which the LDS broadcasts.
template <bool LDS_TABLE>
__device__ __forceinline__ void point_sums(const unsigned short *idx, int cnt, const double *smem, const double *wb,
                                           const double *Mb, int R, double &s1, double &dg, double &off) {
    s1 = 0.0, dg = 0.0, off = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const int ai = idx[i * ACQ_TILE];
        s1 += wb[ai];
        dg += LDS_TABLE ? smem[ai * (2 * R - ai - 1) / 2 + ai] : Mb[(size_t)ai * R + ai];
        double r = 0.0;
#pragma unroll 4
        for (int j = 0; j < i; ++j) {
            const int aj = idx[j * ACQ_TILE];
            r += LDS_TABLE ? smem[aj * (2 * R - aj - 1) / 2 + ai] : Mb[(size_t)aj * R + ai];
        }
        off += r;
    }
}

// sum over the workgroup's 256 threads of two values each, the same tree whatever the values: xor butterfly within a wave
// (every lane ends with the wave's sum), then waves 0 .. 3 in order by thread 0, which alone holds the result.
// red: 8 doubles in LDS that no thread touches between the caller's barrier before this call and its next one after it.
// The score kernels (scores.hip) and the predict kernels (predict.hip) sum their tiles with this one tree.
__device__ __forceinline__ void tile_sum2(double &u, double &v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        u += __shfl_xor(u, o);
        v += __shfl_xor(v, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = u;
        red[4 + wave] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u = ((red[0] + red[1]) + red[2]) + red[3];
        v = ((red[4] + red[5]) + red[6]) + red[7];
    }
}

// Utility of the target kinds (include/bark_hip.h) for one candidate and forest: -(1/S) sum_s g(mu, sd, t_s), s = 0 .. S-1.
// What does not depend on the target is formed once: the reciprocal of the standard deviation and, for MES, log(sd E).
// `t` is the same address in every lane (the forest's row of `targets`), so the loads are scalar.
constexpr double ACQ_SQRT1_2 = 0.70710678118654752440;      // 1 / sqrt(2)
constexpr double ACQ_INV_SQRT_2PI = 0.39894228040143267794;  // 1 / sqrt(2 pi)
constexpr double ACQ_SQRT_2PI_E = 4.13273135412249293847;    // sqrt(2 pi e)

template <int KIND>
__device__ __forceinline__ double acq_target_term(double mu, double var, const double *__restrict__ t, int S) {
    const double sd = sqrt(var > 0.0 ? var : 0.0);
    double gs = 0.0;
    if (KIND == BARK_ACQ_MES) {
        const double inv = 1.0 / (sd + 1e-7);
        const double h1 = log(sd * ACQ_SQRT_2PI_E);
        for (int s = 0; s < S; ++s) {
            const double gam = (t[s] - mu) * inv;
            const double cdf = 0.5 * erfc(-gam * ACQ_SQRT1_2);
            const double pdf = exp(-0.5 * (gam * gam)) * ACQ_INV_SQRT_2PI;
            double inner = ACQ_SQRT_2PI_E * sd * cdf;
            if (inner <= 0.0) inner = 1e-10;
            gs += h1 - (log(inner) - gam * pdf / (2.0 * cdf + 1e-10));
        }
    } else if (sd > 0.0) {
        const double inv = 1.0 / sd;
        for (int s = 0; s < S; ++s) {
            const double d = t[s] - mu;
            const double z = d * inv;
            const double cdf = 0.5 * erfc(-z * ACQ_SQRT1_2);
            if (KIND == BARK_ACQ_EI)
                gs += d * cdf + sd * (exp(-0.5 * (z * z)) * ACQ_INV_SQRT_2PI);
            else
                gs += cdf;
        }
    } else {  // a point mass at mu; a NaN target stays NaN
        for (int s = 0; s < S; ++s) {
            const double d = t[s] - mu;
            if (KIND == BARK_ACQ_EI)
                gs += d < 0.0 ? 0.0 : d;
            else
                gs += d > 0.0 ? 1.0 : (d <= 0.0 ? 0.0 : d);
        }
    }
    return -(gs / (double)S);
}

}  // namespace bark
