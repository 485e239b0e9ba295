// Importance weights of the forest samples of a fitted posterior (contract in include/bark_hip.h): the weight update
// (forest_weights_kernel, bark_forest_weights_hip) and the gather of state rows that a subset or a resampling copies
// (posterior_gather_kernel, bark_leaf_posterior_gather_hip; both states are laid out by posterior_state, leaf_state.h).
// Neither kernel uses an atomic: the update is one workgroup with plain loads, wave shuffles and one LDS stage; the gather
// writes every output element from exactly one thread.
#include <cmath>
#include <vector>

#include "common.h"

namespace bark {
namespace {

constexpr int WEIGHTS_THREADS = 256;  // forest_weights_kernel: one workgroup of four waves

// One value per workgroup from one per thread, in an order that depends on nothing but the thread index: the xor butterfly
// inside a wave (every lane ends with the wave's value), the four wave values through LDS, combined 0 .. 3 by every thread.
// The barrier in front lets a second call reuse `stage`.
template <class Op>
__device__ __forceinline__ double weights_reduce(double v, double *stage, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) stage[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = stage[0];
    for (int k = 1; k < WEIGHTS_THREADS / 64; ++k) r = op(r, stage[k]);
    return r;
}

// l_b = log_w[b] + increment[b] (either may be absent: 0), or -inf for a forest that is dead: info[b] != 0, an increment
// that is not finite, a log weight of -inf (or NaN, or +inf: no weight at all).
__device__ __forceinline__ double weights_term(const double *log_w, const double *inc, const int32_t *info, int b) {
    const double lw = log_w ? log_w[b] : 0.0;
    const double ic = inc ? inc[b] : 0.0;
    const bool dead = (info && info[b] != 0) || !isfinite(ic) || !isfinite(lw);
    return dead ? -INFINITY : lw + ic;
}

// M = max_b l_b;  S = sum_b exp(l_b - M);  log_w_out[b] = l_b - M - log S;  w_out[b] = exp(log_w_out[b]);
// stats = { M + log S (the log normaliser), 1 / sum_b w_b^2 (the effective sample size), max_b w_b }.
// Thread t owns forests t, t + 256, ... and adds them in that order; the per-thread values meet in weights_reduce.  Hence the
// order of every sum depends on B alone and two runs agree bit for bit.  No forest alive: stats[0] = -inf, all else NaN.
__global__ __launch_bounds__(WEIGHTS_THREADS) void forest_weights_kernel(const double *__restrict__ log_w_in,
                                                                         const double *__restrict__ increment,
                                                                         const int32_t *__restrict__ info, int B,
                                                                         double *__restrict__ log_w_out, double *__restrict__ w_out,
                                                                         double *__restrict__ stats) {
    __shared__ double stage[WEIGHTS_THREADS / 64];
    const int tid = threadIdx.x;
    auto fmax2 = [](double a, double b) { return a > b ? a : b; };
    auto add2 = [](double a, double b) { return a + b; };
    double mx = -INFINITY;
    for (int b = tid; b < B; b += WEIGHTS_THREADS) mx = fmax2(mx, weights_term(log_w_in, increment, info, b));
    mx = weights_reduce(mx, stage, fmax2);
    if (mx == -INFINITY) {  // the same value in every thread: the whole workgroup leaves, no barrier is left waiting
        for (int b = tid; b < B; b += WEIGHTS_THREADS) {
            log_w_out[b] = NAN;
            w_out[b] = NAN;
        }
        if (tid == 0) {
            stats[0] = -INFINITY;
            stats[1] = NAN;
            stats[2] = NAN;
        }
        return;
    }
    double sum = 0.0;
    for (int b = tid; b < B; b += WEIGHTS_THREADS) sum += exp(weights_term(log_w_in, increment, info, b) - mx);
    sum = weights_reduce(sum, stage, add2);
    const double lsum = log(sum);
    double sq = 0.0, top = 0.0;
    for (int b = tid; b < B; b += WEIGHTS_THREADS) {
        const double l = weights_term(log_w_in, increment, info, b) - mx - lsum;
        const double w = exp(l);
        log_w_out[b] = l;
        w_out[b] = w;
        sq += w * w;
        top = fmax2(top, w);
    }
    sq = weights_reduce(sq, stage, add2);
    top = weights_reduce(top, stage, fmax2);
    if (tid == 0) {
        stats[0] = mx + lsum;
        stats[1] = 1.0 / sq;
        stats[2] = top;
    }
}

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_TILE = 2 * GATHER_THREADS * 4;  // doubles of a matrix per workgroup: four 16-byte items per thread

// Row k of the output state from row index[k] of the input state: grid (tiles of a matrix, n).  A matrix is R^2 doubles at
// the byte offset 8 R^2 b of a 256-byte aligned area, so with R odd every other matrix starts 8 bytes off a 16-byte
// boundary.  When source and destination rows are both 16-byte aligned the pairs go as double2 and a last odd element alone;
// otherwise every element goes 8 bytes wide.  The workgroup of tile 0 also copies w (R doubles, 8 bytes wide: R^2 dwarfs it)
// and the status word.  index is range-checked by the caller; a thread never touches an element of another thread.
__global__ __launch_bounds__(GATHER_THREADS) void posterior_gather_kernel(const double *__restrict__ Min, const double *__restrict__ win,
                                                                          const int32_t *__restrict__ iin,
                                                                          const long long *__restrict__ index, int R,
                                                                          double *__restrict__ Mout, double *__restrict__ wout,
                                                                          int32_t *__restrict__ iout) {
    const int k = blockIdx.y, tid = threadIdx.x;
    const size_t b = (size_t)index[k], RR = (size_t)R * R;
    const double *src = Min + b * RR;
    double *dst = Mout + (size_t)k * RR;
    const size_t e0 = (size_t)blockIdx.x * GATHER_TILE;
    const size_t e1 = e0 + GATHER_TILE < RR ? e0 + GATHER_TILE : RR;  // e0 is even: a tile keeps the row's alignment
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const size_t pairs = (e1 - e0) / 2;
        const double2 *s2 = reinterpret_cast<const double2 *>(src + e0);
        double2 *d2 = reinterpret_cast<double2 *>(dst + e0);
        for (size_t p = tid; p < pairs; p += GATHER_THREADS) d2[p] = s2[p];
        if (tid == 0 && ((e1 - e0) & 1)) dst[e1 - 1] = src[e1 - 1];
    } else {
        for (size_t e = e0 + tid; e < e1; e += GATHER_THREADS) dst[e] = src[e];
    }
    if (blockIdx.x == 0) {
        for (int c = tid; c < R; c += GATHER_THREADS) wout[(size_t)k * R + c] = win[b * R + c];
        if (tid == 0) iout[k] = iin[b];
    }
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_forest_weights_hip(const double *log_w_in, const double *increment, const int32_t *info, int64_t B, double *log_w_out,
                            double *w_out, double *stats_out, void *stream) {
    static const char *name = "bark_forest_weights_hip";
    error_buffer()[0] = 0;
    if (!log_w_out || !w_out || !stats_out) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (B < 1 || B > (1 << 24)) return fail(BARK_ERR_ARG, "%s: between 1 and 2^24 forests (got %lld)", name, (long long)B);
    hipLaunchKernelGGL(forest_weights_kernel, dim3(1), dim3(WEIGHTS_THREADS), 0, static_cast<hipStream_t>(stream), log_w_in, increment,
                       info, (int)B, log_w_out, w_out, stats_out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_leaf_posterior_gather_hip(const void *state_in, int64_t B_in, int64_t R, const int64_t *index, int64_t n, void *state_out,
                                   void *stream) {
    static const char *name = "bark_leaf_posterior_gather_hip";
    error_buffer()[0] = 0;
    if (!state_in || !index || !state_out) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (B_in < 1 || R < 1 || R > 8192 || n < 1 || n > 65535)
        return fail(BARK_ERR_ARG, "%s: bad shape B_in=%lld R=%lld n=%lld (R <= 8192, 1 <= n <= 65535)", name, (long long)B_in,
                    (long long)R, (long long)n);
    if ((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 255)
        return fail(BARK_ERR_ARG, "%s: the states must be 256-byte aligned", name);
    const PosteriorState in = posterior_state(const_cast<void *>(state_in), R, B_in), out = posterior_state(state_out, R, n);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(state_in), b0 = reinterpret_cast<uintptr_t>(state_out);
    if (a0 < b0 + out.total && b0 < a0 + in.total) return fail(BARK_ERR_ARG, "%s: state_in and state_out overlap", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the bounds pass: a host copy of the index, so that no row outside state_in is ever read
    std::vector<int64_t> host((size_t)n);
    BARK_HIP_CHECK(hipMemcpyAsync(host.data(), index, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    BARK_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t k = 0; k < n; ++k)
        if (host[(size_t)k] < 0 || host[(size_t)k] >= B_in)
            return fail(BARK_ERR_ARG, "%s: index[%lld] = %lld outside [0, %lld)", name, (long long)k, (long long)host[(size_t)k],
                        (long long)B_in);
    const size_t RR = (size_t)R * R;
    hipLaunchKernelGGL(posterior_gather_kernel, dim3((unsigned)((RR + GATHER_TILE - 1) / GATHER_TILE), (unsigned)n), dim3(GATHER_THREADS),
                       0, s, in.Minv, in.w, in.info, reinterpret_cast<const long long *>(index), (int)R, out.Minv, out.w, out.info);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
