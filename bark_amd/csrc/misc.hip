// Small device utilities of the C ABI that keep host-side glue free of array arithmetic:
// the mixture-of-Gaussians moments of tree_gps.py:116-131, a strided device copy, and the two reductions of the sampler's
// N x N state (batched row dot products, the quadratic form y' K_inv y).
#include "common.h"

namespace bark {
namespace {

// partial[0][c] = sum_b mu[b][c],  partial[1][c] = sum_b (var[b][c] + mu[b][c]^2)   (b ascending: reproducible)
__global__ void mixture_partial_kernel(const double *__restrict__ mu, const double *__restrict__ var, int64_t B, int64_t C,
                                       double *__restrict__ partial) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const double m = mu[b * C + c];
        s1 += m;
        s2 += var[b * C + c] + m * m;
    }
    partial[c] = s1;
    partial[C + c] = s2;
}

// tree_gps.py:128-130: mean = S1 / total, var = S2 / total - mean^2
__global__ void mixture_finish_kernel(const double *__restrict__ partial, double total, int64_t C, double *__restrict__ mean,
                                      double *__restrict__ var) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double m = partial[c] / total;
    mean[c] = m;
    var[c] = partial[C + c] / total - m * m;
}

// out[b] = alpha * sum_i A[b][i] * y[i] + beta * c[b]  (one wave per row; fixed order; c may be null)
__global__ __launch_bounds__(64) void rowdot_kernel(const double *__restrict__ A, const double *__restrict__ y, int64_t N,
                                                     int64_t lda, double alpha, const double *__restrict__ c, double beta,
                                                     double *__restrict__ out) {
    const double *row = A + (size_t)blockIdx.x * lda;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 64) s = fma(row[i], y[i], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) out[blockIdx.x] = c ? alpha * s + beta * c[blockIdx.x] : alpha * s;
}

constexpr int THREADS = 256;  // quadform_kernel's workgroup

// y' K_inv y  (quick_inverse.py:38), one workgroup, grid-stride rows
__global__ __launch_bounds__(THREADS) void quadform_kernel(const double *__restrict__ Kinv,
                                                           const double *__restrict__ y, int N, double *out) {
    __shared__ double red[THREADS / 64];
    double total = 0.0;
    for (int r = blockIdx.x; r < N; r += gridDim.x) {
        double s = 0.0;
        for (int c = threadIdx.x; c < N; c += THREADS) s = fma(Kinv[(size_t)r * N + c], y[c], s);
        total = fma(s, y[r], total);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_mixture_partial_hip(const double *mu, const double *var, int64_t B, int64_t C, double *partial, void *stream) {
    error_buffer()[0] = 0;
    if (!mu || !var || !partial || B < 1 || C < 1) return fail(BARK_ERR_ARG, "bark_mixture_partial_hip: bad argument");
    hipLaunchKernelGGL(mixture_partial_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mu,
                       var, B, C, partial);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_mixture_finish_hip(const double *partial, double total, int64_t C, double *mean, double *var, void *stream) {
    error_buffer()[0] = 0;
    if (!partial || !mean || !var || C < 1 || !(total > 0.0)) return fail(BARK_ERR_ARG, "bark_mixture_finish_hip: bad argument");
    hipLaunchKernelGGL(mixture_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       partial, total, C, mean, var);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_copy2d_hip(double *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols, void *stream) {
    error_buffer()[0] = 0;
    if (!dst || !src || rows < 1 || cols < 1 || ldd < cols || lds < cols) return fail(BARK_ERR_ARG, "bark_copy2d_hip: bad argument");
    BARK_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(double), src, (size_t)lds * sizeof(double), (size_t)cols * sizeof(double),
                                    (size_t)rows, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return BARK_OK;
}

int bark_rowdot_hip(const double *A, int64_t B, int64_t N, int64_t lda, const double *y, double alpha, const double *c,
                    double beta, double *out, void *stream_) {
    error_buffer()[0] = 0;
    if (!A || !y || !out || B < 1 || N < 1 || lda < N || B > (1 << 30)) return fail(BARK_ERR_ARG, "bark_rowdot_hip: bad argument");
    hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream_), A, y, N, lda, alpha, c,
                       beta, out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_quadform_hip(const double *K_inv, const double *y, int64_t N, double *out, void *stream_) {
    error_buffer()[0] = 0;
    if (!K_inv || !y || !out || N < 1 || N > (1 << 30)) return fail(BARK_ERR_ARG, "bark_quadform_hip: bad argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    BARK_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(double), stream));
    const int grid = (int)(N < 1024 ? N : 1024);
    hipLaunchKernelGGL(quadform_kernel, dim3(grid), dim3(THREADS), 0, stream, K_inv, y, (int)N, out);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
