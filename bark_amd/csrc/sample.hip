// Joint posterior draws of the latent function at candidates, in leaf space (contract in include/bark_hip.h).
//
// With Z the one-hot leaf matrix, M = I_R + c Z'Z = U'U, w = M^-1 Z'y, c = scale / (m s2), the leaf weights of the
// forest's latent function f(x) = sum_t W[leaf_t(x)] have the posterior  W ~ N(c w, (scale/m) M^-1).  The leaf-space
// sweep with the identity right-hand side (LeafSystem, leafsystem.hip) leaves V = U^-T in the extra block columns, and
// U^-1 U^-T = M^-1, so one draw is  W_s = c w + sqrt(scale/m) V' eps_s.  Two kernels per chunk of forests:
//   sample_weights_kernel   Wt[a][s] = c w[a] + sqrt(scale/m) sum_k V[k][a] eps[s][k]   (fp64 MFMA; leaf-major, so a row
//                           of Wt holds every draw of one leaf)
//   sample_gather_kernel    f[s][x] = sum_t Wt[leaf_t(x)][s]   (trees summed in the fixed order t = 0..m-1); FULL stores
//                           the (S, C) block of the forest, MAX / MIN reduce over the workgroup's candidates instead and
//                           sample_finish_kernel reduces those partials (no float atomics: bit-identical to max / min of
//                           the FULL output, ties to the lowest candidate index).
#include "common.h"

namespace bark {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int WT_A = 64;   // leaves per weights workgroup (16 per wave)
constexpr int WT_S = 64;   // draws per weights workgroup
constexpr int WT_K = 32;   // k rows of V / eps staged per LDS round
constexpr int G_C = 64;    // candidates per gather workgroup
constexpr int MAX_TREES = 64;

// Wt[b][a][s] for a < Rpad, s < Spad (eps is zero outside s < S, k < R).  Wave w owns leaves a0 + 16 w .. + 15 and all
// 64 draws of the tile: four 16 x 16 accumulators of v_mfma_f64_16x16x4_f64 (A[i = l&15][k = l>>4] = V[k][a],
// B[k = l>>4][j = l&15] = eps[s][k], D reg v: row (l>>4) + 4 v, column l&15).  V = U^-T is lower triangular: the k rows
// above the workgroup's first leaf are never staged and the 4-row steps above the wave's first leaf are skipped.
__global__ __launch_bounds__(256) void sample_weights_kernel(const double *__restrict__ V, long ldv, long vstride,
                                                             const double *__restrict__ w, const double *__restrict__ eps,
                                                             int R, int Rpad, int S, int Spad, const double *__restrict__ noise,
                                                             const double *__restrict__ scale, int m, double *__restrict__ Wt) {
    __shared__ double Vs[WT_K][WT_A + 1];
    __shared__ double Es[WT_K][WT_S + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a0 = blockIdx.x * WT_A, s0 = blockIdx.y * WT_S, b = blockIdx.z;
    const double *Vb = V + (size_t)b * vstride;
    const double *Eb = eps + (size_t)b * S * R;
    const int aw = a0 + 16 * wave;
    f64x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = a0; k0 < Rpad; k0 += WT_K) {
        __syncthreads();
        for (int e = tid; e < WT_K * WT_A; e += 256) {  // rows of V: 512-byte segments
            const int kk = e / WT_A, aa = e - kk * WT_A;
            Vs[kk][aa] = Vb[(size_t)(k0 + kk) * ldv + a0 + aa];
        }
        for (int e = tid; e < WT_K * WT_S; e += 256) {  // eps[s][k0 .. k0 + 31]: 256-byte segments, transposed into LDS
            const int ss = e / WT_K, kk = e - ss * WT_K;
            const int k = k0 + kk, s = s0 + ss;
            Es[kk][ss] = (k < R && s < S) ? Eb[(size_t)s * R + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < WT_K; kq += 4) {
            if (k0 + kq + 3 < aw) continue;  // wave-uniform: V[k][a] = 0 for k < a
            const int kr = kq + (lane >> 4);
            const double av = Vs[kr][16 * wave + (lane & 15)];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Es[kr][16 * nt + (lane & 15)], acc[nt], 0, 0, 0);
        }
    }
    const double sigma2 = 1e-6 + noise[b];
    const double sc = scale[b];
    const double coef = sc / ((double)m * sigma2);
    const double root = sqrt(sc / (double)m);
    double *Wb = Wt + (size_t)b * Rpad * Spad;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int a = aw + (lane >> 4) + 4 * v;
        const double mean = a < R ? coef * w[(size_t)b * R + a] : 0.0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int s = s0 + 16 * nt + (lane & 15);
            if (s < Spad) Wb[(size_t)a * Spad + s] = mean + root * acc[nt][v];
        }
    }
}

// One workgroup per (64 candidates, forest).  The first wave decodes the candidates' leaf columns from their one-hot codes
// into LDS, one lane per candidate as leaf_predict_kernel does: the code words of 64 consecutive candidates are one 256-byte
// load, eight words in flight per lane.  (A wave-uniform decode, one candidate per wave at a time through readfirstlane,
// serialises W dependent global loads per candidate: the draws took 4.3 instead of 0.8 ms at B = 256, C = 10^4, S = 16.)
// Then `ST` lanes (16, 32 or 64; ST >= min(S, 64)) run over draws and 256 / ST candidates are in flight, so each tree's
// read is one contiguous segment of a row of Wt.  The (draws x candidates) tile goes through LDS (ST rows, dynamic) so
// that the store of f (B, S, C) is coalesced along c.  RED: 0 FULL, 1 MAX, 2 MIN (partials per workgroup,
// sample_finish_kernel).
template <int RED>
__global__ __launch_bounds__(256) void sample_gather_kernel(const uint32_t *__restrict__ ccodes, int W, int cpad, int C,
                                                            const double *__restrict__ Wt, int Rpad, int Spad, int S, int ST,
                                                            int m, double *__restrict__ f, double *__restrict__ part_v,
                                                            int64_t *__restrict__ part_i) {
    __shared__ unsigned short idx[MAX_TREES][G_C];
    __shared__ int cnt[G_C];
    extern __shared__ double tile[];  // [ST][G_C + 1]
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * G_C, b = blockIdx.y;
    if (tid < G_C) {
        const int c = c0 + tid;
        int n = 0;
        if (c < C)
            for (int w0 = 0; w0 < W; w0 += 8) {
                uint32_t word[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) word[u] = w0 + u < W ? ccodes[((size_t)b * W + w0 + u) * cpad + c] : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    uint32_t bits = word[u];
                    while (bits) {  // bits in increasing order: tree order
                        if (n < m) idx[n][tid] = (unsigned short)(32 * (w0 + u) + __builtin_ctz(bits));
                        bits &= bits - 1;
                        ++n;
                    }
                }
            }
        cnt[tid] = n < m ? n : m;
    }
    __syncthreads();
    const int sl = tid % ST, cg = tid / ST, ng = 256 / ST;
    const double *Wb = Wt + (size_t)b * Rpad * Spad;
    for (int sb = 0; sb < S; sb += ST) {
        const double *col = Wb + sb + sl;  // sb + ST <= Spad
        for (int cl = cg; cl < G_C; cl += ng) {
            const int n = cnt[cl];
            double acc = 0.0;
#pragma unroll 8
            for (int t = 0; t < n; ++t) acc += col[(size_t)idx[t][cl] * Spad];
            tile[sl * (G_C + 1) + cl] = acc;
        }
        __syncthreads();
        const int rows = S - sb < ST ? S - sb : ST;
        if (RED == 0) {
            for (int e = tid; e < rows * G_C; e += 256) {
                const int r = e / G_C, cl = e - r * G_C;
                if (c0 + cl < C) f[((size_t)b * S + sb + r) * C + c0 + cl] = tile[r * (G_C + 1) + cl];
            }
        } else if (tid < rows) {
            const int lim = C - c0 < G_C ? C - c0 : G_C;
            const double *row = tile + tid * (G_C + 1);
            double best = row[0];
            int at = 0;
            for (int cl = 1; cl < lim; ++cl) {
                const double v = row[cl];
                if (RED == 1 ? v > best : v < best) {  // strict: ties keep the lower index
                    best = v;
                    at = cl;
                }
            }
            const size_t o = ((size_t)b * gridDim.x + blockIdx.x) * S + sb + tid;
            part_v[o] = best;
            part_i[o] = c0 + at;
        }
        __syncthreads();
    }
}

// red[b][s] / idx[b][s] over the workgroup partials of sample_gather_kernel, in increasing candidate order
template <int RED>
__global__ void sample_finish_kernel(const double *__restrict__ part_v, const int64_t *__restrict__ part_i, int nblk, int S,
                                     int bc, double *__restrict__ red, int64_t *__restrict__ ridx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bc * S) return;
    const int b = i / S, s = i - b * S;
    const size_t base = (size_t)b * nblk * S + s;
    double best = part_v[base];
    int64_t at = part_i[base];
    for (int k = 1; k < nblk; ++k) {
        const double v = part_v[base + (size_t)k * S];
        if (RED == 1 ? v > best : v < best) {
            best = v;
            at = part_i[base + (size_t)k * S];
        }
    }
    red[i] = best;
    ridx[i] = at;
}

}  // namespace

// draws per gather pass (lanes over draws) and the padded Wt row: a multiple of it, so a pass never reads past the row
static int gather_st(int64_t S) { return S > 32 ? 64 : S > 16 ? 32 : 16; }
int64_t sample_spad(int64_t S) { return round_up(S, gather_st(S)); }
int64_t sample_partials(int64_t C, int64_t S) { return (C + G_C - 1) / G_C * S; }

// Wt (bc, Rpad, Spad) from V (leading dimension ldv, matrix stride vstride), w (bc, R) and eps (bc, S, R)
int sample_weights(const double *V, long ldv, long vstride, const double *w, const double *eps, int R, int Rpad, int S,
                   int Spad, const double *noise, const double *scale, int m, int bc, double *Wt, hipStream_t s) {
    hipLaunchKernelGGL(sample_weights_kernel, dim3((unsigned)(Rpad / WT_A), (unsigned)((Spad + WT_S - 1) / WT_S), (unsigned)bc), dim3(256),
                       0, s, V, ldv, vstride, w, eps, R, Rpad, S, Spad, noise, scale, m, Wt);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// f (bc, S, C) for reduce == BARK_SAMPLE_FULL; otherwise red / ridx (bc, S) through `part` (sample_partials(C, S) x bc
// doubles) and `part_i` (as many int64)
int sample_gather(const uint32_t *ccodes, int W, int cpad, int C, const double *Wt, int Rpad, int Spad, int S, int m, int bc,
                  int reduce, double *f, double *red, int64_t *ridx, double *part, int64_t *part_i, hipStream_t s) {
    if (m > MAX_TREES) return fail(BARK_ERR_ARG, "leaf-space posterior samples support at most %d trees", MAX_TREES);
    const int ST = gather_st(S);
    const int nblk = (C + G_C - 1) / G_C;
    const dim3 g((unsigned)nblk, (unsigned)bc);
    const size_t lds = (size_t)ST * (G_C + 1) * sizeof(double);
    if (reduce == BARK_SAMPLE_FULL)
        hipLaunchKernelGGL(sample_gather_kernel<0>, g, dim3(256), lds, s, ccodes, W, cpad, C, Wt, Rpad, Spad, S, ST, m, f,
                           (double *)nullptr, (int64_t *)nullptr);
    else if (reduce == BARK_SAMPLE_MAX)
        hipLaunchKernelGGL(sample_gather_kernel<1>, g, dim3(256), lds, s, ccodes, W, cpad, C, Wt, Rpad, Spad, S, ST, m,
                           (double *)nullptr, part, part_i);
    else
        hipLaunchKernelGGL(sample_gather_kernel<2>, g, dim3(256), lds, s, ccodes, W, cpad, C, Wt, Rpad, Spad, S, ST, m,
                           (double *)nullptr, part, part_i);
    BARK_LAUNCH_CHECK();
    if (reduce == BARK_SAMPLE_FULL) return BARK_OK;
    return sample_finish(part, part_i, nblk, S, bc, reduce, red, ridx, s);
}

// red / ridx (bc, S) from the partials part[b][k][s] of nblk workgroups, in increasing candidate order (MAX or MIN)
int sample_finish(const double *part, const int64_t *part_i, int nblk, int S, int bc, int reduce, double *red, int64_t *ridx,
                  hipStream_t s) {
    const unsigned fg = (unsigned)((bc * S + 255) / 256);
    if (reduce == BARK_SAMPLE_MAX)
        hipLaunchKernelGGL(sample_finish_kernel<1>, dim3(fg), dim3(256), 0, s, part, part_i, nblk, S, bc, red, ridx);
    else
        hipLaunchKernelGGL(sample_finish_kernel<2>, dim3(fg), dim3(256), 0, s, part, part_i, nblk, S, bc, red, ridx);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace bark
