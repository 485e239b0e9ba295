// Posterior sample paths from a fitted leaf-space posterior (contract in include/bark_hip.h).
//
// A tree kernel has finite rank: a posterior draw of forest b IS a table of R leaf weights, W ~ N(c w, (scale/m) M^-1), and
// the sample path is f(x) = sum_t W[leaf_t(x)].  Two entry points:
//   bark_leaf_posterior_paths_hip   W[p] = c w_b + sqrt(scale_b/m) G_b eps[p],  G_b the lower Cholesky factor of the state's
//                                   M_b^-1, for a list of (forest, draw) pairs.  Every forest that occurs is factorised once
//                                   (paths_factor_kernel: one workgroup per forest, blocked left-looking, 32 x 32 tiles through
//                                   LDS, the matrix in the workspace); eps is the caller's or Box-Muller on Philox
//                                   (paths_normals_kernel); paths_weights_kernel is one wave per (path, leaf).
//   bark_path_scan_hip              f[p][x] = sum_t W[p][col_t(x)] over candidates, trees strictly in the order t = 0..m-1; FULL,
//                                   or MAX / MIN through fixed-order partials per workgroup and sample.hip's finish kernel.
// The path list is a host array: the launches are planned from it, and a table of its runs (one per forest that occurs) goes
// to the device through the context's staging page.  The state is read where posterior_state (leaf_state.h) says its areas are.
#include <cmath>
#include <cstring>

#include "common.h"
#include "philox.h"

namespace bark {
namespace {

constexpr int NB = 32;                          // tile edge of the factorisation
constexpr int64_t PATHS_MAX_LEAVES = 2048;      // one workgroup factorises a forest: R^3 / 3 flops on one CU
constexpr int64_t PATHS_MAX = 4096;             // paths per call: the run table fits the staging page
constexpr size_t PATHS_G_BYTES = (size_t)256 << 20;  // factors resident at a time
constexpr uint32_t PATH_KEY = 0x70617468u;      // "path": keeps the normals apart from every other stream of the same seed
constexpr int PS_TILE = 256;                    // candidates per scan workgroup, one per thread
constexpr int PS_MAX_PT = 16;                   // paths of one forest staged in LDS at a time
constexpr int64_t PS_SLAB = 1 << 16;            // candidates walked and scanned per launch pair
constexpr int PS_MAX_TREES = 64;
constexpr size_t PS_CODE_BYTES = (size_t)64 << 20;  // candidate codes resident at a time
constexpr int PS_MAX_WALK = 16;                 // forests per leaf walk

// the run (forest that occurs) of path p: run_p0 has nr + 1 rising entries, run_p0[0] <= p < run_p0[nr]
__device__ __forceinline__ int run_of(const int32_t *__restrict__ run_p0, int nr, int p) {
    int lo = 0, hi = nr - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (run_p0[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void paths_info_kernel(const int32_t *__restrict__ src, int32_t *__restrict__ dst, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) dst[b] = src ? src[b] : 0;
}

// G (slot) = lower Cholesky factor of M^-1 of forest run_b[r0 + slot], row-major with leading dimension R; the strict upper
// triangle of G is never written and never read.  Left-looking over column panels of NB: tile (i0, j0) of the panel is
//   S = A[i0.., j0..] - sum_{k0 < j0} L[i0.., k0..] L[j0.., k0..]'   (thread (ty, tx) owns S[ty][tx], k in rising order),
// the diagonal tile is factorised in LDS, a tile below it is solved against the diagonal tile row by row.  A forest whose
// status is already non-zero is skipped; a non-positive pivot k (1-based) goes to info[b] and ends the forest.
__global__ __launch_bounds__(1024) void paths_factor_kernel(const double *__restrict__ Minv, const int32_t *__restrict__ run_b, int r0,
                                                            int R, double *__restrict__ G, int32_t *__restrict__ info) {
    __shared__ double Ta[NB][NB + 1], Tb[NB][NB + 1], D[NB][NB + 1];
    __shared__ int bad;
    const int tid = threadIdx.x, tx = tid & (NB - 1), ty = tid >> 5;
    const int b = run_b[r0 + blockIdx.x];
    if (info[b] != 0) return;  // block-uniform, before any barrier
    const double *A = Minv + (size_t)b * R * R;
    double *L = G + (size_t)blockIdx.x * R * R;
    if (tid == 0) bad = 0;
    for (int j0 = 0; j0 < R; j0 += NB) {
        const int nb = R - j0 < NB ? R - j0 : NB;
        for (int i0 = j0; i0 < R; i0 += NB) {
            const int i = i0 + ty, j = j0 + tx;
            double acc = (i < R && j < R) ? A[(size_t)i * R + j] : 0.0;
            for (int k0 = 0; k0 < j0; k0 += NB) {  // whole tiles: j0 is a multiple of NB
                __syncthreads();
                Ta[ty][tx] = j0 + ty < R ? L[(size_t)(j0 + ty) * R + k0 + tx] : 0.0;
                Tb[ty][tx] = i < R ? L[(size_t)i * R + k0 + tx] : 0.0;
                __syncthreads();
#pragma unroll 8
                for (int k = 0; k < NB; ++k) acc -= Tb[ty][k] * Ta[tx][k];
            }
            __syncthreads();
            if (i0 == j0) {
                D[ty][tx] = acc;
                __syncthreads();
                for (int c = 0; c < nb; ++c) {
                    if (tid == 0) {
                        const double dd = D[c][c];
                        if (dd > 0.0) D[c][c] = sqrt(dd); else bad = j0 + c + 1;
                    }
                    __syncthreads();
                    if (bad) break;  // block-uniform
                    if (tx == c && ty > c && ty < nb) D[ty][c] = D[ty][c] / D[c][c];
                    __syncthreads();
                    if (tx > c && tx <= ty && ty < nb) D[ty][tx] -= D[ty][c] * D[tx][c];
                    __syncthreads();
                }
                if (bad) break;
                if (tx <= ty && ty < nb) L[(size_t)i * R + j] = D[ty][tx];
            } else {
                Tb[ty][tx] = acc;
                __syncthreads();
                if (tid < NB && i0 + tid < R) {  // row tid of the tile: x D' = s, columns in rising order
                    double x[NB];
#pragma unroll
                    for (int c = 0; c < NB; ++c) {
                        double s = Tb[tid][c];
#pragma unroll
                        for (int k = 0; k < c; ++k) s -= x[k] * D[c][k];
                        x[c] = c < nb ? s / D[c][c] : 0.0;
                    }
#pragma unroll
                    for (int c = 0; c < NB; ++c)
                        if (c < nb) L[(size_t)(i0 + tid) * R + j0 + c] = x[c];
                }
            }
        }
        if (bad) break;
        __threadfence_block();
    }
    __syncthreads();
    if (tid == 0 && bad) info[b] = bad;
}

// eps[p][a] for a < R: the normals of path p = (b, s).  Key (seed low word, seed high word ^ "path"), counter (b, s, a / 2, 0);
// u1 / u2 are the block's two 64-bit draws, r = sqrt(-2 log(1 - u1)), entry 2 j = r cos(2 pi u2), entry 2 j + 1 = r sin(2 pi u2).
__global__ void paths_normals_kernel(const int32_t *__restrict__ run_b, const int32_t *__restrict__ run_p0, int nr,
                                     const int32_t *__restrict__ draw, int P, int R, uint32_t k0, uint32_t k1,
                                     double *__restrict__ eps) {
    const int half = (R + 1) / 2;
    const int j = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (j >= half || p >= P) return;
    const int b = run_b[run_of(run_p0, nr, p)];
    uint32_t w[4];
    philox(k0, k1, (uint32_t)b, (uint32_t)draw[p], (uint32_t)j, 0u, w);
    const double u1 = uniform53(w[0], w[1]), u2 = uniform53(w[2], w[3]);
    const double r = sqrt(-2.0 * log(1.0 - u1)), th = 6.283185307179586 * u2;
    eps[(size_t)p * R + 2 * j] = r * cos(th);
    if (2 * j + 1 < R) eps[(size_t)p * R + 2 * j + 1] = r * sin(th);
}

// W[p][a] = c w[a] + sqrt(scale/m) sum_{k <= a} G[a][k] eps[p][k]: one wave per (p, a), lane l sums k = l, l + 64, ... in rising
// order and the 64 lane sums are folded by xor-shuffles 32, 16, ..., 1.  Paths p_lo .. p_hi - 1 (those of the resident runs).
__global__ __launch_bounds__(256) void paths_weights_kernel(const double *__restrict__ G, const double *__restrict__ wvec,
                                                            const double *__restrict__ eps, const int32_t *__restrict__ run_b,
                                                            const int32_t *__restrict__ run_p0, int nr, int r0, int p_lo, int R,
                                                            const double *__restrict__ noise, const double *__restrict__ scale, int m,
                                                            const int32_t *__restrict__ info, double *__restrict__ Wout) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6), p = p_lo + blockIdx.y;
    if (a >= R) return;  // no barriers below
    const int r = run_of(run_p0, nr, p), b = run_b[r];
    double *out = Wout + (size_t)p * R + a;
    if (info[b] != 0) {
        if (lane == 0) *out = NAN;
        return;
    }
    const double *row = G + ((size_t)(r - r0) * R + a) * R;
    const double *e = eps + (size_t)p * R;
    double s = 0.0;
    for (int k = lane; k <= a; k += 64) s += row[k] * e[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        const double sigma2 = 1e-6 + noise[b], sc = scale[b];
        const double coef = sc / ((double)m * sigma2), root = sqrt(sc / (double)m);
        *out = coef * wvec[(size_t)b * R + a] + root * s;
    }
}

// ---- scan ----
// One workgroup per (256 candidates of the slab, run).  Every thread decodes its candidate's m leaf ids (16-bit, [tree][lane]
// in LDS) from the one-hot code; then the run's W rows pass through LDS `pt` paths at a time and every thread gathers its m
// entries of each, in tree order, so a store of f is one contiguous segment per wave.  RED: 0 FULL, 1 MAX, 2 MIN: per path
// the workgroup's extreme and its lowest index (wave butterflies on (value, index), then the four waves in order) into
// part[blk][p] — the layout sample_finish reads with one "forest" of P "draws".
template <int RED>
__device__ __forceinline__ bool better(double v, long long i, double bv, long long bi) {
    return (RED == 1 ? v > bv : v < bv) || (v == bv && i < bi);
}

template <int RED>
__global__ __launch_bounds__(256) void path_gather_kernel(const uint32_t *__restrict__ ccodes, int Wd, int cpad, int n, int64_t s0,
                                                          int64_t C, const int32_t *__restrict__ run_b,
                                                          const int32_t *__restrict__ run_p0, int r0, int b_lo,
                                                          const double *__restrict__ Wp, int R, int m, int pt, int P,
                                                          double *__restrict__ f, double *__restrict__ part_v,
                                                          int64_t *__restrict__ part_i) {
    extern __shared__ double smem[];
    double *Wl = smem;                                               // [pt][R]
    double *redv = smem + (size_t)pt * R;                            // [PS_MAX_PT][4]
    long long *redi = reinterpret_cast<long long *>(redv + PS_MAX_PT * 4);
    unsigned short *idx = reinterpret_cast<unsigned short *>(redi + PS_MAX_PT * 4);  // [m][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = r0 + blockIdx.y, b = run_b[r], p0 = run_p0[r], np = run_p0[r + 1] - p0;
    const int c = blockIdx.x * PS_TILE + tid;
    const bool valid = c < n;
    {
        int cnt = 0;
        if (valid) {
            const uint32_t *code = ccodes + (size_t)(b - b_lo) * Wd * cpad + c;
            for (int wd = 0; wd < Wd && cnt < m; ++wd) {
                uint32_t bits = code[(size_t)wd * cpad];
                while (bits && cnt < m) {  // bits in increasing order: tree order
                    const int a = 32 * wd + __builtin_ctz(bits);
                    idx[cnt * PS_TILE + tid] = (unsigned short)(a < R ? a : 0);
                    bits &= bits - 1;
                    ++cnt;
                }
            }
        }
        for (; cnt < m; ++cnt) idx[cnt * PS_TILE + tid] = 0;
    }
    const int64_t gc = s0 + c;
    const size_t blk = (size_t)(s0 / PS_TILE) + blockIdx.x;
    for (int q0 = 0; q0 < np; q0 += pt) {
        const int cnt = np - q0 < pt ? np - q0 : pt;
        __syncthreads();
        const double *src = Wp + (size_t)(p0 + q0) * R;  // cnt consecutive rows
        for (int e = tid; e < cnt * R; e += PS_TILE) Wl[e] = src[e];
        __syncthreads();
        for (int pp = 0; pp < cnt; ++pp) {
            const double *row = Wl + (size_t)pp * R;
            double acc = 0.0;
#pragma unroll 4
            for (int t = 0; t < m; ++t) acc += row[idx[t * PS_TILE + tid]];
            if (RED == 0) {
                if (valid) f[(size_t)(p0 + q0 + pp) * C + gc] = acc;
            } else {
                double v = valid ? acc : (RED == 1 ? -INFINITY : INFINITY);
                long long at = valid ? (long long)gc : 0x7fffffffffffffffll;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double ov = __shfl_xor(v, off);
                    const long long oi = __shfl_xor(at, off);
                    // a NaN row is NaN in every lane; lane 0 of the workgroup's first wave is always a valid candidate
                    if (better<RED>(ov, oi, v, at)) v = ov, at = oi;
                }
                if (lane == 0) redv[pp * 4 + wave] = v, redi[pp * 4 + wave] = at;
            }
        }
        if (RED != 0) {
            __syncthreads();
            if (tid < cnt) {
                double v = redv[tid * 4];
                long long at = redi[tid * 4];
                for (int w = 1; w < 4; ++w)
                    if (better<RED>(redv[tid * 4 + w], redi[tid * 4 + w], v, at)) v = redv[tid * 4 + w], at = redi[tid * 4 + w];
                part_v[blk * P + p0 + q0 + tid] = v;
                part_i[blk * P + p0 + q0 + tid] = at;
            }
        }
    }
}

// an invalid categorical value met by the walks of a chunk of runs: their forests report -1.  The flag is taken (cleared) so
// that the next chunk starts clean, and put back by path_fault_restore_kernel for bark_ctx_status.
__global__ void path_fault_take_kernel(int32_t *fault, int32_t *seen, const int32_t *__restrict__ run_b, int r0, int nr,
                                       int32_t *__restrict__ info) {
    if (!*fault) return;
    for (int r = threadIdx.x; r < nr; r += blockDim.x) info[run_b[r0 + r]] = -1;
    __syncthreads();
    if (threadIdx.x == 0) *seen = 1, *fault = 0;
}
__global__ void path_fault_restore_kernel(int32_t *fault, const int32_t *seen) {
    if (*seen) *fault = 1;
}

// the results of paths whose forest reports a status, and of NaN paths: NaN / -1 (FULL: the rows of the reported forests)
__global__ void path_status_kernel(const int32_t *__restrict__ run_b, const int32_t *__restrict__ run_p0, int nr, int P,
                                   const int32_t *__restrict__ info, double *__restrict__ red, int64_t *__restrict__ ridx,
                                   double *__restrict__ f, int64_t C) {
    const int p = blockIdx.y;
    const bool failed = info[run_b[run_of(run_p0, nr, p)]] != 0;
    if (f) {
        if (!failed) return;
        for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += (int64_t)gridDim.x * blockDim.x)
            f[(size_t)p * C + c] = NAN;
    } else if (blockIdx.x == 0 && threadIdx.x == 0 && (failed || red[p] != red[p])) {
        red[p] = NAN;
        ridx[p] = -1;
    }
}

// ---- host ----
bool paths_shape_ok(int64_t R, int64_t m) { return R >= 1 && R <= PATHS_MAX_LEAVES && m >= 1 && m <= PS_MAX_TREES; }
int64_t factors_resident(int64_t R) {
    const int64_t k = (int64_t)(PATHS_G_BYTES / ((size_t)R * R * sizeof(double)));
    return k < 1 ? 1 : k;
}

struct PathsAreas {
    int32_t *table;  // draw (P) | run_b (P) | run_p0 (P + 1)
    double *G, *eps;
    size_t total;
};
PathsAreas paths_areas(void *ws, int64_t R, int64_t B, int64_t P, bool normals) {
    Carve cv{static_cast<char *>(ws)};
    PathsAreas a;
    const int64_t runs = P < B ? P : B, res = factors_resident(R);
    a.table = cv.take<int32_t>((size_t)3 * P + 1);
    a.G = cv.take<double>((size_t)(runs < res ? runs : res) * R * R);
    a.eps = cv.take<double>(normals ? (size_t)P * R : 0);
    a.total = cv.o;
    return a;
}

// the runs of a non-decreasing path list; -1 if it is not one or names a forest outside 0 .. B - 1
int build_runs(const int32_t *path_forest, int64_t P, int64_t B, int32_t *run_b, int32_t *run_p0) {
    int nr = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int32_t b = path_forest[p];
        if (b < 0 || b >= B || (p > 0 && b < path_forest[p - 1])) return -1;
        if (p == 0 || b != path_forest[p - 1]) run_b[nr] = b, run_p0[nr] = (int32_t)p, ++nr;
    }
    run_p0[nr] = (int32_t)P;
    return nr;
}

// scan: paths staged per LDS round, and the launch's dynamic LDS
int scan_pt(int64_t R) {
    const int64_t k = (48 * 1024) / (R * 8);
    return (int)(k < 1 ? 1 : k > PS_MAX_PT ? PS_MAX_PT : k);
}
size_t scan_lds(int64_t R, int64_t m) {
    return (size_t)scan_pt(R) * R * 8 + PS_MAX_PT * 4 * 16 + (size_t)m * PS_TILE * sizeof(unsigned short);
}
int64_t scan_walk(int64_t R, int64_t C) {  // forests per leaf walk
    const int64_t cpad = round_up(C < PS_SLAB ? C : PS_SLAB, TILE), W = (R + 31) / 32;
    const int64_t k = (int64_t)(PS_CODE_BYTES / ((size_t)W * cpad * 4));
    return k < 1 ? 1 : k > PS_MAX_WALK ? PS_MAX_WALK : k;
}
struct ScanAreas {
    int32_t *table;  // run_b (P) | run_p0 (P + 1)
    int32_t *seen;
    uint32_t *ccodes;
    double *part;
    int64_t *part_i;
    size_t total;
};
ScanAreas scan_areas(void *ws, int64_t R, int64_t P, int64_t C, bool reduce) {
    Carve cv{static_cast<char *>(ws)};
    ScanAreas a;
    const int64_t cpad = round_up(C < PS_SLAB ? C : PS_SLAB, TILE), W = (R + 31) / 32;
    const size_t partials = reduce ? (size_t)((C + PS_TILE - 1) / PS_TILE) * P : 0;
    a.table = cv.take<int32_t>((size_t)2 * P + 1);
    a.seen = cv.take<int32_t>(1);
    a.ccodes = cv.take<uint32_t>((size_t)scan_walk(R, C) * W * cpad);
    a.part = cv.take<double>(partials);
    a.part_i = cv.take<int64_t>(partials);
    a.total = cv.o;
    return a;
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_leaf_posterior_paths_plan(int64_t max_bits, int64_t m, int *route_out, int64_t *max_leaves_out) {
    error_buffer()[0] = 0;
    if (route_out) *route_out = BARK_PATHS_ROUTE_BLOCKED;
    if (max_leaves_out) *max_leaves_out = PATHS_MAX_LEAVES;
    if (!paths_shape_ok(max_bits, m))
        return fail(BARK_ERR_ARG, "sample paths take forests of at most %d trees and %lld leaves (got m = %lld, R = %lld)", PS_MAX_TREES,
                    (long long)PATHS_MAX_LEAVES, (long long)m, (long long)max_bits);
    return BARK_OK;
}

size_t bark_leaf_posterior_paths_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t P, int normals) {
    if (!paths_shape_ok(max_bits, m) || B < 1 || P < 1 || P > PATHS_MAX) return 0;
    return paths_areas(nullptr, max_bits, B, P, normals != 0).total;
}

int bark_leaf_posterior_paths_hip(bark_ctx *ctx, const bark_pack_info *info, const double *noise, const double *scale,
                                  const void *state, size_t state_bytes, const int32_t *path_forest, const int32_t *path_draw,
                                  int64_t P, const double *eps, uint64_t seed, double *W_out, int32_t *info_out, void *workspace,
                                  size_t workspace_bytes, void *stream_) {
    static const char *name = "bark_leaf_posterior_paths_hip";
    error_buffer()[0] = 0;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!info || !noise || !scale || !state || !path_forest || !path_draw || !W_out || !info_out || !workspace)
        return fail(BARK_ERR_ARG, "%s: null argument", name);
    if ((rc = bark_leaf_posterior_paths_plan(info->max_bits, info->m, nullptr, nullptr))) return rc;
    const int64_t B = info->B;
    const int R = (int)info->max_bits, m = (int)info->m;
    if (B < 1 || P < 1 || P > PATHS_MAX)
        return fail(BARK_ERR_ARG, "%s: 1 to %lld paths per call and B >= 1 (got P = %lld, B = %lld)", name, (long long)PATHS_MAX,
                    (long long)P, (long long)B);
    const PosteriorState st = posterior_state(const_cast<void *>(state), R, B);  // read only; its shape is inside the plan's limits
    if (state_bytes < st.total) return fail(BARK_ERR_ARG, "%s: state buffer too small: %zu < %zu bytes", name, state_bytes, st.total);
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(workspace)) & 255)
        return fail(BARK_ERR_ARG, "%s: state and workspace must be 256-byte aligned", name);
    std::vector<int32_t> table((size_t)3 * P + 1);
    int32_t *draw_h = table.data(), *run_b_h = draw_h + P, *run_p0_h = run_b_h + P;
    const int nr = build_runs(path_forest, P, B, run_b_h, run_p0_h);
    if (nr < 0) return fail(BARK_ERR_ARG, "%s: path_forest must be non-decreasing with entries in [0, B)", name);
    for (int64_t p = 0; p < P; ++p) {
        if (path_draw[p] < 0) return fail(BARK_ERR_ARG, "%s: negative draw number", name);
        draw_h[p] = path_draw[p];
    }
    const PathsAreas a = paths_areas(workspace, R, B, P, eps == nullptr);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if ((rc = bark_ctx_upload(ctx, a.table, table.data(), table.size() * sizeof(int32_t), stream_))) return rc;
    const int32_t *draw = a.table, *run_b = a.table + P, *run_p0 = run_b + P;
    const double *Minv = st.Minv, *wvec = st.w;
    hipLaunchKernelGGL(paths_info_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (const int32_t *)st.info, info_out, (int)B);
    BARK_LAUNCH_CHECK();
    if (!eps) {
        hipLaunchKernelGGL(paths_normals_kernel, dim3((unsigned)(((R + 1) / 2 + 127) / 128), (unsigned)P), dim3(128), 0, s, run_b, run_p0,
                           nr, draw, (int)P, R, (uint32_t)seed, (uint32_t)(seed >> 32) ^ PATH_KEY, a.eps);
        BARK_LAUNCH_CHECK();
        eps = a.eps;
    }
    const int res = (int)factors_resident(R);
    for (int r0 = 0; r0 < nr; r0 += res) {
        const int n = nr - r0 < res ? nr - r0 : res;
        hipLaunchKernelGGL(paths_factor_kernel, dim3((unsigned)n), dim3(1024), 0, s, Minv, run_b, r0, R, a.G, info_out);
        BARK_LAUNCH_CHECK();
        const int p_lo = run_p0_h[r0], p_hi = run_p0_h[r0 + n];
        hipLaunchKernelGGL(paths_weights_kernel, dim3((unsigned)((R + 3) / 4), (unsigned)(p_hi - p_lo)), dim3(256), 0, s, a.G, wvec, eps,
                           run_b, run_p0, nr, r0, p_lo, R, noise, scale, m, info_out, W_out);
        BARK_LAUNCH_CHECK();
    }
    return BARK_OK;
}

size_t bark_path_scan_workspace_bytes(int64_t max_bits, int64_t m, int64_t P, int64_t C, int reduce) {
    if (!paths_shape_ok(max_bits, m) || P < 1 || P > PATHS_MAX || C < 1 || C > (1 << 24)) return 0;
    return scan_areas(nullptr, max_bits, P, C, reduce != BARK_SAMPLE_FULL).total;
}

int bark_path_scan_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const int32_t *path_forest,
                       const double *W, int64_t P, const double *cand, int64_t C, int reduce, double *f_out, double *red_out,
                       int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, void *stream_) {
    static const char *name = "bark_path_scan_hip";
    error_buffer()[0] = 0;
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (reduce != BARK_SAMPLE_FULL && reduce != BARK_SAMPLE_MAX && reduce != BARK_SAMPLE_MIN)
        return fail(BARK_ERR_ARG, "%s: unknown reduce %d", name, reduce);
    const bool full = reduce == BARK_SAMPLE_FULL;
    if (!packed || !info || !path_forest || !W || !cand || !info_out || !workspace || (full ? !f_out : (!red_out || !idx_out)))
        return fail(BARK_ERR_ARG, "%s: null argument", name);
    if ((rc = bark_leaf_posterior_paths_plan(info->max_bits, info->m, nullptr, nullptr))) return rc;
    const int64_t B = info->B;
    const int R = (int)info->max_bits, m = (int)info->m;
    if (d < 1 || B < 1 || P < 1 || P > PATHS_MAX || C < 1 || C > (1 << 24))
        return fail(BARK_ERR_ARG, "%s: bad shape d=%lld B=%lld P=%lld (at most %lld) C=%lld (at most 2^24)", name, (long long)d, (long long)B,
                    (long long)P, (long long)PATHS_MAX, (long long)C);
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(BARK_ERR_ARG, "%s: workspace must be 256-byte aligned", name);
    std::vector<int32_t> table((size_t)2 * P + 1);
    int32_t *run_b_h = table.data(), *run_p0_h = run_b_h + P;
    const int nr = build_runs(path_forest, P, B, run_b_h, run_p0_h);
    if (nr < 0) return fail(BARK_ERR_ARG, "%s: path_forest must be non-decreasing with entries in [0, B)", name);
    const ScanAreas a = scan_areas(workspace, R, P, C, !full);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const size_t lds = scan_lds(R, m);
    static const LdsLimit limits[] = {{reinterpret_cast<const void *>(path_gather_kernel<0>), scan_lds(PATHS_MAX_LEAVES, PS_MAX_TREES)},
                                      {reinterpret_cast<const void *>(path_gather_kernel<1>), scan_lds(PATHS_MAX_LEAVES, PS_MAX_TREES)},
                                      {reinterpret_cast<const void *>(path_gather_kernel<2>), scan_lds(PATHS_MAX_LEAVES, PS_MAX_TREES)}};
    static LdsLimitsOnce once;
    if ((rc = raise_lds_limits(once, limits))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    if ((rc = bark_ctx_upload(ctx, a.table, table.data(), table.size() * sizeof(int32_t), stream_))) return rc;
    const int32_t *run_b = a.table, *run_p0 = run_b + P;
    hipLaunchKernelGGL(paths_info_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, (const int32_t *)nullptr, info_out, (int)B);
    BARK_LAUNCH_CHECK();
    BARK_HIP_CHECK(hipMemsetAsync(a.seen, 0, sizeof(int32_t), s));
    const int Wd = (R + 31) / 32, pt = scan_pt(R), walk = (int)scan_walk(R, C);
    for (int r0 = 0; r0 < nr;) {  // chunks of runs whose forests are consecutive: one leaf walk per slab
        int n = 1;
        while (r0 + n < nr && n < walk && run_b_h[r0 + n] == run_b_h[r0] + n) ++n;
        const int b_lo = run_b_h[r0];
        bark_pack_info sub = *info;
        sub.B = n;
        const char *packed_c = static_cast<const char *>(packed) + (size_t)b_lo * m * info->stride * 16;
        for (int64_t s0 = 0; s0 < C; s0 += PS_SLAB) {
            const int64_t ns = C - s0 < PS_SLAB ? C - s0 : PS_SLAB;
            const int cpad = (int)bark_leaf_npad(ns);
            if ((rc = walk_one_hot(packed_c, &sub, cand + (size_t)s0 * d, ns, d, Wd, a.ccodes, ctx->fault, s))) return rc;
            const dim3 g((unsigned)((ns + PS_TILE - 1) / PS_TILE), (unsigned)n);
            if (full)
                hipLaunchKernelGGL(path_gather_kernel<0>, g, dim3(PS_TILE), lds, s, a.ccodes, Wd, cpad, (int)ns, s0, C, run_b, run_p0, r0,
                                   b_lo, W, R, m, pt, (int)P, f_out, (double *)nullptr, (int64_t *)nullptr);
            else if (reduce == BARK_SAMPLE_MAX)
                hipLaunchKernelGGL(path_gather_kernel<1>, g, dim3(PS_TILE), lds, s, a.ccodes, Wd, cpad, (int)ns, s0, C, run_b, run_p0, r0,
                                   b_lo, W, R, m, pt, (int)P, (double *)nullptr, a.part, a.part_i);
            else
                hipLaunchKernelGGL(path_gather_kernel<2>, g, dim3(PS_TILE), lds, s, a.ccodes, Wd, cpad, (int)ns, s0, C, run_b, run_p0, r0,
                                   b_lo, W, R, m, pt, (int)P, (double *)nullptr, a.part, a.part_i);
            BARK_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(path_fault_take_kernel, dim3(1), dim3(64), 0, s, ctx->fault, a.seen, run_b, r0, n, info_out);
        BARK_LAUNCH_CHECK();
        r0 += n;
    }
    hipLaunchKernelGGL(path_fault_restore_kernel, dim3(1), dim3(1), 0, s, ctx->fault, a.seen);
    BARK_LAUNCH_CHECK();
    if (!full && (rc = sample_finish(a.part, a.part_i, (int)((C + PS_TILE - 1) / PS_TILE), (int)P, 1, reduce, red_out, idx_out, s))) return rc;
    const unsigned gx = full ? (unsigned)((C + 4095) / 4096 < 64 ? (C + 4095) / 4096 : 64) : 1u;
    hipLaunchKernelGGL(path_status_kernel, dim3(gx, (unsigned)P), dim3(256), 0, s, run_b, run_p0, nr, (int)P, info_out, red_out, idx_out,
                       full ? f_out : nullptr, C);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
