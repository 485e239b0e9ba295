// Candidates of the acquisition search, generated on the device from the forests' own split structure (include/bark_hip.h,
// "Domain candidates", has the contract; bark_amd/optimizer/domain.py builds the cell table on the host).
//
// A tree kernel's posterior is piecewise constant: the thresholds of all trees of all forest samples cut the range of every
// feature into cells, and the acquisition takes one value on each product cell.  The table holds one representative per cell:
// cell_off (d + 1) int64 and cell_rep (total) fp64, feature f owning the slots cell_off[f] .. cell_off[f + 1] - 1.
//
// Both kernels are store bound.  Mapping: one thread per output ELEMENT in a grid-stride loop, so the 64 lanes of a wave write 64
// consecutive doubles (512 contiguous bytes) whatever d is.  The per-feature offsets sit in LDS as 32-bit words (total <= 2^20),
// the grid's mixed-radix strides behind them, and the representatives behind those when everything fits the 64 KiB every
// kernel may use without raising its limit; otherwise the representatives are read from global memory (they stay in L2).
//
// Draws (modes 0 and 1): philox.h with key = (seed low word, seed high word ^ 0x646F6D61), counter = (i low word, i high word,
// round, block), i the GLOBAL row index; feature f uses draw f of its row — block f / 2, word pair f % 2.  The two features of a
// block each compute it: a row's bits depend on (seed, round, i) only, never on first, n or the launch shape.
#include "common.h"
#include "philox.h"

#include <cmath>

namespace bark {
namespace {

constexpr int64_t DOM_MAX_D = 4096;
constexpr int64_t DOM_MAX_CELLS = (int64_t)1 << 20;
constexpr int64_t DOM_MAX_ROWS = (int64_t)1 << 32;        // rows of one bark_domain_candidates_hip call
constexpr int64_t DOM_MAX_NEIGHBOURS = (int64_t)1 << 24;  // the scan's candidate limit
constexpr int DOM_THREADS = 256;
constexpr unsigned DOM_MAX_GRID = 256 * 32;  // workgroups of a launch: 32 rounds of the CUs, the loop strides over the rest
constexpr size_t DOM_LDS_MAX = 64 * 1024;
constexpr uint32_t DOM_KEY = 0x646F6D61u;    // "doma": keeps a search apart from a sampler run with the same seed
constexpr int FT_CAT = 0, FT_INT = 1;        // forest.py:22-25
constexpr int64_t STRIDE_MAX = INT64_MAX;    // a saturated stride: every index of the grid divides to 0

struct DomainArgs {
    const int64_t *cell_off;
    const double *cell_rep;
    const double *bounds;
    const int64_t *feat_types;
    const double *x;
    double *out;
    int64_t d, total, first, n;
    uint32_t k0, k1, round;
    int mode;
};

// dynamic LDS: off (d + 1) int32 | padding to 8 bytes | stride (d) int64, grid mode only | rep (total) fp64 when REP_LDS
__host__ __device__ inline size_t lds_stride_offset(int64_t d) { return ((size_t)(d + 1) * 4 + 7) & ~(size_t)7; }
inline size_t lds_bytes(int64_t d, int64_t total, bool strides, bool rep) {
    return lds_stride_offset(d) + (strides ? (size_t)d * 8 : 0) + (rep ? (size_t)total * 8 : 0);
}

// the table's front in LDS; slots past the table's end are never addressed: every offset is clamped into 0 .. total
template <bool REP_LDS>
__device__ __forceinline__ const double *stage_table(const DomainArgs &p, bool strides, unsigned char *smem, int32_t *&off,
                                                     int64_t *&stride) {
    off = reinterpret_cast<int32_t *>(smem);
    stride = reinterpret_cast<int64_t *>(smem + lds_stride_offset(p.d));
    double *rep = reinterpret_cast<double *>(stride + (strides ? p.d : 0));
    for (int64_t f = threadIdx.x; f <= p.d; f += DOM_THREADS) {
        const int64_t o = p.cell_off[f];
        off[f] = (int32_t)(o < 0 ? 0 : (o > p.total ? p.total : o));
    }
    if (REP_LDS)
        for (int64_t j = threadIdx.x; j < p.total; j += DOM_THREADS) rep[j] = p.cell_rep[j];
    __syncthreads();
    if (strides) {
        if (threadIdx.x == 0) {  // suffix products of the cell counts, saturating: feature d - 1 varies fastest
            int64_t s = 1;
            for (int64_t f = p.d - 1; f >= 0; --f) {
                stride[f] = s;
                const int64_t c = off[f + 1] - off[f];
                s = (c < 1 || s > STRIDE_MAX / c) ? STRIDE_MAX : s * c;
            }
        }
        __syncthreads();
    }
    return REP_LDS ? rep : p.cell_rep;
}

// k-th set bit (k < popcount)
__device__ __forceinline__ int kth_set_bit(uint64_t mask, int64_t k) {
    for (int64_t j = 0; j < k; ++j) mask &= mask - 1;
    return __builtin_ctzll(mask);
}

template <bool REP_LDS>
__global__ __launch_bounds__(DOM_THREADS) void domain_candidates_kernel(DomainArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t *off = nullptr;
    int64_t *stride = nullptr;
    const double *rep = nullptr;
    if (p.mode != 0) rep = stage_table<REP_LDS>(p, p.mode == 2, smem, off, stride);  // block-uniform: barriers inside
    const int64_t elems = p.n * p.d, step = (int64_t)gridDim.x * DOM_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * DOM_THREADS + threadIdx.x; e < elems; e += step) {
        const int64_t f = e % p.d;
        const uint64_t g = (uint64_t)(p.first + e / p.d);
        double v;
        if (p.mode == 2) {
            const int64_t cells = off[f + 1] - off[f];
            v = cells > 0 ? rep[off[f] + (int64_t)((g / (uint64_t)stride[f]) % (uint64_t)cells)] : NAN;
        } else {
            uint32_t w[4];
            philox(p.k0, p.k1, (uint32_t)g, (uint32_t)(g >> 32), p.round, (uint32_t)(f >> 1), w);
            const double u = (f & 1) ? uniform53(w[2], w[3]) : uniform53(w[0], w[1]);
            if (p.mode == 1) {
                const int64_t cells = off[f + 1] - off[f];
                v = cells > 0 ? rep[off[f] + pick(u, cells)] : NAN;
            } else {
                const double lo = p.bounds[2 * f], hi = p.bounds[2 * f + 1];
                const int64_t ftype = p.feat_types[f];
                if (ftype == FT_CAT) {
                    const uint64_t mask = (uint64_t)(int64_t)hi;
                    const int bits = __popcll(mask);
                    v = bits > 0 ? (double)kth_set_bit(mask, pick(u, bits)) : NAN;  // no category: the leaf walk flags the NaN
                } else if (ftype == FT_INT) {
                    const int64_t ilo = (int64_t)lo, count = (int64_t)hi - ilo + 1;
                    v = count > 0 ? (double)(ilo + pick(u, count)) : NAN;
                } else {
                    v = lo + u * (hi - lo);
                    v = v > hi ? hi : v;
                }
            }
        }
        p.out[e] = v;
    }
}

// out[(k J + j) d + f] = f owns slot j ? cell_rep[j] : x[k d + f]
template <bool REP_LDS>
__global__ __launch_bounds__(DOM_THREADS) void domain_neighbours_kernel(DomainArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t *off = nullptr;
    int64_t *stride = nullptr;
    const double *rep = stage_table<REP_LDS>(p, false, smem, off, stride);
    const int64_t J = p.total, d = p.d, elems = p.n * J * d, step = (int64_t)gridDim.x * DOM_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * DOM_THREADS + threadIdx.x; e < elems; e += step) {
        const int64_t f = e % d, row = e / d, k = row / J;
        const int32_t j = (int32_t)(row % J);
        p.out[e] = (j >= off[f] && j < off[f + 1]) ? rep[j] : p.x[k * d + f];
    }
}

int check_table(const char *who, const int64_t *cell_off, const double *cell_rep, int64_t d, int64_t total) {
    if (!cell_off || !cell_rep) return fail(BARK_ERR_ARG, "%s: null cell table", who);
    if (total < 1 || total > DOM_MAX_CELLS)
        return fail(BARK_ERR_ARG, "%s: %lld cells are outside 1..2^20", who, (long long)total);
    if (total < d) return fail(BARK_ERR_ARG, "%s: %lld cells for %lld features (every feature has at least one)", who, (long long)total, (long long)d);
    return BARK_OK;
}

template <typename Kernel>
int launch(Kernel lds_kernel, Kernel global_kernel, const DomainArgs &a, bool table, bool strides, int64_t elems, hipStream_t stream) {
    bool rep_lds = table && lds_bytes(a.d, a.total, strides, true) <= DOM_LDS_MAX;
    const size_t lds = table ? lds_bytes(a.d, a.total, strides, rep_lds) : 0;
    const int64_t blocks = (elems + DOM_THREADS - 1) / DOM_THREADS;
    const unsigned grid = (unsigned)(blocks < (int64_t)DOM_MAX_GRID ? blocks : (int64_t)DOM_MAX_GRID);
    hipLaunchKernelGGL(rep_lds ? lds_kernel : global_kernel, dim3(grid), dim3(DOM_THREADS), lds, stream, a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_domain_candidates_hip(const int64_t *cell_off, const double *cell_rep, int64_t total, const double *bounds,
                               const int64_t *feat_types, int64_t d, int mode, uint64_t seed, int64_t round, int64_t first, int64_t n,
                               double *out, void *stream) {
    error_buffer()[0] = 0;
    if (mode < BARK_DOMAIN_UNIFORM || mode > BARK_DOMAIN_GRID) return fail(BARK_ERR_ARG, "domain candidates: unknown mode %d", mode);
    if (d < 1 || d > DOM_MAX_D) return fail(BARK_ERR_ARG, "domain candidates: d = %lld is outside 1..%lld", (long long)d, (long long)DOM_MAX_D);
    if (n < 0 || n > DOM_MAX_ROWS) return fail(BARK_ERR_ARG, "domain candidates: n = %lld is outside 0..2^32", (long long)n);
    if (first < 0 || first > INT64_MAX - n) return fail(BARK_ERR_ARG, "domain candidates: first = %lld is negative or first + n overflows", (long long)first);
    if (round < 0 || round > 0xFFFFFFFFll) return fail(BARK_ERR_ARG, "domain candidates: round %lld is outside 0..2^32 - 1", (long long)round);
    if (mode == BARK_DOMAIN_UNIFORM) {
        if (!bounds || !feat_types) return fail(BARK_ERR_ARG, "domain candidates: mode uniform needs bounds and feat_types");
    } else {
        const int rc = check_table("domain candidates", cell_off, cell_rep, d, total);
        if (rc) return rc;
    }
    if (n == 0) return BARK_OK;
    if (!out) return fail(BARK_ERR_ARG, "bark_domain_candidates_hip: null output");
    DomainArgs a{};
    a.cell_off = cell_off, a.cell_rep = cell_rep, a.bounds = bounds, a.feat_types = feat_types, a.out = out;
    a.d = d, a.total = total, a.first = first, a.n = n, a.mode = mode;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32) ^ DOM_KEY, a.round = (uint32_t)round;
    return launch(domain_candidates_kernel<true>, domain_candidates_kernel<false>, a, mode != BARK_DOMAIN_UNIFORM,
                  mode == BARK_DOMAIN_GRID, n * d, static_cast<hipStream_t>(stream));
}

int bark_domain_neighbours_hip(const int64_t *cell_off, const double *cell_rep, int64_t total, int64_t d, const double *x, int64_t K,
                               double *out, void *stream) {
    error_buffer()[0] = 0;
    if (d < 1 || d > DOM_MAX_D) return fail(BARK_ERR_ARG, "domain neighbours: d = %lld is outside 1..%lld", (long long)d, (long long)DOM_MAX_D);
    if (K < 0) return fail(BARK_ERR_ARG, "domain neighbours: K = %lld is negative", (long long)K);
    const int rc = check_table("domain neighbours", cell_off, cell_rep, d, total);
    if (rc) return rc;
    if (K > DOM_MAX_NEIGHBOURS / total)
        return fail(BARK_ERR_ARG, "domain neighbours: %lld points x %lld cells exceed the scan's 2^24 candidates", (long long)K, (long long)total);
    if (K == 0) return BARK_OK;
    if (!x || !out) return fail(BARK_ERR_ARG, "bark_domain_neighbours_hip: null argument");
    DomainArgs a{};
    a.cell_off = cell_off, a.cell_rep = cell_rep, a.x = x, a.out = out;
    a.d = d, a.total = total, a.n = K;
    return launch(domain_neighbours_kernel<true>, domain_neighbours_kernel<false>, a, true, false, K * total * d,
                  static_cast<hipStream_t>(stream));
}

}  // extern "C"
