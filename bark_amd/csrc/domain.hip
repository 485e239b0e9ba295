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
//
// The repair step (bark_domain_repair_hip, "Domain repair" in include/bark_hip.h) sits between "write rows" and "scan rows" when
// the domain carries linear input constraints: one lane per row moves the row inside its own cell until A x <= b holds, or marks
// it infeasible.  Its table is the cells' usable closed intervals (cell_lo, cell_hi), read from global memory.
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

// ---- repair under linear constraints ----------------------------------------------------------------------------------------------
// One lane per row, 256 rows per workgroup, grid-stride over the tiles.  Every workgroup first rebuilds the constraints' small
// front in LDS from the CSR arrays: coefficients, b, tol, the ascending list of TOUCHED features (those with a stored coefficient)
// with their table slices, and per stored coefficient the position of its feature in that list.  A lane then reads only the
// touched columns of its row.  X_LDS keeps them in LDS as [touched feature][lane] — a wave reads or writes 64 consecutive
// doubles, no bank conflict; the host takes this instance when min(d, 64) columns of 256 rows fit beside the front in 64 KiB,
// d <= 24.  Otherwise the row's own memory is the working copy (every lane owns its row).  The cell of a coordinate is not kept:
// a coordinate never leaves its cell, so the binary search over cell_hi finds it again when a move needs the cell's ends.
// Nothing is trusted that could send an address out of bounds: a CSR that does not rise from 0 to at most 1024 entries, a column
// outside 0 .. d - 1, more than 64 touched features or a table slice outside 0 .. total marks every row infeasible and writes
// nothing else.
constexpr int REP_MAX_K = 16, REP_MAX_TOUCHED = 64, REP_MAX_NNZ = REP_MAX_K * REP_MAX_TOUCHED;
constexpr int REP_LDS_MAX_D = 24;  // X_LDS: lds_repair_bytes(24, true) = 60 624 <= 64 KiB

struct RepairArgs {
    const int64_t *cell_off;
    const double *cell_lo, *cell_hi;
    const int64_t *feat_types;
    const int64_t *row_ptr, *col;
    const double *coef, *b, *tol;
    const uint8_t *equality;
    double *rows;
    uint8_t *feasible;
    int64_t d, total, n;
    int K, passes;
};

// dynamic LDS, every area on a 16-byte boundary
struct RepairFront {
    double coef[REP_MAX_NNZ];
    double b[REP_MAX_K], tol[REP_MAX_K];
    int32_t rp[REP_MAX_K + 4];          // K + 1 used
    int32_t tfeat[REP_MAX_TOUCHED];     // touched feature j: its index ...
    int32_t toff[REP_MAX_TOUCHED];      // ... the first slot of its slice of the table ...
    int32_t tcnt[REP_MAX_TOUCHED];      // ... and the slice's length
    int32_t counts[DOM_THREADS];        // touched features per thread's run of features (the compaction's scan)
    int32_t T, bad, pad[2];
    uint8_t slot[REP_MAX_NNZ];          // stored coefficient e reads touched feature slot[e]
    uint8_t tint[REP_MAX_TOUCHED];      // touched feature j is an integer
    uint8_t eq[REP_MAX_K];
};
static_assert(sizeof(RepairFront) % 16 == 0, "the areas behind the front start on 16-byte boundaries");
__host__ __device__ inline size_t lds_repair_pos_bytes(int64_t d) { return ((size_t)d + 15) & ~(size_t)15; }
inline size_t lds_repair_bytes(int64_t d, bool x_lds) {
    return sizeof(RepairFront) + lds_repair_pos_bytes(d) + (x_lds ? (size_t)(d < REP_MAX_TOUCHED ? d : REP_MAX_TOUCHED) * DOM_THREADS * 8 : 0);
}

static_assert(sizeof(RepairFront) + 32 + (size_t)REP_LDS_MAX_D * DOM_THREADS * 8 <= DOM_LDS_MAX, "the X_LDS instance stays within 64 KiB");

// the touched columns of one lane's row
template <bool X_LDS>
struct RepairRow {
    double *xs;         // X_LDS: the tile's column 0 at this lane
    double *row;        // the row in global memory
    const int32_t *tfeat;
    __device__ __forceinline__ double get(int j) const { return X_LDS ? xs[j * DOM_THREADS] : row[tfeat[j]]; }
    __device__ __forceinline__ void set(int j, double v) const {
        if (X_LDS)
            xs[j * DOM_THREADS] = v;
        else
            row[tfeat[j]] = v;
    }
};

// first cell of the slice with x <= hi[c]; cnt when there is none (x above the range, or NaN)
__device__ __forceinline__ int repair_cell(const double *__restrict__ hi, int cnt, double x) {
    int a = 0, z = cnt;
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (x <= hi[mid])
            z = mid;
        else
            a = mid + 1;
    }
    return a;
}

// r_k = (sum_f A_kf x_f) - b_k: from 0.0 over the stored coefficients in order, multiply and add rounded separately
template <bool X_LDS>
__device__ __forceinline__ double repair_residual(const RepairFront &s, const RepairRow<X_LDS> &x, int k) {
    double sum = 0.0;
    for (int e = s.rp[k]; e < s.rp[k + 1]; ++e) sum = __dadd_rn(sum, __dmul_rn(s.coef[e], x.get(s.slot[e])));
    return __dsub_rn(sum, s.b[k]);
}

__device__ __forceinline__ bool repair_fails(double r, bool eq) { return eq ? !(r == 0.0) : !(r <= 0.0); }

template <bool X_LDS>
__global__ __launch_bounds__(DOM_THREADS) void domain_repair_kernel(RepairArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RepairFront &s = *reinterpret_cast<RepairFront *>(smem);
    uint8_t *pos = smem + sizeof(RepairFront);  // (d): touched flag, then the feature's place in the touched list
    double *tile = reinterpret_cast<double *>(smem + sizeof(RepairFront) + lds_repair_pos_bytes(p.d));
    const int tid = threadIdx.x, K = p.K;
    const int d = (int)p.d;

    // ---- the front: block-uniform, barriers inside ----
    if (tid == 0) {
        int bad = p.row_ptr[0] != 0;
        int64_t last = 0;
        s.rp[0] = 0;
        for (int k = 1; k <= K; ++k) {
            const int64_t v = p.row_ptr[k];
            if (v < last || v > REP_MAX_NNZ) bad = 1;
            last = v;
            s.rp[k] = bad ? 0 : (int32_t)v;
        }
        s.bad = bad;
        s.T = 0;
    }
    if (tid < K) s.b[tid] = p.b[tid], s.tol[tid] = p.tol[tid], s.eq[tid] = p.equality[tid] != 0;
    for (int f = tid; f < d; f += DOM_THREADS) pos[f] = 0;
    __syncthreads();
    const int nnz = s.bad ? 0 : s.rp[K];
    for (int e = tid; e < nnz; e += DOM_THREADS) {
        const int64_t c = p.col[e];
        s.coef[e] = p.coef[e];
        if (c < 0 || c >= p.d)
            s.bad = 1;  // every writer stores the same word
        else
            pos[c] = 1;
    }
    __syncthreads();
    // compaction of the flags into the ascending touched list: every thread owns a run of `run` features
    const int run = (d + DOM_THREADS - 1) / DOM_THREADS, f0 = tid * run, f1 = f0 + run < d ? f0 + run : d;
    {
        int cnt = 0;
        for (int f = f0; f < f1; ++f) cnt += pos[f];
        s.counts[tid] = cnt;
    }
    __syncthreads();
    {
        int at = 0;
        for (int t = 0; t < tid; ++t) at += s.counts[t];
        for (int f = f0; f < f1; ++f)
            if (pos[f]) {
                if (at < REP_MAX_TOUCHED) s.tfeat[at] = f;
                pos[f] = (uint8_t)(at & 255);
                ++at;
            }
        if (tid == DOM_THREADS - 1) s.T = at;
    }
    __syncthreads();
    if (s.T > REP_MAX_TOUCHED) s.bad = 1;
    const int T = s.T > REP_MAX_TOUCHED ? 0 : s.T;
    if (tid < T) {
        const int f = s.tfeat[tid];
        const int64_t o0 = p.cell_off[f], o1 = p.cell_off[f + 1];
        if (o0 < 0 || o1 <= o0 || o1 > p.total) s.bad = 1;
        s.toff[tid] = (int32_t)o0, s.tcnt[tid] = (int32_t)(o1 - o0);
        s.tint[tid] = p.feat_types[f] == FT_INT;
    }
    __syncthreads();  // orders the reads of s.T above before nothing else writes it; s.bad is final behind it
    const bool bad = s.bad != 0;
    for (int e = tid; e < nnz && !bad; e += DOM_THREADS) s.slot[e] = pos[p.col[e]];
    __syncthreads();

    // ---- the rows ----
    RepairRow<X_LDS> x;
    x.xs = tile + tid;
    x.tfeat = s.tfeat;
    const int64_t step = (int64_t)gridDim.x * DOM_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * DOM_THREADS + tid; i < p.n; i += step) {
        if (bad) {
            p.feasible[i] = 0;
            continue;
        }
        x.row = p.rows + i * p.d;
        // 1. every touched coordinate lies in a cell of its feature
        bool inside = true;
        for (int j = 0; j < T; ++j) {
            const double v = x.row[s.tfeat[j]];
            if (X_LDS) x.xs[j * DOM_THREADS] = v;
            const int c = repair_cell(p.cell_hi + s.toff[j], s.tcnt[j], v);
            inside = inside && c < s.tcnt[j] && v >= p.cell_lo[s.toff[j] + c];
        }
        if (!inside) {
            p.feasible[i] = 0;
            continue;
        }
        // 2. sequential repair: each violated constraint moves its coordinates, inside their cells, until it holds
        for (int pass = 0; pass < p.passes; ++pass)
            for (int k = 0; k < K; ++k) {
                const bool eq = s.eq[k];
                double r = repair_residual(s, x, k);
                for (int e = s.rp[k]; e < s.rp[k + 1] && repair_fails(r, eq); ++e) {
                    const double a = s.coef[e];
                    const int j = s.slot[e];
                    if (a == 0.0 || (eq && s.tint[j])) continue;
                    const double v = x.get(j);
                    const int c = repair_cell(p.cell_hi + s.toff[j], s.tcnt[j], v);  // c < tcnt[j]: v has not left its cell
                    const double lo = p.cell_lo[s.toff[j] + c], hi = p.cell_hi[s.toff[j] + c];
                    double w = s.tint[j] ? v - copysign(ceil(r / fabs(a)), a) : v - r / a;
                    w = w < lo ? lo : (w > hi ? hi : w);
                    if (w != v) {
                        x.set(j, w);
                        r = repair_residual(s, x, k);
                    }
                }
            }
        // 3. verify
        bool ok = true;
        for (int k = 0; k < K; ++k) {
            const double r = repair_residual(s, x, k);
            ok = ok && (s.eq[k] ? fabs(r) <= s.tol[k] : r <= s.tol[k]);
        }
        if (X_LDS)
            for (int j = 0; j < T; ++j) x.row[s.tfeat[j]] = x.xs[j * DOM_THREADS];
        p.feasible[i] = ok;
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

int bark_domain_repair_hip(const int64_t *cell_off, const double *cell_lo, const double *cell_hi, int64_t total,
                           const int64_t *feat_types, int64_t d, const int64_t *row_ptr, const int64_t *col, const double *coef,
                           const double *b, const double *tol, const uint8_t *equality, int64_t K, int passes, double *rows, int64_t n,
                           uint8_t *feasible_out, void *stream) {
    error_buffer()[0] = 0;
    if (d < 1 || d > DOM_MAX_D) return fail(BARK_ERR_ARG, "domain repair: d = %lld is outside 1..%lld", (long long)d, (long long)DOM_MAX_D);
    if (n < 0 || n > DOM_MAX_ROWS) return fail(BARK_ERR_ARG, "domain repair: n = %lld is outside 0..2^32", (long long)n);
    if (K < 1 || K > REP_MAX_K) return fail(BARK_ERR_ARG, "domain repair: K = %lld constraints are outside 1..%d", (long long)K, REP_MAX_K);
    if (passes < 1 || passes > 64) return fail(BARK_ERR_ARG, "domain repair: passes = %d is outside 1..64", passes);
    if (!cell_off || !cell_lo || !cell_hi) return fail(BARK_ERR_ARG, "domain repair: null cell table");
    if (total < d || total > DOM_MAX_CELLS)
        return fail(BARK_ERR_ARG, "domain repair: %lld cells for %lld features are outside d..2^20", (long long)total, (long long)d);
    if (!feat_types || !row_ptr || !col || !coef || !b || !tol || !equality) return fail(BARK_ERR_ARG, "domain repair: null constraint argument");
    if (n == 0) return BARK_OK;
    if (!rows || !feasible_out) return fail(BARK_ERR_ARG, "bark_domain_repair_hip: null rows or output");
    RepairArgs a{};
    a.cell_off = cell_off, a.cell_lo = cell_lo, a.cell_hi = cell_hi, a.feat_types = feat_types;
    a.row_ptr = row_ptr, a.col = col, a.coef = coef, a.b = b, a.tol = tol, a.equality = equality;
    a.rows = rows, a.feasible = feasible_out, a.d = d, a.total = total, a.n = n, a.K = (int)K, a.passes = passes;
    const bool x_lds = d <= REP_LDS_MAX_D;
    const int64_t blocks = (n + DOM_THREADS - 1) / DOM_THREADS;
    const unsigned grid = (unsigned)(blocks < (int64_t)DOM_MAX_GRID ? blocks : (int64_t)DOM_MAX_GRID);
    hipLaunchKernelGGL(x_lds ? domain_repair_kernel<true> : domain_repair_kernel<false>, dim3(grid), dim3(DOM_THREADS),
                       lds_repair_bytes(d, x_lds), static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
