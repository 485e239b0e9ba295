// Internal helpers shared by the libbarkhip.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/bark_hip.h"
#include "../../include/bark_hip_testing.h"
#include "leaf_state.h"

namespace bark {

// thread-local last-error buffer behind bark_last_error()
char *error_buffer();
int fail(int code, const char *fmt, ...);

#define BARK_HIP_CHECK(expr)                                                                       \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::bark::fail(BARK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                               \
    } while (0)

// Status of the launch just made: hipGetLastError(), or — test hook bark_debug_fail_launch(k), $BARK_TEST_HOOKS processes only — an injected failure of the
// k-th checked launch of the process (the kernel itself was enqueued; what is exercised is the error return path).
hipError_t launch_status();
#define BARK_LAUNCH_CHECK() BARK_HIP_CHECK(::bark::launch_status())

}  // namespace bark

// Per-device context (include/bark_hip.h: bark_ctx_create / bark_ctx_destroy).  Everything an entry point needs
// beyond its arguments lives here, so two host threads with a context (and a stream) each never share state.
struct bark_ctx {
    int device = 0;
    hipStream_t helper = nullptr;             // dense sweep: row launches beside the diag kernel
    hipStream_t helper2 = nullptr;            // dense sweep: look-ahead launches of the split-K bulk (even steps) / pipelined rows
    hipStream_t helper3 = nullptr;            // dense sweep: look-ahead bulk of the odd steps
    std::vector<hipEvent_t> events;           // fork / join events of the sweep (grown on demand, reused)
    hipEvent_t rejoin[3] = {nullptr, nullptr, nullptr};  // helper -> caller joins at the end of a chunk / on an error return
    std::vector<hipStream_t> chain_streams;   // multi-chain sampler step: one stream per chain (general shapes)
    std::vector<hipEvent_t> chain_done;
    hipEvent_t chain_fork = nullptr;
    void *ws = nullptr;                       // bark_ctx_workspace: grow-only device scratch
    size_t ws_bytes = 0;
    int32_t *fault = nullptr;                 // device: set by a leaf walk that met a NaN / inf / negative category
    int32_t *fault_host = nullptr;            // pinned mirror for bark_ctx_status
    char *stage_host = nullptr;               // pinned staging page of the host-pointer entry points (bark_ctx_upload, ..._host_pair)
    char *stage_dev = nullptr;                // its device twin
    hipEvent_t stage_event = nullptr;         // recorded behind the last staged asynchronous copy, on the stream it went to ...
    bool stage_busy = false;                  // ... and not yet waited for: the next staged call does, before it touches the page
};

namespace bark {

// ---------------------------------------------------------------------------------------------------------------
// Host functions that one translation unit defines and another calls: declared here and nowhere else, so the defining
// unit compiles against the declaration its callers use.
// ---------------------------------------------------------------------------------------------------------------
// ctx.hip
// ctx valid and made for the current device?  (entry points call this first)
int check_ctx(const bark_ctx *ctx);
int ctx_events(bark_ctx *ctx, size_t n);          // at least n events in ctx->events
int ctx_chain_streams(bark_ctx *ctx, size_t n);   // at least n chain streams + events

// A kernel that uses more than 64 KiB of dynamic LDS needs its limit raised once per device.  Every unit owns the table of
// its own kernels (and the once-per-device state that goes with it) and calls raise_lds_limits from its launch path, before
// the first launch that can need it; never from a query or a *_workspace_bytes function, which run without a device.
struct LdsLimit {
    const void *kernel;
    size_t bytes;
};
struct LdsLimitsOnce {
    std::once_flag once[64];
    int status[64] = {};
};
// checked; safe from several host threads; a current device outside 0..63 is refused
int raise_lds_limits(LdsLimitsOnce &state, const LdsLimit *table, size_t count);
template <size_t COUNT>
int raise_lds_limits(LdsLimitsOnce &state, const LdsLimit (&table)[COUNT]) {
    return raise_lds_limits(state, table, COUNT);
}

// traverse.hip
// one-hot leaf code with `words` = ceil(max_bits / 32) planes, whatever encoding the Gram kernels would pick
int walk_one_hot(const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d, int words,
                 uint32_t *out, int32_t *fault, hipStream_t stream);
// Gram-kernel leaf codes (encoding chosen from `info`), for the sweep entry points that already hold a context
int walk_codes(const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d, uint32_t *out,
               int32_t *fault, hipStream_t stream);

// gram.hip (the MLL engine fills its workspace with this kernel)
int launch_gram(const uint32_t *leaf1, int npad1, const uint32_t *leaf2, int npad2, int64_t B, int64_t m, int N, int M,
                int Nout, int Mout, const double *shift, const double *scale, const double *noise, double *out, int64_t ld,
                int64_t batch_stride, bool pad_identity, bool upper_only, int rep, int words, hipStream_t stream);

// chol.hip: the lock-step Cholesky sweep for a unit that fills its own systems (leafsystem.hip) — Bc resident R x R matrices
// A = U'U with one right-hand side each, and R identity columns appended when the caller also wants V = U^-T.  Host functions
// over an opaque handle; the sweep's kernels, layout and schedules stay in chol.hip.
struct SystemSweep;
// The chunk's systems as the caller's kernels fill them before system_sweep_factor and read them after it.
struct SystemMats {
    double *A;           // (Bc, npad, ld), matrix stride bstride: the upper triangle of the systems on entry, U on exit
    long ld, bstride;
    double *yz;          // (Bc, npad): the right-hand sides v on entry, z = U^-T v on exit
    double *accum;       // (Bc, 2): the sweep adds |z|^2 and log det A; the caller zeroes it, and its `info` (system_sweep_bind)
    const double *V;     // the identity columns inside A (same ld and bstride): V = U^-T on exit
    int64_t npad, cpad;  // R, and the identity columns (0 without), padded to whole blocks
};
// bytes at the front of the caller's workspace (256-byte aligned); needs no device
size_t system_sweep_bytes(int64_t R, bool identity, int64_t m, int64_t Bc);
// the sweep on `caller` and the context's helper streams; raises this unit's LDS limits first.  Closed by system_sweep_close.
int system_sweep_open(bark_ctx *ctx, hipStream_t caller, void *workspace, int64_t R, bool identity, int64_t m, int64_t Bc,
                      SystemSweep **out);
void system_sweep_close(SystemSweep *s);
// chunk(arg, c0, bc) for the chunks of at most Bc of the B systems, until one fails.  However a chunk returns, every helper
// stream the sweep has put work on is joined back into the caller's stream before this returns.
int system_sweep_chunks(SystemSweep *s, int64_t B, int64_t Bc, int (*chunk)(void *arg, int64_t c0, int64_t bc), void *arg);
// first in a chunk: its size and where the sweep reports its pivot status (bc entries); -> what to fill
const SystemMats &system_sweep_bind(SystemSweep *s, int64_t bc, int32_t *info);
int system_sweep_factor(SystemSweep *s);             // the identity columns when opened with them, then the block steps
int system_sweep_w(SystemSweep *s, double *w);       // after the factor, identity only: w = A^-1 v = V'z (bc, R)
int system_sweep_minv(SystemSweep *s, double *Minv);  // ... and A^-1 = V'V (bc, R, R)

// leafsystem.hip: what the stateless driver shares with the driver of the calls on a fitted state (fitted.hip)
// dst[b] = src[b], b < n: status words from one place to another (a fitted state's and a call's info_out)
int copy_info(const int32_t *src, int32_t *dst, int n, hipStream_t s);
// an invalid categorical value met by a leaf walk since the context's flag was last read (ctx.hip): info[b] = -1, b < n
int fault_info(const int32_t *fault, int32_t *info, int n, hipStream_t s);
// The forests of a call and the chunk of them that is resident: LeafSystem and FittedCall are both one of these, and their
// for_chunks set the chunk before the body runs.
struct ForestChunk {
    bark_ctx *ctx = nullptr;
    hipStream_t caller = nullptr;
    const void *packed = nullptr;
    const bark_pack_info *info = nullptr;
    int64_t d = 0, B = 0, Bc = 0;
    int m = 0, R = 0, W = 0;
    // the current chunk: its first forest, how many, and those forests as a pack of their own for the leaf walks
    int64_t c0 = 0;
    int bc = 0;
    bark_pack_info sub{};
    const char *packed_c = nullptr;

    void set_chunk(int64_t c0_, int64_t n) {
        c0 = c0_, bc = (int)n;
        sub = *info;
        sub.B = n;
        packed_c = static_cast<const char *>(packed) + (size_t)c0 * m * info->stride * 16;
    }
    // one-hot codes (bc, W, npad of n) of n points under the chunk's forests
    int walk(const double *points, int64_t n, uint32_t *codes) const {
        return walk_one_hot(packed_c, &sub, points, n, d, W, codes, ctx->fault, caller);
    }
    // an invalid categorical value met by one of the chunk's walks goes into these bc status words
    int take_fault(int32_t *chunk_info) const { return fault_info(ctx->fault, chunk_info, bc, caller); }
};
// The argument checks of an acquisition scan, stateless or from a state (`name`: the entry point's, for the messages), and
// the variant that bark_acquisition_plan resolves for the forests' shape -> *var.
int check_scan_args(const char *name, const bark_pack_info *info, const double *cand, int64_t C, const double *pending, int64_t P,
                    const int64_t *skip_idx, int64_t n_skip, const double *targets, int64_t S, double kappa, int kind, int variant,
                    const double *best_out, const int64_t *idx_out, int *var);
// The chunk's part of an acquisition scan: the LDS image into `tab` when var == 1, then slab by slab of the C candidates the
// walk into `ccodes` and acq_scan into acc (3, C).  w (bc, R) and Minv (bc, R, R) are the chunk's, already conditioned on any
// pending points; noise, scale, targets (B, S) and weights (B,) or null are the call's, indexed from the chunk's first forest.
int scan_chunk(const ForestChunk &ck, int var, int kind, const double *cand, int64_t C, const double *w, const double *Minv,
               double *tab, uint32_t *ccodes, double *acc, const double *noise, const double *scale, double kappa,
               const double *targets, int64_t S, const double *weights);

// leafspace.hip: launchers of the leaf-space entry points (LeafSystem, leafsystem.hip)
// leaf_inverse_kernel keeps the leaf lists of its 64 columns in dynamic LDS, m x 64 16-bit ids, so it takes forests of at
// most 160 KiB / 128 B = 1280 trees
constexpr int LEAF_INV_MAX_TREES = 1280;
int leafspace_prepare(const uint32_t *codes, int W, int npad, unsigned long long *planes, int R, int Rpad,
                      const double *noise, const double *scale, int m, int bc, double *A, long ld, long bstride,
                      const double *y, int N, double *yz, double *accum, int32_t *info, hipStream_t s);
int leafspace_sumsq(const double *y, int N, double *out, hipStream_t s);
int leafspace_predict(const uint32_t *ccodes, int W, int cpad, int C, const double *w, const double *Minv, int R,
                      const double *noise, const double *scale, int m, int bc, double *mu, double *var, hipStream_t s);
int leafspace_inverse(const uint32_t *codes, int W, int npad, int N, const double *Minv, const double *w, int R,
                      const double *y, const double *noise, const double *scale, int m, int bc, double *Wm, double *kinv,
                      double *kinv_y, const int32_t *accept, hipStream_t s);
int leafspace_finish(const double *accum, const double *yy, const double *noise, const double *scale, int m, int bc, int N,
                     int include_2pi, double *mll, hipStream_t s);
int noise_scale_decide(const double *new_mll, const double *state, const double *noise, const double *log_q_prior,
                       const double *log_u, const int32_t *info, const int32_t *fault, int nc, int32_t *accept_out,
                       hipStream_t s);
int noise_scale_state(const double *kinv_y, const double *y, int N, const double *new_mll, const int32_t *accept, int nc,
                      double *state, hipStream_t s);

// sample.hip
int64_t sample_spad(int64_t S);                    // padded Wt row: a multiple of the draws per gather pass
int64_t sample_partials(int64_t C, int64_t S);
// Wt (bc, Rpad, Spad) from V (leading dimension ldv, matrix stride vstride), w (bc, R) and eps (bc, S, R)
int sample_weights(const double *V, long ldv, long vstride, const double *w, const double *eps, int R, int Rpad, int S,
                   int Spad, const double *noise, const double *scale, int m, int bc, double *Wt, hipStream_t s);
// f (bc, S, C) for reduce == BARK_SAMPLE_FULL; otherwise red / ridx (bc, S) through `part` (sample_partials(C, S) x bc
// doubles) and `part_i` (as many int64)
int sample_gather(const uint32_t *ccodes, int W, int cpad, int C, const double *Wt, int Rpad, int Spad, int S, int m, int bc,
                  int reduce, double *f, double *red, int64_t *ridx, double *part, int64_t *part_i, hipStream_t s);
// the reduction's second step alone (MAX or MIN): red / ridx (bc, S) from partials laid out part[b][k][s], k < nblk in
// increasing candidate order; paths.hip feeds it the partials of its own scan
int sample_finish(const double *part, const int64_t *part_i, int nblk, int S, int bc, int reduce, double *red, int64_t *ridx,
                  hipStream_t s);

// acquire.hip
constexpr int ACQ_TILE = 256;               // points per workgroup of the scan and the score kernels, one per thread
constexpr size_t ACQ_LDS_MAX = 160 * 1024;  // all of a CU's LDS: one workgroup per CU
int64_t acq_partials(int64_t C);
// dynamic LDS of a scan / score launch: the tile's leaf lists and, with lds_table, the forest's image in front of them
size_t scan_lds_bytes(int64_t R, int64_t m, bool lds_table);
size_t acq_table_doubles(int64_t R);
// M^-1 of the chunk's forests conditioned on the P pending points whose codes are pcodes (bc, W, ppad)
int acq_condition(const uint32_t *pcodes, int W, int ppad, int P, double *Minv, int R, const double *noise, const double *scale,
                  int m, int bc, const int32_t *info, hipStream_t s);
// ... out of place (P >= 1): dst (bc, R, R) = src conditioned; src, e.g. a fitted state, is only read
int acq_condition_from(const uint32_t *pcodes, int W, int ppad, int P, const double *src, double *dst, int R, const double *noise,
                       const double *scale, int m, int bc, const int32_t *info, hipStream_t s);
// M^-1 and w (bc, R) conditioned in place on the P points with values (include/bark_hip.h, bark_leaf_posterior_observe_hip):
// values / eps / values_out / logpred_out are the chunk's rows, b0 its first forest (for the Philox counter)
int acq_observe(const uint32_t *pcodes, int W, int ppad, int P, double *Minv, double *w, int R, const double *noise,
                const double *scale, int m, int bc, const int32_t *info, int mode, const double *values, int value_stride,
                const double *eps, uint64_t seed, int64_t b0, int64_t draw, double *values_out, double *logpred_out, hipStream_t s);
// image of the chunk for the LDS variant
int acq_pack(const double *Minv, const double *w, int R, int bc, double *tab, hipStream_t s);
// variant: 1 LDS, 2 global (resolved by bark_acquisition_plan); n candidates of one slab against the bc forests of the chunk;
// kind: BARK_ACQ_*, the target kinds with the chunk's targets (bc, S); weights: the chunk's rows of the normalised forest
// weights (every term times its forest's weight, weight 0 skipped), or null for the equal-weight scan
int acq_scan(int variant, int kind, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
             const double *tab, int R, const double *noise, const double *scale, int m, int bc, double kappa, const double *targets,
             int S, int first, double *acc, size_t astride, const double *weights, hipStream_t s);
// weights (B,) or null as given to acq_scan: with them nothing is divided by B and a forest of weight 0 cannot fail the call
int acq_finish(const double *acc, int64_t C, int B, double kappa, int kind, const int64_t *skip, int n_skip, double *acq_out,
               double *part_v, int64_t *part_i, const int32_t *info, const double *weights, double *best, int64_t *best_i,
               hipStream_t s);

// scores.hip (launchers of bark_predictive_scores_hip, leafsystem.hip; predict's scores, fitted.hip, end in score_forests too)
// n points of one slab, whose first tile is tile0 of the call's `tiles`, against the bc forests of the chunk: the mixture's
// running state per point in the slab's part of acc (3, C; row stride astride) and one partial pair per (forest, tile) in
// fpart (bc, tiles, 2).  variant as acq_scan; mode: BARK_SCORE_*; info: the chunk's sweep status; yp: the slab's targets
int score_scan(int variant, int mode, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
               const double *tab, int R, const double *noise, const double *scale, int m, int bc, const int32_t *info,
               const double *yp, int first, double *acc, size_t astride, double *fpart, int tiles, int tile0, hipStream_t s);
// rows (bc, 2) of per_forest_out from fpart, the tiles in index order
int score_forests(const double *fpart, int tiles, int bc, double *rows, hipStream_t s);
// the per-point mixture terms (values_out (2, C) or null), their sums through mpart (tiles, 2), and NaN wherever info says so
int score_finish(const double *acc, int64_t C, int B, const double *yp, double *values_out, double *mpart, const int32_t *info,
                 double *per_forest_out, double *mixture_out, hipStream_t s);

// predict.hip (launchers of bark_leaf_posterior_predict_hip, fitted.hip)
// n points of one slab against the bc forests of the chunk, as score_scan: West's recurrence per point in the slab's part of
// acc (4, C; row stride astride).  weights: the chunk's rows of the normalised weights, or null (every forest weighs wq);
// info: the chunk's status in the state; fmu / fvar: the chunk's first rows of the per-forest output (row stride fstride) or
// null.  scores: also yp, sacc (3, C; score_scan's rows) and fpart (bc, tiles, 2) from tile0 on
int predict_scan(int variant, bool scores, const uint32_t *ccodes, int W, int cpad, int n, const double *wvec, const double *Minv,
                 const double *tab, int R, const double *noise, const double *scale, int m, int bc, const int32_t *info,
                 const double *weights, double wq, int observation, const double *yp, int first, double *acc, size_t astride,
                 double *sacc, double *fmu, double *fvar, size_t fstride, double *fpart, int tiles, int tile0, hipStream_t s);
// out[q ostride + c], q < Q <= 16, c < n: the mixture's quantiles from the stored rows of all B forests; probs / zscores: host
int predict_quantiles(const double *fmu, const double *fvar, size_t fstride, int n, int B, const double *weights, double wq,
                      const double *probs, const double *zscores, int Q, const int32_t *flag, double *out, size_t ostride,
                      hipStream_t s);
// *flag = a forest of non-zero weight has a non-zero status
int predict_flag(const int32_t *info, const double *weights, int B, int32_t *flag, hipStream_t s);
// moments_out (2, C) from acc; under the flag NaN there and in quantiles_out (Q, C); NaN rows of forest_out (2, B, C) or null
// for the forests with a non-zero status
int predict_finish(const double *acc, int64_t C, int B, const int32_t *info, const int32_t *flag, double *moments_out,
                   double *forest_out, double *quantiles_out, int Q, hipStream_t s);
// score_finish for the weighted mixture (weights null: that function's arithmetic); mpart (tiles, 2)
int predict_score_finish(const double *acc, const double *sacc, int64_t C, int B, const double *weights, const double *yp,
                         double *values_out, double *mpart, const int32_t *info, const int32_t *flag, double *per_forest_out,
                         double *mixture_out, hipStream_t s);

// covariance.hip (launchers of bark_leaf_posterior_covariance_hip, fitted.hip)
// cov_b = (scale_b / m) Z_1 M_b^-1 Z_2' of the chunk's forests into out (bc, C1, C2), from the codes of the C1 row points and
// of the C2 column points (symmetric: the same codes; then only the tiles of one triangle are computed and every entry is
// stored twice).  variant: 1 keeps a tile's T in LDS, 2 reads M^-1 from global memory (bark_acquisition_plan resolves it: a
// table that fits the scan's LDS gives a T tile that fits half a CU's).  weights: the chunk's rows or null; a forest of weight 0
// is left alone.  observation: s2_b onto the diagonal
int cov_tiles(int variant, const uint32_t *codes1, int cpad1, int C1, const uint32_t *codes2, int cpad2, int C2, int W, const double *Minv,
              int R, const double *noise, const double *scale, int m, int bc, const double *weights, int symmetric, int observation,
              double *out, hipStream_t s);
// the chunk's forests of non-zero weight, in order, onto the running sum mix (C1, C2) (first: it starts at zero):
// w_b (cov_b + (mu1_b - mean1)(mu2_b - mean2)'), with cov (bc, C1, C2), mu1 (bc, C1) and mu2 (bc, C2) the chunk's rows
int cov_accumulate(const double *cov, int64_t C1, int64_t C2, const double *mu1, const double *mean1, const double *mu2,
                   const double *mean2, const double *weights, double wq, int bc, int first, double *mix, hipStream_t s);
// after the last chunk: mix (or null) divided by *Wsum, NaN under the flag; NaN blocks of forest_out (B, C1, C2) or null for
// the forests of weight 0 or with a non-zero status
int cov_finish(double *mix, int64_t C1, int64_t C2, const double *Wsum, const int32_t *flag, const int32_t *info, const double *weights,
               int B, double *forest_out, hipStream_t s);

// fidelity.hip (launchers of bark_fidelity_gain_fitted_hip, fitted.hip)
constexpr int FID_MOMENTS = 6;  // doubles per (forest, candidate) between the moments and the quadrature kernel
size_t fidelity_moments_lds_bytes(int64_t m);
// n pairs (query, target) whose codes are qcodes / tcodes (bc, W, cpad) against the bc forests of the chunk: mom
// (bc, FID_MOMENTS, n) and the values of the pairs that need no quadrature in g (bc, n).  targets (bc, S) and weights (bc) or
// null are the chunk's rows; a forest of weight 0 is skipped (its row of g is NaN)
int fidelity_moments(const uint32_t *qcodes, const uint32_t *tcodes, int W, int cpad, int n, const double *wvec, const double *Minv,
                     int R, const double *noise, const double *scale, int m, int bc, const double *targets, int S,
                     const double *weights, double *mom, double *g, hipStream_t s);
// the separated pairs of mom -> g; grid (lo, hi, n_a, pad, G) as in include/bark_hip.h
int fidelity_quadrature(const double *mom, int n, int bc, const double *targets, int S, double lo, double hi, int n_a, double pad,
                        int G, double *g, hipStream_t s);
// acc (n) takes the chunk's rows of g in forest order (first: it starts at zero); then, after the last chunk, the gains
int fidelity_accumulate(const double *g, int n, int bc, const double *weights, int first, double *acc, hipStream_t s);
int fidelity_finish(const double *acc, int C, int B, const double *weights, const int32_t *info, double *gain_out,
                    double *per_forest_out, hipStream_t s);

constexpr size_t STAGE_BYTES = 64 * 1024;  // bark_ctx::stage_host / stage_dev
constexpr int NODE_BYTES = 26;          // forest.py:8-19, packed
constexpr uint32_t LEAF_FLAG = 0x80000000u;
constexpr uint32_t CAT_FLAG = 0x40000000u;
constexpr uint32_t FEAT_MASK = 0x3FFFFFFFu;

constexpr int TILE = 128;  // Cholesky block size == MFMA tile edge per workgroup
constexpr int MAX_LEAF_WORDS = 112;  // leaf-code dwords per point the Gram kernels can stage in LDS

inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

// Number of differing bytes of two dwords that each pack 4 dense leaf ids (one tree per byte): a tree pair
// agrees iff its byte of a ^ b is zero.  Ids < 128 keep bit 7 clear, so `x + 0x7f7f7f7f` cannot carry
// between bytes (SEVEN_BIT); the general form masks first.  forest.py:87 `np.equal(x1_leaves, x2_leaves)`.
template <bool SEVEN_BIT>
__device__ __forceinline__ uint32_t mismatched_bytes(uint32_t a, uint32_t b) {
    const uint32_t x = a ^ b;
    uint32_t z;
    if (SEVEN_BIT)
        z = (x + 0x7f7f7f7fu) & 0x80808080u;
    else
        z = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return __popc(z);
}

// leaf-code encodings (include/bark_hip.h): how the Gram kernels turn two code words into a count
enum LeafRep { REP_BYTES8 = 0, REP_BYTES7 = 1, REP_BITS = 2 };
inline LeafRep leaf_rep(const bark_pack_info *info) {
    if (bark_leaf_encoding(info) == BARK_LEAF_BITS) return REP_BITS;
    return info->max_leaves <= 128 ? REP_BYTES7 : REP_BYTES8;
}
// Launch decisions of the front end as pure host functions of the shape (traverse.hip, gram.hip): the launchers launch what these
// return and bark_frontend_variant_query (include/bark_hip_testing.h) reports it.
struct WalkVariant {
    bool grouped;       // leaf_walk_grouped_kernel (codes only), else leaf_walk_kernel
    bool nodes_lds;     // grouped: the forest's packed nodes are walked in LDS
    bool x_lds;         // the point rows sit in LDS (always when grouped); MODE 0: and the results are staged there
    unsigned grid_x;    // workgroups per forest of the kernel taken
    int64_t plain_wgs;  // grid of the one-thread-per-point kernel, which the grouped rule looks at
    size_t lds;         // dynamic LDS of the launch
};
WalkVariant walk_variant(int mode, const bark_pack_info *info, int64_t N, int64_t d, int words);
struct GramVariant {
    int tile_rows, tile_cols;  // output tile of a workgroup
    bool vec2;                 // every output row starts on a 16-byte boundary
    size_t lds;                // dynamic LDS of the launch: the two code strips
};
GramVariant gram_variant(int words, int64_t ld, int64_t batch_stride, uintptr_t out_address);
// per code word: number of disagreeing trees (byte encodings) or of agreeing trees (one-hot bits)
template <int REP>
__device__ __forceinline__ uint32_t code_count(uint32_t a, uint32_t b) {
    if (REP == REP_BITS) return __popc(a & b);
    return mismatched_bytes<REP == REP_BYTES7>(a, b);
}
// trees that agree, from the accumulated per-word counts
template <int REP>
__device__ __forceinline__ int agree_count(uint32_t acc, int m) {
    return REP == REP_BITS ? (int)acc : m - (int)acc;
}

// Root-to-leaf walk of one point through one packed tree (wire format of pack.cpp) — forest.py:28-47 `_pass_one_through_tree`:
//   categorical:  (1 << int(x[f])) & int(threshold) != 0 -> left ;  otherwise:  x[f] <= float64(float32 threshold) -> left ;
//   NaN compares false -> right.  Bounded by the packer's max_depth.  Shared by traverse.hip and the one-launch kernel of N <= 128.
template <bool X_IN_LDS>
__device__ __forceinline__ uint4 walk_tree(const uint4 *__restrict__ tree, int max_depth, const double *xrow,
                                           int32_t *__restrict__ fault) {
    uint4 n = tree[0];
    for (int step = 0; step < max_depth && !(n.x & LEAF_FLAG); ++step) {
        const uint32_t f = n.x & FEAT_MASK;
        const double xv = xrow[f];
        bool left;
        if (n.x & CAT_FLAG) {
            const double xt = trunc(xv);  // int(): toward zero
            // `1 << int(x)` raises in the reference for NaN / inf / x <= -1 (forest.py:38): flag it, the host raises
            if (!(xt >= 0.0 && xt < INFINITY)) *fault = 1;
            left = (xt >= 0.0 && xt < 32.0) ? ((n.y >> (uint32_t)xt) & 1u) : false;
        } else {
            left = xv <= (double)__uint_as_float(n.y);
        }
        n = tree[left ? n.z : n.w];
    }
    return n;
}

}  // namespace bark
