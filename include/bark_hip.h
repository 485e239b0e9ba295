/*
 * bark_hip.h — C ABI of libbarkhip.so: the MI355X (gfx950) forest-kernel Gram + GP
 * marginal-log-likelihood / posterior engine behind the `bark.forest`,
 * `bark.tree_kernels` and `bark.fitting` Python API of TobyBoyne/bark.
 *
 * The reference has no FFI layer (it is Python + numba); its boundary for this path is a
 * set of module-level Python functions taking numpy arrays.  Each entry point below names
 * the reference function (path:line under /root/reference/src/bark) it serves.  The
 * binding a maintainer adds on the reference side is a ctypes stub — see INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; `int` status return, 0 == BARK_OK; message via bark_last_error()
 *    (thread-local).  The library never aborts and never frees/retains caller buffers.
 *  - `*_hip` entry points take DEVICE pointers (e.g. torch `tensor.data_ptr()`) and a
 *    `hipStream_t` passed as `void*` (NULL = default stream).  They only enqueue work:
 *    no allocation, no host synchronisation, so they are hipGraph-capturable (after one
 *    un-captured call with the same context, which creates its helper streams and events).
 *  - entry points that walk trees or fork helper streams take a `bark_ctx*` first: the per-device context that owns
 *    those streams/events, a scratch buffer and the categorical-fault flag.  The library is re-entrant per context:
 *    host threads that use one context (and one stream) each share no mutable state (SURVEY §8b Ownership /
 *    Threading; the reference's callers are single-threaded Python, bark_sampler.py / tree_gps.py).
 *  - `*_pack*` entry points are HOST functions on host pointers (format conversion only).
 *  - all matrices are row-major float64; feature matrices X are (N, d) row-major float64.
 */
#ifndef BARK_HIP_H
#define BARK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BARK_HIP_VERSION 210 /* 0.2.1: host-pointer entry points (bark_dev_alloc, bark_ctx_upload, ..._host_pair) */

enum {
    BARK_OK = 0,
    BARK_ERR_ARG = 1,         /* bad shape / null pointer / unsupported size */
    BARK_ERR_TREE = 2,        /* malformed tree: child index >= node_limit, cycle, feature_idx >= d */
    BARK_ERR_CATEGORICAL = 3, /* categorical threshold is not a bitmask in [0, 2^32) */
    BARK_ERR_HIP = 4,         /* a HIP runtime call failed (launch error etc.) */
    BARK_ERR_WORKSPACE = 5    /* workspace too small */
};

/* MLL conventions (bit flags) */
enum {
    BARK_MLL_INCLUDE_SCALE = 1, /* K_s = scale*K + (1e-6+noise) I   (bark_sampler.py:153-156) */
    BARK_MLL_INCLUDE_2PI = 2,   /* subtract n*log(2*pi)             (examples/mcmc/mcmc_record_mll.py:73) */
    BARK_MLL_RHS_IDENTITY = 4   /* right-hand-side block = I (C must equal N, cand ignored): cov_out receives
                                   K_s^-1 and mu_out receives K_s^-1 y  (bark/optimizer/opt_model.py:54-59,101) */
};

int bark_version(void);
/* Last error message of the calling thread ("" if none).  Pointer valid until the next call. */
const char *bark_last_error(void);
/* Process-wide switch (returns the previous setting; default on, off when $BARK_NO_DEVICE_WAIT is set).  On: sweeps of
 * few resident matrices — bound by the dependent chain diag -> solve -> diag (bark_sampler.py:153-162 with one chain,
 * BASELINE configs c2 / c5) — hand the completion of their row launches over to the caller's stream through a
 * device-side progress counter that the diagonal-block kernel waits for (bounded: 2 s), instead of a cross-stream
 * event wait between two kernels of that stream.  It needs the library's helper streams to run beside the caller's;
 * where they cannot (every stream of the process serialised onto one hardware queue), the wait times out and the call
 * reports info_out[b] = -3: DRAIN THE DEVICE (hipDeviceSynchronize — the entry point has joined its helper streams into
 * the caller's stream, so synchronising that stream is enough), switch the mechanism off and call again; the results and the
 * workspace of the timed-out call are not valid.  A time-out is sticky within a chunk (every later wait gives up at once:
 * the call costs one 2 s bound, not one per block step).  Off by default when $AMD_SERIALIZE_KERNEL / $HIP_LAUNCH_BLOCKING
 * serialise dispatch.  Never used under stream capture. */
int bark_device_wait(int on);
/* Host-side self-check of the workgroup -> (matrix, tile) map the sweep kernels share (XCD-aware placement: speed only, but a
 * map that skipped or doubled a pair would be a wrong result): 0 when the launch grid of `ntiles` tiles x `Bc` matrices
 * reaches every pair exactly once, else the number of pairs missed or reached twice.  No GPU needed. */
int bark_xcd_map_selftest(int ntiles, int Bc);

/* ---------------------------------------------------------------------------------------
 * Context — replaces nothing in the reference (pure functions on numpy arrays, forest.py:58-111); it is where the
 * state a GPU implementation needs between calls lives instead of in process globals.
 * ------------------------------------------------------------------------------------- */
typedef struct bark_ctx bark_ctx;
/* One context per (host thread, device).  Does not change the current device. */
int bark_ctx_create(int device, bark_ctx **out);
/* Frees the helper streams, events, scratch and flag.  Synchronise the streams used with the context first. */
void bark_ctx_destroy(bark_ctx *ctx);
/* Grow-only, 256-byte aligned device scratch owned by the context (the `workspace` arguments below may point into
 * it, or at any caller-owned device buffer).  *ptr_out stays valid until a later call asks for more bytes. */
int bark_ctx_workspace(bark_ctx *ctx, size_t bytes, void **ptr_out);
size_t bark_ctx_workspace_bytes(const bark_ctx *ctx);
/* Reads and clears the categorical-fault flag (synchronises `stream`).  *cat_fault_out != 0: a leaf walk enqueued with
 * this context evaluated a categorical split on a NaN / inf / negative value, where the reference raises inside
 * `1 << int(x)` (forest.py:38).  The MLL / posterior entry points report the same condition as info_out[b] = -1. */
int bark_ctx_status(bark_ctx *ctx, void *stream, int32_t *cat_fault_out);

/* ---------------------------------------------------------------------------------------
 * Host-pointer entry points — the ABI for a caller that has no tensor library: the reference's sampler is numba nopython
 * code (bark_sampler.py:120 `@njit _run_bark_sampler_multichain`, :216 `@njit _step_bark_sampler`), which can call C through
 * ctypes function pointers with integers, floats and array addresses only.  With these it can hold its chain state in HBM
 * (bark_sampler.py:153-162: K_inv by bark_mll_batched_hip + BARK_MLL_RHS_IDENTITY) and evaluate every tree proposal
 * (bark_sampler.py:233-257) from the two host trees it already has.  INTEGRATION.md §4 shows the caller.
 * ------------------------------------------------------------------------------------- */
/* hipMalloc / hipFree on the context's device (bark_dev_free synchronises the device, as hipFree does). */
int bark_dev_alloc(bark_ctx *ctx, size_t bytes, void **ptr_out);
int bark_dev_free(bark_ctx *ctx, void *ptr);
/* Host -> device on `stream`; `src_host` may be reused when the call returns (blocks of up to 64 KiB are staged through the
 * context's pinned page and copied asynchronously, larger ones are copied synchronously).  The three staged entry points of a
 * context (this one, bark_ctx_download, bark_tree_swap_eval_host_pair) share that page and may be given different streams:
 * each waits for the event recorded behind the previous staged copy, on whatever stream it went to, before it touches the
 * page.  One host thread per context, as everywhere. */
int bark_ctx_upload(bark_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes, void *stream);
/* Device -> host; synchronises `stream`. */
int bark_ctx_download(bark_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes, void *stream);
int bark_stream_sync(bark_ctx *ctx, void *stream);
/* One tree proposal of `_step_bark_sampler` (bark_sampler.py:233-257) from the trees as the sampler holds them:
 * pair26 = [forest[tree_idx], new_nodes], 2 x L packed 26-byte records in HOST memory; feat_types HOST int64 (d,);
 * K_inv (N, N), X (N, d), y (N,) DEVICE; s = sqrt(scale / m) (bark_sampler.py:231).  Packs the pair, stages it through the
 * context's pinned page, runs bark_tree_swap_eval_hip and returns on the HOST
 *   scalars_host_out[0] = y'K^-1 y - y'K'^-1 y ,  scalars_host_out[1] = log|K'| - log|K| ,  *r_out = leaves of the pair,
 * so new_mll = 0.5 (-(quad - scalars[0]) - (logdet + scalars[1])) (quick_inverse.py:38).  An accepted proposal is committed by
 * bark_lowrank_swap_apply_hip(K_inv, N, *r_out, workspace, K_inv, stream).  workspace >= bark_tree_swap_workspace_bytes(N, 64)
 * covers every pair this entry point accepts (more than 64 leaves in the pair: BARK_ERR_ARG).  Synchronises `stream`.
 * NaN / inf scalars: ask bark_lowrank_status_hip (singular update, quick_inverse.py:19,31) and bark_ctx_status. */
int bark_tree_swap_eval_host_pair(bark_ctx *ctx, const double *K_inv, int64_t N, const void *pair26, int64_t L,
                                  const int64_t *feat_types, int64_t d, const double *X, double s, const double *y,
                                  double *scalars_host_out, int64_t *r_out, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* ---------------------------------------------------------------------------------------
 * Forest container  (forest.py:8-19 NODE_RECORD_DTYPE: packed 26-byte records)
 *
 * bark_forest_pack converts B*m trees of L packed 26-byte node records (host memory,
 * C-contiguous (B, m, L)) into the device wire format: per tree `stride` 16-byte nodes in
 * depth-first order (root = slot 0), containing only the nodes reachable from the root.
 *   node.w0  internal: feature_idx | (is_categorical << 30);   leaf: 0x80000000 | dense_leaf_id
 *   node.w1  internal: float32 threshold bits, or the uint32 category bitmask;  leaf: original node index
 *   node.w2/w3  internal: compact index of left/right child;  leaf: w2 = position of the leaf's bit in the
 *               forest's one-hot code (trees own consecutive bit fields, one bit per reachable leaf)
 * `feat_types` is the reference's int64 array (0 = Cat, 1 = Int, 2 = Cont; forest.py:22-25).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int64_t B, m, L;      /* as passed in */
    int64_t stride;       /* nodes per tree in the packed array (max reachable nodes, >= 1) */
    int64_t max_leaves;   /* max number of reachable leaves in any tree (dense ids < max_leaves) */
    int64_t max_depth;    /* longest root-to-leaf walk (edges) */
    int64_t packed_bytes; /* B*m*stride*16 */
    int64_t max_bits;     /* max over forests of sum_t (#reachable leaves of tree t): width of the one-hot code */
} bark_pack_info;

/* Pass 1: validate + measure.  Fills *info. */
int bark_forest_pack_info(const void *nodes26, int64_t B, int64_t m, int64_t L, const int64_t *feat_types,
                          int64_t d, bark_pack_info *info);
/* Pass 2: write info->packed_bytes bytes to `packed` (host). */
int bark_forest_pack(const void *nodes26, const int64_t *feat_types, int64_t d, const bark_pack_info *info,
                     void *packed);

/* ---------------------------------------------------------------------------------------
 * Leaf traversal   — forest.py:28-67 (_pass_one_through_tree / pass_through_forest)
 * ------------------------------------------------------------------------------------- */
/* (N, m) uint32 leaf NODE indices for each of the B forests: out is (B, N, m) uint32, C order —
 * bit-identical to pass_through_forest(nodes[b], X, feat_types). */
int bark_leaf_indices_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                          int64_t d, uint32_t *out, void *stream);

/* Leaf codes consumed by the Gram kernels: out is (B, W, Npad) uint32, W = bark_leaf_words(info),
 * Npad = bark_leaf_npad(N), point index fastest.  Two encodings, chosen from `info` alone
 * (bark_leaf_encoding): 
 *   BARK_LEAF_BITS  one-hot: tree t owns L_t consecutive bits (L_t = its reachable leaves), a point sets the
 *                   bit of the leaf it reaches in every tree; then  #agreeing trees = popcount(z_i & z_j)
 *                   (2 VALU per 32 bits).  Chosen when max_bits < 64 * ceil(m/4), and always for trees with
 *                   more than 256 leaves.
 *   BARK_LEAF_BYTES 4 dense 8-bit leaf ids per dword; a tree pair agrees iff its byte of z_i ^ z_j is zero.
 * Every plane entry N <= i < Npad is written as ZERO, in both encodings and by every walk kernel: all B * W * Npad words are
 * defined after the call and nothing behind them is touched.  At most 112 words per point (else BARK_ERR_ARG). */
enum { BARK_LEAF_BYTES = 0, BARK_LEAF_BITS = 1 };
int64_t bark_leaf_npad(int64_t N);
int bark_leaf_encoding(const bark_pack_info *info);
int64_t bark_leaf_words(const bark_pack_info *info);
int bark_leaf_codes_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                        int64_t d, uint32_t *out, void *stream);

/* One-hot leaf vectors — forest.py:70-75 get_leaf_vectors: out[i * ldo + c] = value if leaves[i * ldl] == ids[c] else 0
 * (`np.equal(leaves[:, None], all_leaves[None, :])`, optionally scaled as bark_sampler.py:233-236 does).  leaves: leaf
 * node indices of one tree (element stride ldl, e.g. a column of bark_leaf_indices_hip's output); ids: the r distinct
 * reached leaves in ascending order (np.unique on the host: N * 4 bytes). */
int bark_onehot_match_hip(const uint32_t *leaves, int64_t N, int64_t ldl, const uint32_t *ids, int64_t r, double value,
                          double *out, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------
 * Gram matrix   — forest.py:78-111 (forest_gram_matrix / batched_forest_gram_matrix / _no_null)
 *   out[b][i][j] = (1.0/m) * #{t : leaf_t(x1_i) == leaf_t(x2_j)}          (bit-exact)
 * optionally followed, in this order, by
 *   - shift[b]            (forest.py:111  `sim_mat - num_null_trees / num_trees`)
 *   * scale[b]            (forest.py:111 `* scale`; tree_gps.py:97; bark_sampler.py:153)
 *   + (1e-6 + noise[b])   on the diagonal (tree_gps.py:100, mcmc_record_mll.py:67)
 * each rounded separately, as numpy does.  shift / scale / noise may be NULL (skipped).
 * leaf1/leaf2 come from bark_leaf_codes_hip for x1 / x2 with the same `info` (pass the same pointer when
 * x1 is x2).  out is (B, N, ld) float64, row stride `ld` >= M, batch stride `batch_stride` elements.
 * ------------------------------------------------------------------------------------- */
int bark_gram_from_leaves_hip(const uint32_t *leaf1, int64_t N, const uint32_t *leaf2, int64_t M,
                              const bark_pack_info *info, const double *shift, const double *scale,
                              const double *noise, double *out, int64_t ld, int64_t batch_stride, void *stream);

/* ---------------------------------------------------------------------------------------
 * Batched marginal log-likelihood — mcmc_record_mll.py:57-74, bark_sampler.py:153-162 +
 * quick_inverse.py:37-38.  One evaluation per forest sample b:
 *   K_s = [scale_b *] K_b + (1e-6 + noise_b) I ;  mll_b = 0.5(-y' K_s^-1 y - log|K_s| [- n log 2pi])
 * computed by a blocked fp64 Cholesky (A = U'U, MFMA panels) instead of the reference's LU
 * inv + slogdet; agreement is by tolerance (rtol 1e-9, atol 1e-8), see DESIGN.md.
 *
 * Optional posterior predictive (tree_gps.py:80-113) in the same sweep: pass C > 0 candidates
 * and get mu (B, C) and var (B, C) = scale_b - diag(K_xX K_s^-1 K_Xx)   (scale always applied,
 * as forest_predict does).
 *
 * Full covariance (tree_gps.py:108 with diag=False): pass cov_out (B, C, C) to also get
 *   cov_b = scale_b - K_xX K_s^-1 K_Xx     (every entry, as numpy broadcasting does).
 * With BARK_MLL_RHS_IDENTITY the right-hand-side block is the identity instead of K_Xx: cov_out = K_s^-1
 * (no `scale -`), mu_out = K_s^-1 y, var_out = diag(K_s^-1) — the explicit inverse the acquisition builder
 * consumes.  `shift` (B,) or NULL subtracts n_null/m before scaling (forest.py:102-111 no-null kernel).
 *
 * workspace: device buffer of at least bark_mll_workspace_bytes(N, C, m, Bc) bytes, where Bc
 * (1 <= Bc <= B) is the number of forests resident / factorised concurrently; B is processed in chunks of Bc.
 * info_out (device, B int32): 0, or 1-based index of the first non-positive pivot (not PD), or -3 when a device-side
 *   wait timed out (bark_device_wait), or -1 when a leaf walk
 * of the call met an invalid categorical value (see bark_ctx_status).  The pivot index is LAPACK potrf's `info` of that
 *   matrix alone, eliminated in order (only the first failure of a matrix is reported); an invalid categorical
 *   value takes precedence: -1 replaces it in every matrix of the chunk.  A matrix with info_out[b] > 0 is swept to the end with 1.0 in the place of each non-positive
 *   pivot: its own outputs (mll_out[b] and row b of mu_out, var_out, cov_out) are unspecified — possibly not finite —
 *   and must not be used.  The other matrices of the call are not affected: their info_out and every one of their
 *   outputs have the bits they have in a call where matrix b is positive definite.  The same holds for info_out of the
 *   leaf-space entry points below (a non-positive-definite M = I_R + c Z'Z, i.e. a negative scale).
 * ------------------------------------------------------------------------------------- */
size_t bark_mll_workspace_bytes(int64_t N, int64_t C, int64_t m, int64_t Bc);

/* Which launch schedule bark_mll_batched_hip takes for a shape — replaces nothing in the reference (its `inv` + `slogdet`,
 * examples/mcmc/mcmc_record_mll.py:63-73, have one schedule); a debug / documentation query: the same function the entry
 * point itself configures its sweep from, so DESIGN.md's table of schedules per BASELINE config can be asserted by a test
 * and a tuning constant cannot silently move a shape onto another schedule.  No GPU needed.
 *   leaf_words: bark_leaf_words(info) of the forests (decides whether the Gram is fused into the row kernels);
 *   timing != 0: as a call with a bark_mll_timing (the one-launch evaluation of N <= 128 is not taken then).
 * dev_wait / dev_gate are reported as the process-wide switch stands (bark_device_wait), outside stream capture. */
enum {
    BARK_SCHED_ONE_BLOCK = 0,        /* N <= 128, MLL only: leaf walk + one launch per chunk */
    BARK_SCHED_PLAIN = 1,            /* diag(j) || rows(j), then solve(j) */
    BARK_SCHED_PAIRED = 2,           /* plain with two block rows per row launch (chunks of a multiple of 256 matrices) */
    BARK_SCHED_PIPELINED = 3,        /* rows(j) over k < j-1 two steps ahead; consumers apply the last block row */
    BARK_SCHED_SPLITK = 4,           /* split-K layout (A materialised, slab scratch), no look-ahead step */
    BARK_SCHED_SPLITK_LOOKAHEAD = 5, /* split-K layout with look-ahead bulk launches */
    BARK_SCHED_TWO_BLOCK = 6,        /* 128 < N <= 256, MLL only: leaf walk + one launch per chunk (two block rows in one kernel) */
    BARK_SCHED_MULTI_BLOCK = 7       /* 256 < N <= 768, MLL only: the same with three to six block rows */
};
typedef struct {
    int32_t n_chunks, chunk, last_chunk;  /* chunks of `chunk` matrices, the last one of `last_chunk` */
    int32_t schedule, last_schedule;      /* BARK_SCHED_* of the full chunks / of the last chunk */
    int32_t splitk_layout, fused_gram;    /* slab scratch + materialised A; A generated inside the row kernels */
    int32_t dev_wait, dev_gate, pre_update; /* device-side hand-over, gate kernels, diag_pre_kernel (full chunks) */
    int32_t lookahead_steps, splitk_steps;  /* block steps with a look-ahead bulk / with any split-K launch (full chunks) */
    int32_t nrb, ncb;                     /* block rows, block columns incl. candidate blocks */
} bark_mll_plan;
int bark_mll_plan_query(int64_t N, int64_t C, int64_t m, int64_t B, int64_t Bc, int leaf_words, int timing, bark_mll_plan *out);

typedef struct {
    float total_ms;     /* the whole call on the caller's stream */
    float gram_ms;      /* leaf traversal + Gram fill + rhs init, summed over chunks */
    float chol_ms;      /* factorisation sequence (diag + panel + solve, finish, reductions) = total - gram */
    float diag_ms;      /* of which: diag_kernel  (128x128 potrf + inverse + z_j)            */
    float panel_ms;     /* of which: row_kernel / split-K kernels (fp64 MFMA trailing-panel update, K = 128 j) */
    float solve_ms;     /* of which: solve_kernel (MFMA triangular solve by the block inverse) */
    int64_t n_diag_launches, n_panel_launches, n_solve_launches;
    double panel_flops; /* fp64 flops executed by the row / split-K launches */
    double solve_flops; /* fp64 flops executed by the solve_kernel launches */
} bark_mll_timing;

int bark_mll_batched_hip(bark_ctx *ctx,
                         const void *packed, const bark_pack_info *info, /* forests (device / host info) */
                         const double *X, int64_t N, int64_t d,         /* training inputs (device) */
                         const double *y,                               /* (N,) targets (device) */
                         const double *noise, const double *scale,      /* (B,) device; scale may be NULL */
                         const double *shift,                           /* (B,) device or NULL */
                         int flags,                                     /* BARK_MLL_* */
                         const double *cand, int64_t C,                 /* (C, d) candidates or NULL/0 */
                         double *mll_out,                               /* (B,) device */
                         double *mu_out, double *var_out,               /* (B, C) device or NULL */
                         double *cov_out,                               /* (B, C, C) device or NULL */
                         int32_t *info_out,                             /* (B,) device */
                         void *workspace, size_t workspace_bytes, int64_t Bc,
                         bark_mll_timing *timing, /* optional (host); when non-NULL the call synchronises */
                         void *stream);

/* ---------------------------------------------------------------------------------------
 * Leaf-space MLL — the same quantity as bark_mll_batched_hip (mcmc_record_mll.py:57-74 / bark_sampler.py:153-162
 * conventions via `flags`), computed without ever forming the N x N matrix: K = (1/m) Z Z' with Z the one-hot
 * leaf matrix (N x R, R = info->max_bits), so
 *   log|K_s| = N log s2 + log|I_R + c Z'Z| ,   y'K_s^-1 y = (y'y - c v'(I_R + c Z'Z)^-1 v) / s2 ,
 *   s2 = 1e-6 + noise, c = scale / (m s2), v = Z'y .
 * O(N R^2 / 64 + R^3) instead of O(N^3): an exact algebraic alternative (agreement with the dense path to
 * ~1e-12 relative at noise 0.1; it loses digits as noise -> 0 through the subtraction y'y - c v'M^-1 v).
 * It is NOT the Gram + Cholesky work the benchmark metric counts and bench.py never times it as `value`.
 * Posterior (tree_gps.py:80-113, diagonal) in the same leaf space, with M = I_R + c Z'Z, w = M^-1 v and L(x) the m
 * leaves a candidate x reaches (Z'K_s^-1 Z = (m/scale)(I - M^-1)):
 *   mu(x) = c * sum_{a in L(x)} w_a ,    var(x) = (scale/m) * sum_{a,b in L(x)} (M^-1)_ab .
 * Pass C candidates (+ mu_out, var_out (B, C), scale, BARK_MLL_INCLUDE_SCALE); at most 64 trees.
 * ------------------------------------------------------------------------------------- */
size_t bark_mll_leafspace_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C);
int bark_mll_leafspace_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                           const double *y, const double *noise, const double *scale, int flags, const double *cand,
                           int64_t C, double *mll_out, double *mu_out, double *var_out, int32_t *info_out,
                           void *workspace, size_t workspace_bytes, int64_t Bc, void *stream);

/* Explicit inverse in the same leaf space — what the sampler rebuilds after every noise/scale proposal
 * (bark_sampler.py:267-272: inv + slogdet of scale K + (1e-6 + noise) I) and the acquisition builder reads
 * (opt_model.py:54-59) — without factorising the N x N matrix:
 *   K_s^-1 = (I - c Z M^-1 Z') / s2 ,   K_s^-1 y = (y - c Z w) / s2 ,   log|K_s| = -2 mll - y'K_s^-1 y
 * (mll in the convention selected by `flags`, as above).  kinv_out: (B, N, N); kinv_y_out: (B, N) or NULL.
 * Cost: the R x R sweep with an identity right-hand side + N R m + N^2 m gathered adds.
 * Limits: m <= 1280 trees (the leaf lists of a 64-column output tile, m x 64 16-bit ids, sit in the 160 KiB of LDS) and
 * R <= 8192 leaves, else BARK_ERR_ARG before anything is launched. */
size_t bark_kernel_inverse_leafspace_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc);
int bark_kernel_inverse_leafspace_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                                      int64_t d, const double *y, const double *noise, const double *scale, int flags,
                                      double *mll_out, double *kinv_out, double *kinv_y_out, int32_t *info_out,
                                      void *workspace, size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Joint posterior draws of the latent function at C candidates, in the same leaf space (no observation noise).
 * With M = I_R + c Z'Z = U'U, w = M^-1 Z'y and c = scale / (m s2) as above, f(x) = sum_t W[leaf_t(x)] and the leaf
 * weights have the posterior  W ~ N(c w, (scale/m) M^-1).  The sweep with an identity right-hand side leaves
 * V = U^-T (U^-1 U^-T = M^-1), so for each forest b and draw s:
 *   f[b,s,x] = c_b sum_t w_b[col_t(x)] + sqrt(scale_b/m) sum_t (V_b' eps[b,s])[col_t(x)]
 * i.e. cov_s(f(x), f(x')) = scale K(x, x') - K(x, X) K_s^-1 K(X, x'), the true posterior covariance (rank <= R, no C x C
 * matrix and no jitter).  eps: (B, S, R) device, R = info->max_bits; column a of forest b is bit a of that forest's
 * one-hot leaf code (the packer's order); entries a >= R_b (the forest's own leaf count) have no effect.
 * reduce = BARK_SAMPLE_FULL: f_out (B, S, C).  BARK_SAMPLE_MAX / MIN: red_out (B, S) = max / min over the candidates
 * of the same values, bit for bit, idx_out (B, S) int64 = its candidate index (ties: the lowest); f_out unused.
 * Trees are summed in the fixed order t = 0..m-1: the draws do not depend on the launch shape.  Limits: m <= 64 trees,
 * R <= 8192 (else BARK_ERR_ARG).  A non-positive-definite M is reported through info_out (k > 0) and a bad categorical
 * value as -1, as on the leaf-space MLL path.  workspace >= bark_posterior_samples_workspace_bytes(N, R, m, Bc, C, S).
 * ------------------------------------------------------------------------------------- */
#define BARK_SAMPLE_FULL 0 /* f_out (B, S, C) */
#define BARK_SAMPLE_MAX 1  /* red_out (B, S) = max over candidates, idx_out (B, S) int64 = its index */
#define BARK_SAMPLE_MIN 2  /* ... min */
size_t bark_posterior_samples_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t S);
int bark_posterior_samples_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                               int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                               int64_t C, const double *eps, int64_t S, int reduce, double *f_out, double *red_out,
                               int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                               void *stream);

/* ---------------------------------------------------------------------------------------
 * Acquisition scan: the lower confidence bound of the forest samples' posteriors over C candidates and its minimiser, in
 * the same leaf space, without the (B, C) arrays of mu and var (the reference's end-to-end test defines the acquisition,
 * tests/optimization/test_optimality.py:60-63: acqf(x) = mean_b(mu_b(x) - kappa sqrt(var_b(x))); its proposal must not be
 * worse than the minimum of acqf over random candidates).  With L(x) = a_0 < a_1 < ... the bits of candidate x's one-hot
 * code (one leaf per tree, in tree order) and w_b, M_b^-1, c_b as above:
 *   mu_b(x)  = c_b sum_i w_b[a_i]
 *   var_b(x) = (scale_b / m) ( sum_i (M_b^-1)[a_i][a_i] + 2 sum_i ( sum_{j<i} (M_b^-1)[a_j][a_i] ) )
 * (the quadratic form of leaf_predict over the upper triangle: m (m + 1) / 2 reads instead of m^2).  Per candidate three
 * sums run over the forests: sum_b (mu_b - kappa sqrt(max(var_b, 0))), sum_b mu_b and sum_b (var_b + mu_b^2).
 *   kind = BARK_ACQ_LCB_MEAN:     acq[x] = (1/B) sum_b (mu_b - kappa sd_b)
 *   kind = BARK_ACQ_LCB_MIXTURE:  acq[x] = mu_mix - kappa sqrt(max(var_mix, 0)),  mu_mix = (1/B) sum_b mu_b,
 *                                 var_mix = (1/B) sum_b (var_b + mu_b^2) - mu_mix^2        (tree_gps.py:116-131)
 * best_out / idx_out: the minimum of acq over the candidates and its index (ties: the lowest index); acq_out: (C,) or NULL.
 * If any info_out[b] != 0 (non-positive-definite M: k > 0; invalid categorical value: -1) they are NaN and -1.
 * Summation order (part of the contract): leaves in code-bit order within a candidate as written above, forests strictly
 * b = 0 .. B-1 across chunks.  The result therefore depends neither on Bc nor on the variant, bit for bit.
 * variant: 0 auto, 1 the forest's packed upper triangle of M^-1 and w staged in LDS (R (R + 1) / 2 + R doubles beside the
 * leaf lists of the workgroup's 256 candidates, m x 256 16-bit ids, in the 160 KiB of a CU), 2 the same arithmetic with
 * M^-1 and w read from global memory; auto takes 1 where it fits.  bark_acquisition_plan answers which one a shape takes
 * (*variant_out) and the dynamic LDS of that launch (*lds_bytes_out; for a refused variant = 1 the bytes it would need);
 * it and the workspace query are pure host code.
 * Limits, refused with BARK_ERR_ARG before any launch: m <= 64 trees, R <= 8192 leaves, 1 <= C <= 2^24, unknown kind or
 * variant, variant = 1 where the LDS does not hold the table, kappa not finite.  The call only enqueues (no allocation, no
 * host synchronisation).  Extra memory: the leaf-space posterior workspace of one chunk with the codes of at most 65536
 * candidates at a time, Bc (R (R + 1) / 2 + R) doubles, and 3 C + C / 128 doubles.
 * ------------------------------------------------------------------------------------- */
#define BARK_ACQ_LCB_MEAN 0
#define BARK_ACQ_LCB_MIXTURE 1
#define BARK_ACQ_EI 2  /* the target kinds: bark_acquisition_scan_targets_hip only */
#define BARK_ACQ_PI 3
#define BARK_ACQ_MES 4
size_t bark_acquisition_scan_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C);
int bark_acquisition_plan(int64_t max_bits, int64_t m, int variant /* 0 auto, 1 LDS, 2 global */, int *variant_out,
                          int64_t *lds_bytes_out);
int bark_acquisition_scan_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                              const double *y, const double *noise, const double *scale, const double *cand, int64_t C,
                              double kappa, int kind, int variant, double *acq_out /* (C,) or NULL */, double *best_out /* 1 */,
                              int64_t *idx_out /* 1 */, int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes,
                              int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Acquisition scan conditioned on pending points, with candidates excluded from the arg-min: what a batch of proposals
 * needs ("these points are being evaluated already").  bark_acquisition_scan_hip is the P = 0, n_skip = 0 call of it.
 * Both take the confidence bounds only (kind 0 / 1); the kinds that need targets go through bark_acquisition_scan_targets_hip.
 * pending: (P, d) device, or NULL with P = 0.  Each pending point x* is treated as observed at the forest's own posterior
 * mean ("kriging believer"), with the same noise.  With M = I_R + c Z'Z, w = M^-1 Z'y, c = scale / (m s2) as above and z the
 * one-hot row of x* (its m leaves L(x*) set), per forest:
 *     t = M^-1 z   (the sum of the m columns of M^-1 named by L(x*)),   q = z't,
 *     M^-1 <- M^-1 - (c / (1 + c q)) t t',   w unchanged:
 * the innovation y* - c z'w of the fantasised observation is zero, so w' = w + t (y* - c z'w) / (1 + c q) = w.  Hence
 * mu_b(x) is the mean given the real data and var_b(x) the posterior variance of forest b given X and the pending points,
 * i.e. what appending them to the training inputs gives (the variance depends on no y).  Nothing of size N or C is touched.
 * Order (part of the contract): pending points in the order given, each update seeing the previous one; within a point the
 * leaves in code-bit order; entries (i, j) and (j, i) subtract the same product.  Like the scan, the result depends neither
 * on Bc nor on the variant, bit for bit; two orders of the same pending points agree to rounding only.
 * skip_idx: (n_skip,) device int64 candidate indices, or NULL with n_skip = 0.  A listed candidate keeps its value in acq_out
 * but never wins the minimum; entries outside [0, C) have no effect; with every candidate listed best_out / idx_out are
 * NaN / -1.  An invalid categorical value in a pending point reports info_out[b] = -1, as in a candidate; forests with
 * info_out[b] != 0 are not conditioned.
 * Limits, refused with BARK_ERR_ARG before any launch: 0 <= P <= 64, 0 <= n_skip <= 64, and the scan's own.  The call only
 * enqueues.  Extra memory over the scan: the codes of the pending points, Bc ceil(R / 32) 128 words when P > 0.
 * As every leaf-space route the downdate loses digits as noise -> 0 (c grows, 1 + c q cancels against M^-1's own scale).
 * ------------------------------------------------------------------------------------- */
size_t bark_acquisition_scan_pending_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P);
int bark_acquisition_scan_pending_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                                      int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                                      int64_t C, const double *pending /* (P, d) or NULL */, int64_t P,
                                      const int64_t *skip_idx /* (n_skip,) or NULL */, int64_t n_skip, double kappa, int kind,
                                      int variant, double *acq_out /* (C,) or NULL */, double *best_out /* 1 */,
                                      int64_t *idx_out /* 1 */, int32_t *info_out /* (B,) */, void *workspace,
                                      size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Acquisition scan against targets: expected improvement, probability of improvement and min-value entropy search (the
 * reference's information gain at the target fidelity, information_based_fidelity.py:39-87, fed by the minima of joint
 * draws, thompson_sampling.generate_fstar_samples), next to the confidence bounds.  bark_acquisition_scan_pending_hip is the
 * targets = NULL call of it; kinds 0 / 1 ignore targets and S.
 * targets: (B, S) device, row b the targets t_{b,s} of forest b (an incumbent, or draws of the minimum f*).  The library
 * minimises, so every target kind returns the negated utility and best_out / idx_out name the maximiser of the utility
 * (ties: the lowest index; NaN never wins).  With mu = mu_b(x), var = var_b(x) exactly as the scan forms them above,
 * sd = sqrt(max(var, 0)), t = t_{b,s}, Phi(z) = 0.5 erfc(-z / sqrt 2), phi(z) = exp(-z^2 / 2) / sqrt(2 pi), E = sqrt(2 pi e):
 *   BARK_ACQ_EI:   z = (t - mu) / sd,  g = (t - mu) Phi(z) + sd phi(z);        sd == 0: g = max(t - mu, 0)
 *   BARK_ACQ_PI:   g = Phi(z);                                                 sd == 0: g = t > mu ? 1 : 0
 *   BARK_ACQ_MES:  gam = (t - mu) / (sd + 1e-7), cdf = Phi(gam), pdf = phi(gam), inner = E sd cdf (1e-10 where inner <= 0),
 *                  g = log(sd E) - ( log(inner) - gam pdf / (2 cdf + 1e-10) )   -- the reference's formula with its guards;
 *                  sd == 0 gives g = -inf, an acquisition of +inf: such a candidate never wins
 *   acq[x] = -(1/B) sum_b ( (1/S) sum_s g )
 * in fp64 with the device library's erfc, exp and log.  The quotients by sd and sd + 1e-7 are products with one reciprocal
 * per (candidate, forest); 1 / sqrt 2 and 1 / sqrt(2 pi) are constants.  A NaN target makes the acquisition of every
 * candidate NaN (under sd == 0 too), so none wins.
 * Summation order (part of the contract): s = 0 .. S-1 within a forest, then the division by S; forests strictly
 * b = 0 .. B-1 across chunks, the division by B in the finish.  As for the confidence bounds the result depends neither on
 * Bc nor on the variant, bit for bit.  S targets repeated k times agree with the S targets to rounding only.
 * kappa is ignored by the target kinds but must still be finite.  Pending points and skip_idx act as described above: the
 * conditioning comes before the scan and does not know the kind.
 * Limits, refused with BARK_ERR_ARG before any launch: the pending entry point's; unknown kind; a target kind with
 * targets == NULL, S < 1 or S > 1024.  The call only enqueues.  No memory beyond the pending entry point's: the targets are
 * read where they are, through wave-uniform addresses, and the plan (bark_acquisition_plan) is that of the other kinds.
 * ------------------------------------------------------------------------------------- */
size_t bark_acquisition_scan_targets_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P);
int bark_acquisition_scan_targets_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                                      int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                                      int64_t C, const double *pending /* (P, d) or NULL */, int64_t P,
                                      const int64_t *skip_idx /* (n_skip,) or NULL */, int64_t n_skip,
                                      const double *targets /* (B, S) or NULL for kinds 0 / 1 */, int64_t S, double kappa,
                                      int kind, int variant, double *acq_out /* (C,) or NULL */, double *best_out /* 1 */,
                                      int64_t *idx_out /* 1 */, int32_t *info_out /* (B,) */, void *workspace,
                                      size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fitted leaf-space posterior: fit once, then scan and condition from the state.  Every scan above starts from nothing: it
 * walks the N training points, forms and factorises M = I_R + c Z'Z per forest, solves for w and M^-1, scores the candidates
 * and drops all of it.  These entry points keep what the candidates are scored with, in a buffer the caller owns.
 * state: device, 256-byte aligned, bark_leaf_posterior_bytes(R, m, B) bytes: M^-1 (B, R, R) fp64, w (B, R) fp64 and the
 *   sweep's status per forest (B int32), each area rounded up to 256 bytes: align(8 B R^2) + align(8 B R) + align(4 B).  The
 *   query returns 0 for a shape the scan refuses (m > 64, R > 8192, B < 1).  The state depends on (packed, X, y, noise,
 *   scale) only; the calls that read it take packed / info / noise / scale again, for the candidate walk and the constants,
 *   and they must be the ones it was fitted with.  No X, no y, nothing of size N after the fit.
 * bark_leaf_posterior_fit_hip: per chunk of Bc forests exactly the opening sequence of bark_acquisition_scan_hip (leaf walk,
 *   M, the R x R sweep with an identity right-hand side, w = V'z, M^-1 = V'V), with the two results written into the state in
 *   place.  info_out[b] and the state's status: 0, k > 0 (pivot k of M_b not positive) or -1 (invalid categorical value in X).
 *   A scan from the state therefore reads the bits the stateless scan with the same Bc computes (the sweep's schedule may
 *   depend on Bc, hence "the same").  workspace >= bark_leaf_posterior_fit_workspace_bytes(N, R, m, Bc): the sweep's areas
 *   and the codes of the N points; no candidate, scan or pending areas.
 * bark_acquisition_scan_fitted_hip: bark_acquisition_scan_targets_hip from the state — all five kinds, pending, skip_idx,
 *   targets, variant and every formula and summation order as documented above; acq_scan / acq_finish are the same kernels.
 *   The state is not modified: with P > 0 the chunk's M^-1 is conditioned into a scratch area of the workspace, the first
 *   downdate reading the state and writing the scratch, the others in place there, with the arithmetic and order of the
 *   pending entry point.  Hence the result equals that of the stateless call with the Bc of the fit, bit for bit, and does
 *   not depend on this call's Bc.  info_out[b]: the state's status, or -1 for an invalid categorical value in a candidate or
 *   pending point of this call; any non-zero entry makes best_out / idx_out NaN / -1.
 *   workspace >= bark_acquisition_scan_fitted_workspace_bytes(R, m, Bc, C, P, variant) (0 for a refused shape or variant):
 *   the codes of at most 65536 candidates for Bc forests, Bc (R (R + 1) / 2 + R) doubles when the LDS variant runs,
 *   3 C + C / 128 doubles, and with P > 0 the pending codes and Bc R^2 doubles of scratch.
 * bark_leaf_posterior_condition_hip: the state conditioned in place on P more points, in the order given — the downdates
 *   of the pending entry point applied to the state's M^-1 (w does not change).  Conditioning on P1 points and then on P2
 *   is, bit for bit, conditioning on the P1 + P2 in that order, and a later plain scan equals the stateless scan with those
 *   pending points.  This is the step between the picks of a greedy batch: one downdate per forest instead of a refit.
 *   0 <= P <= 64 per call.  An invalid categorical value in a point sets info_out and the state's status to -1: that state's
 *   M^-1 is no longer meaningful.  Forests whose status is non-zero are left alone.
 *   workspace >= bark_leaf_posterior_condition_workspace_bytes(R, m, Bc, P): the pending codes.
 * bark_leaf_posterior_observe_hip: the state conditioned in place on P more points WITH values — observations or fantasies —
 *   in the order given.  Per forest and point, z the one-hot row of the point, every update seeing the ones before it:
 *       t = M^-1 z        q = z't        s = z'w        mu = c s        v = (scale / m) q + s2     (predictive of the observation)
 *       w <- w + t (y* - mu) / (1 + c q)        M^-1 <- M^-1 - (c / (1 + c q)) t t'        logpred += -1/2 ( log v + (y* - mu)^2 / v )
 *   which is exactly the state a refit on the data plus (points, y*) gives, and logpred = MLL(data + new) - MLL(data) in the
 *   convention without the 2 pi term.  t, q and the rewrite of M^-1 are the condition call's operations in its order, so M^-1
 *   ends with the bits bark_leaf_posterior_condition_hip leaves; s sums w over the point's leaves in code-bit order from 0.0
 *   (the scan's order for mu).  y* of point p under forest b, by mode:
 *     BARK_OBSERVE_VALUES  values[b value_stride + p]: value_stride = 0 for one (P,) vector shared by all forests, P for (B, P).
 *       With y* = mu this is the condition call; a constant is the "constant liar".
 *     BARK_OBSERVE_SAMPLE  mu + sqrt(v) e: by the chain rule the P values are one joint draw from the forest's predictive at
 *       the P points (noise included).  e = eps[b P + p] when eps (B, P) is given; otherwise Box-Muller on Philox4x32-10 with
 *       key = (seed low word, seed high word ^ 0x66616E74 "fant") and counter = (b, draw, p / 2, 0), u1 / u2 / r / th as for the
 *       sample paths below: even p takes r cos th, odd p takes r sin th.  A fantasy is a function of (seed, b, draw, p) and
 *       the state only, not of Bc.  values is ignored in this mode.
 *   values_out (B, P) or NULL: the values used.  logpred_out (B,) or NULL: logpred summed over p = 0 .. P-1 in that order.
 *   Forests whose status is non-zero are left alone and their rows of both outputs are NaN.  The values are not read back: a
 *   NaN or infinite value gives a NaN w and nothing is reported.  An invalid categorical value in a point sets info_out and
 *   the state's status to -1, as for the condition call.  0 <= P <= 64 per call; P = 0 launches nothing but the copy of the
 *   status into info_out and writes neither output.  0 <= draw < 2^32.
 *   workspace >= bark_leaf_posterior_observe_workspace_bytes(R, m, Bc, P): the codes of the points.
 *   Refused with BARK_ERR_ARG before any launch, beside the limits below: points == NULL with P > 0, an unknown mode,
 *   BARK_OBSERVE_VALUES without values, a value_stride other than 0 or P.
 * Weighted forest samples.  After an observation the B forests are still a sample of the OLD tree posterior; the exact
 * correction is one importance weight per forest, w_b <- w_b p_b(y_new | data), with p_b the predictive density that
 * bark_leaf_posterior_observe_hip writes into logpred_out while it updates the state.  Three entry points make the state a
 * weighted sample; none of them changes a result of the entry points above.
 * bark_forest_weights_hip: l_b = log_w_in[b] + increment[b] (a NULL array counts as zeros), M = max_b l_b,
 *   S = sum_b exp(l_b - M), log_w_out[b] = l_b - M - log S, w_out[b] = exp(log_w_out[b]) and
 *   stats_out = { M + log S, 1 / sum_b w_out[b]^2, max_b w_out[b] }: the log normaliser (for a predictive increment the log
 *   predictive density of the weighted mixture, when log_w_in is normalised), the effective sample size, the largest weight.
 *   A forest is dead — l_b = -inf, log_w_out[b] = -inf, w_out[b] = 0 — when info[b] != 0 (info (B,) int32 or NULL), when its
 *   increment is not finite or when its log_w_in is not finite (-inf: dead before).  If no forest is alive stats_out[0] is
 *   -inf and every other output is NaN; the caller keeps its old weights.  One workgroup of 256 threads: thread t folds the
 *   forests t, t + 256, ... in that order, the 256 values meet in a xor butterfly per wave and one LDS stage of four.  The
 *   order depends on B alone, so two runs give the same bits.  No atomics.  All arrays device, fp64 except info; the outputs
 *   must not overlap the inputs.  1 <= B <= 2^24.  No workspace.
 * bark_acquisition_scan_fitted_weighted_hip: bark_acquisition_scan_fitted_hip with `weights` (device, (B,), non-negative, summing to 1:
 *   the caller normalises).  Every per-forest term of the scan is multiplied by weights[b] before it is added — the three
 *   sums of the confidence bounds, so kind 1 gets the weighted moments mu = sum_b w_b mu_b, var = sum_b w_b (var_b + mu_b^2)
 *   - mu^2, and the one sum of the target kinds — and the finish does not divide by B.  A forest whose weight is exactly 0.0 is
 *   skipped whole by the scan (no table, no leaf lists, no arithmetic) and its status is ignored: info_out still reports it,
 *   but only a failed forest of non-zero weight makes best_out / idx_out NaN / -1.  With one weight 1.0 and the others 0.0 the
 *   result has the bits of the plain scan of that forest alone (1.0 t and 0.0 + t are exact, nothing is divided).  Pending
 *   points condition the scratch copy of every forest whatever its weight; skip_idx, targets, variant and Bc behave as above,
 *   and the result does not depend on Bc.  weights == NULL is bark_acquisition_scan_fitted_hip itself, bit for bit: the
 *   equal-weight kernels run.  The weights are not read back: a negative or NaN weight gives a meaningless result and no
 *   status.  The workspace is that of the unweighted call.
 * bark_leaf_posterior_gather_hip: state_out (layout of bark_leaf_posterior_bytes(R, m, n)) row k = state_in row index[k], for
 *   M^-1 (R^2 doubles), w (R doubles) and the status word, k < n; repeats and any order allowed.  index: DEVICE int64 (n,).
 *   The entry copies it to the host and refuses an entry outside [0, B_in) before the kernel is launched, so the call
 *   synchronises the stream once.  Loads and stores are 16 bytes wide where both row bases are 16-byte aligned, with the last
 *   element alone when R^2 is odd, and 8 bytes wide otherwise (R odd puts every other matrix 8 bytes off).  Refused with
 *   BARK_ERR_ARG: a null pointer, R outside 1 .. 8192, n outside 1 .. 65535, a state that is not 256-byte aligned, and
 *   state_in / state_out that overlap anywhere in their bark_leaf_posterior_bytes extents.  noise, scale, the packed forests
 *   and the weights are the caller's to gather.
 * Limits, refused with BARK_ERR_ARG before any launch: those of bark_acquisition_scan_targets_hip; a state buffer smaller
 * than bark_leaf_posterior_bytes or not 256-byte aligned.  The calls only enqueue; the queries are pure host code.
 * ------------------------------------------------------------------------------------- */
size_t bark_leaf_posterior_bytes(int64_t max_bits, int64_t m, int64_t B);
size_t bark_leaf_posterior_fit_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc);
int bark_leaf_posterior_fit_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                                const double *y, const double *noise, const double *scale, void *state, size_t state_bytes,
                                int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream);
size_t bark_acquisition_scan_fitted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P, int variant);
int bark_acquisition_scan_fitted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                     const double *scale, const void *state, size_t state_bytes, const double *cand, int64_t C,
                                     const double *pending /* (P, d) or NULL */, int64_t P,
                                     const int64_t *skip_idx /* (n_skip,) or NULL */, int64_t n_skip,
                                     const double *targets /* (B, S) or NULL for kinds 0 / 1 */, int64_t S, double kappa, int kind,
                                     int variant, double *acq_out /* (C,) or NULL */, double *best_out /* 1 */,
                                     int64_t *idx_out /* 1 */, int32_t *info_out /* (B,) */, void *workspace,
                                     size_t workspace_bytes, int64_t Bc, void *stream);
size_t bark_leaf_posterior_condition_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P);
int bark_leaf_posterior_condition_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                      const double *scale, const double *pending /* (P, d) */, int64_t P, void *state,
                                      size_t state_bytes, int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes,
                                      int64_t Bc, void *stream);
#define BARK_OBSERVE_VALUES 0
#define BARK_OBSERVE_SAMPLE 1
size_t bark_leaf_posterior_observe_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P);
int bark_leaf_posterior_observe_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                    const double *scale, const double *points /* (P, d) */, int64_t P,
                                    const double *values /* (P,) or (B, P) or NULL */, int64_t value_stride, int mode,
                                    const double *eps /* (B, P) or NULL */, uint64_t seed, int64_t draw, void *state,
                                    size_t state_bytes, double *values_out /* (B, P) or NULL */,
                                    double *logpred_out /* (B,) or NULL */, int32_t *info_out /* (B,) */, void *workspace,
                                    size_t workspace_bytes, int64_t Bc, void *stream);

int bark_forest_weights_hip(const double *log_w_in /* (B,) or NULL */, const double *increment /* (B,) or NULL */,
                            const int32_t *info /* (B,) or NULL */, int64_t B, double *log_w_out /* (B,) */, double *w_out /* (B,) */,
                            double *stats_out /* 3 */, void *stream);
size_t bark_acquisition_scan_fitted_weighted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P,
                                                             int variant);
int bark_acquisition_scan_fitted_weighted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d,
                                              const double *noise, const double *scale, const void *state, size_t state_bytes,
                                              const double *cand, int64_t C, const double *pending /* (P, d) or NULL */, int64_t P,
                                              const int64_t *skip_idx /* (n_skip,) or NULL */, int64_t n_skip,
                                              const double *targets /* (B, S) or NULL for kinds 0 / 1 */, int64_t S, double kappa,
                                              int kind, int variant, const double *weights /* (B,) or NULL */,
                                              double *acq_out /* (C,) or NULL */, double *best_out /* 1 */, int64_t *idx_out /* 1 */,
                                              int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes, int64_t Bc,
                                              void *stream);
int bark_leaf_posterior_gather_hip(const void *state_in, int64_t B_in, int64_t R, const int64_t *index /* device (n,) */, int64_t n,
                                   void *state_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Information gain of a (query, target) pair from a fitted posterior: which fidelity is worth paying for.  The reference
 * (information_based_fidelity.py:16-36, 90-167) makes the fidelity an input feature; given a proposed x it asks, per fidelity l,
 * how much observing f(x, l) tells about the minimum f* of the target-fidelity function, and divides by the cost.
 * BARK_ACQ_MES above is the l = target half; this entry point is the whole of it.  It reads the state of
 * bark_leaf_posterior_fit_hip and does not know which column is the fidelity:
 *   query  (C, d) device: query[c] is the point that would be evaluated;
 *   target (C, d) device: target[c] is the point whose function's minimum the draws targets[b][s] ((B, S) device) describe.
 * Per forest b and pair c, with a_0 < a_1 < ... the leaves of query[c] and b_0 < b_1 < ... those of target[c] (code-bit order):
 *   mu_m, var_m of query[c] and mu_0, var_0 of target[c] exactly as the scan forms mu_b(x), var_b(x) (same sums, same order);
 *   cov = (scale_b / m) sum_i sum_j (M_b^-1)[a_i][b_j], i in the outer loop, j in the inner loop, one accumulator from 0.0:
 *   the posterior covariance of the two values, one more bilinear form in the M^-1 of the state;
 *   sd = sqrt(max(var, 0)); E, Phi, phi as for BARK_ACQ_MES.  Grid parameters (lo, hi, n_a, pad, G); the reference's are
 *   (-10, 10, 100, 0.25, 250).  The rules, in this order:
 *   1. sd_m == 0: g = -inf, as for BARK_ACQ_MES.
 *   2. the two leaf lists are equal (query[c] == target[c] among others): g = (1/S) sum_s of the BARK_ACQ_MES g on
 *      (mu_m, sd_m, t_s), s = 0 .. S-1 — the same device function as the scan's, so the bits are the scan's.
 *      DEVIATION: the reference decides this by `fidelity == 0`, per call; here every forest decides for itself.  A forest
 *      whose trees do not separate the two points sees ONE random variable, whose entropy given f* is the closed form; the
 *      reference's quadrature with s^2 = 0 only approximates it.
 *   3. otherwise (the reference's _entropy_low_fidelity with its guards):
 *        H1 = log(sd_m E),  s2 = var_0 - cov^2 / (var_m + 1e-9),  u(f) = mu_0 + cov (f - mu_m) / (var_m + 1e-9)
 *        Psi_s(f) = Phi((t_s - u(f)) / (sqrt(max(s2, 0)) + 1e-9)) phi((f - mu_m) / (sd_m + 1e-9))
 *        Z_s = 1 / (Phi((t_s - mu_0) / (sd_0 + 1e-9)) sd_m + 1e-10)
 *      support: f_k = lo + k (hi - lo) / (n_a - 1), k live when sum_s |Psi_s(f_k)| > 1e-8; fmin = min live f_k - pad,
 *        fmax = max live f_k + pad; no live k: g = NaN (the reference would raise).
 *      quadrature: f_j = fmin + j (fmax - fmin) / (G - 1), y_{s,j} = xlogy(z, z) with z = Z_s Psi_s(f_j) (0 at z == 0),
 *        I_s the uniform trapezoid of y_{s,.}, H2 = -(1/S) sum_s I_s, g = H1 - H2.
 *      max(s2, 0) is a guard the reference lacks (it takes the root of a negative s2 and asserts on the NaN).
 *      The quotients by sd_m + 1e-9, sd_0 + 1e-9 and sqrt(max(s2, 0)) + 1e-9 are products with one reciprocal per pair.
 *   gain_out[c] = sum_b wgt_b g_{b,c}: with weights == NULL the plain sum over b divided once by B (as the scan's finish does);
 *   with weights (device, (B,), normalised by the caller) every g is multiplied by weights[b] before it is added, nothing is
 *   divided, and a forest of weight exactly 0.0 is skipped whole, as in the weighted scan.  The gain is not negated: the
 *   caller maximises it.  per_forest_out (B, C) or NULL: g_{b,c} itself; NaN rows for skipped and for failed forests.
 * Order (part of the contract).  Forests strictly b = 0 .. B-1 across chunks.  Inside a separated pair: the sum over s of
 *   |Psi_s(f_k)| runs s = 0 .. S-1; at every quadrature point j the column q_j = sum_s y_{s,j} runs s = 0 .. S-1; one wave of
 *   64 lanes owns the pair, lane l adds w_j q_j (w = 1/2 at j = 0 and G - 1, else 1) for j = l, l + 64, ... in that order from
 *   0.0, the 64 lane sums meet in a xor butterfly (offsets 32, 16, 8, 4, 2, 1), the result is multiplied by (fmax - fmin) /
 *   (G - 1) and divided by S.  The result therefore does not depend on Bc, bit for bit, and two runs give the same bits.
 * info_out[b]: the state's status, or -1 for an invalid categorical value in query or target; a non-zero entry of a forest
 *   of non-zero weight makes every gain NaN.
 * Limits, refused with BARK_ERR_ARG before any launch (and before the context is looked at): m <= 64, R <= 8192,
 *   1 <= C <= 65536, 1 <= S <= 1024, 2 <= n_a <= 1024, 2 <= G <= 4096, lo < hi and pad >= 0, all finite; a null query, target,
 *   targets or gain_out; then the fitted calls' (state size and alignment).  The call only enqueues: no allocation, no host
 *   synchronisation.  M^-1 is read from global memory.
 * workspace >= bark_fidelity_gain_fitted_workspace_bytes(R, m, Bc, C, S) (pure host code; 0 for a refused shape): the codes
 *   of the 2 C points for Bc forests, 7 Bc C + C doubles.  S is checked but adds nothing: the targets stay where they are.
 * ------------------------------------------------------------------------------------- */
size_t bark_fidelity_gain_fitted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t S);
int bark_fidelity_gain_fitted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                  const double *scale, const void *state, size_t state_bytes, const double *query /* (C, d) */,
                                  const double *target /* (C, d) */, int64_t C, const double *targets /* (B, S) */, int64_t S,
                                  const double *weights /* (B,) or NULL */, double lo, double hi, int64_t n_a, double pad,
                                  int64_t G, double *gain_out /* (C,) */, double *per_forest_out /* (B, C) or NULL */,
                                  int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sample paths from a fitted posterior (Thompson sampling).  A tree kernel has finite rank, so a posterior draw of forest b
 * is exactly a table of R leaf weights, W ~ N(c_b w_b, (scale_b / m) M_b^-1), and the sample path is the function
 * f(x) = sum_t W[col_t(x)]: once the table exists it is evaluated anywhere, later, with m gathers per point.
 * A path is a pair (forest b, draw number s).  The path list is given as two HOST arrays, path_forest (P,) int32,
 * non-decreasing, entries in [0, B), and path_draw (P,) int32 >= 0; both are read before the call returns.  A forest that
 * does not occur costs nothing: it is neither factorised nor walked.
 * bark_leaf_posterior_paths_hip: for path p with b = path_forest[p], s = path_draw[p]
 *     W_out[p, :] = c_b w_b + sqrt(scale_b / m) G_b eps[p, :]          c_b = scale_b / (m s2_b) as everywhere above
 *   with G_b the lower Cholesky factor (positive diagonal, hence unique) of the state's M_b^-1 — after
 *   bark_leaf_posterior_condition_hip the conditioned matrix, so paths of a conditioned state respect the pending points.
 *   Every forest that occurs is factorised once per call.  Row a of the product is sum_{k <= a} G[a][k] eps[p][k].
 *   eps: (P, R) device, row p the standard normals of path p; or NULL: entry a of path (b, s) is then Box-Muller on
 *   Philox4x32-10 with key = (seed low word, seed high word ^ 0x70617468 "path") and counter = (b, s, a / 2, 0): with
 *   u1, u2 the block's two 64-bit draws (words (0, 1) and (2, 3), u = (x >> 11) 2^-53), r = sqrt(-2 log(1 - u1)) and
 *   th = 6.283185307179586 u2, the even entry is r cos th and the odd one r sin th.  A path is therefore a function of
 *   (seed, b, s) and the state only: not of P, of the other paths, of any chunking or of a launch shape.
 *   info_out[b]: the state's status; or k > 0 when pivot k (1-based) of the factorisation of M_b^-1 is not positive.  The rows
 *   of a forest with a non-zero info_out are NaN.  state / noise / scale / info as for the calls above (no packed forests).
 *   Route: bark_leaf_posterior_paths_plan(R, m, &route, &max_leaves), pure host code, answers which factorisation a shape
 *   takes and its limit.  There is one route, BARK_PATHS_ROUTE_BLOCKED: one workgroup per forest, left-looking over column
 *   panels of 32, the 32 x 32 tiles through LDS and the factor in the workspace; it takes R <= 2048 (one CU does R^3 / 3
 *   flops) and m <= 64.  Anything else is BARK_ERR_ARG from the plan and from the call, before any launch; never rerouted.
 *   workspace >= bark_leaf_posterior_paths_workspace_bytes(R, m, B, P, eps == NULL): the run table, min(P, B, 256 MiB / 8 R^2)
 *   factors of R^2 doubles (more forests are factorised in rounds) and, without eps, the P R normals.
 * bark_path_scan_hip: W (P, R) device — rows as W_out above, any values — evaluated at cand (C, d) device:
 *     f[p, x] = sum_{t = 0 .. m-1} W[p][col_t^{b(p)}(x)]
 *   the trees summed strictly in the order t = 0 .. m-1 starting from 0.0 (the order of bark_posterior_samples_hip), so the
 *   value depends on no launch shape and a host loop reproduces it bit for bit.  reduce = BARK_SAMPLE_FULL: f_out (P, C).
 *   BARK_SAMPLE_MAX / MIN: red_out (P,) the extreme over the candidates of those same bits and idx_out (P,) int64 its index
 *   (ties: the lowest); fixed-order partials per workgroup of 256 candidates, then the finish kernel of
 *   bark_posterior_samples_hip; no floating-point atomics.  Candidates are walked in slabs of at most 65536, only under the
 *   forests that occur, at most 16 consecutive forests per walk.  info_out[b]: 0, or -1 when a walk that covered forest b met
 *   an invalid categorical value (the forests walked together share the flag); the results of such a forest's paths are NaN
 *   / -1.  A path whose value is NaN (a NaN row of W) has idx_out = -1.
 *   workspace >= bark_path_scan_workspace_bytes(R, m, P, C, reduce): the run table, the codes of one slab for the forests of
 *   one walk, and for MAX / MIN 16 bytes per (path, 256 candidates).
 * Limits, refused with BARK_ERR_ARG before any launch: 1 <= P <= 4096 per call, 1 <= C <= 2^24, the plan's, a path list that
 * is not non-decreasing or names a forest outside [0, B), a negative draw number, a short or misaligned state.  The byte
 * queries return 0 for a refused shape and are pure host code.  The calls only enqueue, after copying the run table through
 * the context's staging page (which waits for an earlier staged copy of the same context, nothing else).
 * ------------------------------------------------------------------------------------- */
#define BARK_PATHS_ROUTE_BLOCKED 1
int bark_leaf_posterior_paths_plan(int64_t max_bits, int64_t m, int *route_out, int64_t *max_leaves_out);
size_t bark_leaf_posterior_paths_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t P, int normals);
int bark_leaf_posterior_paths_hip(bark_ctx *ctx, const bark_pack_info *info, const double *noise, const double *scale,
                                  const void *state, size_t state_bytes, const int32_t *path_forest /* host (P,) */,
                                  const int32_t *path_draw /* host (P,) */, int64_t P, const double *eps /* (P, R) or NULL */,
                                  uint64_t seed, double *W_out /* (P, R) */, int32_t *info_out /* (B,) */, void *workspace,
                                  size_t workspace_bytes, void *stream);
size_t bark_path_scan_workspace_bytes(int64_t max_bits, int64_t m, int64_t P, int64_t C, int reduce);
int bark_path_scan_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d,
                       const int32_t *path_forest /* host (P,) */, const double *W /* (P, R) */, int64_t P, const double *cand,
                       int64_t C, int reduce, double *f_out /* (P, C) or NULL */, double *red_out /* (P,) */,
                       int64_t *idx_out /* (P,) */, int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * Predictive scores: how well the forest samples predict targets y_c at C points, in the same leaf space and again without
 * (B, C) arrays — what the reference's bark.utils.metrics (gaussian_log_likelihood, nlpd, mse; metrics.py:5-39) gives when fed
 * forest_predict's output, per forest and for the equally weighted mixture of the forests.  With
 *   l_bc = log N(y_c; mu_bc, var_bc) = -0.5 log(2 pi var_bc) - 0.5 (y_c - mu_bc)^2 / var_bc:
 *   per_forest_out[b] = ( sum_c l_bc,  sum_c (y_c - mu_bc)^2 )                                     (B, 2)
 *   mixture_out       = ( sum_c log( (1/B) sum_b exp l_bc ),  sum_c (y_c - (1/B) sum_b mu_bc)^2 )  (2,)
 *   values_out        = the two per-point terms of mixture_out, (2, C), or NULL
 * so the reference's nlpd column of forest b is -per_forest_out[b][0] / C.
 * mode = BARK_SCORE_HELDOUT: points (C, d) are held-out inputs; mu_bc and var_bc are those of forest_predict(diag=True), i.e.
 *   the scan's mu_b(x) and var_b(x) above, formed the same way (var is the latent variance: no noise is added).
 * mode = BARK_SCORE_LOO: points must be the training inputs X and y_points the training targets y (C == N is checked; the
 *   contents are the caller's responsibility).  (mu_bi, var_bi) is the leave-one-out predictive of observation i: with
 *   K_s = scale K + s2 I the matrix the leaf-space MLL factors (s2 = 1e-6 + noise), alpha = K_s^-1 y, kappa_i = [K_s^-1]_ii,
 *       mu_i = y_i - alpha_i / kappa_i,   var_i = 1 / kappa_i.
 *   From K_s^-1 = (I - c Z M^-1 Z') / s2 (Woodbury, c = scale / (m s2), M = I_R + c Z'Z, w = M^-1 Z'y) and z_i the one-hot
 *   row of point i:   kappa_i = (1 - c q_i) / s2,  q_i = z_i' M^-1 z_i;   alpha_i = (y_i - c z_i'w) / s2,  z_i'w = sum_k w[a_k],
 *   hence             mu_i = y_i - (y_i - c sum_k w[a_k]) / (1 - c q_i),   var_i = s2 / (1 - c q_i):
 *   the two per-point sums of the scan, evaluated at the training points; no N x N matrix is formed.  var_i is the variance of
 *   the observation (it contains s2), unlike the held-out latent variance.
 * Order (part of the contract): a point's leaves in code-bit order; the log-sum-exp over forests is the online recurrence
 *   top = max(mx, l), se = se exp(mx - top) + exp(l - top), mx = top  (mx = -inf, se = 0 before forest 0),  result mx + log(se / B),
 * over b = 0 .. B-1 across chunks; sums over points run by a fixed tree within each tile of 256 points (xor butterfly in a
 * wave, then waves 0 .. 3) and over the tiles in index order.  No float atomics: the results depend neither on Bc nor on the
 * variant, bit for bit.
 * A forest with info_out[b] != 0 leaves NaN in its row of per_forest_out and in both entries of mixture_out; the other rows are
 * what a call without that forest gives.  A NaN in y_points propagates into every sum its point enters.  var <= 0 is not
 * clamped: the logarithm then yields NaN or an infinity, which propagates likewise (a posterior variance is positive unless
 * rounding wins, as noise -> 0).
 * variant and its plan, and the limits refused with BARK_ERR_ARG before any launch, are the scan's: m <= 64, R <= 8192,
 * 1 <= C <= 2^24, variant = 1 where the LDS does not hold the table; also an unknown mode and, for BARK_SCORE_LOO, C != N.
 * The call only enqueues.  Extra memory: the scan's, plus 2 (Bc + 1) ceil(C / 256) doubles of tile partials.
 * ------------------------------------------------------------------------------------- */
#define BARK_SCORE_HELDOUT 0
#define BARK_SCORE_LOO 1
size_t bark_predictive_scores_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C);
int bark_predictive_scores_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                               int64_t d, const double *y, const double *noise, const double *scale, const double *points,
                               int64_t C, const double *y_points /* (C,) */, int mode, int variant,
                               double *per_forest_out /* (B, 2) */, double *mixture_out /* 2 */,
                               double *values_out /* (2, C) or NULL */, int32_t *info_out /* (B,) */, void *workspace,
                               size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Predictions from a fitted posterior: what a surrogate is asked for first.  The state of bark_leaf_posterior_fit_hip, as
 * bark_leaf_posterior_condition_hip / bark_leaf_posterior_observe_hip left it, read at C points (points (C, d) device) under
 * the forest weights w_b: weights (device, (B,), non-negative, summing to 1: the caller normalises) or NULL for 1 / B each.
 * Per forest b and point c, mu_bc and var_bc are the scan's mu_b(x) and var_b(x) above, formed the same way (the latent
 * variance); with observation = 1, var_bc + s2_b (s2 = 1e-6 + noise): the predictive of an observation.  Outputs:
 *   moments_out (2, C)       mean_c and var_c of the weighted mixture sum_b w_b N(mu_bc, var_bc), i.e. what the reference's
 *                            mixture_of_gaussians_as_normal gives for equal weights, by West's weighted one-pass recurrence over
 *                            the forests with w_b != 0 in forest order, from W = mean = S = V = 0:
 *                                W += w;  delta = mu - mean;  mean += (w / W) delta;  S += (w delta)(mu - mean);  V += w var
 *                            mean_c = mean, var_c = (V + S) / W: the law of total variance without the cancellation of
 *                            sum w (var + mu^2) - mean^2 (y is not standardised here).  Every operation as written, rounded once.
 *                            With one weight 1.0 and the others 0.0, mean_c = mu_bc and var_c = var_bc exactly.
 *   forest_out (2, B, C)     mu_bc then var_bc, or NULL.
 *   quantiles_out (Q, C)     for probs[q] = p the t with F_c(t) = sum_b w_b (1/2) erfc(-(t - mu_bc) / (sd_bc sqrt 2)) = p,
 *                            sd_bc = sqrt(max(var_bc, 0)); a forest with sd_bc = 0 is a step at mu_bc.  probs and zscores are HOST
 *                            arrays (Q,), zscores[q] = Phi^-1(probs[q]) (the caller's; it only places the bracket); both are read
 *                            before the call returns.  Bracket: lo = min_b, hi = max_b of mu_bc + z sd_bc over the forests with
 *                            w_b != 0; F(lo) >= p gives lo, F(hi) < p gives hi, so one live forest gives mu + z sd itself.  Inside,
 *                            a Newton step on the mixture density, kept strictly inside a bracket that every evaluation tightens
 *                            (bisection otherwise), until the step no longer moves t or no double lies between the ends.  F is
 *                            summed over b = 0 .. B-1 from 0.0 and reads only the stored mu_bc, var_bc and w_b.
 *   per_forest_out (B, 2), mixture_out (2,), values_out (2, C) or NULL: the predictive scores of y_points (device, (C,))
 *                            as defined for bark_predictive_scores_hip, mode BARK_SCORE_HELDOUT, on mu_bc, var_bc above, with
 *                            the weighted mixture:  log sum_b w_b exp l_bc  by the same online recurrence on l_bc + log w_b,
 *                            result mx + log(se), and (y_c - mean_c)^2 with the recurrence's mean.  With weights == NULL the
 *                            recurrence runs on l_bc, the results are mx + log(se / B) and (y_c - (sum_b mu_bc) / B)^2: the
 *                            arithmetic of bark_predictive_scores_hip, whose bits a call on the freshly fitted state returns.
 * Order (part of the contract): a point's leaves in code-bit order, forests b = 0 .. B-1 across chunks, the sums over points
 *   by the tile tree and tile order of bark_predictive_scores_hip.  No float atomics.  No result depends on Bc or on the
 *   variant, bit for bit, the quantiles included.
 * A forest whose weight is exactly 0.0 is skipped whole and its status ignored, as in bark_acquisition_scan_fitted_weighted_hip;
 *   its rows of forest_out and per_forest_out are NaN.  info_out[b]: the state's status, or -1 for an invalid categorical value
 *   met by a walk of this call.  A non-zero entry of a forest of non-zero weight makes every entry of moments_out,
 *   quantiles_out, mixture_out and values_out's sums NaN and its own rows of forest_out and per_forest_out NaN; the other rows
 *   are what a call without that forest gives.  The weights are not read back: a negative or NaN weight gives a meaningless
 *   result and no status.
 * Limits, refused with BARK_ERR_ARG before any launch (and before the context is looked at): those of the fitted scan
 *   (m <= 64, R <= 8192, 1 <= C <= 2^24, a state buffer of bark_leaf_posterior_bytes aligned to 256, variant = 1 only where the
 *   LDS holds the table); 0 <= Q <= 16; a probs[q] outside (0, 1) or not finite, a zscores[q] not finite; probs or zscores NULL
 *   with Q > 0; quantiles_out NULL with Q > 0 or given with Q = 0; moments_out or points NULL; y_points, per_forest_out and
 *   mixture_out given in part; values_out without them; observation other than 0 or 1.  Nothing is rerouted.  The call only
 *   enqueues: no allocation, no host synchronisation.
 * workspace >= bark_leaf_posterior_predict_workspace_bytes(R, m, B, Bc, C, Q, want_forest, want_scores, variant) (pure host
 *   code; 0 for a refused shape): the codes of one slab of at most 65536 points for Bc forests, the LDS image of Bc forests
 *   when that variant runs, 4 C doubles and a flag word; with want_scores 3 C + 2 (B + 1) ceil(C / 256) doubles more; with
 *   Q > 0 and no forest_out (want_forest = 0), 2 B min(C, 65536) doubles for mu_bc, var_bc of one slab.
 * ------------------------------------------------------------------------------------- */
size_t bark_leaf_posterior_predict_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t Bc, int64_t C, int64_t Q,
                                                   int want_forest, int want_scores, int variant);
int bark_leaf_posterior_predict_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                    const double *scale, const void *state, size_t state_bytes, const double *points /* (C, d) */,
                                    int64_t C, const double *weights /* (B,) or NULL */, int observation,
                                    const double *y_points /* (C,) or NULL */, const double *probs /* host (Q,) */,
                                    const double *zscores /* host (Q,) */, int64_t Q, int variant, double *moments_out /* (2, C) */,
                                    double *forest_out /* (2, B, C) or NULL */, double *quantiles_out /* (Q, C) or NULL */,
                                    double *per_forest_out /* (B, 2) or NULL */, double *mixture_out /* 2 or NULL */,
                                    double *values_out /* (2, C) or NULL */, int32_t *info_out /* (B,) */, void *workspace,
                                    size_t workspace_bytes, int64_t Bc, void *stream);

/* ---------------------------------------------------------------------------------------
 * Joint covariance from a fitted posterior: the one quantity of the state that is not marginal.  The state of
 * bark_leaf_posterior_fit_hip, as bark_leaf_posterior_condition_hip / bark_leaf_posterior_observe_hip left it, read at the C1
 * points x1 (C1, d) and the C2 points x2 (C2, d) (device) under the forest weights w_b: weights (device, (B,), normalised by
 * the caller) or NULL for 1 / B each.  With z(x) the one-hot leaf row of x (m ones) the posterior covariance of the latent
 * values at x and x' under forest b is
 *     cov_b(x, x') = (scale_b / m) z(x)' M_b^-1 z(x')       ( = scale_b K(x, x') - scale_b K(x, X) K_s^-1 scale_b K(X, x') )
 * the bilinear form of bark_fidelity_gain_fitted_hip's `cov`, for every pair of a C1 x C2 block.  Nothing of size N is read.
 * Per forest b and pair (i, j), with a_0 < a_1 < ... the leaves of x1[i] and b_0 < b_1 < ... those of x2[j] (code-bit order):
 *     T_b[i][r]   = sum_k (M_b^-1)[a_k][r]                 k in order, one accumulator from 0.0
 *     cov_b[i][j] = (scale_b / m) sum_l T_b[i][b_l]        l in order, one accumulator from 0.0, then the one product
 *   Two stages (part of the contract): m row sums per x1 point, then m gathers per entry, instead of m^2 reads per entry.
 *   The diagonal of a symmetric call therefore agrees with bark_leaf_posterior_predict_hip's var_bc (which sums the upper
 *   triangle, dg + 2 off) to rounding, not bit for bit; and cov_b[i][j] agrees with the fidelity gain's `cov` of the same pair to
 *   rounding (that sum runs over single entries, these over row sums).
 * Symmetric call, x2 == NULL: x2 = x1 and C2 = C1 (the C2 argument is ignored).  The entries with i >= j are computed by the
 *   rule above as row i and column j, and entry (j, i) is a copy of entry (i, j): the output is symmetric in bits, and its lower
 *   triangle has the bits of the general call with x2 = x1.  Only the tiles of that triangle are computed.
 * observation = 1 (the symmetric call only): s2_b = 1e-6 + noise_b is added to the diagonal of cov_b before anything else uses
 *   it: the covariance of observations at the points.  Two different evaluations share no noise, so there is no such term
 *   between x1 and a given x2, even where a row of x2 equals a row of x1.
 * Outputs (at least one):
 *   forest_out (B, C1, C2)   cov_b, or NULL.
 *   mixture_out (C1, C2)     the covariance of the weighted mixture by the law of total covariance in a two-pass form that
 *                            does not cancel.  mean_i and mean_j are the means of bark_leaf_posterior_predict_hip's recurrence
 *                            at x1[i] and x2[j] (the same kernel: predict's bits), mu_bi the scan's mu_b(x1[i]), and
 *                                mixture[i][j] = ( sum_b w_b ( cov_b[i][j] + (mu_bi - mean_i) (mu_bj - mean_j) ) ) / W,  W = sum_b w_b
 *                            both sums over the forests with w_b != 0 in forest order b = 0 .. B-1 across chunks, from 0.0,
 *                            every operation as written, rounded once.  With one weight 1.0 and the others 0.0,
 *                            mixture == cov_b exactly.  Or NULL: then no mean is formed.
 * Order (part of the contract): as above; no float atomics.  No result depends on Bc or on the variant, bit for bit.
 * A forest whose weight is exactly 0.0 is skipped whole and its status ignored; its block of forest_out is NaN.  info_out[b]: the
 *   state's status, or -1 for an invalid categorical value met by a walk of this call.  A non-zero entry of a forest of
 *   non-zero weight makes every entry of mixture_out NaN and its own block of forest_out NaN; the other blocks are what a call
 *   without that forest gives.  The state is not modified.  The weights are not read back.
 * variant: 1 keeps T_b of a workgroup's 32 rows in LDS (32 R doubles beside the leaf lists of its 32 + 64 points) and gathers
 *   from there; 2 keeps no T and sums every T_b[i][b_l] it needs from M^-1 in global memory, in the same order.  0 takes 1 where
 *   bark_acquisition_plan does: a table of R (R + 1) / 2 + R doubles that fits a CU's LDS means R <= 200, and then 32 R doubles
 *   and the lists stay below 64 KiB, so two workgroups share a CU.  One plan for every reader of the state; variant = 1 past
 *   it is refused.
 * Limits, refused with BARK_ERR_ARG before any launch (and before the context is looked at): those of the fitted scan (m <= 64,
 *   R <= 8192, a state buffer of bark_leaf_posterior_bytes aligned to 256, the plan's variant); 1 <= C1, C2 <= 65536 (one slab of
 *   codes per side); forest_out and mixture_out both NULL; observation other than 0 or 1; observation = 1 with x2 given; x1
 *   NULL.  Nothing is rerouted.  The call only enqueues: no allocation, no host synchronisation.
 * workspace >= bark_leaf_posterior_covariance_workspace_bytes(R, m, B, Bc, C1, C2, symmetric, want_forest, want_mixture,
 *   variant) (pure host code; 0 for a refused shape; symmetric != 0: C2 is ignored): the codes of the C1 + C2 points (C1 when
 *   symmetric) for Bc forests and a flag word; with want_mixture (4 + 2 B) doubles per point; without want_forest the chunk's
 *   blocks, Bc C1 C2 doubles.
 * ------------------------------------------------------------------------------------- */
size_t bark_leaf_posterior_covariance_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t Bc, int64_t C1, int64_t C2,
                                                      int symmetric, int want_forest, int want_mixture, int variant);
int bark_leaf_posterior_covariance_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                       const double *scale, const void *state, size_t state_bytes, const double *x1 /* (C1, d) */,
                                       int64_t C1, const double *x2 /* (C2, d) or NULL */, int64_t C2,
                                       const double *weights /* (B,) or NULL */, int observation, int variant,
                                       double *forest_out /* (B, C1, C2) or NULL */, double *mixture_out /* (C1, C2) or NULL */,
                                       int32_t *info_out /* (B,) */, void *workspace, size_t workspace_bytes, int64_t Bc,
                                       void *stream);

/* ---------------------------------------------------------------------------------------
 * Woodbury / determinant-lemma updates — quick_inverse.py:13-33 (the per-tree step of the sampler,
 * bark_sampler.py:233-257).  With mul = -1 if `subtract` else +1:
 *   K_out         = K_inv - K_inv U (mul I + U' K_inv U)^-1 U' K_inv          (low_rank_inv_update)
 *   logabsdet_out = log|det(I + mul U' K_inv U)|                              (low_rank_det_update adds K_logdet)
 * K_inv, K_out: (N, N) device (K_out may alias K_inv or be NULL); U: (N, r) device, r <= 64;
 * logabsdet_out: device scalar or NULL.  `symmetric != 0` promises K_inv == K_inv' and saves one pass.
 * ------------------------------------------------------------------------------------- */
size_t bark_lowrank_workspace_bytes(int64_t N, int64_t r);
int bark_lowrank_update_hip(const double *K_inv, int64_t N, const double *U, int64_t r, int subtract, int symmetric,
                            double *K_out, double *logabsdet_out, void *workspace, size_t workspace_bytes,
                            void *stream);
/* *singular_out (HOST) = 1-based column of the first exactly-zero pivot of (mul I + U' K_inv U) met by the last
 * bark_lowrank_update_hip / swap evaluation that used `workspace` with this (N, r), or 0.  Synchronises `stream`.
 * The reference's np.linalg.solve / slogdet raise LinAlgError there (quick_inverse.py:19,31). */
int bark_lowrank_status_hip(void *workspace, int64_t N, int64_t r, int32_t *singular_out, void *stream);

/* Fused tree swap for the sampler's per-tree step (bark_sampler.py:233-257): the reference chains
 * subtract(U_old) -> add(U_new) -> mll on K_inv (about nine passes over the N x N matrix) before it can
 * accept or reject.  With U = [U_old U_new] (N x (r_old + r_new), r_old + r_new <= 64), C = diag(-I, +I):
 *   eval : ONE pass, Y = K_inv U; scalars_out[0] = v'(C+G)^-1 v  (v = Y'y, G = U'Y)  so that
 *          y'K'^-1 y = y'K^-1 y - scalars_out[0];   scalars_out[1] = log|det(C+G)| = log|K'| - log|K|
 *   apply: K_out = K_inv - Y (C+G)^-1 Y'   from the workspace left by eval (accepted proposals only).
 * K_inv symmetric; workspace >= bark_lowrank_workspace_bytes(N, r_old + r_new). */
int bark_lowrank_swap_eval_hip(const double *K_inv, int64_t N, const double *U, int64_t r_old, int64_t r_new,
                               const double *y, double *scalars_out, void *workspace, size_t workspace_bytes,
                               void *stream);
int bark_lowrank_swap_apply_hip(const double *K_inv, int64_t N, int64_t r, void *workspace, double *K_out,
                                void *stream);

/* The same proposal evaluated straight from the two trees (bark_sampler.py:233-257 incl. get_leaf_vectors,
 * forest.py:70-75): `packed`/`info` = wire format of ONE forest made of the pair [old tree, new tree]
 * (bark_forest_pack, B = 1, m = 2).  The pair's one-hot leaf code is [U_old U_new] / s with one column per leaf
 * of each tree (unreached leaves give zero columns, which change neither scalar).  r_old = leaves of the old tree
 * (max_bits of bark_forest_pack_info on that tree alone), s = sqrt(scale / m).  scalars_out as above.  The
 * workspace (>= bark_tree_swap_workspace_bytes(N, info->max_bits)) begins with the swap_eval layout:
 * bark_lowrank_swap_apply_hip(K_inv, N, info->max_bits, workspace, K_out, stream) commits the proposal. */
size_t bark_tree_swap_workspace_bytes(int64_t N, int64_t r);
int bark_tree_swap_eval_hip(bark_ctx *ctx, const double *K_inv, int64_t N, const void *packed, const bark_pack_info *info,
                            const double *X, int64_t d, int64_t r_old, double s, const double *y, double *scalars_out,
                            void *workspace, size_t workspace_bytes, void *stream);

/* The proposals of several independent chains (bark_sampler.py:147) in one call.  K_inv: (nc, N, N) device;
 * packed/info: nc forests of two trees [old, new] (B = nc, m = 2); r_old, s: HOST arrays (nc); scalars_out: device
 * (nc, 2) as in bark_lowrank_swap_eval_hip; workspace: bark_tree_swap_chains_workspace_bytes(N, info->max_bits, nc)
 * bytes (nc per-chain blocks of *chain_stride_bytes, then the leaf codes of all chains).  1 <= nc <= 64.
 * With N even and at most 16 leaves per pair every kernel takes the chain index from its grid (one launch sequence
 * for all chains); otherwise each chain's single-chain sequence runs on its own stream forked from `stream`.
 * ..._apply_chains: K_inv[b] is rewritten in place for every b with accept[b] != 0 (HOST int32 array). */
size_t bark_tree_swap_chains_workspace_bytes(int64_t N, int64_t r, int64_t nc, size_t *chain_stride_bytes);
int bark_tree_swap_eval_chains_hip(bark_ctx *ctx, const double *K_inv, int64_t N, int64_t nc, const void *packed,
                                   const bark_pack_info *info, const double *X, int64_t d, const int64_t *r_old,
                                   const double *s, const double *y, double *scalars_out, void *workspace,
                                   size_t workspace_bytes, void *stream);
int bark_lowrank_swap_apply_chains_hip(double *K_inv, int64_t N, int64_t nc, int64_t r, const int32_t *accept,
                                       void *workspace, size_t workspace_bytes, void *stream);

/* One sweep over the trees of nc chains with the Metropolis decision taken on the DEVICE — the per-tree loop of
 * bark_sampler.py:233-264 without a host round trip per tree.  Step t < n_steps swaps one tree per chain:
 *   packed + packed_offsets[t] (bytes, HOST array), infos[t] (HOST array): wire format of the step's nc pairs
 *                                          [old tree, new tree]  (bark_forest_pack with B = nc, m = 2)
 *   r_old[t * nc + b] (HOST)               leaves of chain b's old tree;  s[b] (HOST) = sqrt(scale_b / m)
 *   log_q_prior, log_u (DEVICE, (n_steps, nc))   proposal ratio and log of the uniform draw of bark_sampler.py:258
 * Per step: evaluate (as bark_tree_swap_eval_chains_hip), accept iff log_u <= min(log_q_prior + 0.5 (dquad - dlogdet), 0),
 * rewrite K_inv[b] of the accepted chains.  state (DEVICE, (nc, 2)): y'K^-1 y and log|K| per chain, updated in place.
 * accept_out (DEVICE int32, (n_steps, nc)): 1 accepted, 0 rejected, -1 singular r x r system (the reference raises
 * LinAlgError).  Nothing synchronises: the host reads accept_out and state once per sweep.
 * workspace >= bark_tree_swap_chains_workspace_bytes(N, r_max, nc, NULL) + 16 * nc bytes, r_max = max_t infos[t].max_bits. */
int bark_tree_sweep_chains_hip(bark_ctx *ctx, double *K_inv, int64_t N, int64_t nc, int64_t n_steps, const void *packed,
                               const int64_t *packed_offsets, const bark_pack_info *infos, const double *X, int64_t d,
                               const int64_t *r_old, const double *s, const double *y, const double *log_q_prior,
                               const double *log_u, double *state, int32_t *accept_out, void *workspace,
                               size_t workspace_bytes, void *stream);

/* The same sweep in ONE kernel launch for small N: one workgroup per chain keeps K_inv[b] in LDS (variant 1) or works on it in
 * global memory, where one workgroup's matrix stays in L2 (variant 2), and loops over the steps itself — walk, Y = K_inv U in
 * column form, the r x r system C + U'Y by elimination with partial pivoting, the decision above, the rewrite — with workgroup
 * barriers as its only synchronisation.  Opt-in: the sums run in another order than in bark_tree_sweep_chains_hip, so K_inv
 * agrees with that path to rounding, not bit for bit.  The rewrite gives entries (i, j) and (j, i) the same bits; K_inv must be
 * symmetric on entry (it is read by columns).
 * Limits: 1 <= N <= 512, 2 <= leaves per [old, new] pair <= 16, at most 64 packed nodes per tree (infos[t].stride: the pair is
 * walked in 2 KiB of LDS; a tree of 15 leaves has 29), 1 <= nc <= 64, 0 < r_old < r, and d small enough for the X rows to sit in
 * LDS beside the rest (N * (d | 1) * 8 bytes: d <= 9 beside K_inv at N = 128, d <= 21 at N = 512;
 * bark_tree_sweep_resident_query answers for a shape).  Anything else: BARK_ERR_ARG before any launch — use
 * bark_tree_sweep_chains_hip.
 * A single kernel cannot read the per-step HOST arrays, and *_hip entry points neither allocate nor copy, so the caller builds a
 * step table on the host and uploads it like `packed`:
 *   bark_tree_sweep_resident_table (host -> host) validates the limits and writes int64 words: per step
 *   {packed_offsets[t], infos[t].stride, infos[t].max_depth, infos[t].max_bits} (n_steps x 4), then r_old (n_steps x nc);
 *   packed_offsets must be multiples of 16.
 * state, accept_out, log_q_prior, log_u: as in bark_tree_sweep_chains_hip; s is a DEVICE array (nc,) here.  The call enqueues
 * exactly one kernel, does not synchronise and can be captured in a hipGraph.  The launch is sized for 16 leaves per pair (the
 * entry point sees no host copy of the steps), so the variant depends on N and d only.  workspace: bark_tree_sweep_resident_workspace_bytes bytes, not touched today. */
size_t bark_tree_sweep_resident_table_bytes(int64_t n_steps, int64_t nc);
int bark_tree_sweep_resident_table(const int64_t *packed_offsets, const bark_pack_info *infos, const int64_t *r_old,
                                   int64_t n_steps, int64_t nc, void *table_host_out);
size_t bark_tree_sweep_resident_workspace_bytes(int64_t N, int64_t r_max, int64_t nc);
int bark_tree_sweep_resident_hip(bark_ctx *ctx, double *K_inv, int64_t N, int64_t nc, int64_t n_steps, const void *packed,
                                 const void *table_dev, const double *X, int64_t d, const double *s_dev, const double *y,
                                 const double *log_q_prior, const double *log_u, double *state, int32_t *accept_out,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* Which instance a shape takes: *variant_out = 0 unsupported (returns BARK_ERR_ARG with the reason), 1 K_inv in LDS, 2 K_inv
 * through global memory; the launch's dynamic LDS and workgroup size.  Unsupported: N, d outside the limits above, r_max outside
 * 2..16, max_nodes_bytes (packed bytes of the largest pair, 2 * stride * 16) above 2048.  Among the supported shapes the variant
 * follows from N and d alone.  Pure host code: works without a GPU. */
int bark_tree_sweep_resident_query(int64_t N, int64_t r_max, int64_t d, int64_t max_nodes_bytes, int *variant_out,
                                   int64_t *lds_bytes_out, int *threads_out);

/* The other half of the sampler step — the noise/scale proposal of bark_sampler.py:266-282 — for the same nc chains, again
 * decided on the DEVICE.  packed/info: the nc CURRENT forests (info->B == nc, after the sweep's accepted trees were copied
 * in); new_noise, new_scale, log_q_prior, log_u: DEVICE (nc,).  Per chain b, in leaf space (one R x R sweep for all chains,
 * as bark_kernel_inverse_leafspace_hip with Bc = nc and BARK_MLL_INCLUDE_SCALE):
 *   new_mll = MLL of forest b at (new_noise[b], new_scale[b]);   cur_mll = 0.5 (-state[2b] - state[2b+1])
 *   accept iff log_u[b] <= log_q_prior[b] + (new_mll - cur_mll) and log_u[b] <= 0   (a NaN compares false: rejected)
 * accept_out (DEVICE int32, (nc,)):
 *    1  accepted: K_inv[b] = (I - c Z M^-1 Z') / s2 written in place, state[2b] = y'K^-1 y, state[2b+1] = -2 new_mll - state[2b]
 *    0  rejected — also whenever 1e-6 + new_noise[b] is not positive (new_mll is NaN)
 *   -1  I + c Z'Z met a non-positive pivot (e.g. a negative proposed scale; the reference has no such check, np.linalg.inv
 *       of a singular matrix raises LinAlgError)
 *   -2  a leaf walk met an invalid categorical value: every chain of the call (bark_ctx_status reads and clears the flag)
 * For every value but 1 no byte of K_inv[b] or state[b] is written, and the N x R and N x N passes of such a chain do not
 * run (their workgroups return at once; what that saves has not been measured).  Nothing synchronises; the host reads accept_out and
 * state once.  The caller keeps noise and scale and applies the mask.  Limits: 1 <= nc <= 64, m <= 1280 trees, R <= 8192
 * leaves, else BARK_ERR_ARG before anything is launched.
 * workspace >= bark_noise_scale_step_chains_workspace_bytes(N, info->max_bits, info->m, nc). */
size_t bark_noise_scale_step_chains_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t nc);
int bark_noise_scale_step_chains_hip(bark_ctx *ctx, double *K_inv, int64_t N, int64_t nc, const void *packed,
                                     const bark_pack_info *info, const double *X, int64_t d, const double *y,
                                     const double *new_noise, const double *new_scale, const double *log_q_prior,
                                     const double *log_u, double *state, int32_t *accept_out, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Leaf-space sampler chains — the same two halves of `_step_bark_sampler` (bark_sampler.py:233-264 the tree loop, :266-282 the
 * noise/scale proposal) on a chain state that never holds an N x N matrix: with Z the N x R one-hot leaf matrix, s2 = 1e-6 + noise,
 * c = scale / (m s2), M = I_R + c Z'Z and v = Z'y (the leaf-space block above), a chain keeps P = M^-1 (Rcap x Rcap), the
 * bit-planes of its leaves, v, q = v'Pv and log|M|.  Swapping a tree removes its r_old rows and columns of M and borders in the
 * r_new of the proposal:  O(R^2 r + R r N / 64) per proposal and about 8 Rcap^2 + Rcap N / 8 bytes per chain, whatever N is,
 * where bark_tree_sweep_chains_hip reads (and on accept rewrites) 8 N^2 bytes.  Opt-in: cond(M) ~ N scale / s2, so the path
 * loses digits as noise -> 0 like every leaf-space route; decisions and scalars agree with the dense
 * sweep to the project's bars at noise >= 1e-2.
 *
 * state: one opaque device block of bark_leafchain_bytes(N, Rcap, m, lcap, nc) bytes, nc chains of `chain_bytes` each, written by
 * ..._init_hip and updated in place by ..._sweep_hip / ..._noise_scale_hip; the five shape arguments must be those of init.
 *   Rcap  slots (rows of P) per chain: the leaves of the forest plus room to grow; unused slots are identity rows of P
 *   lcap  most leaves a tree may have (old or new)
 * Leaves are numbered per tree in the packer's order (bark_forest_pack, depth first, left child first); leaves that no point
 * reaches are kept (an identity row).  mstate (DEVICE, (nc, 2)): y'K_s^-1 y and log|K_s| per chain, as `state` of
 * bark_tree_sweep_chains_hip: 0.5 (-mstate[0] - mstate[1]) is quick_inverse.mll.
 * Limits, refused with BARK_ERR_ARG before any launch: 1 <= nc <= 64, m <= 64 trees, lcap <= 32, Rcap <= 1024, at most 64 packed
 * nodes per tree.  A leaf walk that meets an invalid categorical value sets the context's flag (bark_ctx_status).
 * Every ..._hip entry point enqueues ONE kernel (one workgroup per chain, workgroup barriers only), does not allocate or
 * synchronise, and can be captured in a hipGraph.  workspace >= bark_leafchain_workspace_bytes(...) for all of them.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int64_t state_bytes, chain_bytes, workspace_bytes; /* the state block, one chain of it, the scratch of a call */
    int32_t plane_words;                                /* uint64 words per bit-plane, ceil(N / 64) */
    int32_t workgroups, threads, launches_per_sweep;    /* launch shape of a sweep */
    int32_t max_chains, max_trees, max_leaves, max_slots, max_nodes; /* the limits above (filled even when the shape is refused) */
} bark_leafchain_plan;
/* Pure host code (works without a GPU): the limits, the bytes and the launch shape for a shape; BARK_ERR_ARG with the reason. */
int bark_leafchain_query(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc, int64_t d, bark_leafchain_plan *out);
size_t bark_leafchain_bytes(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc);           /* 0: shape refused */
size_t bark_leafchain_workspace_bytes(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc);
/* Initial state of every chain (bark_sampler.py:153-162 in leaf space): packed/info = the nc forests (B = nc, m trees);
 * nleaves (DEVICE int32, (nc, m)): leaves of every tree (bark_forest_pack_info of the tree alone); noise, scale (DEVICE, (nc,)).
 * Walks the forests, builds planes, v and M, inverts M.  info_out (DEVICE int32, (nc,)): 0, or -1 when M met a non-positive
 * pivot (a negative scale), or -2 when the leaf table does not fit the shape (nothing else of that chain is written). */
int bark_leafchain_init_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                            const void *packed, const bark_pack_info *info, const int32_t *nleaves, const double *X, int64_t d,
                            const double *y, const double *noise, const double *scale, double *mstate, int32_t *info_out,
                            void *workspace, size_t workspace_bytes, void *stream);
/* The tree loop of bark_sampler.py:233-264 for nc chains in one launch.  Step t swaps tree tree_index[t] of every chain:
 *   packed + packed_offsets[t], infos[t]: the step's nc NEW trees (bark_forest_pack with B = nc, m = 1); the old tree's slots
 *   are known from the tree index.  log_q_prior, log_u (DEVICE, (n_steps, nc)), accept_out (DEVICE int32, (n_steps, nc)):
 *   as in bark_tree_sweep_chains_hip — accept iff log_u <= log_q_prior + (mll' - mll) and log_u <= 0 (a NaN compares false);
 *   -1: P_TT or S met a non-positive pivot, the chain is latched for the rest of the sweep and not touched again.
 * The kernel cannot read host arrays, so the caller builds a step table and uploads it like `packed`:
 *   bark_leafchain_sweep_table (host -> host) validates the limits and writes int64 words: per step {packed_offsets[t],
 *   infos[t].stride, infos[t].max_depth, tree_index[t]}, then r_new (n_steps x nc, leaves of each new tree).  nleaves (HOST
 *   int32, (nc, m)) are the chains' present leaf counts: with them it checks that the free slots cover the sweep in the worst
 *   case over the accept masks (sum over trees of the largest leaf count the tree can have <= Rcap), else BARK_ERR_ARG — the
 *   device never overflows its slot stack.  On accept the new leaves reuse the old tree's slots, then pop free ones; a shrinking
 *   tree pushes its leftovers. */
size_t bark_leafchain_sweep_table_bytes(int64_t n_steps, int64_t nc);
int bark_leafchain_sweep_table(const int64_t *packed_offsets, const bark_pack_info *infos, const int64_t *tree_index,
                               const int64_t *r_new, const int32_t *nleaves, int64_t n_steps, int64_t nc, int64_t m, int64_t lcap,
                               int64_t Rcap, void *table_host_out);
int bark_leafchain_sweep_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                             int64_t n_steps, const void *packed, const void *table_dev, const double *X, int64_t d,
                             const double *y, const double *log_q_prior, const double *log_u, double *mstate,
                             int32_t *accept_out, void *workspace, size_t workspace_bytes, void *stream);
/* The noise/scale proposal of bark_sampler.py:266-282 from the resident planes (no walk): M at the proposed values is rebuilt in
 * the workspace and inverted.  new_noise, new_scale, log_q_prior, log_u (DEVICE, (nc,)); rule and codes of
 * bark_noise_scale_step_chains_hip: 1 accepted (P, log|M|, q, noise, scale and mstate replaced), 0 rejected (also whenever
 * 1e-6 + new_noise is not positive), -1 non-positive pivot (e.g. a negative scale).  For every value but 1 nothing is written. */
int bark_leafchain_noise_scale_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                                   const double *new_noise, const double *new_scale, const double *log_q_prior,
                                   const double *log_u, double *mstate, int32_t *accept_out, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* Canonical view of the state (tree-major, leaves in the packer's order) — what a later predict / draw path reads
 * (tree_gps.py:80-113 in leaf space): P_out (nc, Rcap, Rcap) = M^-1 of the chain's leaves, identity beyond them; v_out (nc, Rcap);
 * nleaves_out (DEVICE int32, (nc, m)). */
int bark_leafchain_export_hip(bark_ctx *ctx, const void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                              double *P_out, double *v_out, int32_t *nleaves_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Tree proposals — tree_proposals.py:187-256 (get_tree_proposal) for every (chain, tree) of a sweep in ONE launch, and the
 * commit of the accepted ones.  Forests are the reference's packed 26-byte records, (nc, m, L), in DEVICE memory.
 *   new_nodes    (nc, m, L) records: nodes.copy() with exactly the records grow / prune / change assign
 *   log_q_prior  (nc, m) fp64: tree_q_ratio + tree_prior_ratio; -inf for a rejected proposal (new tree = old tree)
 *   log_u        (nc, m) fp64: log of the uniform of bark_sampler.py:259
 *   detail       (nc, m, 4) int32: kind (0 grow, 1 prune, 2 change), node (-1: none), feature (-1: none), status
 *   status       0 valid | 1 no valid node | 2 invalid discrete split | 3 fewer than two inactive slots | 4 a grow would
 *                exceed max_leaves.  3 and 4 are rejected proposals (the reference raises OverflowError for 3).
 * Draws: Philox4x32-10, key = (seed low word, seed high word), counter = (chain_offset + chain, tree_offset + tree, sweep,
 * block); words (0,1) and (2,3) of a block are one 64-bit draw each, low word first, u = (x >> 11) * 2^-53:
 *   block 0: kind, node;  block 1: feature, threshold or mask;  block 2: accept.
 *   kind = searchsorted(cumsum(weights / sum), u);  node = valid[floor(u n)];  feature = floor(u d);
 *   categorical: 1 + floor(u (2^k - 2)) spread over the k set bits;  integer: lo + floor(u (hi - lo));  continuous:
 *   lo + u (hi - lo) in fp64, rounded to float32 on store;  every floor(u n) is capped at n - 1.
 * Limits (refused before any launch): 1 <= nc m <= 2^22, 1 <= L <= 256, 1 <= d <= 2^20, 1 <= max_leaves <= L, weights
 * non-negative and finite with a positive sum, 0 < alpha < 1, beta >= 0 and finite, 0 <= sweep < 2^32, offsets within 32 bits,
 * record buffers on even addresses and distinct.  bounds (d, 2) fp64 in the reference's bitmask encoding (categorical:
 * [0, mask]), feat_types (d) int64; both DEVICE.  One launch, no allocation, no synchronisation: capturable.
 * bark_tree_proposals_commit_hip: nodes[c, tree_index[t]] <- new_nodes[c, tree_index[t]] wherever accept[t, c] > 0 (the
 * (n_steps, nc) int32 tensor the sweeps write; tree_index DEVICE int64).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    double alpha, beta;
    double weights[3];    /* grow, prune, change; normalised by their sum */
    int64_t max_leaves;
    int64_t chain_offset; /* added to the chain / tree index in the counter: a sub-batch draws what the whole batch draws */
    int64_t tree_offset;
} bark_proposal_params;
typedef struct {
    int64_t nodes_bytes;  /* of one (nc, m, L) record buffer; 0 when the shape is refused */
    int32_t max_slots, max_features, max_proposals, threads, workgroups;
} bark_tree_proposals_plan;
int bark_tree_proposals_query(int64_t L, int64_t d, int64_t max_leaves, int64_t nc, int64_t m, bark_tree_proposals_plan *plan_out);
int bark_tree_proposals_hip(bark_ctx *ctx, const void *nodes, int64_t nc, int64_t m, int64_t L, const double *bounds,
                            const int64_t *feat_types, int64_t d, const bark_proposal_params *params, uint64_t seed, int64_t sweep,
                            void *new_nodes, double *log_q_prior, double *log_u, int32_t *detail, void *stream);
int bark_tree_proposals_commit_hip(void *nodes, const void *new_nodes, const int32_t *accept, const int64_t *tree_index,
                                   int64_t n_steps, int64_t nc, int64_t m, int64_t L, void *stream);

/* ---------------------------------------------------------------------------------------
 * Domain candidates — the search space of the reference's `propose` (optimizer/opt_core.py, proposals.py) as rows for the
 * acquisition scan.  The posterior of a tree kernel is piecewise constant: the thresholds of all trees of all forest samples
 * cut the range of every feature into cells, the acquisition takes one value on each product cell, and one representative
 * per cell stands for all of its points.  The cell table (built on the host, bark_amd/optimizer/domain.py; DEVICE memory here):
 *   cell_off (d + 1) int64: feature f owns the slots cell_off[f] .. cell_off[f + 1] - 1;  cell_rep (total) fp64.
 * bark_domain_candidates_hip writes rows first .. first + n - 1 of a conceptual candidate list into out (n, d) fp64, row-major:
 *   mode = BARK_DOMAIN_UNIFORM  continuous: lo + u (hi - lo), capped at hi;  integer: lo + floor(u (hi - lo + 1));  categorical:
 *                               the floor(u k)-th of the k set bits of the mask.  Reads bounds (d, 2) fp64 in the reference's
 *                               bitmask encoding and feat_types (d) int64, both DEVICE; the table may be NULL.
 *   mode = BARK_DOMAIN_CELLS    feature f takes cell_rep[cell_off[f] + floor(u cells_f)]: uniform over cells, not over volume.
 *   mode = BARK_DOMAIN_GRID     no draws: row i is the i-th element of the Cartesian product of the cells, feature d - 1 varying
 *                               fastest (itertools.product), decoded as mixed radix in 64-bit arithmetic.  The caller keeps
 *                               first + n within the grid.
 *   Draws: Philox4x32-10 as the tree proposals use it, key = (seed low word, seed high word ^ 0x646F6D61), counter = (i low
 *   word, i high word, round, block) with i the GLOBAL row index; feature f uses draw f of its row: block f / 2, word pair
 *   f % 2; every floor(u n) is capped at n - 1.  A row depends on (seed, round, i) only — not on first, n or the launch.
 *   bounds and feat_types are read in mode uniform only and may be NULL otherwise.
 * bark_domain_neighbours_hip: x (K, d) -> out (K total, d); row (k, j) is x[k] with the feature that owns slot j replaced by
 *   cell_rep[j] (moves inside the point's own cell are kept: the layout is fixed).
 * Limits (refused before any launch): 1 <= d <= 4096, d <= total <= 2^20, 0 <= n <= 2^32, first >= 0, 0 <= round < 2^32,
 * K total <= 2^24 (the scan's candidate limit), a null table where the mode reads it.  n == 0 / K == 0: nothing is launched.
 * One launch each, no allocation, no synchronisation: capturable.
 * ------------------------------------------------------------------------------------- */
#define BARK_DOMAIN_UNIFORM 0
#define BARK_DOMAIN_CELLS 1
#define BARK_DOMAIN_GRID 2
int bark_domain_candidates_hip(const int64_t *cell_off, const double *cell_rep, int64_t total, const double *bounds,
                               const int64_t *feat_types, int64_t d, int mode, uint64_t seed, int64_t round, int64_t first, int64_t n,
                               double *out, void *stream);
int bark_domain_neighbours_hip(const int64_t *cell_off, const double *cell_rep, int64_t total, int64_t d, const double *x, int64_t K,
                               double *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Domain repair — the reference's `propose` under the domain's linear input constraints (opt_core.py:90-99,
 * bofire_mixed/constraints.py:122-133, proposals.py:56-66,150-202: "the feasible point closest to the centre" of a cell), as one
 * step between "write rows" and "scan rows".  A cell is a box and moving a row inside its cell does not change one bit of its
 * acquisition value, so every row is moved inside its own cell to a point with A x <= b (or = b), or marked infeasible.
 *   The table: cell_off (d + 1) int64 as above, cell_lo / cell_hi (total) fp64 the USABLE closed interval of every cell (built by
 *   bark_amd/optimizer/domain.py `cell_boxes`: a continuous cell (a, b] that is not its feature's first starts at nextafter(a)),
 *   ascending and disjoint per feature; feat_types (d) int64.
 *   The constraints, CSR: row_ptr (K + 1) int64 rising from 0, col (nnz) int64 ascending per row, coef (nnz) fp64; row k means
 *   sum_f A_kf x_f <= b[k], or = b[k] where equality[k] != 0; tol (K) fp64 is the absolute slack of the final test.
 * Per row of rows (n, d) fp64, in place; a feature is TOUCHED when some row of A stores a coefficient for it:
 *   1. cell lookup: for every touched f, c = the first cell with x_f <= cell_hi[c] (binary search).  No such cell, x_f < cell_lo[c]
 *      or a NaN x_f: feasible_out = 0 and the row is left as it was.  Untouched features are neither read nor written.
 *   2. `passes` times, for k = 0 .. K - 1:  r = (sum_f A_kf x_f) - b_k, the sum from 0.0 over the row's stored coefficients in
 *      order, multiply and add rounded separately (no FMA).  While r > 0 (equality: r != 0), walk the row's coefficients in order:
 *      continuous x_f <- clamp(x_f - r / A_kf, lo_c, hi_c); integer (inequality rows only) x_f <- clamp(x_f - sign(A_kf)
 *      ceil(r / |A_kf|), lo_c, hi_c); r is recomputed by the full sum after every change.  A zero coefficient, and an integer
 *      feature of an equality row, moves nothing.
 *   3. feasible_out = AND_k (r_k <= tol_k), |r_k| <= tol_k for equality rows, r_k recomputed once more.  An infeasible row
 *      keeps what the passes left in it.
 * Sound, always: a row marked feasible satisfies every constraint within tol and lies in its original cell — its leaf codes, and
 *   so its acquisition value, are unchanged bit for bit.
 * Complete when the rows of A have pairwise disjoint supports (K = 1 included): a row is marked feasible whenever its cell passes
 *   the closed box test sum_f min(A_kf lo, A_kf hi) <= b_k (equality: min <= b_k <= max), up to the rounding that tol absorbs.
 * A heuristic when supports overlap: a later constraint can undo an earlier one, feasible cells can be missed; an infeasible
 *   point is never marked feasible.  No LP is built.
 * Limits (refused before any launch): 1 <= d <= 4096, d <= total <= 2^20, 0 <= n <= 2^32, 1 <= K <= 16, 1 <= passes <= 64, a
 * null pointer (rows and feasible_out may be NULL when n == 0, which launches nothing).  The constraint arrays are DEVICE memory
 * and cannot be read before the launch: the kernel marks EVERY row infeasible, and writes nothing else, when row_ptr does not
 * rise from 0 to at most 1024, a column lies outside 0 .. d - 1, more than 64 features are touched, or a touched feature's slice
 * of the table lies outside 0 .. total.  One launch, no allocation, no synchronisation: capturable.
 * ------------------------------------------------------------------------------------- */
int bark_domain_repair_hip(const int64_t *cell_off, const double *cell_lo, const double *cell_hi, int64_t total,
                           const int64_t *feat_types, int64_t d, const int64_t *row_ptr /* (K + 1) */,
                           const int64_t *col /* nnz, ascending per row */, const double *coef /* nnz */, const double *b,
                           const double *tol, const uint8_t *equality, int64_t K, int passes, double *rows /* (n, d) in/out */,
                           int64_t n, uint8_t *feasible_out /* (n) */, void *stream);

/* quick_inverse.py:37-38 mll(K_inv, K_logdet, y) = 0.5 * (-y' K_inv y - K_logdet), on device. */
int bark_quadform_hip(const double *K_inv, const double *y, int64_t N, double *out, void *stream);
/* out[b] = alpha * sum_i A[b * lda + i] * y[i] + beta * c[b] for b < B (c may be NULL) — e.g. log|K_s| =
 * -(y' K_s^-1 y) - 2 mll from the rows K_s^-1 y of the inverse export (opt_model.py:101) and the MLL vector. */
int bark_rowdot_hip(const double *A, int64_t B, int64_t N, int64_t lda, const double *y, double alpha, const double *c,
                    double beta, double *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mixture of Gaussians over forest samples — tree_gps.py:116-131 (mixture_of_gaussians_as_normal):
 *   E[Y] = mean_b mu_b ;  Var[Y] = mean_b (var_b + mu_b^2) - E[Y]^2
 * in two steps so that shards of samples on several GPUs combine with one all-reduce(sum) of `partial`:
 *   partial (2, C): [sum_b mu_b, sum_b (var_b + mu_b^2)] over the B local samples; finish divides by the global count.
 * ------------------------------------------------------------------------------------- */
int bark_mixture_partial_hip(const double *mu, const double *var, int64_t B, int64_t C, double *partial, void *stream);
int bark_mixture_finish_hip(const double *partial, double total, int64_t C, double *mean, double *var, void *stream);

/* Strided device-to-device copy of a rows x cols float64 block (hipMemcpy2DAsync): assembling [U_old U_new] from two
 * leaf-vector matrices (bark_sampler.py:233-236) without host arithmetic on device data. */
int bark_copy2d_hip(double *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols, void *stream);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU exchanges over RCCL — replaces nothing in the reference, which evaluates the forest samples
 * of `batched_forest_gram_matrix` (forest.py:92-98) one after the other in one process.  One process per GPU holds a
 * contiguous block of samples; the ONLY data that crosses GPUs is the (B,) vector of log-likelihoods
 * (examples/mcmc/mcmc_record_mll.py:72-74) and, for the posterior, the 2 C partial sums of the mixture moments
 * (tree_gps.py:116-131).  librccl is loaded at run time; every function fails with BARK_ERR_HIP when it is absent.
 *   bark_comm_unique_id   128 bytes, generated by ONE rank and handed to the others by the caller (socket, file, MPI ...)
 *   bark_comm_create      collective over `world` ranks: communicator of this rank on `device`
 *   bark_allgather_mll    out[r * n_local + i] = local_r[i] for every rank r (equal block sizes; device pointers; enqueued
 *                         on `stream`)
 *   bark_allreduce_f64    in place over all ranks: sum (op_max == 0) or maximum (op_max != 0) */
int bark_comm_unique_id(void *id_out);
int bark_comm_create(const void *id, int rank, int world, int device, void **comm_out);
void bark_comm_destroy(void *comm);
int bark_allgather_mll(void *comm, const double *local, int64_t n_local, double *out, void *stream);
int bark_allreduce_f64(void *comm, double *buf, int64_t n, int op_max, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BARK_HIP_H */
