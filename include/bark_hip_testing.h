/* bark_hip_testing.h — hooks for the test-suite only.  NOT part of the drop-in boundary (include/bark_hip.h): nothing on the
 * reference's side binds these, and they are inert unless the process was started with $BARK_TEST_HOOKS set (the variable is
 * read once, when libbarkhip.so is loaded; tests/conftest.py sets it). */
#ifndef BARK_HIP_TESTING_H
#define BARK_HIP_TESTING_H

#ifdef __cplusplus
extern "C" {
#endif

/* The k-th launch from now on whose status the library checks reports hipErrorLaunchFailure, so that the error-return paths —
 * helper streams forked, stream capture open — can be exercised on a healthy device (tests/test_gpu_context.py).  k <= 0
 * switches it off; returns the previous countdown.  Process-wide, hence a test hook: without $BARK_TEST_HOOKS it returns -1 and
 * does nothing, and the library's launch checks do not look at it. */
long bark_debug_fail_launch(long k);

/* Which kernel variants the front end takes for a shape: the leaf walks of N points of d features through the forests of `info`
 * (bark_leaf_codes_hip, bark_leaf_indices_hip) and the Gram fill of an N x M block from their codes into an output of row stride
 * `ld`, batch stride `batch_stride` (elements) and base address `out_mod16` modulo 16 (bark_gram_from_leaves_hip).  It is what
 * the launchers themselves decide from (walk_variant, gram_variant: traverse.hip, gram.hip), so a test can name "the plain walk"
 * or "the narrow tile" without restating a threshold, and stops reaching its variant loudly when a constant moves.  M enters only
 * through the Gram's output layout; for the walk of x2 query again with N = M.  Pure host code: no GPU, no state, and therefore
 * NOT gated by $BARK_TEST_HOOKS.  Requires bark_hip.h (bark_pack_info). */
typedef struct {
    int32_t encoding, words;   /* bark_leaf_encoding(info), bark_leaf_words(info) */
    int32_t codes_grouped;     /* codes: leaf_walk_grouped_kernel (a point's trees over 8 threads), else leaf_walk_kernel */
    int32_t codes_nodes_lds;   /* grouped: the forest's packed nodes are copied to LDS and walked there */
    int32_t codes_x_lds;       /* the point rows sit in LDS (always when grouped), else they are read from global memory */
    int32_t codes_workgroups;  /* grid of the one-thread-per-point kernel, the figure the grouped rule compares */
    int32_t indices_staged;    /* indices (MODE 0): point rows in LDS and results staged there in 32-tree chunks, else direct */
    int32_t gram_rep;          /* 0 = bytes with ids up to 255, 1 = bytes with ids < 128 (7-bit compare), 2 = one-hot bits */
    int32_t gram_tile_rows, gram_tile_cols; /* output tile of a Gram workgroup: 32 x 128 (wide) or 64 x 64 (narrow) */
    int32_t gram_vec2;         /* every output row starts on a 16-byte boundary: 16-byte stores throughout, else shifted pairs */
} bark_frontend_variant;
int bark_frontend_variant_query(const bark_pack_info *info, int64_t N, int64_t M, int64_t d, int64_t ld, int64_t batch_stride,
                                int out_mod16, bark_frontend_variant *out);

/* The sampler's Metropolis decision as every device path takes it (metropolis_accept, csrc/sampler_step.h), evaluated on the
 * host: 1 accept, 0 reject, for log(u), log_q_prior and new_mll - cur_mll.  Pure host code, NOT gated by $BARK_TEST_HOOKS. */
int bark_debug_metropolis(double log_u, double log_q_prior, double mll_delta);

#ifdef __cplusplus
}
#endif
#endif
