// What every device route of the sampler has to agree on, defined once (not part of the ABI): the Metropolis decision, the
// per-sweep step table of the two one-launch sweeps, the in-wave fence and the chain limit.  Included by lowrank.hip,
// sweep_resident.hip, leafchain.hip, leafspace.hip and leafsystem.hip.
#pragma once
#include "common.h"

namespace bark {
// chains of one call, on every route: the multi-launch and one-launch sweeps, the leaf-space chains, the noise/scale steps
constexpr int SAMPLER_MAX_CHAINS = 64;

// The Metropolis decision (bark_sampler.py:256-264, :266-282), for the tree proposals and the noise/scale proposals alike:
//   log_alpha = log_q_prior + (new_mll - cur_mll);   accept iff log(u) <= min(log_alpha, 0)
// with Python's min: min(nan, 0) is nan and rejects, and so does a NaN log_u.  fmin(NaN, 0) is 0 and would accept every such
// proposal, so the rule is written as two comparisons, each false on a NaN.  +inf for log_alpha accepts whenever log_u <= 0; the
// boundary log_u == log_alpha accepts.  The ChainBatch / LeafChainBatch front ends replace each other only while the multi-launch
// sweep (small_kernel's decide branch, decide_kernel), the one-launch sweep, the leaf-space sweep and both noise/scale steps
// decide by this one function.  A caller forms mll_delta itself, in the order of operations of its own path, and keeps its own
// codes around the call (-1 singular / latched / bad pivot, -2 categorical fault, the non-positive-noise reject).
__host__ __device__ __forceinline__ int metropolis_accept(double log_u, double log_q_prior, double mll_delta) {
    const double log_alpha = log_q_prior + mll_delta;
    return (log_u <= log_alpha && log_u <= 0.0) ? 1 : 0;
}
// One wave runs the small r x r algebra in LDS while the other waves of the workgroup wait at the next barrier: inside that
// wave LDS traffic is ordered by the fence (s_waitcnt) and the lanes run in lock step.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- step table of a one-launch sweep (bark_tree_sweep_resident_table, bark_leafchain_sweep_table), int64 words ----
//   step t:  [t * 4 ..]  byte offset of the step's nodes in the packed buffer, packed nodes per tree (stride), max depth, and one
//            word of the path's own (one-launch sweep: leaves of the [old, new] pair; leaf-space chains: index of the tree)
//   then a (steps, chains) column of leaf counts (one-launch sweep: r_old; leaf-space chains: r_new)
constexpr int STEP_TABLE_WORDS = 4;
// what a path packs per step, and the words of its refusals (the two builders grew apart in theirs; callers match on them)
struct StepPackRule {
    const char *path, *pack, *stride_tail;  // "one-launch sweep", "one [old, new] pair", what follows "at most %d"
    int m, stride_max;                      // trees per chain in a step's pack; packed nodes per tree that the kernel walks from LDS
    bool low_stride_with_range;             // stride < 1 is reported with the offset and the depth, not as a node count
};
// one step's pack: B, m, 1 <= stride <= stride_max, offset >= 0 and a multiple of 16, depth in 0..2^24; sets the error message
inline int step_pack_check(const StepPackRule &rule, int64_t t, int64_t offset, const bark_pack_info &in, int64_t nc) {
    if (in.B != nc || in.m != rule.m)
        return fail(BARK_ERR_ARG, "step %lld: pack %s per chain (B = chains, m = %d)", (long long)t, rule.pack, rule.m);
    if (in.stride > rule.stride_max || (in.stride < 1 && !rule.low_stride_with_range))
        return fail(BARK_ERR_ARG, "%s, step %lld: %lld packed nodes in a tree, at most %d%s", rule.path, (long long)t,
                    (long long)in.stride, rule.stride_max, rule.stride_tail);
    if (offset < 0 || offset % 16 != 0 || in.stride < 1 || in.max_depth < 0 || in.max_depth > (1 << 24))
        return fail(BARK_ERR_ARG, "step %lld: bad offset%s or depth", (long long)t, rule.low_stride_with_range ? ", stride" : "");
    return BARK_OK;
}
// word3: the path's own word of every step; null takes the pack's max_bits
inline void step_table_write(int64_t *out, const int64_t *offsets, const bark_pack_info *infos, const int64_t *word3,
                             const int64_t *column, int64_t n_steps, int64_t nc) {
    for (int64_t t = 0; t < n_steps; ++t, out += STEP_TABLE_WORDS)
        out[0] = offsets[t], out[1] = infos[t].stride, out[2] = infos[t].max_depth, out[3] = word3 ? word3[t] : infos[t].max_bits;
    for (int64_t e = 0; e < n_steps * nc; ++e) out[e] = column[e];
}
// step t of chain b as the kernels read it.  The builder checked every field; the stride is clamped all the same, so that a
// table from elsewhere never overruns the LDS that holds the nodes.  Clamps of word3 and column belong to the path.
struct StepEntry {
    int64_t offset;
    int stride, max_depth, word3, column;
};
__device__ __forceinline__ StepEntry step_entry(const int64_t *table, int t, int n_steps, int nc, int b, int stride_max) {
    const int64_t *hd = table + (size_t)t * STEP_TABLE_WORDS;
    return {hd[0], min(max((int)hd[1], 1), stride_max), (int)hd[2], (int)hd[3],
            (int)table[(size_t)n_steps * STEP_TABLE_WORDS + (size_t)t * nc + b]};
}
}  // namespace bark
