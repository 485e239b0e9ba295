// Tree proposals of the sampler (reference: src/bark/fitting/tree_proposals.py:187-256 `get_tree_proposal`, with
// tree_traversal.py:29-86 and bit_operations.py:34-58), drawn on the device for every (chain, tree) of a sweep in ONE launch, and
// the commit that copies the accepted proposals over the resident forests.  include/bark_hip.h, "Tree proposals", has the
// contract; DESIGN.md section 9 the draw layout and the deviations.
//
// Mapping: one wave per (chain, tree), four waves per workgroup, no LDS, no barrier.  Lanes stride over the L slots of the
// container; __ballot / popcount give the valid nodes, the k-th of them and the first two inactive slots.  Everything that is
// one value per proposal (the draws, the ancestor walk, the two log-ratios) is computed by all 64 lanes on the same operands —
// loads of one address broadcast — so nothing has to be moved between lanes and lane 0 stores the results.  The feature is
// drawn before the walk, which therefore tracks one interval (or one category mask): no per-thread d x 2 array, no scratch.
//
// Records are the packed 26-byte structs of forest.py:8-19; a container starts on an even address (26 L is even), so records
// are read and written as 13 16-bit words.  The lane that owns a changed slot writes the changed record, every other record is
// copied as it is — stale fields of inactive slots and of a pruned node included, as nodes.copy() keeps them.
//
// Draws: Philox4x32-10, key = (seed low, seed high), counter = (chain, tree, sweep, block).  Word pairs (0,1) and (2,3) of a
// block are one 64-bit draw x each (low word first), u = (x >> 11) * 2^-53:
//   block 0: draw 0 kind, draw 1 node;  block 1: draw 2 feature, draw 3 threshold or mask;  block 2: draw 4 accept.
// A proposal's bits depend on (seed, sweep, chain, tree) only.
#include "common.h"
#include "philox.h"

#include <cmath>

namespace bark {
namespace {

constexpr int PR_MAX_L = 256;               // slots of a container: four ballots per pass
constexpr int PR_WORDS = PR_MAX_L / 64;
constexpr int PR_WAVES = 4;                 // proposals per workgroup
constexpr int64_t PR_MAX_PROPOSALS = (int64_t)1 << 22;
constexpr int64_t PR_MAX_D = (int64_t)1 << 20;
constexpr int FT_CAT = 0, FT_INT = 1;       // forest.py:22-25

struct Rec {  // one record as 13 halfwords; field offsets 0 | 1 5 9 13 17 21 | 25
    uint16_t h[13];
};
__device__ __forceinline__ Rec rec_load(const uint16_t *p) {
    Rec r;
#pragma unroll
    for (int k = 0; k < 13; ++k) r.h[k] = p[k];
    return r;
}
__device__ __forceinline__ void rec_store(uint16_t *p, const Rec &r) {
#pragma unroll
    for (int k = 0; k < 13; ++k) p[k] = r.h[k];
}
template <int OFF>  // OFF odd: the 32-bit field at byte OFF
__device__ __forceinline__ void rec_set32(Rec &r, uint32_t v) {
    constexpr int k = OFF / 2;
    r.h[k] = (uint16_t)((r.h[k] & 0x00ffu) | ((v & 0xffu) << 8));
    r.h[k + 1] = (uint16_t)(v >> 8);
    r.h[k + 2] = (uint16_t)((r.h[k + 2] & 0xff00u) | (v >> 24));
}
__device__ __forceinline__ void rec_set_is_leaf(Rec &r, uint32_t v) { r.h[0] = (uint16_t)((r.h[0] & 0xff00u) | (v & 0xffu)); }
__device__ __forceinline__ void rec_set_active(Rec &r, uint32_t v) { r.h[12] = (uint16_t)((r.h[12] & 0x00ffu) | ((v & 0xffu) << 8)); }

// field reads straight from the container (byte loads: fields sit on odd offsets)
__device__ __forceinline__ uint32_t rd8(const unsigned char *tree, uint32_t slot, int off) { return tree[(size_t)slot * NODE_BYTES + off]; }
__device__ __forceinline__ uint32_t rd32(const unsigned char *tree, uint32_t slot, int off) {
    const unsigned char *p = tree + (size_t)slot * NODE_BYTES + off;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
constexpr int O_LEAF = 0, O_FEAT = 1, O_THR = 5, O_LEFT = 9, O_RIGHT = 13, O_PARENT = 17, O_DEPTH = 21, O_ACTIVE = 25;

// philox, uniform53 and pick: philox.h
// k-th set bit (k < popcount) of a wave-uniform mask
__device__ __forceinline__ int kth_bit(uint64_t mask, int k) {
    for (int j = 0; j < k; ++j) mask &= mask - 1;
    return __builtin_ctzll(mask);
}

struct ProposeArgs {
    const unsigned char *nodes;
    unsigned char *new_nodes;
    const double *bounds;
    const int64_t *feat_types;
    double *log_q_prior, *log_u;
    int32_t *detail;
    int64_t nc, m, L, d, max_leaves;
    double alpha, beta, cum0, cum1;
    uint32_t k0, k1, sweep, chain0, tree0;
};

struct Patch {  // what grow / prune / change assign (tree_proposals.py:146-183)
    int kind;   // -1: nothing changes
    uint32_t node, left, right, feature, thr_bits, depth, parent;
};
// the new tree's view of a slot's flags and children, for the count of tree_proposals.py:107
__device__ __forceinline__ uint32_t new_is_leaf(const unsigned char *tree, const Patch &pt, uint32_t i) {
    if (i == pt.node) return 0;
    if (i == pt.left || i == pt.right) return 1;
    return rd8(tree, i, O_LEAF);
}

__global__ __launch_bounds__(64 * PR_WAVES) void propose_kernel(ProposeArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * PR_WAVES + (threadIdx.x >> 6);
    if (w >= p.nc * p.m) return;  // whole waves leave: no barrier follows
    const int64_t c = w / p.m, t = w % p.m;
    const int L = (int)p.L;
    const unsigned char *tree = p.nodes + (size_t)w * L * NODE_BYTES;
    unsigned char *out = p.new_nodes + (size_t)w * L * NODE_BYTES;

    uint32_t b0[4], b1[4], b2[4];
    const uint32_t cc = p.chain0 + (uint32_t)c, ct = p.tree0 + (uint32_t)t;
    philox(p.k0, p.k1, cc, ct, p.sweep, 0u, b0);
    philox(p.k0, p.k1, cc, ct, p.sweep, 1u, b1);
    philox(p.k0, p.k1, cc, ct, p.sweep, 2u, b2);
    const double u_kind = uniform53(b0[0], b0[1]), u_node = uniform53(b0[2], b0[3]);
    const double u_feat = uniform53(b1[0], b1[1]), u_thr = uniform53(b1[2], b1[3]);
    const double u_acc = uniform53(b2[0], b2[1]);

    // searchsorted(cumsum(weights), u) (tree_proposals.py:195), the last kind when rounding leaves the sum below u
    const int kind = u_kind <= p.cum0 ? 0 : (u_kind <= p.cum1 ? 1 : 2);

    // pass 1: terminal nodes, singly internal nodes, inactive slots (tree_traversal.py:29-46, tree_proposals.py:46-58)
    uint64_t term[PR_WORDS], single[PR_WORDS], idle[PR_WORDS];
#pragma unroll
    for (int q = 0; q < PR_WORDS; ++q) {
        const int i = q * 64 + lane;
        bool is_term = false, is_single = false, is_idle = false;
        if (q * 64 < L) {  // wave-uniform
            if (i < L) {
                const uint32_t act = rd8(tree, i, O_ACTIVE), leaf = rd8(tree, i, O_LEAF);
                is_idle = act == 0;
                is_term = (act & leaf) != 0;
                const uint32_t l = rd32(tree, i, O_LEFT), r = rd32(tree, i, O_RIGHT);
                if (l < (uint32_t)L && r < (uint32_t)L)  // a child outside the container: not a valid node (the reference would raise)
                    is_single = (act & (1u - leaf) & rd8(tree, l, O_LEAF) & rd8(tree, r, O_LEAF) & 0xffu) != 0;
            }
        }
        term[q] = __ballot(is_term), single[q] = __ballot(is_single), idle[q] = __ballot(is_idle);
    }
    int n_term = 0, n_single = 0, n_idle = 0;
#pragma unroll
    for (int q = 0; q < PR_WORDS; ++q) n_term += __popcll(term[q]), n_single += __popcll(single[q]), n_idle += __popcll(idle[q]);

    int status = 0;
    int32_t node = -1, feature = -1;
    Patch pt;
    pt.kind = -1, pt.node = pt.left = pt.right = 0xFFFFFFFFu, pt.feature = pt.thr_bits = pt.depth = pt.parent = 0;
    double lqp = -INFINITY;

    const int n_valid = kind == 0 ? n_term : n_single;
    if (n_valid == 0) {
        status = 1;  // tree_proposals.py:207
    } else {
        int k = (int)pick(u_node, n_valid);  // np.random.choice: uniform over the valid nodes in ascending slot order
#pragma unroll
        for (int q = 0; q < PR_WORDS; ++q) {
            const uint64_t msk = kind == 0 ? term[q] : single[q];
            const int cnt = __popcll(msk);
            if (node < 0 && k < cnt) node = q * 64 + kth_bit(msk, k);
            k -= cnt;
        }
        const uint32_t depth = rd32(tree, node, O_DEPTH);
        if (kind != 1) {
            // the rule (tree_proposals.py:78-97) on the node's subspace (tree_traversal.py:49-86), for the drawn feature alone
            feature = (int32_t)pick(u_feat, p.d);
            const int64_t ftype = p.feat_types[feature];
            double lo = p.bounds[2 * feature], hi = p.bounds[2 * feature + 1];
            uint32_t cur = (uint32_t)node;
            for (int hop = 0; hop < L && cur != 0; ++hop) {  // at most L ancestors: a parent cycle ends the walk
                const uint32_t par = rd32(tree, cur, O_PARENT);
                if (par >= (uint32_t)L) break;
                if (rd32(tree, par, O_FEAT) == (uint32_t)feature) {
                    const double thr = (double)__uint_as_float(rd32(tree, par, O_THR));
                    const bool is_left = cur == rd32(tree, par, O_LEFT);
                    if (ftype == FT_CAT) {
                        const int64_t avail = (int64_t)hi;
                        if (is_left) {
                            hi = (double)((int64_t)thr & avail);
                        } else {
                            int64_t full = 1;
                            while (avail >= full && full < ((int64_t)1 << 62)) full <<= 1;
                            hi = (double)((int64_t)((double)(full - 1) - thr) & avail);
                        }
                    } else if (is_left) {
                        hi = hi < thr ? hi : thr;  // min(thr, hi)
                    } else {
                        const double bound = thr + (ftype == FT_INT ? 1.0 : 0.0);
                        lo = lo > bound ? lo : bound;  // max(thr + int_delta, lo)
                    }
                }
                cur = par;
            }
            float thr_new;
            if (ftype == FT_CAT) {
                const uint64_t avail = (uint64_t)(int64_t)hi;
                const int nbits = __popcll(avail);
                uint64_t mask = 0;
                if (nbits >= 2) {  // bit_operations.py:34-58: a value in [1, 2^k - 2] spread over the set bits
                    uint64_t draw = 1 + (uint64_t)pick(u_thr, ((int64_t)1 << nbits) - 2);
                    for (uint64_t rest = avail; rest; rest &= rest - 1, draw >>= 1) mask |= (draw & 1) << __builtin_ctzll(rest);
                }
                thr_new = (float)mask;
                if (mask == 0) status = 2;  // tree_proposals.py:226-230
            } else if (ftype == FT_INT) {
                const int64_t ilo = (int64_t)lo, ihi = (int64_t)hi;
                if (lo == hi || ihi <= ilo) {
                    thr_new = (float)hi;
                    status = 2;  // the upper bound marks "no split" (tree_proposals.py:86-89, 232-236)
                } else {
                    thr_new = (float)(double)(ilo + pick(u_thr, ihi - ilo));  // always below hi
                }
            } else {
                thr_new = (float)(lo + u_thr * (hi - lo));
            }
            pt.feature = (uint32_t)feature, pt.thr_bits = __float_as_uint(thr_new);
        }
        if (status == 0 && kind == 0) {
            if (n_idle < 2) status = 3;                          // tree_proposals.py:58
            else if (n_term + 1 > p.max_leaves) status = 4;
        }
        if (status == 0) {
            pt.kind = kind, pt.node = (uint32_t)node, pt.depth = depth;
            // log(alpha) + 2 log(1 - alpha / (2 + depth)^beta) - log((1 + depth)^beta - alpha)   (tree_proposals.py:134-138)
            const double dd = (double)depth;
            const double prior = log(p.alpha) + 2.0 * log(1.0 - p.alpha / pow(2.0 + dd, p.beta)) + -log(pow(1.0 + dd, p.beta) - p.alpha);
            if (kind == 0) {
                int found = 0;
#pragma unroll
                for (int q = 0; q < PR_WORDS; ++q) {
                    uint64_t msk = idle[q];
                    while (msk && found < 2) {
                        (found == 0 ? pt.left : pt.right) = (uint32_t)(q * 64 + __builtin_ctzll(msk));
                        msk &= msk - 1, ++found;
                    }
                }
                pt.parent = rd32(tree, node, O_PARENT);
                // singly internal nodes of the grown tree (tree_proposals.py:105-109)
                int w1 = 0;
#pragma unroll
                for (int q = 0; q < PR_WORDS; ++q) {
                    const uint32_t i = (uint32_t)(q * 64 + lane);
                    bool is_single = false;
                    if (q * 64 < L && i < (uint32_t)L) {
                        const bool changed = i == pt.node || i == pt.left || i == pt.right;
                        const uint32_t act = changed ? 1u : rd8(tree, i, O_ACTIVE);
                        const uint32_t l = i == pt.node ? pt.left : ((i == pt.left || i == pt.right) ? 0u : rd32(tree, i, O_LEFT));
                        const uint32_t r = i == pt.node ? pt.right : ((i == pt.left || i == pt.right) ? 0u : rd32(tree, i, O_RIGHT));
                        if (l < (uint32_t)L && r < (uint32_t)L)
                            is_single = (act & (1u - new_is_leaf(tree, pt, i)) & new_is_leaf(tree, pt, l) & new_is_leaf(tree, pt, r) & 0xffu) != 0;
                    }
                    w1 += __popcll(__ballot(is_single));
                }
                lqp = (log((double)n_term) - log((double)w1)) + prior;
            } else if (kind == 1) {
                pt.left = rd32(tree, node, O_LEFT), pt.right = rd32(tree, node, O_RIGHT);  // inside the container: the node is singly internal
                lqp = (log((double)n_single) - log((double)(n_term - 1))) + -prior;
            } else {
                lqp = 0.0;
            }
        }
    }

    // the copy, with the changed records changed by the lane that owns them
    for (int i = lane; i < L; i += 64) {
        Rec r = rec_load(reinterpret_cast<const uint16_t *>(tree + (size_t)i * NODE_BYTES));
        if (pt.kind == 0) {
            if ((uint32_t)i == pt.left || (uint32_t)i == pt.right) {  // (1, 0, 0, 0, 0, node, depth + 1, 1)
                rec_set_is_leaf(r, 1), rec_set32<O_FEAT>(r, 0), rec_set32<O_THR>(r, 0), rec_set32<O_LEFT>(r, 0), rec_set32<O_RIGHT>(r, 0);
                rec_set32<O_PARENT>(r, pt.node), rec_set32<O_DEPTH>(r, pt.depth + 1), rec_set_active(r, 1);
            } else if ((uint32_t)i == pt.node) {  // (0, feature, threshold, left, right, parent, depth, 1)
                rec_set_is_leaf(r, 0), rec_set32<O_FEAT>(r, pt.feature), rec_set32<O_THR>(r, pt.thr_bits), rec_set32<O_LEFT>(r, pt.left);
                rec_set32<O_RIGHT>(r, pt.right), rec_set32<O_PARENT>(r, pt.parent), rec_set32<O_DEPTH>(r, pt.depth), rec_set_active(r, 1);
            }
        } else if (pt.kind == 1) {
            if ((uint32_t)i == pt.left || (uint32_t)i == pt.right) rec_set_active(r, 0);
            if ((uint32_t)i == pt.node) rec_set_is_leaf(r, 1);
        } else if (pt.kind == 2 && (uint32_t)i == pt.node) {
            rec_set32<O_FEAT>(r, pt.feature), rec_set32<O_THR>(r, pt.thr_bits);
        }
        rec_store(reinterpret_cast<uint16_t *>(out + (size_t)i * NODE_BYTES), r);
    }
    if (lane == 0) {
        p.log_q_prior[w] = lqp;
        p.log_u[w] = log(u_acc);  // bark_sampler.py:259
        p.detail[4 * w + 0] = kind, p.detail[4 * w + 1] = node, p.detail[4 * w + 2] = feature, p.detail[4 * w + 3] = status;
    }
}

// nodes[c, tree_index[t]] <- new_nodes[c, tree_index[t]] wherever accept[t, c] > 0; one workgroup per (t, c).  A tree named by
// two steps is copied from the same source twice.
__global__ __launch_bounds__(64) void commit_kernel(unsigned char *nodes, const unsigned char *new_nodes, const int32_t *accept,
                                                    const int64_t *tree_index, int64_t nc, int64_t m, int64_t L) {
    const int64_t t = blockIdx.x / nc, c = blockIdx.x % nc;
    if (accept[t * nc + c] <= 0) return;
    const int64_t k = tree_index[t];
    if (k < 0 || k >= m) return;
    const size_t base = (size_t)(c * m + k) * L * NODE_BYTES;
    const uint16_t *src = reinterpret_cast<const uint16_t *>(new_nodes + base);
    uint16_t *dst = reinterpret_cast<uint16_t *>(nodes + base);
    for (int64_t i = threadIdx.x; i < L * (NODE_BYTES / 2); i += 64) dst[i] = src[i];
}

int check_shape(const char *who, int64_t L, int64_t d, int64_t max_leaves, int64_t nc, int64_t m) {
    if (nc < 1 || m < 1 || nc > PR_MAX_PROPOSALS || m > PR_MAX_PROPOSALS || nc * m > PR_MAX_PROPOSALS)
        return fail(BARK_ERR_ARG, "%s: %lld chains x %lld trees are outside 1..2^22 proposals", who, (long long)nc, (long long)m);
    if (L < 1 || L > PR_MAX_L) return fail(BARK_ERR_ARG, "%s: a container of %lld slots is outside 1..%d", who, (long long)L, PR_MAX_L);
    if (d < 1 || d > PR_MAX_D) return fail(BARK_ERR_ARG, "%s: d = %lld is outside 1..2^20", who, (long long)d);
    if (max_leaves < 1 || max_leaves > L)
        return fail(BARK_ERR_ARG, "%s: max_leaves = %lld is outside 1..%lld (the container)", who, (long long)max_leaves, (long long)L);
    return BARK_OK;
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_tree_proposals_query(int64_t L, int64_t d, int64_t max_leaves, int64_t nc, int64_t m, bark_tree_proposals_plan *plan_out) {
    error_buffer()[0] = 0;
    if (!plan_out) return fail(BARK_ERR_ARG, "bark_tree_proposals_query: null argument");
    *plan_out = bark_tree_proposals_plan{};
    plan_out->max_slots = PR_MAX_L;
    plan_out->max_features = (int32_t)PR_MAX_D;
    plan_out->max_proposals = (int32_t)PR_MAX_PROPOSALS;
    plan_out->threads = 64 * PR_WAVES;
    const int rc = check_shape("tree proposals", L, d, max_leaves, nc, m);
    if (rc) return rc;
    plan_out->workgroups = (int32_t)((nc * m + PR_WAVES - 1) / PR_WAVES);
    plan_out->nodes_bytes = nc * m * L * NODE_BYTES;
    return BARK_OK;
}

int bark_tree_proposals_hip(bark_ctx *ctx, const void *nodes, int64_t nc, int64_t m, int64_t L, const double *bounds,
                            const int64_t *feat_types, int64_t d, const bark_proposal_params *params, uint64_t seed, int64_t sweep,
                            void *new_nodes, double *log_q_prior, double *log_u, int32_t *detail, void *stream) {
    error_buffer()[0] = 0;
    if (!params) return fail(BARK_ERR_ARG, "bark_tree_proposals_hip: null params");
    int rc = check_shape("tree proposals", L, d, params->max_leaves, nc, m);
    if (rc) return rc;
    if (!(params->alpha > 0.0 && params->alpha < 1.0)) return fail(BARK_ERR_ARG, "tree proposals: alpha = %g is outside (0, 1)", params->alpha);
    if (!(params->beta >= 0.0 && params->beta < INFINITY)) return fail(BARK_ERR_ARG, "tree proposals: beta = %g is negative or not finite", params->beta);
    double sum = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!(params->weights[k] >= 0.0 && params->weights[k] < INFINITY))
            return fail(BARK_ERR_ARG, "tree proposals: weight %d = %g is negative or not finite", k, params->weights[k]);
        sum += params->weights[k];
    }
    if (!(sum > 0.0 && sum < INFINITY)) return fail(BARK_ERR_ARG, "tree proposals: the weights sum to %g, not to a positive number", sum);
    if (sweep < 0 || sweep > 0xFFFFFFFFll) return fail(BARK_ERR_ARG, "tree proposals: sweep %lld is outside 0..2^32 - 1", (long long)sweep);
    if (params->chain_offset < 0 || params->tree_offset < 0 || params->chain_offset + nc > 0xFFFFFFFFll || params->tree_offset + m > 0xFFFFFFFFll)
        return fail(BARK_ERR_ARG, "tree proposals: chain / tree offsets leave the 32-bit counter words");
    rc = check_ctx(ctx);
    if (rc) return rc;
    if (!nodes || !bounds || !feat_types || !new_nodes || !log_q_prior || !log_u || !detail)
        return fail(BARK_ERR_ARG, "bark_tree_proposals_hip: null argument");
    if (((uintptr_t)nodes | (uintptr_t)new_nodes) & 1) return fail(BARK_ERR_ARG, "bark_tree_proposals_hip: record buffers must start on an even address");
    if (nodes == new_nodes) return fail(BARK_ERR_ARG, "bark_tree_proposals_hip: new_nodes must not be nodes");
    ProposeArgs a{};
    a.nodes = static_cast<const unsigned char *>(nodes), a.new_nodes = static_cast<unsigned char *>(new_nodes);
    a.bounds = bounds, a.feat_types = feat_types, a.log_q_prior = log_q_prior, a.log_u = log_u, a.detail = detail;
    a.nc = nc, a.m = m, a.L = L, a.d = d, a.max_leaves = params->max_leaves;
    a.alpha = params->alpha, a.beta = params->beta;
    // np.cumsum(p / p.sum()) of bark_sampler.py:41-46, in that order of operations
    a.cum0 = params->weights[0] / sum, a.cum1 = a.cum0 + params->weights[1] / sum;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.sweep = (uint32_t)sweep;
    a.chain0 = (uint32_t)params->chain_offset, a.tree0 = (uint32_t)params->tree_offset;
    hipLaunchKernelGGL(propose_kernel, dim3((unsigned)((nc * m + PR_WAVES - 1) / PR_WAVES)), dim3(64 * PR_WAVES), 0,
                       static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_tree_proposals_commit_hip(void *nodes, const void *new_nodes, const int32_t *accept, const int64_t *tree_index, int64_t n_steps,
                                   int64_t nc, int64_t m, int64_t L, void *stream) {
    error_buffer()[0] = 0;
    const int rc = check_shape("tree proposals commit", L, 1, 1, nc, m);
    if (rc) return rc;
    if (n_steps < 1 || n_steps * nc > PR_MAX_PROPOSALS)
        return fail(BARK_ERR_ARG, "tree proposals commit: %lld steps x %lld chains are outside 1..2^22", (long long)n_steps, (long long)nc);
    if (!nodes || !new_nodes || !accept || !tree_index || nodes == new_nodes)
        return fail(BARK_ERR_ARG, "bark_tree_proposals_commit_hip: null or aliased argument");
    if (((uintptr_t)nodes | (uintptr_t)new_nodes) & 1) return fail(BARK_ERR_ARG, "bark_tree_proposals_commit_hip: record buffers must start on an even address");
    hipLaunchKernelGGL(commit_kernel, dim3((unsigned)(n_steps * nc)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<unsigned char *>(nodes), static_cast<const unsigned char *>(new_nodes), accept, tree_index, nc, m, L);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
