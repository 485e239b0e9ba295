// Host side of the leaf-space entry points: MLL and posterior, explicit inverse, joint draws, the acquisition scans, the
// predictive scores and the sampler's noise/scale step.  They factorise I_R + c Z'Z (R x R) instead of K_s (N x N).
// LeafSystem is what all of them share: one workspace layout (leaf_areas), one opening sequence and the per-chunk steps.  An
// entry point checks its own arguments, says what it keeps in the workspace (LeafNeeds), opens the system and hands
// for_chunks a body that lists the steps it takes.
// The kernels are elsewhere: the R x R Cholesky sweep in chol.hip (reached through SystemSweep, common.h), the leaf-space
// kernels in leafspace.hip, sample.hip, acquire.hip, scores.hip and predict.hip; this unit's only kernels move status words
// (fault_info_kernel, copy_info_kernel).
// A fitted posterior (bark_leaf_posterior_*_hip, bark_acquisition_scan_fitted_hip) is the part of that state which outlives
// a call: M^-1, w and the sweep's status of all B forests in a buffer of the caller's (PosteriorState).
#include <cmath>

#include "sampler_step.h"  // -> common.h

namespace bark {
namespace {

constexpr int64_t ACQ_SLAB = 1 << 16;  // candidates walked and scanned per launch pair: bounds the code buffer (Bc, W, slab)
constexpr int64_t ACQ_MAX_PENDING = 64, ACQ_MAX_SKIP = 64, ACQ_MAX_TARGETS = 1024;

// what a call keeps in its workspace besides the R x R sweep's own areas, the leaf codes of the N points and y'y
struct LeafNeeds {
    int64_t cand = 0;         // candidate columns whose one-hot codes are resident at a time
    bool identity = false;    // R identity columns appended to the sweep: it also yields V = U^-T, hence w = M^-1 v = V'z
    bool minv = false;        // ... and M^-1 = V'V itself (Bc, R, R)
    bool rowsum = false;      // the (Bc, N, R) row-sum scratch of the N x N expansion
    int64_t S = 0;            // S joint draws at the `cand` candidates: Wt (Bc, Rpad, Spad) and the partials of their max / min
    int64_t scan = 0;         // acquisition scan over this many candidates: LDS image (Bc, tri + R), running sums (3, scan) and
                              // the per-workgroup minima of the finish
    bool chain_step = false;  // noise/scale step: new_mll and the sweep's info (Bc each), K^-1 y (Bc, N)
    int64_t pending = 0;      // acquisition scan conditioned on this many pending points: their one-hot codes
    bool scores = false;      // predictive scores at the `scan` points: tile partials of the mixture sums (tiles, 2) and of the
                              // per-forest sums (Bc, tiles, 2)
};

// 256-byte aligned areas handed out front to back; base == nullptr: sizes only
struct Carve {
    char *base;
    size_t o = 0;
    template <class T> T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + o) : nullptr;
        o = align256(o + n * sizeof(T));
        return p;
    }
};

struct LeafAreas {
    // (the R x R sweep's workspace — N := R; candidates := the R identity columns — is at the front: system_sweep_bytes)
    int64_t R, Rpad, W, npad, cpad, Spad, ppad;
    uint32_t *codes, *ccodes;    // one-hot leaf codes of the N points / of the resident candidates (Bc, W, npad | cpad)
    uint32_t *pcodes;            // ... of the scan's pending points (Bc, W, ppad)
    unsigned long long *planes;  // bit planes of `codes` (Bc, 32 W, npad / 64)
    double *yy;                  // y'y
    double *Minv, *w, *Wm, *Wt;  // see LeafNeeds; an area the call does not need is empty
    double *tab, *acc;           // acquisition scan
    double *part;                // (value, index) partial results: of the draws' max / min, or of the scan's finish
    int64_t *part_i;
    double *spart;               // predictive scores: see LeafNeeds
    double *new_mll, *kinv_y;  // noise/scale step
    int32_t *sweep_info;
    size_t total;
};

// The whole workspace of a leaf-space call with Bc forests resident.  Every *_workspace_bytes function and every entry point
// gets its sizes and pointers here, so the two cannot disagree.
LeafAreas leaf_areas(void *workspace, int64_t N, int64_t R, int64_t m, int64_t Bc, const LeafNeeds &q) {
    LeafAreas a;
    a.R = R;
    a.Rpad = round_up(R, TILE);
    a.W = (R + 31) / 32;
    a.npad = round_up(N, TILE);
    a.cpad = q.cand > 0 ? round_up(q.cand, TILE) : 0;
    a.Spad = q.S > 0 ? sample_spad(q.S) : 0;
    a.ppad = q.pending > 0 ? round_up(q.pending, TILE) : 0;
    const size_t nb = (size_t)Bc;
    const size_t partials = nb * (q.S > 0 ? sample_partials(q.cand, q.S) : 0) + acq_partials(q.scan);
    Carve cv{static_cast<char *>(workspace), system_sweep_bytes(R, q.identity, m, Bc)};
    a.codes = cv.take<uint32_t>(nb * a.W * a.npad);
    a.planes = cv.take<unsigned long long>(nb * 32 * a.W * (a.npad / 64));
    a.yy = cv.take<double>(8);
    a.ccodes = cv.take<uint32_t>(nb * a.W * a.cpad);
    a.Minv = cv.take<double>(q.minv ? nb * R * R : 0);
    a.w = cv.take<double>(q.identity ? nb * R : 0);
    a.Wm = cv.take<double>(q.rowsum ? nb * N * R : 0);
    a.Wt = cv.take<double>(nb * a.Rpad * a.Spad);
    a.tab = cv.take<double>(q.scan > 0 ? nb * acq_table_doubles(R) : 0);
    a.acc = cv.take<double>((size_t)3 * q.scan);
    a.part = cv.take<double>(partials);
    a.part_i = cv.take<int64_t>(partials);
    a.new_mll = cv.take<double>(q.chain_step ? nb : 0);
    a.sweep_info = cv.take<int32_t>(q.chain_step ? nb : 0);
    a.kinv_y = cv.take<double>(q.chain_step ? nb * N : 0);
    a.pcodes = cv.take<uint32_t>(nb * a.W * a.ppad);
    a.spart = cv.take<double>(q.scores ? (nb + 1) * 2 * acq_partials(q.scan) : 0);
    a.total = cv.o;
    return a;
}

LeafNeeds mll_needs(int64_t C) {  // MLL; posterior at C candidates from w and M^-1
    LeafNeeds q;
    q.cand = C;
    q.identity = q.minv = C > 0;
    return q;
}
LeafNeeds inverse_needs() {  // explicit K_s^-1 = (I - c Z M^-1 Z') / sigma2
    LeafNeeds q;
    q.identity = q.minv = q.rowsum = true;
    return q;
}
LeafNeeds samples_needs(int64_t C, int64_t S) {  // draws need V and w, not M^-1 itself
    LeafNeeds q;
    q.cand = C;
    q.identity = true;
    q.S = S;
    return q;
}
LeafNeeds scan_needs(int64_t C, int64_t P) {  // the posterior's areas with the codes of one slab of candidates
    LeafNeeds q = mll_needs(C < ACQ_SLAB ? C : ACQ_SLAB);
    q.scan = C;
    q.pending = P;
    return q;
}
LeafNeeds fit_needs() {  // the sweep with the identity columns; w and M^-1 go straight into the caller's state
    LeafNeeds q;
    q.identity = true;
    return q;
}
LeafNeeds scores_needs(int64_t C) {  // the scan's areas (its three sums per point hold the mixture's state) and the tile partials
    LeafNeeds q = scan_needs(C, 0);
    q.scores = true;
    return q;
}
LeafNeeds chain_step_needs() {
    LeafNeeds q = inverse_needs();
    q.chain_step = true;
    return q;
}

// a leaf walk of this call met an invalid categorical value: every sample of the chunk reports it (info = -1)
__global__ void fault_info_kernel(const int32_t *fault, int32_t *info, int Bc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < Bc && *fault) info[b] = -1;
}

// status words from one place to another (a fitted state's and a call's info_out)
__global__ void copy_info_kernel(const int32_t *__restrict__ src, int32_t *__restrict__ dst, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) dst[b] = src[b];
}

// A fitted posterior in a buffer of the caller's: M^-1 (B, R, R), w (B, R), then the sweep's status per forest, each area
// 256-byte aligned.  bark_leaf_posterior_bytes and the entry points get sizes and pointers here.  base == nullptr: sizes only.
struct PosteriorState {
    double *Minv, *w;
    int32_t *info;
    size_t total;
};
PosteriorState posterior_state(void *base, int64_t R, int64_t B) {
    Carve cv{static_cast<char *>(base)};
    PosteriorState st;
    st.Minv = cv.take<double>((size_t)B * R * R);
    st.w = cv.take<double>((size_t)B * R);
    st.info = cv.take<int32_t>((size_t)B);
    st.total = cv.o;
    return st;
}
bool posterior_shape_ok(int64_t R, int64_t m, int64_t B) { return R >= 1 && R <= 8192 && m >= 1 && m <= ACQ_MAX_TREES && B >= 1; }

// The workspace of the calls that start from a fitted state (nothing of size N): the codes of one slab of candidates and of
// the pending points for Bc forests, the LDS image when that variant runs, the scan's sums and partials, and the scratch
// M^-1 that the pending points are conditioned into.  C == 0: conditioning only.
struct FittedAreas {
    int64_t W, cpad, ppad;
    uint32_t *ccodes, *pcodes;
    double *tab, *acc, *part, *Minv;
    int64_t *part_i;
    size_t total;
};
FittedAreas fitted_areas(void *workspace, int64_t R, int64_t Bc, int64_t C, int64_t P, bool lds_table, bool scratch) {
    FittedAreas a;
    a.W = (R + 31) / 32;
    a.cpad = C > 0 ? round_up(C < ACQ_SLAB ? C : ACQ_SLAB, TILE) : 0;
    a.ppad = P > 0 ? round_up(P, TILE) : 0;
    const size_t nb = (size_t)Bc, partials = C > 0 ? acq_partials(C) : 0;
    Carve cv{static_cast<char *>(workspace)};
    a.ccodes = cv.take<uint32_t>(nb * a.W * a.cpad);
    a.pcodes = cv.take<uint32_t>(nb * a.W * a.ppad);
    a.tab = cv.take<double>(lds_table ? nb * acq_table_doubles(R) : 0);
    a.acc = cv.take<double>((size_t)3 * C);
    a.part = cv.take<double>(partials);
    a.part_i = cv.take<int64_t>(partials);
    a.Minv = cv.take<double>(scratch && P > 0 ? nb * R * R : 0);
    a.total = cv.o;
    return a;
}

// What the calls on a fitted state share: the checks (nothing is launched before a refusal), the state's areas, the chunk
// size.  They factorise nothing, so there is no sweep and no LeafSystem.
struct FittedCall {
    bark_ctx *ctx = nullptr;
    hipStream_t caller = nullptr;
    const void *packed = nullptr;
    const bark_pack_info *info = nullptr;
    int64_t d = 0, B = 0, Bc = 0;
    int m = 0, R = 0;
    PosteriorState st{};

    int open(const char *name, bark_ctx *ctx_, const void *packed_, const bark_pack_info *info_, int64_t d_, const double *noise,
             const double *scale, const void *state, size_t state_bytes, const void *info_out, const void *workspace, int64_t Bc_,
             void *stream) {
        int rc = check_ctx(ctx_);
        if (rc) return rc;
        if (!packed_ || !info_ || !noise || !scale || !state || !info_out || !workspace) return fail(BARK_ERR_ARG, "%s: null argument", name);
        ctx = ctx_, packed = packed_, info = info_, d = d_, B = info->B, Bc = Bc_;
        if (d < 1 || B < 1 || Bc < 1) return fail(BARK_ERR_ARG, "%s: bad shape d=%lld B=%lld Bc=%lld", name, (long long)d, (long long)B, (long long)Bc);
        if (!posterior_shape_ok(info->max_bits, info->m, B))
            return fail(BARK_ERR_ARG, "%s: a fitted posterior holds forests of at most %d trees and 8192 leaves (got m = %lld, R = %lld)", name,
                        ACQ_MAX_TREES, (long long)info->m, (long long)info->max_bits);
        if (Bc > B) Bc = B;
        if (Bc > 65535) Bc = 65535;
        m = (int)info->m, R = (int)info->max_bits;
        st = posterior_state(const_cast<void *>(state), R, B);
        if (state_bytes < st.total) return fail(BARK_ERR_ARG, "%s: state buffer too small: %zu < %zu bytes", name, state_bytes, st.total);
        if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(workspace)) & 255)
            return fail(BARK_ERR_ARG, "%s: state and workspace must be 256-byte aligned", name);
        caller = static_cast<hipStream_t>(stream);
        return BARK_OK;
    }
    // the forests c0 .. c0 + n - 1 as a pack of their own, for the leaf walks
    const char *chunk(int64_t c0, int64_t n, bark_pack_info &sub) const {
        sub = *info;
        sub.B = n;
        return static_cast<const char *>(packed) + (size_t)c0 * m * info->stride * 16;
    }
    int copy_info(const int32_t *src, int32_t *dst, int n) const {
        hipLaunchKernelGGL(copy_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, caller, src, dst, n);
        BARK_LAUNCH_CHECK();
        return BARK_OK;
    }
    // an invalid categorical value met by a walk of this call goes into these status words
    int fault_info(int32_t *dst, int n) const {
        hipLaunchKernelGGL(fault_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, caller, ctx->fault, dst, n);
        BARK_LAUNCH_CHECK();
        return BARK_OK;
    }
};

struct LeafSystem {
    bark_ctx *ctx = nullptr;
    hipStream_t caller = nullptr;
    const void *packed = nullptr;
    const bark_pack_info *info = nullptr;
    const double *X = nullptr, *y = nullptr;
    int64_t N = 0, d = 0, B = 0, Bc = 0;
    int m = 0, R = 0, W = 0;
    LeafAreas a{};
    SystemSweep *sw = nullptr;  // the R x R sweep (chol.hip)
    // the current chunk (for_chunks): its forests, and how many
    bark_pack_info sub{};
    const char *packed_c = nullptr;
    int bc = 0;
    // ... and, from factor_chunk on, its systems in the sweep's workspace and the sweep's status
    const SystemMats *mats = nullptr;
    int32_t *chunk_info = nullptr;

    LeafSystem() = default;
    LeafSystem(const LeafSystem &) = delete;
    LeafSystem &operator=(const LeafSystem &) = delete;
    ~LeafSystem() { system_sweep_close(sw); }

    // Everything the entry points have in common up to the first chunk: the checks (nothing is launched before a refusal;
    // `name` is the entry point's, for the messages), the layout for at most Bc resident forests, the sweep, and y'y.
    // C: the entry point's candidate count (0: none), for the range check only.
    int open(const char *name, bark_ctx *ctx_, const void *packed_, const bark_pack_info *info_, const double *X_, int64_t N_,
             int64_t d_, const double *y_, const double *noise, const void *info_out, void *workspace, size_t workspace_bytes,
             int64_t Bc_, int64_t C, const LeafNeeds &needs, void *stream) {
        int rc = check_ctx(ctx_);
        if (rc) return rc;
        if (!packed_ || !info_ || !X_ || !y_ || !noise || !info_out || !workspace) return fail(BARK_ERR_ARG, "%s: null argument", name);
        ctx = ctx_, packed = packed_, info = info_, X = X_, y = y_, N = N_, d = d_, B = info->B, Bc = Bc_;
        if (N < 1 || d < 1 || B < 1 || info->m < 1 || Bc < 1 || C < 0 || N > (1 << 24) || C > (1 << 24))
            return fail(BARK_ERR_ARG, "%s: bad shape N=%lld d=%lld B=%lld m=%lld Bc=%lld C=%lld", name, (long long)N, (long long)d,
                        (long long)B, (long long)info->m, (long long)Bc, (long long)C);
        if (info->max_bits < 1 || info->max_bits > 8192)
            return fail(BARK_ERR_ARG, "%s: the leaf-space path supports at most 8192 leaves per forest (got %lld)", name,
                        (long long)info->max_bits);
        if (Bc > B) Bc = B;
        if (Bc > 65535) Bc = 65535;
        m = (int)info->m, R = (int)info->max_bits;
        a = leaf_areas(workspace, N, R, m, Bc, needs);
        W = (int)a.W;
        if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
        if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(BARK_ERR_ARG, "workspace must be 256-byte aligned");
        caller = static_cast<hipStream_t>(stream);
        // the R x R sweep: N := R points, no leaf codes (A is filled by leafspace_prepare)
        if ((rc = system_sweep_open(ctx, caller, workspace, R, needs.identity, m, Bc, &sw))) return rc;
        return leafspace_sumsq(y, (int)N, a.yy, caller);
    }

    // body(c0) for each chunk of at most Bc forests, c0 its first forest; sub / packed_c / bc describe it to the steps below
    template <class F> int for_chunks(F &&body) {
        auto chunk = [&](int64_t c0, int64_t n) -> int {
            sub = *info;
            sub.B = n;
            bc = (int)n;
            packed_c = static_cast<const char *>(packed) + (size_t)c0 * m * info->stride * 16;
            return body(c0);
        };
        using Chunk = decltype(chunk);
        return system_sweep_chunks(
            sw, B, Bc, [](void *f, int64_t c0, int64_t n) -> int { return (*static_cast<Chunk *>(f))(c0, n); }, &chunk);
    }

    // leaf walk, I + c Z'Z and v = Z'y, the identity right-hand side when the call needs it, the R x R sweep and, with `mll`,
    // the MLL.  noise / scale / info_out / mll: the chunk's.  `info_out` receives the sweep's pivot status.
    int factor_chunk(const double *noise, const double *scale, int32_t *info_out, double *mll, int include_2pi) {
        int rc;
        const SystemMats &p = system_sweep_bind(sw, bc, info_out);
        mats = &p;
        chunk_info = info_out;
        if ((rc = walk_one_hot(packed_c, &sub, X, N, d, W, a.codes, ctx->fault, caller))) return rc;
        rc = leafspace_prepare(a.codes, W, (int)a.npad, a.planes, R, (int)a.Rpad, noise, scale, m, bc, p.A, p.ld, p.bstride, y, (int)N,
                               p.yz, p.accum, info_out, caller);
        if (rc) return rc;
        if ((rc = system_sweep_factor(sw))) return rc;
        if (mll) return leafspace_finish(p.accum, a.yy, noise, scale, m, bc, (int)N, include_2pi, mll, caller);
        return BARK_OK;
    }

    // w = M^-1 v = V'z from the swept chunk (the kernel of the dense posterior mean)
    int solve_w() { return system_sweep_w(sw, a.w); }
    // ... and M^-1 = V'V (the kernel of the dense inverse export)
    int solve_w_minv() { return solve_w_minv_into(a.w, a.Minv); }
    // the same two launches with the chunk's outputs (bc, R) and (bc, R, R) somewhere else: a fitted state
    int solve_w_minv_into(double *w, double *Minv) {
        const int rc = system_sweep_w(sw, w);
        if (rc) return rc;
        return system_sweep_minv(sw, Minv);
    }
    // one-hot codes of n candidates (at most LeafNeeds::cand) under the chunk's forests -> a.ccodes
    int walk_candidates(const double *cand, int64_t n) {
        return walk_one_hot(packed_c, &sub, cand, n, d, W, a.ccodes, ctx->fault, caller);
    }
    // ... of the scan's P pending points -> a.pcodes
    int walk_pending(const double *pending, int64_t P) {
        return walk_one_hot(packed_c, &sub, pending, P, d, W, a.pcodes, ctx->fault, caller);
    }
    // an invalid categorical value met by one of the chunk's walks goes into its forests' info
    int close_chunk() {
        hipLaunchKernelGGL(fault_info_kernel, dim3((unsigned)((bc + 255) / 256)), dim3(256), 0, caller, ctx->fault, chunk_info, bc);
        BARK_LAUNCH_CHECK();
        return BARK_OK;
    }
};

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

size_t bark_kernel_inverse_leafspace_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, inverse_needs()).total;
}

size_t bark_mll_leafspace_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1 || C < 0) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, mll_needs(C)).total;
}

size_t bark_posterior_samples_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t S) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1 || C < 1 || S < 1) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, samples_needs(C, S)).total;
}

size_t bark_noise_scale_step_chains_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t nc) {
    if (N < 1 || max_bits < 1 || m < 1 || nc < 1) return 0;
    return leaf_areas(nullptr, N, max_bits, m, nc, chain_step_needs()).total;
}

size_t bark_acquisition_scan_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1 || C < 1) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, scan_needs(C, 0)).total;
}

size_t bark_acquisition_scan_pending_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1 || C < 1 || P < 0 || P > ACQ_MAX_PENDING) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, scan_needs(C, P)).total;
}

// the targets stay where the caller has them: nothing is added to the workspace
size_t bark_acquisition_scan_targets_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P) {
    return bark_acquisition_scan_pending_workspace_bytes(N, max_bits, m, Bc, C, P);
}

size_t bark_predictive_scores_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc, int64_t C) {
    if (N < 1 || max_bits < 1 || m < 1 || Bc < 1 || C < 1) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, scores_needs(C)).total;
}

int bark_mll_leafspace_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                           const double *y, const double *noise, const double *scale, int flags, const double *cand,
                           int64_t C, double *mll_out, double *mu_out, double *var_out, int32_t *info_out,
                           void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!mll_out) return fail(BARK_ERR_ARG, "bark_mll_leafspace_hip: null argument");
    if (C > 0 && (!cand || !mu_out || !var_out || !scale || !(flags & BARK_MLL_INCLUDE_SCALE)))
        return fail(BARK_ERR_ARG, "leaf-space posterior needs cand, mu_out, var_out, scale and BARK_MLL_INCLUDE_SCALE");
    if ((flags & BARK_MLL_INCLUDE_SCALE) && !scale) return fail(BARK_ERR_ARG, "BARK_MLL_INCLUDE_SCALE without scale");
    if (flags & BARK_MLL_RHS_IDENTITY) return fail(BARK_ERR_ARG, "leaf-space path computes the MLL only");
    LeafSystem sys;
    int rc = sys.open("bark_mll_leafspace_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, C,
                      mll_needs(C), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    const bool use_scale = (flags & BARK_MLL_INCLUDE_SCALE) != 0;
    return sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, use_scale ? scale + c0 : nullptr, info_out + c0, mll_out + c0,
                                 (flags & BARK_MLL_INCLUDE_2PI) ? 1 : 0);
        if (r) return r;
        if (C > 0) {
            if ((r = sys.solve_w_minv()) || (r = sys.walk_candidates(cand, C))) return r;
            r = leafspace_predict(a.ccodes, sys.W, (int)a.cpad, (int)C, a.w, a.Minv, sys.R, noise + c0, scale + c0, sys.m, sys.bc,
                                  mu_out + (size_t)c0 * C, var_out + (size_t)c0 * C, sys.caller);
            if (r) return r;
        }
        return sys.close_chunk();
    });
}

int bark_kernel_inverse_leafspace_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                                      const double *y, const double *noise, const double *scale, int flags,
                                      double *mll_out, double *kinv_out, double *kinv_y_out, int32_t *info_out,
                                      void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!kinv_out) return fail(BARK_ERR_ARG, "bark_kernel_inverse_leafspace_hip: kinv_out is null");
    if (info && info->m > LEAF_INV_MAX_TREES)  // leaf_inverse_kernel's leaf lists must fit its LDS
        return fail(BARK_ERR_ARG, "leaf-space inverse supports at most %d trees (got %lld)", LEAF_INV_MAX_TREES, (long long)info->m);
    if (!mll_out) return fail(BARK_ERR_ARG, "bark_kernel_inverse_leafspace_hip: null argument");
    if ((flags & BARK_MLL_INCLUDE_SCALE) && !scale) return fail(BARK_ERR_ARG, "BARK_MLL_INCLUDE_SCALE without scale");
    if (flags & BARK_MLL_RHS_IDENTITY) return fail(BARK_ERR_ARG, "leaf-space path computes the MLL only");
    LeafSystem sys;
    int rc = sys.open("bark_kernel_inverse_leafspace_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes,
                      Bc, 0, inverse_needs(), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    const bool use_scale = (flags & BARK_MLL_INCLUDE_SCALE) != 0;
    return sys.for_chunks([&](int64_t c0) -> int {
        const double *scale_c = use_scale ? scale + c0 : nullptr;
        int r = sys.factor_chunk(noise + c0, scale_c, info_out + c0, mll_out + c0, (flags & BARK_MLL_INCLUDE_2PI) ? 1 : 0);
        if (r || (r = sys.solve_w_minv())) return r;
        r = leafspace_inverse(a.codes, sys.W, (int)a.npad, (int)N, a.Minv, a.w, sys.R, y, noise + c0, scale_c, sys.m, sys.bc, a.Wm,
                              kinv_out + (size_t)c0 * N * N, kinv_y_out ? kinv_y_out + (size_t)c0 * N : nullptr, nullptr, sys.caller);
        if (r) return r;
        return sys.close_chunk();
    });
}

// Joint draws at the candidates: eps (B, S, R), and f_out (B, S, C) for BARK_SAMPLE_FULL or red_out / idx_out (B, S) for
// BARK_SAMPLE_MAX / MIN.  No MLL.
int bark_posterior_samples_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                               int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                               int64_t C, const double *eps, int64_t S, int reduce, double *f_out, double *red_out,
                               int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                               void *stream_) {
    error_buffer()[0] = 0;
    if (reduce != BARK_SAMPLE_FULL && reduce != BARK_SAMPLE_MAX && reduce != BARK_SAMPLE_MIN)
        return fail(BARK_ERR_ARG, "bark_posterior_samples_hip: unknown reduce %d", reduce);
    const bool full = reduce == BARK_SAMPLE_FULL;
    if (!info || !cand || !eps || !scale || (full ? !f_out : (!red_out || !idx_out)))
        return fail(BARK_ERR_ARG, "bark_posterior_samples_hip: null argument");
    if (C < 1 || S < 1 || S > (1 << 20))
        return fail(BARK_ERR_ARG, "bark_posterior_samples_hip: bad shape C=%lld S=%lld", (long long)C, (long long)S);
    if (info->m > 64) return fail(BARK_ERR_ARG, "leaf-space posterior samples support at most 64 trees (got %lld)", (long long)info->m);
    LeafSystem sys;
    int rc = sys.open("bark_posterior_samples_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, C,
                      samples_needs(C, S), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    return sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, scale + c0, info_out + c0, nullptr, 0);
        if (r || (r = sys.solve_w()) || (r = sys.walk_candidates(cand, C))) return r;
        // Wt = c w 1' + sqrt(scale/m) V' E', then the gather over the candidates' leaves (sample.hip)
        const SystemMats &p = *sys.mats;
        r = sample_weights(p.V, p.ld, p.bstride, a.w, eps + (size_t)c0 * S * sys.R, sys.R, (int)a.Rpad, (int)S, (int)a.Spad, noise + c0,
                           scale + c0, sys.m, sys.bc, a.Wt, sys.caller);
        if (r) return r;
        r = sample_gather(a.ccodes, sys.W, (int)a.cpad, (int)C, a.Wt, (int)a.Rpad, (int)a.Spad, (int)S, sys.m, sys.bc, reduce,
                          full ? f_out + (size_t)c0 * S * C : nullptr, full ? nullptr : red_out + (size_t)c0 * S,
                          full ? nullptr : idx_out + (size_t)c0 * S, a.part, a.part_i, sys.caller);
        if (r) return r;
        return sys.close_chunk();
    });
}

// Acquisition scan (include/bark_hip.h, kernels in acquire.hip): w and M^-1 of a chunk of forests are consumed by
// acq_scan_kernel slab by slab of candidates before the next chunk is prepared; the finish after the last chunk.  With pending
// points M^-1 is conditioned on them first (acq_condition_kernel), so neither variant of the scan knows about them, and no
// kind does.  The target kinds read the chunk's rows of `targets` (B, S) in the scan.
int bark_acquisition_scan_targets_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                                      int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                                      int64_t C, const double *pending, int64_t P, const int64_t *skip_idx, int64_t n_skip,
                                      const double *targets, int64_t S, double kappa, int kind, int variant, double *acq_out,
                                      double *best_out, int64_t *idx_out, int32_t *info_out, void *workspace,
                                      size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!info || !scale || !cand || !best_out || !idx_out) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: null argument");
    if (C < 1) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: bad shape C=%lld", (long long)C);
    if (P < 0 || P > ACQ_MAX_PENDING || n_skip < 0 || n_skip > ACQ_MAX_SKIP)
        return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: at most %lld pending points and %lld skipped candidates (got %lld, %lld)",
                    (long long)ACQ_MAX_PENDING, (long long)ACQ_MAX_SKIP, (long long)P, (long long)n_skip);
    if ((P > 0 && !pending) || (n_skip > 0 && !skip_idx)) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: null argument");
    if (kind < BARK_ACQ_LCB_MEAN || kind > BARK_ACQ_MES) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: unknown kind %d", kind);
    const bool lcb = kind == BARK_ACQ_LCB_MEAN || kind == BARK_ACQ_LCB_MIXTURE;
    if (!lcb && !targets) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: kind %d needs targets", kind);
    if (!lcb && (S < 1 || S > ACQ_MAX_TARGETS))
        return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: between 1 and %lld targets per forest (got %lld)",
                    (long long)ACQ_MAX_TARGETS, (long long)S);
    if (!std::isfinite(kappa)) return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: kappa is not finite");
    int var = 0, rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, variant, &var, nullptr))) return rc;
    LeafSystem sys;
    rc = sys.open("bark_acquisition_scan_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, C,
                  scan_needs(C, P), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    rc = sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, scale + c0, info_out + c0, nullptr, 0);
        if (r || (r = sys.solve_w_minv())) return r;
        if (P > 0) {
            if ((r = sys.walk_pending(pending, P))) return r;
            r = acq_condition(a.pcodes, sys.W, (int)a.ppad, (int)P, a.Minv, sys.R, noise + c0, scale + c0, sys.m, sys.bc,
                              info_out + c0, sys.caller);
            if (r) return r;
        }
        if (var == 1 && (r = acq_pack(a.Minv, a.w, sys.R, sys.bc, a.tab, sys.caller))) return r;
        for (int64_t s0 = 0; s0 < C; s0 += ACQ_SLAB) {
            const int64_t n = C - s0 < ACQ_SLAB ? C - s0 : ACQ_SLAB;
            if ((r = sys.walk_candidates(cand + (size_t)s0 * d, n))) return r;
            r = acq_scan(var, lcb ? BARK_ACQ_LCB_MEAN : kind, a.ccodes, sys.W, (int)bark_leaf_npad(n), (int)n, a.w, a.Minv, a.tab, sys.R,
                         noise + c0, scale + c0, sys.m, sys.bc, kappa, lcb ? nullptr : targets + (size_t)c0 * S, lcb ? 0 : (int)S,
                         c0 == 0, a.acc + s0, (size_t)C, nullptr, sys.caller);
            if (r) return r;
        }
        return sys.close_chunk();
    });
    if (rc) return rc;
    return acq_finish(a.acc, C, (int)sys.B, kappa, kind, skip_idx, (int)n_skip, acq_out, a.part, a.part_i, info_out, nullptr, best_out,
                      idx_out, sys.caller);
}

// the confidence bounds only: the two entry points without targets refuse every other kind
int bark_acquisition_scan_pending_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                                      int64_t d, const double *y, const double *noise, const double *scale, const double *cand,
                                      int64_t C, const double *pending, int64_t P, const int64_t *skip_idx, int64_t n_skip,
                                      double kappa, int kind, int variant, double *acq_out, double *best_out, int64_t *idx_out,
                                      int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (kind != BARK_ACQ_LCB_MEAN && kind != BARK_ACQ_LCB_MIXTURE)
        return fail(BARK_ERR_ARG, "bark_acquisition_scan_hip: unknown kind %d", kind);
    return bark_acquisition_scan_targets_hip(ctx, packed, info, X, N, d, y, noise, scale, cand, C, pending, P, skip_idx, n_skip, nullptr,
                                             0, kappa, kind, variant, acq_out, best_out, idx_out, info_out, workspace, workspace_bytes,
                                             Bc, stream_);
}

int bark_acquisition_scan_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                              const double *y, const double *noise, const double *scale, const double *cand, int64_t C,
                              double kappa, int kind, int variant, double *acq_out, double *best_out, int64_t *idx_out,
                              int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    return bark_acquisition_scan_pending_hip(ctx, packed, info, X, N, d, y, noise, scale, cand, C, nullptr, 0, nullptr, 0, kappa, kind,
                                             variant, acq_out, best_out, idx_out, info_out, workspace, workspace_bytes, Bc, stream_);
}

// ---- fitted posterior (include/bark_hip.h): fit once, scan and condition from the state ----

size_t bark_leaf_posterior_bytes(int64_t max_bits, int64_t m, int64_t B) {
    if (!posterior_shape_ok(max_bits, m, B)) return 0;
    return posterior_state(nullptr, max_bits, B).total;
}

size_t bark_leaf_posterior_fit_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc) {
    if (N < 1 || Bc < 1 || !posterior_shape_ok(max_bits, m, 1)) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, fit_needs()).total;
}

size_t bark_acquisition_scan_fitted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P, int variant) {
    int var = 0;
    if (Bc < 1 || C < 1 || C > (1 << 24) || P < 0 || P > ACQ_MAX_PENDING || bark_acquisition_plan(max_bits, m, variant, &var, nullptr)) {
        error_buffer()[0] = 0;  // a query reports through its value only
        return 0;
    }
    return fitted_areas(nullptr, max_bits, Bc, C, P, var == 1, true).total;
}

size_t bark_leaf_posterior_condition_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P) {
    if (Bc < 1 || P < 0 || P > ACQ_MAX_PENDING || !posterior_shape_ok(max_bits, m, 1)) return 0;
    return fitted_areas(nullptr, max_bits, Bc, 0, P, false, false).total;
}

// The opening sequence of the scan, chunk by chunk, with the sweep's two outputs and its status pointed into the state: no
// copy.  The status words reach info_out once, after the last chunk.
int bark_leaf_posterior_fit_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N, int64_t d,
                                const double *y, const double *noise, const double *scale, void *state, size_t state_bytes,
                                int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!info || !scale || !state) return fail(BARK_ERR_ARG, "bark_leaf_posterior_fit_hip: null argument");
    int rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, 0, nullptr, nullptr))) return rc;
    if (info->B < 1) return fail(BARK_ERR_ARG, "bark_leaf_posterior_fit_hip: bad shape B=%lld", (long long)info->B);
    const PosteriorState st = posterior_state(state, info->max_bits, info->B);
    if (state_bytes < st.total)
        return fail(BARK_ERR_ARG, "bark_leaf_posterior_fit_hip: state buffer too small: %zu < %zu bytes", state_bytes, st.total);
    if (reinterpret_cast<uintptr_t>(state) & 255) return fail(BARK_ERR_ARG, "bark_leaf_posterior_fit_hip: state must be 256-byte aligned");
    LeafSystem sys;
    rc = sys.open("bark_leaf_posterior_fit_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, 0,
                  fit_needs(), stream_);
    if (rc) return rc;
    const size_t R = (size_t)sys.R;
    rc = sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, scale + c0, st.info + c0, nullptr, 0);
        if (r || (r = sys.solve_w_minv_into(st.w + (size_t)c0 * R, st.Minv + (size_t)c0 * R * R))) return r;
        return sys.close_chunk();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(copy_info_kernel, dim3((unsigned)((sys.B + 255) / 256)), dim3(256), 0, sys.caller, st.info, info_out, (int)sys.B);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

// The scan of bark_acquisition_scan_targets_hip from its `P > 0` on, with M^-1 and w read from the state.  The state is only
// read: pending points condition a copy of the chunk's M^-1 in the workspace (acq_condition_from_kernel).  info_out starts
// as the state's status and takes the faults of this call's walks.
//
// weights (device, (B,), normalised by the caller) or null: bark_acquisition_scan_fitted_weighted_hip.  The weighted
// instantiation of the scan and the finish without the division by B; a chunk whose first forests have weight 0 still passes
// `first`, because the kernel starts its sums at zero whichever forest it skips.  Pending points condition the scratch copy
// of every forest, whatever its weight: that kernel does not know about weights.
static int scan_fitted(const char *name, bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                       const double *scale, const void *state, size_t state_bytes, const double *cand, int64_t C, const double *pending,
                       int64_t P, const int64_t *skip_idx, int64_t n_skip, const double *targets, int64_t S, double kappa, int kind,
                       int variant, const double *weights, double *acq_out, double *best_out, int64_t *idx_out, int32_t *info_out,
                       void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!info || !cand || !best_out || !idx_out) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (C < 1 || C > (1 << 24)) return fail(BARK_ERR_ARG, "%s: bad shape C=%lld", name, (long long)C);
    if (P < 0 || P > ACQ_MAX_PENDING || n_skip < 0 || n_skip > ACQ_MAX_SKIP)
        return fail(BARK_ERR_ARG, "%s: at most %lld pending points and %lld skipped candidates (got %lld, %lld)", name,
                    (long long)ACQ_MAX_PENDING, (long long)ACQ_MAX_SKIP, (long long)P, (long long)n_skip);
    if ((P > 0 && !pending) || (n_skip > 0 && !skip_idx)) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (kind < BARK_ACQ_LCB_MEAN || kind > BARK_ACQ_MES) return fail(BARK_ERR_ARG, "%s: unknown kind %d", name, kind);
    const bool lcb = kind == BARK_ACQ_LCB_MEAN || kind == BARK_ACQ_LCB_MIXTURE;
    if (!lcb && !targets) return fail(BARK_ERR_ARG, "%s: kind %d needs targets", name, kind);
    if (!lcb && (S < 1 || S > ACQ_MAX_TARGETS))
        return fail(BARK_ERR_ARG, "%s: between 1 and %lld targets per forest (got %lld)", name, (long long)ACQ_MAX_TARGETS, (long long)S);
    if (!std::isfinite(kappa)) return fail(BARK_ERR_ARG, "%s: kappa is not finite", name);
    int var = 0, rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, variant, &var, nullptr))) return rc;
    FittedCall fc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FittedAreas a = fitted_areas(workspace, fc.R, fc.Bc, C, P, var == 1, true);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const int R = fc.R, m = fc.m, W = (int)a.W;
    const PosteriorState &st = fc.st;
    if ((rc = fc.copy_info(st.info, info_out, (int)fc.B))) return rc;
    for (int64_t c0 = 0; c0 < fc.B; c0 += fc.Bc) {
        const int bc = (int)(fc.B - c0 < fc.Bc ? fc.B - c0 : fc.Bc);
        bark_pack_info sub;
        const char *packed_c = fc.chunk(c0, bc, sub);
        const double *w = st.w + (size_t)c0 * R;
        const double *Minv = st.Minv + (size_t)c0 * R * R;
        if (P > 0) {
            if ((rc = walk_one_hot(packed_c, &sub, pending, P, fc.d, W, a.pcodes, ctx->fault, fc.caller))) return rc;
            rc = acq_condition_from(a.pcodes, W, (int)a.ppad, (int)P, Minv, a.Minv, R, noise + c0, scale + c0, m, bc, st.info + c0,
                                    fc.caller);
            if (rc) return rc;
            Minv = a.Minv;
        }
        if (var == 1 && (rc = acq_pack(Minv, w, R, bc, a.tab, fc.caller))) return rc;
        for (int64_t s0 = 0; s0 < C; s0 += ACQ_SLAB) {
            const int64_t n = C - s0 < ACQ_SLAB ? C - s0 : ACQ_SLAB;
            if ((rc = walk_one_hot(packed_c, &sub, cand + (size_t)s0 * fc.d, n, fc.d, W, a.ccodes, ctx->fault, fc.caller))) return rc;
            rc = acq_scan(var, lcb ? BARK_ACQ_LCB_MEAN : kind, a.ccodes, W, (int)bark_leaf_npad(n), (int)n, w, Minv, a.tab, R, noise + c0,
                          scale + c0, m, bc, kappa, lcb ? nullptr : targets + (size_t)c0 * S, lcb ? 0 : (int)S, c0 == 0, a.acc + s0,
                          (size_t)C, weights ? weights + c0 : nullptr, fc.caller);
            if (rc) return rc;
        }
        if ((rc = fc.fault_info(info_out + c0, bc))) return rc;
    }
    return acq_finish(a.acc, C, (int)fc.B, kappa, kind, skip_idx, (int)n_skip, acq_out, a.part, a.part_i, info_out, weights, best_out,
                      idx_out, fc.caller);
}

int bark_acquisition_scan_fitted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                     const double *scale, const void *state, size_t state_bytes, const double *cand, int64_t C,
                                     const double *pending, int64_t P, const int64_t *skip_idx, int64_t n_skip, const double *targets,
                                     int64_t S, double kappa, int kind, int variant, double *acq_out, double *best_out,
                                     int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                                     void *stream_) {
    return scan_fitted("bark_acquisition_scan_fitted_hip", ctx, packed, info, d, noise, scale, state, state_bytes, cand, C, pending, P,
                       skip_idx, n_skip, targets, S, kappa, kind, variant, nullptr, acq_out, best_out, idx_out, info_out, workspace,
                       workspace_bytes, Bc, stream_);
}

// the weights stay where the caller has them: nothing is added to the workspace
size_t bark_acquisition_scan_fitted_weighted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P,
                                                             int variant) {
    return bark_acquisition_scan_fitted_workspace_bytes(max_bits, m, Bc, C, P, variant);
}

int bark_acquisition_scan_fitted_weighted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d,
                                              const double *noise, const double *scale, const void *state, size_t state_bytes,
                                              const double *cand, int64_t C, const double *pending, int64_t P,
                                              const int64_t *skip_idx, int64_t n_skip, const double *targets, int64_t S, double kappa,
                                              int kind, int variant, const double *weights, double *acq_out, double *best_out,
                                              int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                                              void *stream_) {
    return scan_fitted("bark_acquisition_scan_fitted_weighted_hip", ctx, packed, info, d, noise, scale, state, state_bytes, cand, C,
                       pending, P, skip_idx, n_skip, targets, S, kappa, kind, variant, weights, acq_out, best_out, idx_out, info_out,
                       workspace, workspace_bytes, Bc, stream_);
}

// ---- information gain of a (query, target) pair from the state (include/bark_hip.h; kernels in fidelity.hip) ----

constexpr int64_t FID_MAX_CAND = 1 << 16, FID_MAX_ADAPT = 1024, FID_MAX_GRID = 4096;

// The workspace of the gain: the codes of the C query and the C target points for Bc forests, the moments of the chunk's
// pairs, their values (unused when the caller takes per_forest_out: the kernels then write the chunk's rows there), and the
// running sums.
struct FidelityAreas {
    int64_t W, cpad;
    uint32_t *qcodes, *tcodes;
    double *mom, *g, *acc;
    size_t total;
};
static FidelityAreas fidelity_areas(void *workspace, int64_t R, int64_t Bc, int64_t C) {
    FidelityAreas a;
    a.W = (R + 31) / 32;
    a.cpad = round_up(C, TILE);
    const size_t nb = (size_t)Bc;
    Carve cv{static_cast<char *>(workspace)};
    a.qcodes = cv.take<uint32_t>(nb * a.W * a.cpad);
    a.tcodes = cv.take<uint32_t>(nb * a.W * a.cpad);
    a.mom = cv.take<double>(nb * FID_MOMENTS * C);
    a.g = cv.take<double>(nb * C);
    a.acc = cv.take<double>((size_t)C);
    a.total = cv.o;
    return a;
}
static bool fidelity_shape_ok(int64_t max_bits, int64_t m, int64_t C, int64_t S) {
    return posterior_shape_ok(max_bits, m, 1) && C >= 1 && C <= FID_MAX_CAND && S >= 1 && S <= ACQ_MAX_TARGETS;
}

// the targets stay where the caller has them and Z_s lives in LDS: S is checked, and adds nothing
size_t bark_fidelity_gain_fitted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t S) {
    if (Bc < 1 || !fidelity_shape_ok(max_bits, m, C, S)) return 0;
    return fidelity_areas(nullptr, max_bits, Bc > 65535 ? 65535 : Bc, C).total;
}

// Per chunk: the two walks, the moments of every pair (which settle the pairs a forest does not separate), the quadrature of
// the others, and the chunk's values added to the sums in forest order; the finish after the last chunk.  The state is only
// read.  Every argument is checked before the context is, so a refusal needs no device.
int bark_fidelity_gain_fitted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                  const double *scale, const void *state, size_t state_bytes, const double *query,
                                  const double *target, int64_t C, const double *targets, int64_t S, const double *weights,
                                  double lo, double hi, int64_t n_a, double pad, int64_t G, double *gain_out, double *per_forest_out,
                                  int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_fidelity_gain_fitted_hip";
    error_buffer()[0] = 0;
    if (!info || !query || !target || !targets || !gain_out) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (!posterior_shape_ok(info->max_bits, info->m, 1))
        return fail(BARK_ERR_ARG, "%s: at most %d trees and 8192 leaves per forest (got m = %lld, R = %lld)", name, ACQ_MAX_TREES,
                    (long long)info->m, (long long)info->max_bits);
    if (C < 1 || C > FID_MAX_CAND) return fail(BARK_ERR_ARG, "%s: between 1 and %lld pairs (got %lld)", name, (long long)FID_MAX_CAND, (long long)C);
    if (S < 1 || S > ACQ_MAX_TARGETS)
        return fail(BARK_ERR_ARG, "%s: between 1 and %lld targets per forest (got %lld)", name, (long long)ACQ_MAX_TARGETS, (long long)S);
    if (n_a < 2 || n_a > FID_MAX_ADAPT)
        return fail(BARK_ERR_ARG, "%s: between 2 and %lld support points (got %lld)", name, (long long)FID_MAX_ADAPT, (long long)n_a);
    if (G < 2 || G > FID_MAX_GRID)
        return fail(BARK_ERR_ARG, "%s: between 2 and %lld quadrature points (got %lld)", name, (long long)FID_MAX_GRID, (long long)G);
    if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(pad) || !(lo < hi) || !(pad >= 0.0))
        return fail(BARK_ERR_ARG, "%s: the grid needs finite lo < hi and a finite pad >= 0 (got %g, %g, %g)", name, lo, hi, pad);
    FittedCall fc;
    int rc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FidelityAreas a = fidelity_areas(workspace, fc.R, fc.Bc, C);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const int R = fc.R, m = fc.m, W = (int)a.W, n = (int)C, cpad = (int)bark_leaf_npad(C);
    const PosteriorState &st = fc.st;
    if ((rc = fc.copy_info(st.info, info_out, (int)fc.B))) return rc;
    for (int64_t c0 = 0; c0 < fc.B; c0 += fc.Bc) {
        const int bc = (int)(fc.B - c0 < fc.Bc ? fc.B - c0 : fc.Bc);
        bark_pack_info sub;
        const char *packed_c = fc.chunk(c0, bc, sub);
        const double *tg = targets + (size_t)c0 * S, *wt = weights ? weights + c0 : nullptr;
        double *g = per_forest_out ? per_forest_out + (size_t)c0 * C : a.g;  // (bc, C) either way
        if ((rc = walk_one_hot(packed_c, &sub, query, C, fc.d, W, a.qcodes, ctx->fault, fc.caller))) return rc;
        if ((rc = walk_one_hot(packed_c, &sub, target, C, fc.d, W, a.tcodes, ctx->fault, fc.caller))) return rc;
        rc = fidelity_moments(a.qcodes, a.tcodes, W, cpad, n, st.w + (size_t)c0 * R, st.Minv + (size_t)c0 * R * R, R, noise + c0,
                              scale + c0, m, bc, tg, (int)S, wt, a.mom, g, fc.caller);
        if (rc || (rc = fidelity_quadrature(a.mom, n, bc, tg, (int)S, lo, hi, (int)n_a, pad, (int)G, g, fc.caller))) return rc;
        if ((rc = fidelity_accumulate(g, n, bc, wt, c0 == 0, a.acc, fc.caller))) return rc;
        if ((rc = fc.fault_info(info_out + c0, bc))) return rc;
    }
    return fidelity_finish(a.acc, n, (int)fc.B, weights, info_out, gain_out, per_forest_out, fc.caller);
}

// The state conditioned in place on P more points, in the order given (acq_condition_kernel on the state's M^-1; w does not
// change).  A fault of the walk marks the state's status too: its M^-1 has then been conditioned on a leaf that means nothing.
int bark_leaf_posterior_condition_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                      const double *scale, const double *pending, int64_t P, void *state, size_t state_bytes,
                                      int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_leaf_posterior_condition_hip";
    error_buffer()[0] = 0;
    if (!info) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (P < 0 || P > ACQ_MAX_PENDING)
        return fail(BARK_ERR_ARG, "%s: at most %lld pending points (got %lld)", name, (long long)ACQ_MAX_PENDING, (long long)P);
    if (P > 0 && !pending) return fail(BARK_ERR_ARG, "%s: null argument", name);
    FittedCall fc;
    int rc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FittedAreas a = fitted_areas(workspace, fc.R, fc.Bc, 0, P, false, false);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const PosteriorState &st = fc.st;
    for (int64_t c0 = 0; P > 0 && c0 < fc.B; c0 += fc.Bc) {
        const int bc = (int)(fc.B - c0 < fc.Bc ? fc.B - c0 : fc.Bc);
        bark_pack_info sub;
        const char *packed_c = fc.chunk(c0, bc, sub);
        if ((rc = walk_one_hot(packed_c, &sub, pending, P, fc.d, (int)a.W, a.pcodes, ctx->fault, fc.caller))) return rc;
        rc = acq_condition(a.pcodes, (int)a.W, (int)a.ppad, (int)P, st.Minv + (size_t)c0 * fc.R * fc.R, fc.R, noise + c0, scale + c0, fc.m,
                           bc, st.info + c0, fc.caller);
        if (rc || (rc = fc.fault_info(st.info + c0, bc))) return rc;
    }
    return fc.copy_info(st.info, info_out, (int)fc.B);
}

size_t bark_leaf_posterior_observe_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P) {
    return bark_leaf_posterior_condition_workspace_bytes(max_bits, m, Bc, P);
}

// The state conditioned in place on P more points with values, in the order given (acq_observe_kernel on the state's M^-1 and
// w): bark_leaf_posterior_condition_hip's checks, chunks, walk and fault handling.  The values stay on the device: they are
// not read back, so a NaN value gives a NaN w and no status.
int bark_leaf_posterior_observe_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                    const double *scale, const double *points, int64_t P, const double *values, int64_t value_stride,
                                    int mode, const double *eps, uint64_t seed, int64_t draw, void *state, size_t state_bytes,
                                    double *values_out, double *logpred_out, int32_t *info_out, void *workspace,
                                    size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_leaf_posterior_observe_hip";
    error_buffer()[0] = 0;
    if (!info) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (P < 0 || P > ACQ_MAX_PENDING)
        return fail(BARK_ERR_ARG, "%s: at most %lld points per call (got %lld)", name, (long long)ACQ_MAX_PENDING, (long long)P);
    if (P > 0 && !points) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (mode != BARK_OBSERVE_VALUES && mode != BARK_OBSERVE_SAMPLE) return fail(BARK_ERR_ARG, "%s: unknown mode %d", name, mode);
    if (mode == BARK_OBSERVE_VALUES && !values) return fail(BARK_ERR_ARG, "%s: BARK_OBSERVE_VALUES needs values", name);
    if (value_stride != 0 && value_stride != P)
        return fail(BARK_ERR_ARG, "%s: value_stride is 0 (one vector for all forests) or P (got %lld)", name, (long long)value_stride);
    if (draw < 0 || draw > 0xFFFFFFFFll) return fail(BARK_ERR_ARG, "%s: draw number outside 0 .. 2^32 - 1", name);
    FittedCall fc;
    int rc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FittedAreas a = fitted_areas(workspace, fc.R, fc.Bc, 0, P, false, false);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const PosteriorState &st = fc.st;
    for (int64_t c0 = 0; P > 0 && c0 < fc.B; c0 += fc.Bc) {
        const int bc = (int)(fc.B - c0 < fc.Bc ? fc.B - c0 : fc.Bc);
        bark_pack_info sub;
        const char *packed_c = fc.chunk(c0, bc, sub);
        if ((rc = walk_one_hot(packed_c, &sub, points, P, fc.d, (int)a.W, a.pcodes, ctx->fault, fc.caller))) return rc;
        rc = acq_observe(a.pcodes, (int)a.W, (int)a.ppad, (int)P, st.Minv + (size_t)c0 * fc.R * fc.R, st.w + (size_t)c0 * fc.R, fc.R,
                         noise + c0, scale + c0, fc.m, bc, st.info + c0, mode, values ? values + (size_t)c0 * value_stride : nullptr,
                         (int)value_stride, eps ? eps + (size_t)c0 * P : nullptr, seed, c0, draw,
                         values_out ? values_out + (size_t)c0 * P : nullptr, logpred_out ? logpred_out + c0 : nullptr, fc.caller);
        if (rc || (rc = fc.fault_info(st.info + c0, bc))) return rc;
    }
    return fc.copy_info(st.info, info_out, (int)fc.B);
}

// ---- predictions from the state (include/bark_hip.h; kernels in predict.hip) ----

constexpr int64_t PRED_MAX_PROBS = 16;

// The workspace of the predict call: the codes of one slab of points for Bc forests, the LDS image when that variant runs,
// the (4, C) recurrence state, the flag word, with scores the (3, C) score state and the tile partials of the mixture
// (tiles, 2) and of all B forests (B, tiles, 2: the slabs are the outer loop, so a forest's tiles are complete only at the
// end), and mu_b / var_b of one slab (2, B, slab) when quantiles are asked for and forest_out does not hold them.
struct PredictAreas {
    int64_t W, cpad, slab;
    uint32_t *ccodes;
    double *tab, *acc, *sacc, *mpart, *fpart, *fslab;
    int32_t *flag;
    size_t total;
};
static PredictAreas predict_areas(void *workspace, int64_t R, int64_t B, int64_t Bc, int64_t C, int64_t Q, bool want_forest,
                                  bool want_scores, bool lds_table) {
    PredictAreas a;
    a.W = (R + 31) / 32;
    a.slab = C < ACQ_SLAB ? C : ACQ_SLAB;
    a.cpad = round_up(a.slab, TILE);
    const size_t nb = (size_t)Bc, tiles = (size_t)acq_partials(C);
    Carve cv{static_cast<char *>(workspace)};
    a.ccodes = cv.take<uint32_t>(nb * a.W * a.cpad);
    a.tab = cv.take<double>(lds_table ? nb * acq_table_doubles(R) : 0);
    a.acc = cv.take<double>((size_t)4 * C);
    a.flag = cv.take<int32_t>(1);
    a.sacc = cv.take<double>(want_scores ? (size_t)3 * C : 0);
    a.mpart = cv.take<double>(want_scores ? 2 * tiles : 0);
    a.fpart = cv.take<double>(want_scores ? (size_t)B * 2 * tiles : 0);
    a.fslab = cv.take<double>(Q > 0 && !want_forest ? (size_t)2 * B * a.slab : 0);
    a.total = cv.o;
    return a;
}

size_t bark_leaf_posterior_predict_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t Bc, int64_t C, int64_t Q,
                                                   int want_forest, int want_scores, int variant) {
    int var = 0;
    if (B < 1 || Bc < 1 || C < 1 || C > (1 << 24) || Q < 0 || Q > PRED_MAX_PROBS || bark_acquisition_plan(max_bits, m, variant, &var, nullptr)) {
        error_buffer()[0] = 0;  // a query reports through its value only
        return 0;
    }
    if (Bc > B) Bc = B;
    if (Bc > 65535) Bc = 65535;
    return predict_areas(nullptr, max_bits, B, Bc, C, Q, want_forest != 0, want_scores != 0, var == 1).total;
}

// Slab by slab of points, and inside a slab chunk by chunk of forests: the walk and predict_scan_kernel; after a slab's last
// chunk its quantiles, from the rows the scan stored.  The finish after the last slab.  The state is only read.  Every
// argument is checked before the context is, so a refusal needs no device.
int bark_leaf_posterior_predict_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                    const double *scale, const void *state, size_t state_bytes, const double *points, int64_t C,
                                    const double *weights, int observation, const double *y_points, const double *probs,
                                    const double *zscores, int64_t Q, int variant, double *moments_out, double *forest_out,
                                    double *quantiles_out, double *per_forest_out, double *mixture_out, double *values_out,
                                    int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_leaf_posterior_predict_hip";
    error_buffer()[0] = 0;
    if (!info || !points || !moments_out || !state) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (C < 1 || C > (1 << 24)) return fail(BARK_ERR_ARG, "%s: bad shape C=%lld", name, (long long)C);
    if (Q < 0 || Q > PRED_MAX_PROBS)
        return fail(BARK_ERR_ARG, "%s: between 0 and %lld probabilities per call (got %lld)", name, (long long)PRED_MAX_PROBS, (long long)Q);
    if (Q > 0 && (!probs || !zscores)) return fail(BARK_ERR_ARG, "%s: quantiles need probs and zscores", name);
    if ((Q > 0) != (quantiles_out != nullptr)) return fail(BARK_ERR_ARG, "%s: quantiles_out is given exactly when Q > 0", name);
    for (int64_t q = 0; q < Q; ++q)
        if (!(probs[q] > 0.0 && probs[q] < 1.0) || !std::isfinite(zscores[q]))
            return fail(BARK_ERR_ARG, "%s: every probability must lie strictly inside (0, 1), with a finite zscore (got %g, %g)", name,
                        probs[q], zscores[q]);
    const bool want_scores = y_points != nullptr;
    if (want_scores != (per_forest_out != nullptr) || want_scores != (mixture_out != nullptr))
        return fail(BARK_ERR_ARG, "%s: y_points, per_forest_out and mixture_out are given together or not at all", name);
    if (values_out && !want_scores) return fail(BARK_ERR_ARG, "%s: values_out needs y_points", name);
    if (observation != 0 && observation != 1) return fail(BARK_ERR_ARG, "%s: observation is 0 or 1 (got %d)", name, observation);
    int var = 0, rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, variant, &var, nullptr))) return rc;
    if (info->B < 1) return fail(BARK_ERR_ARG, "%s: bad shape B=%lld", name, (long long)info->B);
    const size_t need_state = posterior_state(nullptr, info->max_bits, info->B).total;
    if (state_bytes < need_state) return fail(BARK_ERR_ARG, "%s: state buffer too small: %zu < %zu bytes", name, state_bytes, need_state);
    if (reinterpret_cast<uintptr_t>(state) & 255) return fail(BARK_ERR_ARG, "%s: state and workspace must be 256-byte aligned", name);
    FittedCall fc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const int R = fc.R, m = fc.m, B = (int)fc.B;
    const PredictAreas a = predict_areas(workspace, R, B, fc.Bc, C, Q, forest_out != nullptr, want_scores, var == 1);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const int W = (int)a.W, tiles = (int)acq_partials(C);
    const PosteriorState &st = fc.st;
    const double wq = 1.0 / (double)B;
    const bool one_chunk = fc.Bc >= fc.B;
    if ((rc = fc.copy_info(st.info, info_out, B))) return rc;
    if (var == 1 && one_chunk && (rc = acq_pack(st.Minv, st.w, R, B, a.tab, fc.caller))) return rc;
    for (int64_t s0 = 0; s0 < C; s0 += ACQ_SLAB) {
        const int64_t n = C - s0 < ACQ_SLAB ? C - s0 : ACQ_SLAB;
        // where the scan stores mu_b / var_b of this slab, row b of all B forests at b * fstride: the caller's array or the slab
        // (an area of no bytes still has an address: the slab is named only when it was asked for)
        double *slab = Q > 0 && !forest_out ? a.fslab : nullptr;
        double *fmu = forest_out ? forest_out + s0 : slab;
        double *fvar = forest_out ? forest_out + (size_t)B * C + s0 : (slab ? slab + (size_t)B * a.slab : nullptr);
        const size_t fstride = forest_out ? (size_t)C : (size_t)a.slab;
        for (int64_t c0 = 0; c0 < fc.B; c0 += fc.Bc) {
            const int bc = (int)(fc.B - c0 < fc.Bc ? fc.B - c0 : fc.Bc);
            bark_pack_info sub;
            const char *packed_c = fc.chunk(c0, bc, sub);
            const double *w = st.w + (size_t)c0 * R, *Minv = st.Minv + (size_t)c0 * R * R;
            if (var == 1 && !one_chunk && (rc = acq_pack(Minv, w, R, bc, a.tab, fc.caller))) return rc;
            if ((rc = walk_one_hot(packed_c, &sub, points + (size_t)s0 * fc.d, n, fc.d, W, a.ccodes, ctx->fault, fc.caller))) return rc;
            rc = predict_scan(var, want_scores, a.ccodes, W, (int)bark_leaf_npad(n), (int)n, w, Minv, a.tab, R, noise + c0, scale + c0, m,
                              bc, st.info + c0, weights ? weights + c0 : nullptr, wq, observation,
                              want_scores ? y_points + s0 : nullptr, c0 == 0, a.acc + s0, (size_t)C, want_scores ? a.sacc + s0 : nullptr,
                              fmu ? fmu + (size_t)c0 * fstride : nullptr, fmu ? fvar + (size_t)c0 * fstride : nullptr, fstride,
                              want_scores ? a.fpart + (size_t)c0 * tiles * 2 : nullptr, tiles, (int)(s0 / ACQ_TILE), fc.caller);
            if (rc || (rc = fc.fault_info(info_out + c0, bc))) return rc;
        }
        if (Q > 0) {
            if ((rc = predict_flag(info_out, weights, B, a.flag, fc.caller))) return rc;
            rc = predict_quantiles(fmu, fvar, fstride, (int)n, B, weights, wq, probs, zscores, (int)Q, a.flag, quantiles_out + s0, (size_t)C,
                                   fc.caller);
            if (rc) return rc;
        }
    }
    if ((rc = predict_flag(info_out, weights, B, a.flag, fc.caller))) return rc;
    if (want_scores) {
        if ((rc = score_forests(a.fpart, tiles, B, per_forest_out, fc.caller))) return rc;
        rc = predict_score_finish(a.acc, a.sacc, C, B, weights, y_points, values_out, a.mpart, info_out, a.flag, per_forest_out,
                                  mixture_out, fc.caller);
        if (rc) return rc;
    }
    return predict_finish(a.acc, C, B, info_out, a.flag, moments_out, forest_out, quantiles_out, (int)Q, fc.caller);
}

// Predictive scores (include/bark_hip.h, kernels in scores.hip): the scan's sequence with the points in place of the
// candidates; the per-forest rows are finished chunk by chunk, the mixture after the last chunk.
int bark_predictive_scores_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, const double *X, int64_t N,
                               int64_t d, const double *y, const double *noise, const double *scale, const double *points,
                               int64_t C, const double *y_points, int mode, int variant, double *per_forest_out,
                               double *mixture_out, double *values_out, int32_t *info_out, void *workspace,
                               size_t workspace_bytes, int64_t Bc, void *stream_) {
    error_buffer()[0] = 0;
    if (!info || !scale || !points || !y_points || !per_forest_out || !mixture_out)
        return fail(BARK_ERR_ARG, "bark_predictive_scores_hip: null argument");
    if (C < 1) return fail(BARK_ERR_ARG, "bark_predictive_scores_hip: bad shape C=%lld", (long long)C);
    if (mode != BARK_SCORE_HELDOUT && mode != BARK_SCORE_LOO) return fail(BARK_ERR_ARG, "bark_predictive_scores_hip: unknown mode %d", mode);
    if (mode == BARK_SCORE_LOO && C != N)
        return fail(BARK_ERR_ARG, "bark_predictive_scores_hip: leave-one-out scores are taken at the N = %lld training points (got C = %lld)",
                    (long long)N, (long long)C);
    int var = 0, rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, variant, &var, nullptr))) return rc;
    LeafSystem sys;
    rc = sys.open("bark_predictive_scores_hip", ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, C,
                  scores_needs(C), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    const int tiles = (int)acq_partials(C);
    double *mpart = a.spart, *fpart = a.spart + (size_t)2 * tiles;
    rc = sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, scale + c0, info_out + c0, nullptr, 0);
        if (r || (r = sys.solve_w_minv())) return r;
        if (var == 1 && (r = acq_pack(a.Minv, a.w, sys.R, sys.bc, a.tab, sys.caller))) return r;
        for (int64_t s0 = 0; s0 < C; s0 += ACQ_SLAB) {
            const int64_t n = C - s0 < ACQ_SLAB ? C - s0 : ACQ_SLAB;
            if ((r = sys.walk_candidates(points + (size_t)s0 * d, n))) return r;
            r = score_scan(var, mode, a.ccodes, sys.W, (int)bark_leaf_npad(n), (int)n, a.w, a.Minv, a.tab, sys.R, noise + c0,
                           scale + c0, sys.m, sys.bc, info_out + c0, y_points + s0, c0 == 0, a.acc + s0, (size_t)C, fpart, tiles,
                           (int)(s0 / ACQ_TILE), sys.caller);
            if (r) return r;
        }
        if ((r = score_forests(fpart, tiles, sys.bc, per_forest_out + 2 * c0, sys.caller))) return r;
        return sys.close_chunk();
    });
    if (rc) return rc;
    return score_finish(a.acc, C, (int)sys.B, y_points, values_out, mpart, info_out, per_forest_out, mixture_out, sys.caller);
}

// The noise/scale half of the sampler step for nc chains (include/bark_hip.h): the MLL + inverse sequence for one chunk of nc
// forests, with the Metropolis decision between the MLL and the N x N expansion, which only accepted chains run.  The
// decision reads the fault flag itself, so the chunk is not closed.
int bark_noise_scale_step_chains_hip(bark_ctx *ctx, double *K_inv, int64_t N, int64_t nc, const void *packed,
                                     const bark_pack_info *info, const double *X, int64_t d, const double *y,
                                     const double *new_noise, const double *new_scale, const double *log_q_prior,
                                     const double *log_u, double *state, int32_t *accept_out, void *workspace,
                                     size_t workspace_bytes, void *stream_) {
    error_buffer()[0] = 0;
    if (!K_inv || !info || !new_scale || !log_q_prior || !log_u || !state)
        return fail(BARK_ERR_ARG, "bark_noise_scale_step_chains_hip: null argument");
    if (nc < 1 || nc > SAMPLER_MAX_CHAINS)
        return fail(BARK_ERR_ARG, "bark_noise_scale_step_chains_hip: 1 to %d chains (got %lld)", SAMPLER_MAX_CHAINS, (long long)nc);
    if (info->B != nc)
        return fail(BARK_ERR_ARG, "bark_noise_scale_step_chains_hip: %lld packed forests for %lld chains", (long long)info->B,
                    (long long)nc);
    if (info->m > LEAF_INV_MAX_TREES)
        return fail(BARK_ERR_ARG, "bark_noise_scale_step_chains_hip: at most %d trees (got %lld)", LEAF_INV_MAX_TREES,
                    (long long)info->m);
    LeafSystem sys;
    int rc = sys.open("bark_noise_scale_step_chains_hip", ctx, packed, info, X, N, d, y, new_noise, accept_out, workspace,
                      workspace_bytes, nc, 0, chain_step_needs(), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    return sys.for_chunks([&](int64_t) -> int {
        const int bc = sys.bc;
        int r = sys.factor_chunk(new_noise, new_scale, a.sweep_info, a.new_mll, 0);
        if (r) return r;
        r = noise_scale_decide(a.new_mll, state, new_noise, log_q_prior, log_u, a.sweep_info, ctx->fault, bc, accept_out, sys.caller);
        // w and M^-1 for every chain (R x R); the N x R and N x N passes run for accepted chains only
        if (r || (r = sys.solve_w_minv())) return r;
        r = leafspace_inverse(a.codes, sys.W, (int)a.npad, (int)N, a.Minv, a.w, sys.R, y, new_noise, new_scale, sys.m, bc, a.Wm, K_inv,
                              a.kinv_y, accept_out, sys.caller);
        if (r) return r;
        return noise_scale_state(a.kinv_y, y, (int)N, a.new_mll, accept_out, bc, state, sys.caller);
    });
}

}  // extern "C"
