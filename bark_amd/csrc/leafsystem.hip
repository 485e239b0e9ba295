// Host side of the leaf-space entry points: MLL and posterior, explicit inverse, joint draws, the acquisition scans, the
// predictive scores and the sampler's noise/scale step.  They factorise I_R + c Z'Z (R x R) instead of K_s (N x N).
// LeafSystem is what all of them share: one workspace layout (leaf_areas), one opening sequence and the per-chunk steps.  An
// entry point checks its own arguments, says what it keeps in the workspace (LeafNeeds), opens the system and hands
// for_chunks a body that lists the steps it takes.
// The kernels are elsewhere: the R x R Cholesky sweep in chol.hip (reached through SystemSweep, common.h), the leaf-space
// kernels in leafspace.hip, sample.hip, acquire.hip and scores.hip; this unit's only kernels move status words
// (fault_info_kernel, copy_info_kernel).
// A fitted posterior is the part of that state which outlives a call: M^-1, w and the sweep's status of all B forests in a
// buffer of the caller's (PosteriorState, leaf_state.h).  bark_leaf_posterior_fit_hip writes it and is a LeafSystem call, so
// it lives here; the calls that start from it are in fitted.hip, which shares with this unit what common.h lists under
// `leafsystem.hip`: the two status launchers, the chunk of forests, and the checks and the per-chunk part of the scan.
#include <cmath>

#include "sampler_step.h"  // -> common.h

namespace bark {
namespace {

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

struct LeafSystem : ForestChunk {
    const double *X = nullptr, *y = nullptr;
    int64_t N = 0;
    LeafAreas a{};
    SystemSweep *sw = nullptr;  // the R x R sweep (chol.hip)
    // from factor_chunk on: the current chunk's systems in the sweep's workspace and the sweep's status
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

    // body(c0) for each chunk of at most Bc forests, c0 its first forest; the chunk (ForestChunk) is set for the steps below
    template <class F> int for_chunks(F &&body) {
        auto chunk = [&](int64_t b0, int64_t n) -> int {
            set_chunk(b0, n);
            return body(b0);
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
        if ((rc = walk(X, N, a.codes))) return rc;
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
    // an invalid categorical value met by one of the chunk's walks goes into its forests' info
    int close_chunk() { return take_fault(chunk_info); }
};

}  // namespace

int copy_info(const int32_t *src, int32_t *dst, int n, hipStream_t s) {
    hipLaunchKernelGGL(copy_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int fault_info(const int32_t *fault, int32_t *info, int n, hipStream_t s) {
    hipLaunchKernelGGL(fault_info_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fault, info, n);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int check_scan_args(const char *name, const bark_pack_info *info, const double *cand, int64_t C, const double *pending, int64_t P,
                    const int64_t *skip_idx, int64_t n_skip, const double *targets, int64_t S, double kappa, int kind, int variant,
                    const double *best_out, const int64_t *idx_out, int *var) {
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
    return bark_acquisition_plan(info->max_bits, info->m, variant, var, nullptr);
}

// both confidence bounds scan as BARK_ACQ_LCB_MEAN and take no targets: they differ in the finish only
int scan_chunk(const ForestChunk &ck, int var, int kind, const double *cand, int64_t C, const double *w, const double *Minv,
               double *tab, uint32_t *ccodes, double *acc, const double *noise, const double *scale, double kappa,
               const double *targets, int64_t S, const double *weights) {
    const bool lcb = kind == BARK_ACQ_LCB_MEAN || kind == BARK_ACQ_LCB_MIXTURE;
    const int64_t c0 = ck.c0;
    int rc;
    if (var == 1 && (rc = acq_pack(Minv, w, ck.R, ck.bc, tab, ck.caller))) return rc;
    return for_slabs(C, [&](int64_t s0, int64_t n) -> int {
        const int r = ck.walk(cand + (size_t)s0 * ck.d, n, ccodes);
        if (r) return r;
        return acq_scan(var, lcb ? BARK_ACQ_LCB_MEAN : kind, ccodes, ck.W, (int)bark_leaf_npad(n), (int)n, w, Minv, tab, ck.R, noise + c0,
                        scale + c0, ck.m, ck.bc, kappa, lcb ? nullptr : targets + (size_t)c0 * S, lcb ? 0 : (int)S, c0 == 0, acc + s0,
                        (size_t)C, weights ? weights + c0 : nullptr, ck.caller);
    });
}

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
            if ((r = sys.solve_w_minv()) || (r = sys.walk(cand, C, a.ccodes))) return r;
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
        if (r || (r = sys.solve_w()) || (r = sys.walk(cand, C, a.ccodes))) return r;
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
    static const char *name = "bark_acquisition_scan_hip";
    if (!scale) return fail(BARK_ERR_ARG, "%s: null argument", name);
    int var = 0, rc;
    if ((rc = check_scan_args(name, info, cand, C, pending, P, skip_idx, n_skip, targets, S, kappa, kind, variant, best_out, idx_out, &var)))
        return rc;
    LeafSystem sys;
    rc = sys.open(name, ctx, packed, info, X, N, d, y, noise, info_out, workspace, workspace_bytes, Bc, C, scan_needs(C, P), stream_);
    if (rc) return rc;
    const LeafAreas &a = sys.a;
    rc = sys.for_chunks([&](int64_t c0) -> int {
        int r = sys.factor_chunk(noise + c0, scale + c0, info_out + c0, nullptr, 0);
        if (r || (r = sys.solve_w_minv())) return r;
        if (P > 0) {
            if ((r = sys.walk(pending, P, a.pcodes))) return r;
            r = acq_condition(a.pcodes, sys.W, (int)a.ppad, (int)P, a.Minv, sys.R, noise + c0, scale + c0, sys.m, sys.bc,
                              info_out + c0, sys.caller);
            if (r) return r;
        }
        r = scan_chunk(sys, var, kind, cand, C, a.w, a.Minv, a.tab, a.ccodes, a.acc, noise, scale, kappa, targets, S, nullptr);
        if (r) return r;
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

// ---- fitted posterior (include/bark_hip.h): the fit; the calls that start from the state are in fitted.hip ----

size_t bark_leaf_posterior_fit_workspace_bytes(int64_t N, int64_t max_bits, int64_t m, int64_t Bc) {
    if (N < 1 || Bc < 1 || !posterior_shape_ok(max_bits, m, 1)) return 0;
    return leaf_areas(nullptr, N, max_bits, m, Bc, fit_needs()).total;
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
    return copy_info(st.info, info_out, (int)sys.B, sys.caller);
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
        r = for_slabs(C, [&](int64_t s0, int64_t n) -> int {
            const int q = sys.walk(points + (size_t)s0 * d, n, a.ccodes);
            if (q) return q;
            return score_scan(var, mode, a.ccodes, sys.W, (int)bark_leaf_npad(n), (int)n, a.w, a.Minv, a.tab, sys.R, noise + c0,
                              scale + c0, sys.m, sys.bc, info_out + c0, y_points + s0, c0 == 0, a.acc + s0, (size_t)C, fpart, tiles,
                              (int)(s0 / ACQ_TILE), sys.caller);
        });
        if (r || (r = score_forests(fpart, tiles, sys.bc, per_forest_out + 2 * c0, sys.caller))) return r;
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
