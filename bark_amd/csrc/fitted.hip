// Host side of the calls that start from a fitted leaf-space posterior (include/bark_hip.h): the acquisition scan from the
// state, plain and weighted, the fidelity gain, condition / observe, which change the state in place, predict and the joint
// covariance.  The state (PosteriorState, leaf_state.h) is written by bark_leaf_posterior_fit_hip, a LeafSystem call
// (leafsystem.hip); these calls factorise nothing, so they have no sweep and no LeafSystem.  FittedCall is what they share: the
// checks, the state's areas, the chunk loop and its per-chunk steps.  An entry point checks its own arguments, opens the call,
// carves its workspace and hands for_chunks a body.
// This unit defines no kernel: the scan's are in acquire.hip, the others in fidelity.hip, predict.hip, covariance.hip and
// scores.hip, and the two that move status words in leafsystem.hip.
#include <cmath>

#include "common.h"

namespace bark {
namespace {

// The workspace of the scan from a state and of condition / observe (nothing of size N): the codes of one slab of candidates
// and of the pending points for Bc forests, the LDS image when that variant runs, the scan's sums and partials, and the
// scratch M^-1 that the pending points are conditioned into.  C == 0: conditioning only.
struct FittedAreas {
    int64_t cpad, ppad;
    uint32_t *ccodes, *pcodes;
    double *tab, *acc, *part, *Minv;
    int64_t *part_i;
    size_t total;
};
FittedAreas fitted_areas(void *workspace, int64_t R, int64_t Bc, int64_t C, int64_t P, bool lds_table, bool scratch) {
    FittedAreas a;
    const int64_t W = (R + 31) / 32;
    a.cpad = C > 0 ? round_up(C < ACQ_SLAB ? C : ACQ_SLAB, TILE) : 0;
    a.ppad = P > 0 ? round_up(P, TILE) : 0;
    const size_t nb = (size_t)Bc, partials = C > 0 ? acq_partials(C) : 0;
    Carve cv{static_cast<char *>(workspace)};
    a.ccodes = cv.take<uint32_t>(nb * W * a.cpad);
    a.pcodes = cv.take<uint32_t>(nb * W * a.ppad);
    a.tab = cv.take<double>(lds_table ? nb * acq_table_doubles(R) : 0);
    a.acc = cv.take<double>((size_t)3 * C);
    a.part = cv.take<double>(partials);
    a.part_i = cv.take<int64_t>(partials);
    a.Minv = cv.take<double>(scratch && P > 0 ? nb * R * R : 0);
    a.total = cv.o;
    return a;
}

// What the calls on a fitted state share.  Nothing is launched before a refusal, and open looks at its arguments and their
// shape before it looks at the context: a call with a bad argument and a bad context reports the argument, so such a refusal
// needs no device.  The state's size and the alignment of the two buffers come after the context; an entry point that
// promises those refusals without a device too (predict) asks check_state first.
struct FittedCall : ForestChunk {
    const double *noise = nullptr, *scale = nullptr;
    PosteriorState st{};

    static int check_state(const char *name, const bark_pack_info *info, const void *state, size_t state_bytes) {
        const size_t need = posterior_state(nullptr, info->max_bits, info->B).total;
        if (state_bytes < need) return fail(BARK_ERR_ARG, "%s: state buffer too small: %zu < %zu bytes", name, state_bytes, need);
        if (reinterpret_cast<uintptr_t>(state) & 255) return fail(BARK_ERR_ARG, "%s: state and workspace must be 256-byte aligned", name);
        return BARK_OK;
    }
    int open(const char *name, bark_ctx *ctx_, const void *packed_, const bark_pack_info *info_, int64_t d_, const double *noise_,
             const double *scale_, const void *state, size_t state_bytes, const void *info_out, const void *workspace, int64_t Bc_,
             void *stream) {
        if (!packed_ || !info_ || !noise_ || !scale_ || !state || !info_out || !workspace) return fail(BARK_ERR_ARG, "%s: null argument", name);
        packed = packed_, info = info_, d = d_, B = info->B, Bc = Bc_, noise = noise_, scale = scale_;
        if (d < 1 || B < 1 || Bc < 1) return fail(BARK_ERR_ARG, "%s: bad shape d=%lld B=%lld Bc=%lld", name, (long long)d, (long long)B, (long long)Bc);
        if (!posterior_shape_ok(info->max_bits, info->m, B))
            return fail(BARK_ERR_ARG, "%s: a fitted posterior holds forests of at most %d trees and 8192 leaves (got m = %lld, R = %lld)", name,
                        ACQ_MAX_TREES, (long long)info->m, (long long)info->max_bits);
        int rc;
        if ((rc = check_ctx(ctx_)) || (rc = check_state(name, info, state, state_bytes))) return rc;
        if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(BARK_ERR_ARG, "%s: state and workspace must be 256-byte aligned", name);
        if (Bc > B) Bc = B;
        if (Bc > 65535) Bc = 65535;
        ctx = ctx_, m = (int)info->m, R = (int)info->max_bits, W = (R + 31) / 32;
        st = posterior_state(const_cast<void *>(state), R, B);
        caller = static_cast<hipStream_t>(stream);
        return BARK_OK;
    }
    // body() for each chunk of at most Bc forests, until one fails; the accessors below describe the chunk to it
    template <class F> int for_chunks(F &&body) {
        for (int64_t b0 = 0; b0 < B; b0 += Bc) {
            set_chunk(b0, B - b0 < Bc ? B - b0 : Bc);
            const int rc = body();
            if (rc) return rc;
        }
        return BARK_OK;
    }
    // the chunk's rows of the state and of the call's noise and scale
    double *w() const { return st.w + (size_t)c0 * R; }
    double *Minv() const { return st.Minv + (size_t)c0 * R * R; }
    int32_t *status() const { return st.info + c0; }
    const double *noise_c() const { return noise + c0; }
    const double *scale_c() const { return scale + c0; }
    // the faults of the chunk's walks into its part of dst (B status words: the state's, or the call's info_out)
    int close_chunk(int32_t *dst) const { return take_fault(dst + c0); }
    int copy_status(int32_t *info_out) const { return copy_info(st.info, info_out, (int)B, caller); }
};

// condition and observe: the state changed in place by `step`, chunk by chunk, from the codes of the P points in a.pcodes.
// A fault of the walk marks the state's status too: its M^-1 has then been conditioned on a leaf that means nothing.
template <class Step>
int update_state(const char *name, bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                 const double *scale, const double *points, int64_t P, void *state, size_t state_bytes, int32_t *info_out,
                 void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_, Step &&step) {
    if (P > 0 && !points) return fail(BARK_ERR_ARG, "%s: null argument", name);
    FittedCall fc;
    int rc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FittedAreas a = fitted_areas(workspace, fc.R, fc.Bc, 0, P, false, false);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    rc = P == 0 ? BARK_OK : fc.for_chunks([&]() -> int {
        int r = fc.walk(points, P, a.pcodes);
        if (r || (r = step(fc, a))) return r;
        return fc.close_chunk(fc.st.info);
    });
    if (rc) return rc;
    return fc.copy_status(info_out);
}

// ---- information gain of a (query, target) pair from the state (kernels in fidelity.hip) ----

constexpr int64_t FID_MAX_CAND = 1 << 16, FID_MAX_ADAPT = 1024, FID_MAX_GRID = 4096;

// The workspace of the gain: the codes of the C query and the C target points for Bc forests, the moments of the chunk's
// pairs, their values (unused when the caller takes per_forest_out: the kernels then write the chunk's rows there), and the
// running sums.
struct FidelityAreas {
    int64_t cpad;
    uint32_t *qcodes, *tcodes;
    double *mom, *g, *acc;
    size_t total;
};
FidelityAreas fidelity_areas(void *workspace, int64_t R, int64_t Bc, int64_t C) {
    FidelityAreas a;
    const int64_t W = (R + 31) / 32;
    a.cpad = round_up(C, TILE);
    const size_t nb = (size_t)Bc;
    Carve cv{static_cast<char *>(workspace)};
    a.qcodes = cv.take<uint32_t>(nb * W * a.cpad);
    a.tcodes = cv.take<uint32_t>(nb * W * a.cpad);
    a.mom = cv.take<double>(nb * FID_MOMENTS * C);
    a.g = cv.take<double>(nb * C);
    a.acc = cv.take<double>((size_t)C);
    a.total = cv.o;
    return a;
}
bool fidelity_shape_ok(int64_t max_bits, int64_t m, int64_t C, int64_t S) {
    return posterior_shape_ok(max_bits, m, 1) && C >= 1 && C <= FID_MAX_CAND && S >= 1 && S <= ACQ_MAX_TARGETS;
}

// ---- predictions from the state (kernels in predict.hip) ----

constexpr int64_t PRED_MAX_PROBS = 16;

// The workspace of the predict call: the codes of one slab of points for Bc forests, the LDS image when that variant runs,
// the (4, C) recurrence state, the flag word, with scores the (3, C) score state and the tile partials of the mixture
// (tiles, 2) and of all B forests (B, tiles, 2: the slabs are the outer loop, so a forest's tiles are complete only at the
// end), and mu_b / var_b of one slab (2, B, slab) when quantiles are asked for and forest_out does not hold them.
struct PredictAreas {
    int64_t cpad, slab;
    uint32_t *ccodes;
    double *tab, *acc, *sacc, *mpart, *fpart, *fslab;
    int32_t *flag;
    size_t total;
};
PredictAreas predict_areas(void *workspace, int64_t R, int64_t B, int64_t Bc, int64_t C, int64_t Q, bool want_forest, bool want_scores,
                           bool lds_table) {
    PredictAreas a;
    const int64_t W = (R + 31) / 32;
    a.slab = C < ACQ_SLAB ? C : ACQ_SLAB;
    a.cpad = round_up(a.slab, TILE);
    const size_t nb = (size_t)Bc, tiles = (size_t)acq_partials(C);
    Carve cv{static_cast<char *>(workspace)};
    a.ccodes = cv.take<uint32_t>(nb * W * a.cpad);
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

// ---- joint covariance from the state (kernels in covariance.hip) ----

constexpr int64_t COV_MAX_POINTS = ACQ_SLAB;  // points per side: one slab of codes

// The workspace of the covariance call: the codes of the C1 row points and, unless the call is symmetric, of the C2 column
// points for Bc forests; for the mixture the (4, C) recurrence state and mu_b / var_b (2, B, C) of each side (predict_scan's)
// and the flag word; and the blocks of one chunk (Bc, C1, C2) when the caller takes no forest_out to hold them.
struct CovAreas {
    int64_t cpad1, cpad2;
    uint32_t *codes1, *codes2;
    double *acc1, *acc2, *fm1, *fm2, *cov;
    int32_t *flag;
    size_t total;
};
CovAreas cov_areas(void *workspace, int64_t R, int64_t B, int64_t Bc, int64_t C1, int64_t C2, bool symmetric, bool want_forest,
                   bool want_mixture) {
    CovAreas a;
    const int64_t W = (R + 31) / 32;
    a.cpad1 = round_up(C1, TILE);
    a.cpad2 = symmetric ? a.cpad1 : round_up(C2, TILE);
    const size_t nb = (size_t)Bc;
    Carve cv{static_cast<char *>(workspace)};
    a.codes1 = cv.take<uint32_t>(nb * W * a.cpad1);
    a.codes2 = cv.take<uint32_t>(symmetric ? 0 : nb * W * a.cpad2);
    a.acc1 = cv.take<double>(want_mixture ? (size_t)4 * C1 : 0);
    a.acc2 = cv.take<double>(want_mixture && !symmetric ? (size_t)4 * C2 : 0);
    a.fm1 = cv.take<double>(want_mixture ? (size_t)2 * B * C1 : 0);
    a.fm2 = cv.take<double>(want_mixture && !symmetric ? (size_t)2 * B * C2 : 0);
    a.flag = cv.take<int32_t>(1);
    a.cov = cv.take<double>(want_forest ? 0 : nb * C1 * C2);
    a.total = cv.o;
    if (symmetric) a.codes2 = a.codes1, a.acc2 = a.acc1, a.fm2 = a.fm1;
    return a;
}
bool cov_points_ok(int64_t C) { return C >= 1 && C <= COV_MAX_POINTS; }

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

size_t bark_leaf_posterior_bytes(int64_t max_bits, int64_t m, int64_t B) {
    if (!posterior_shape_ok(max_bits, m, B)) return 0;
    return posterior_state(nullptr, max_bits, B).total;
}

size_t bark_acquisition_scan_fitted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P, int variant) {
    int var = 0;
    if (Bc < 1 || C < 1 || C > (1 << 24) || P < 0 || P > ACQ_MAX_PENDING || bark_acquisition_plan(max_bits, m, variant, &var, nullptr)) {
        error_buffer()[0] = 0;  // a query reports through its value only
        return 0;
    }
    return fitted_areas(nullptr, max_bits, Bc, C, P, var == 1, true).total;
}

// the weights stay where the caller has them: nothing is added to the workspace
size_t bark_acquisition_scan_fitted_weighted_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t C, int64_t P,
                                                             int variant) {
    return bark_acquisition_scan_fitted_workspace_bytes(max_bits, m, Bc, C, P, variant);
}

// The scan of bark_acquisition_scan_targets_hip from its `P > 0` on, with M^-1 and w read from the state.  The state is only
// read: pending points condition a copy of the chunk's M^-1 in the workspace (acq_condition_from_kernel).  info_out starts
// as the state's status and takes the faults of this call's walks.
//
// weights (device, (B,), normalised by the caller) or null, which is bark_acquisition_scan_fitted_hip.  The weighted
// instantiation of the scan and the finish without the division by B; a chunk whose first forests have weight 0 still passes
// `first`, because the kernel starts its sums at zero whichever forest it skips.  Pending points condition the scratch copy
// of every forest, whatever its weight: that kernel does not know about weights.
int bark_acquisition_scan_fitted_weighted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d,
                                              const double *noise, const double *scale, const void *state, size_t state_bytes,
                                              const double *cand, int64_t C, const double *pending, int64_t P,
                                              const int64_t *skip_idx, int64_t n_skip, const double *targets, int64_t S, double kappa,
                                              int kind, int variant, const double *weights, double *acq_out, double *best_out,
                                              int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                                              void *stream_) {
    static const char *name = "bark_acquisition_scan_fitted_hip";  // in the messages of both entry points
    error_buffer()[0] = 0;
    int var = 0, rc;
    if ((rc = check_scan_args(name, info, cand, C, pending, P, skip_idx, n_skip, targets, S, kappa, kind, variant, best_out, idx_out, &var)))
        return rc;
    FittedCall fc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const FittedAreas a = fitted_areas(workspace, fc.R, fc.Bc, C, P, var == 1, true);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    if ((rc = fc.copy_status(info_out))) return rc;
    rc = fc.for_chunks([&]() -> int {
        int r;
        const double *Minv = fc.Minv();
        if (P > 0) {
            if ((r = fc.walk(pending, P, a.pcodes))) return r;
            r = acq_condition_from(a.pcodes, fc.W, (int)a.ppad, (int)P, Minv, a.Minv, fc.R, fc.noise_c(), fc.scale_c(), fc.m, fc.bc,
                                   fc.status(), fc.caller);
            if (r) return r;
            Minv = a.Minv;
        }
        r = scan_chunk(fc, var, kind, cand, C, fc.w(), Minv, a.tab, a.ccodes, a.acc, noise, scale, kappa, targets, S, weights);
        if (r) return r;
        return fc.close_chunk(info_out);
    });
    if (rc) return rc;
    return acq_finish(a.acc, C, (int)fc.B, kappa, kind, skip_idx, (int)n_skip, acq_out, a.part, a.part_i, info_out, weights, best_out,
                      idx_out, fc.caller);
}

int bark_acquisition_scan_fitted_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                     const double *scale, const void *state, size_t state_bytes, const double *cand, int64_t C,
                                     const double *pending, int64_t P, const int64_t *skip_idx, int64_t n_skip, const double *targets,
                                     int64_t S, double kappa, int kind, int variant, double *acq_out, double *best_out,
                                     int64_t *idx_out, int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc,
                                     void *stream_) {
    return bark_acquisition_scan_fitted_weighted_hip(ctx, packed, info, d, noise, scale, state, state_bytes, cand, C, pending, P, skip_idx,
                                                     n_skip, targets, S, kappa, kind, variant, nullptr, acq_out, best_out, idx_out,
                                                     info_out, workspace, workspace_bytes, Bc, stream_);
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
    const int n = (int)C, cpad = (int)bark_leaf_npad(C);
    if ((rc = fc.copy_status(info_out))) return rc;
    rc = fc.for_chunks([&]() -> int {
        const int64_t c0 = fc.c0;
        const double *tg = targets + (size_t)c0 * S, *wt = weights ? weights + c0 : nullptr;
        double *g = per_forest_out ? per_forest_out + (size_t)c0 * C : a.g;  // (bc, C) either way
        int r;
        if ((r = fc.walk(query, C, a.qcodes)) || (r = fc.walk(target, C, a.tcodes))) return r;
        r = fidelity_moments(a.qcodes, a.tcodes, fc.W, cpad, n, fc.w(), fc.Minv(), fc.R, fc.noise_c(), fc.scale_c(), fc.m, fc.bc, tg,
                             (int)S, wt, a.mom, g, fc.caller);
        if (r || (r = fidelity_quadrature(a.mom, n, fc.bc, tg, (int)S, lo, hi, (int)n_a, pad, (int)G, g, fc.caller))) return r;
        if ((r = fidelity_accumulate(g, n, fc.bc, wt, c0 == 0, a.acc, fc.caller))) return r;
        return fc.close_chunk(info_out);
    });
    if (rc) return rc;
    return fidelity_finish(a.acc, n, (int)fc.B, weights, info_out, gain_out, per_forest_out, fc.caller);
}

size_t bark_leaf_posterior_condition_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P) {
    if (Bc < 1 || P < 0 || P > ACQ_MAX_PENDING || !posterior_shape_ok(max_bits, m, 1)) return 0;
    return fitted_areas(nullptr, max_bits, Bc, 0, P, false, false).total;
}

// The state conditioned in place on P more points, in the order given (acq_condition_kernel on the state's M^-1; w does not
// change).
int bark_leaf_posterior_condition_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                      const double *scale, const double *pending, int64_t P, void *state, size_t state_bytes,
                                      int32_t *info_out, void *workspace, size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_leaf_posterior_condition_hip";
    error_buffer()[0] = 0;
    if (!info) return fail(BARK_ERR_ARG, "%s: null argument", name);
    if (P < 0 || P > ACQ_MAX_PENDING)
        return fail(BARK_ERR_ARG, "%s: at most %lld pending points (got %lld)", name, (long long)ACQ_MAX_PENDING, (long long)P);
    return update_state(name, ctx, packed, info, d, noise, scale, pending, P, state, state_bytes, info_out, workspace, workspace_bytes, Bc,
                        stream_, [&](const FittedCall &fc, const FittedAreas &a) -> int {
                            return acq_condition(a.pcodes, fc.W, (int)a.ppad, (int)P, fc.Minv(), fc.R, fc.noise_c(), fc.scale_c(), fc.m,
                                                 fc.bc, fc.status(), fc.caller);
                        });
}

size_t bark_leaf_posterior_observe_workspace_bytes(int64_t max_bits, int64_t m, int64_t Bc, int64_t P) {
    return bark_leaf_posterior_condition_workspace_bytes(max_bits, m, Bc, P);
}

// The state conditioned in place on P more points with values, in the order given (acq_observe_kernel on the state's M^-1 and
// w).  The values stay on the device: they are not read back, so a NaN value gives a NaN w and no status.
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
    if (mode != BARK_OBSERVE_VALUES && mode != BARK_OBSERVE_SAMPLE) return fail(BARK_ERR_ARG, "%s: unknown mode %d", name, mode);
    if (mode == BARK_OBSERVE_VALUES && !values) return fail(BARK_ERR_ARG, "%s: BARK_OBSERVE_VALUES needs values", name);
    if (value_stride != 0 && value_stride != P)
        return fail(BARK_ERR_ARG, "%s: value_stride is 0 (one vector for all forests) or P (got %lld)", name, (long long)value_stride);
    if (draw < 0 || draw > 0xFFFFFFFFll) return fail(BARK_ERR_ARG, "%s: draw number outside 0 .. 2^32 - 1", name);
    return update_state(name, ctx, packed, info, d, noise, scale, points, P, state, state_bytes, info_out, workspace, workspace_bytes, Bc,
                        stream_, [&](const FittedCall &fc, const FittedAreas &a) -> int {
                            const size_t c0 = (size_t)fc.c0;
                            return acq_observe(a.pcodes, fc.W, (int)a.ppad, (int)P, fc.Minv(), fc.w(), fc.R, fc.noise_c(), fc.scale_c(),
                                               fc.m, fc.bc, fc.status(), mode, values ? values + c0 * value_stride : nullptr,
                                               (int)value_stride, eps ? eps + c0 * P : nullptr, seed, fc.c0, draw,
                                               values_out ? values_out + c0 * P : nullptr, logpred_out ? logpred_out + c0 : nullptr,
                                               fc.caller);
                        });
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
// argument, the state's size and alignment included, is checked before the context is, so a refusal needs no device.
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
    if ((rc = FittedCall::check_state(name, info, state, state_bytes))) return rc;
    FittedCall fc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const int R = fc.R, B = (int)fc.B;
    const PredictAreas a = predict_areas(workspace, R, B, fc.Bc, C, Q, forest_out != nullptr, want_scores, var == 1);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const int tiles = (int)acq_partials(C);
    const double wq = 1.0 / (double)B;
    const bool one_chunk = fc.Bc >= fc.B;
    if ((rc = fc.copy_status(info_out))) return rc;
    if (var == 1 && one_chunk && (rc = acq_pack(fc.st.Minv, fc.st.w, R, B, a.tab, fc.caller))) return rc;
    rc = for_slabs(C, [&](int64_t s0, int64_t n) -> int {
        // where the scan stores mu_b / var_b of this slab, row b of all B forests at b * fstride: the caller's array or the slab
        // (an area of no bytes still has an address: the slab is named only when it was asked for)
        double *slab = Q > 0 && !forest_out ? a.fslab : nullptr;
        double *fmu = forest_out ? forest_out + s0 : slab;
        double *fvar = forest_out ? forest_out + (size_t)B * C + s0 : (slab ? slab + (size_t)B * a.slab : nullptr);
        const size_t fstride = forest_out ? (size_t)C : (size_t)a.slab;
        int r = fc.for_chunks([&]() -> int {
            const size_t c0 = (size_t)fc.c0;
            int q;
            if (var == 1 && !one_chunk && (q = acq_pack(fc.Minv(), fc.w(), R, fc.bc, a.tab, fc.caller))) return q;
            if ((q = fc.walk(points + (size_t)s0 * fc.d, n, a.ccodes))) return q;
            q = predict_scan(var, want_scores, a.ccodes, fc.W, (int)bark_leaf_npad(n), (int)n, fc.w(), fc.Minv(), a.tab, R, fc.noise_c(),
                             fc.scale_c(), fc.m, fc.bc, fc.status(), weights ? weights + c0 : nullptr, wq, observation,
                             want_scores ? y_points + s0 : nullptr, c0 == 0, a.acc + s0, (size_t)C, want_scores ? a.sacc + s0 : nullptr,
                             fmu ? fmu + c0 * fstride : nullptr, fmu ? fvar + c0 * fstride : nullptr, fstride,
                             want_scores ? a.fpart + c0 * tiles * 2 : nullptr, tiles, (int)(s0 / ACQ_TILE), fc.caller);
            if (q) return q;
            return fc.close_chunk(info_out);
        });
        if (r || Q == 0) return r;
        if ((r = predict_flag(info_out, weights, B, a.flag, fc.caller))) return r;
        return predict_quantiles(fmu, fvar, fstride, (int)n, B, weights, wq, probs, zscores, (int)Q, a.flag, quantiles_out + s0, (size_t)C,
                                 fc.caller);
    });
    if (rc || (rc = predict_flag(info_out, weights, B, a.flag, fc.caller))) return rc;
    if (want_scores) {
        if ((rc = score_forests(a.fpart, tiles, B, per_forest_out, fc.caller))) return rc;
        rc = predict_score_finish(a.acc, a.sacc, C, B, weights, y_points, values_out, a.mpart, info_out, a.flag, per_forest_out,
                                  mixture_out, fc.caller);
        if (rc) return rc;
    }
    return predict_finish(a.acc, C, B, info_out, a.flag, moments_out, forest_out, quantiles_out, (int)Q, fc.caller);
}

size_t bark_leaf_posterior_covariance_workspace_bytes(int64_t max_bits, int64_t m, int64_t B, int64_t Bc, int64_t C1, int64_t C2,
                                                      int symmetric, int want_forest, int want_mixture, int variant) {
    if (symmetric) C2 = C1;
    if (B < 1 || Bc < 1 || !cov_points_ok(C1) || !cov_points_ok(C2) || (!want_forest && !want_mixture) ||
        bark_acquisition_plan(max_bits, m, variant, nullptr, nullptr)) {
        error_buffer()[0] = 0;  // a query reports through its value only
        return 0;
    }
    if (Bc > B) Bc = B;
    if (Bc > 65535) Bc = 65535;
    return cov_areas(nullptr, max_bits, B, Bc, C1, C2, symmetric != 0, want_forest != 0, want_mixture != 0).total;
}

// With a mixture, first chunk by chunk the walks and predict_scan_kernel at the row and the column points: the means of the
// mixture, its W and mu_b of every forest.  Then chunk by chunk the walks, the chunk's blocks (into forest_out, or into the
// workspace) and their sum onto mixture_out in forest order; the finish after the last chunk.  The state is only read.  Every
// argument, the state's size and alignment included, is checked before the context is, so a refusal needs no device.
int bark_leaf_posterior_covariance_hip(bark_ctx *ctx, const void *packed, const bark_pack_info *info, int64_t d, const double *noise,
                                       const double *scale, const void *state, size_t state_bytes, const double *x1, int64_t C1,
                                       const double *x2, int64_t C2, const double *weights, int observation, int variant,
                                       double *forest_out, double *mixture_out, int32_t *info_out, void *workspace,
                                       size_t workspace_bytes, int64_t Bc, void *stream_) {
    static const char *name = "bark_leaf_posterior_covariance_hip";
    error_buffer()[0] = 0;
    if (!info || !x1 || !state) return fail(BARK_ERR_ARG, "%s: null argument", name);
    const bool symmetric = x2 == nullptr;
    if (symmetric) C2 = C1;
    if (!cov_points_ok(C1) || !cov_points_ok(C2))
        return fail(BARK_ERR_ARG, "%s: between 1 and %lld points per side (got %lld and %lld)", name, (long long)COV_MAX_POINTS,
                    (long long)C1, (long long)C2);
    if (!forest_out && !mixture_out) return fail(BARK_ERR_ARG, "%s: forest_out, mixture_out or both must be given", name);
    if (observation != 0 && observation != 1) return fail(BARK_ERR_ARG, "%s: observation is 0 or 1 (got %d)", name, observation);
    if (observation && !symmetric)
        return fail(BARK_ERR_ARG, "%s: observation noise belongs to the symmetric call (x2 == NULL): two evaluations share none", name);
    int var = 0, rc;
    if ((rc = bark_acquisition_plan(info->max_bits, info->m, variant, &var, nullptr))) return rc;
    if (info->B < 1) return fail(BARK_ERR_ARG, "%s: bad shape B=%lld", name, (long long)info->B);
    if ((rc = FittedCall::check_state(name, info, state, state_bytes))) return rc;
    FittedCall fc;
    if ((rc = fc.open(name, ctx, packed, info, d, noise, scale, state, state_bytes, info_out, workspace, Bc, stream_))) return rc;
    const int R = fc.R, B = (int)fc.B;
    const bool mix = mixture_out != nullptr;
    const CovAreas a = cov_areas(workspace, R, B, fc.Bc, C1, C2, symmetric, forest_out != nullptr, mix);
    if (workspace_bytes < a.total) return fail(BARK_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, a.total);
    const double wq = 1.0 / (double)B;
    const size_t n12 = (size_t)C1 * C2;
    if ((rc = fc.copy_status(info_out))) return rc;
    if (mix) {
        // predict's recurrence at both sides, M^-1 read from global memory (its bits do not depend on its variant): rows W and
        // mean of acc, mu_b in the first B rows of fm
        rc = fc.for_chunks([&]() -> int {
            const size_t c0 = (size_t)fc.c0;
            const double *wt = weights ? weights + c0 : nullptr;
            int r;
            if ((r = fc.walk(x1, C1, a.codes1))) return r;
            r = predict_scan(2, false, a.codes1, fc.W, (int)a.cpad1, (int)C1, fc.w(), fc.Minv(), nullptr, R, fc.noise_c(), fc.scale_c(), fc.m,
                             fc.bc, fc.status(), wt, wq, 0, nullptr, c0 == 0, a.acc1, (size_t)C1, nullptr, a.fm1 + c0 * C1,
                             a.fm1 + ((size_t)B + c0) * C1, (size_t)C1, nullptr, 0, 0, fc.caller);
            if (r || symmetric) return r;
            if ((r = fc.walk(x2, C2, a.codes2))) return r;
            return predict_scan(2, false, a.codes2, fc.W, (int)a.cpad2, (int)C2, fc.w(), fc.Minv(), nullptr, R, fc.noise_c(), fc.scale_c(),
                                fc.m, fc.bc, fc.status(), wt, wq, 0, nullptr, c0 == 0, a.acc2, (size_t)C2, nullptr, a.fm2 + c0 * C2,
                                a.fm2 + ((size_t)B + c0) * C2, (size_t)C2, nullptr, 0, 0, fc.caller);
        });
        if (rc) return rc;
    }
    rc = fc.for_chunks([&]() -> int {
        const size_t c0 = (size_t)fc.c0;
        const double *wt = weights ? weights + c0 : nullptr;
        double *blocks = forest_out ? forest_out + c0 * n12 : a.cov;  // (bc, C1, C2) either way
        int r;
        if ((r = fc.walk(x1, C1, a.codes1))) return r;
        if (!symmetric && (r = fc.walk(x2, C2, a.codes2))) return r;
        r = cov_tiles(var, a.codes1, (int)a.cpad1, (int)C1, a.codes2, (int)a.cpad2, (int)C2, fc.W, fc.Minv(), R, fc.noise_c(), fc.scale_c(),
                      fc.m, fc.bc, wt, symmetric, observation, blocks, fc.caller);
        if (r) return r;
        if (mix && (r = cov_accumulate(blocks, C1, C2, a.fm1 + c0 * C1, a.acc1 + C1, a.fm2 + c0 * C2, a.acc2 + C2, wt, wq, fc.bc, c0 == 0,
                                       mixture_out, fc.caller)))
            return r;
        return fc.close_chunk(info_out);
    });
    if (rc) return rc;
    if (mix && (rc = predict_flag(info_out, weights, B, a.flag, fc.caller))) return rc;
    return cov_finish(mixture_out, C1, C2, a.acc1, a.flag, info_out, weights, B, forest_out, fc.caller);
}

}  // extern "C"
