// One-launch tree sweep for small N — the per-tree Metropolis loop of bark_sampler.py:233-264 with K_inv resident on one CU
// per chain (include/bark_hip.h: bark_tree_sweep_resident_hip).
//
// bark_tree_sweep_chains_hip (lowrank.hip) enqueues five or six small dependent launches per proposal, ~59 us whatever N is;
// the arithmetic of a proposal at N ~ 100 is about a microsecond.  Here grid = chains, one workgroup of 1024 threads per chain,
// and the workgroup loops over the steps itself.  No workgroup waits on another: barriers of the workgroup are the only
// synchronisation.  Per step, for its chain:
//   1. walk      the N points through the [old, new] pair (walk_tree, X rows and the pair's nodes in LDS):
//                one code word per point, the bit of its old leaf and the bit of its new leaf (r <= 16 leaves per pair)
//   2. Y         Y[i][c] = s * sum_{k : leaf(k) = c} K_inv[k][i]  (column form: K_inv is symmetric), thread = (column i, row
//                segment), the segments summed into LDS in segment order;  then G = U'Y and v = Y'y, one wave per row of G
//   3. algebra   den = C + G, Gauss-Jordan with partial pivoting -> den^-1, log|det|, v'den^-1 v: small_kernel's arithmetic,
//                run by ONE wave (a workgroup barrier per elimination stage would cost more than the stage)
//   4. decision  decide_kernel's two-comparison rule; an exactly zero pivot column latches the chain at -1
//   5. rewrite   K_inv -= Y den^-1 Y' in place.  With Z = Y S, S the symmetrised den^-1, entry (i, j) is
//                sum_c Y[lo][c] Z[hi][c], lo = min(i, j), hi = max(i, j): both orders of a pair evaluate the same products in the same order, so (i, j) and (j, i) get
//                the same bits and the column form stays valid for the next step.
// K_IN_LDS: K_inv[b] is copied into LDS at the start (row pitch round_up(N, 16), column index XOR (row & 15): rows and columns
// are both conflict-free) and written back once at the end, if a step accepted.  Otherwise the workgroup works on K_inv[b] in
// global memory (L2-resident for one workgroup); after a rewrite: fence, barrier, fence before the next step reads it.
// Z overlays the X rows / codes / nodes / r x r scratch, all dead by then; the X rows are staged again after a rewrite.
#include <type_traits>

#include "sampler_step.h"  // -> common.h

namespace bark {
namespace {

constexpr int SR_THREADS = 1024, SR_WAVES = SR_THREADS / 64;
constexpr int SR_RMAX = 16;                   // leaves per [old, new] pair: one 16-bit code per point
constexpr int SR_NMAX = 512;
constexpr int SR_NODE_BYTES = 2048;           // LDS of a step's packed pair: at most 64 packed nodes per tree (a tree of <= 15 leaves has <= 29)
constexpr int SR_STRIDE_MAX = SR_NODE_BYTES / (2 * 16);
constexpr int SR_AUG_LD = 2 * SR_RMAX + 1;    // [den | I], odd pitch
constexpr size_t SR_LDS_MAX = 160 * 1024;

// dynamic-LDS layout (bytes from the base; every offset a multiple of 16) and the variant, from the shape alone
struct SrPlan {
    int variant;  // 0 unsupported, 1 K_inv in LDS, 2 K_inv in global memory
    int np, sd;   // row pitch of K (LDS), Y', Z' in doubles; row pitch of the X rows
    unsigned off_y, off_r, off_codes, off_aug, off_v, off_misc, off_nodes;  // X rows and Z' start at off_r
    size_t lds;
};

SrPlan sr_plan(int64_t N, int64_t d) {
    SrPlan p{};
    if (N < 1 || N > SR_NMAX || d < 1 || d > (1 << 20)) return p;
    p.np = (int)round_up(N, 16);
    p.sd = (int)(d | 1);
    const size_t yt = (size_t)SR_RMAX * p.np * sizeof(double);
    const size_t xb = (size_t)round_up(N * p.sd * (int64_t)sizeof(double), 16), cb = (size_t)round_up(N * 4, 16);
    const size_t aug = (size_t)SR_RMAX * SR_AUG_LD * sizeof(double), vb = SR_RMAX * sizeof(double), misc = 64;
    const size_t small = xb + cb + aug + vb + misc + SR_NODE_BYTES;
    const size_t region = small > yt ? small : yt;
    const size_t kl = (size_t)N * p.np * sizeof(double);
    p.variant = kl + yt + region <= SR_LDS_MAX ? 1 : yt + region <= SR_LDS_MAX ? 2 : 0;
    p.off_y = p.variant == 1 ? (unsigned)kl : 0u;
    p.off_r = p.off_y + (unsigned)yt;
    p.off_codes = (unsigned)xb;  // relative to off_r from here on
    p.off_aug = p.off_codes + (unsigned)cb;
    p.off_v = p.off_aug + (unsigned)aug;
    p.off_misc = p.off_v + (unsigned)vb;
    p.off_nodes = p.off_misc + (unsigned)misc;
    p.lds = (p.variant == 1 ? kl : 0) + yt + region;
    return p;
}

struct SrArgs {
    double *K;
    int N, nc, n_steps, d;
    const unsigned char *packed;
    const int64_t *table;
    const double *X, *s, *y, *log_q_prior, *log_u;
    double *state;
    int32_t *accept_out, *fault;
    SrPlan plan;
};

template <bool K_IN_LDS>
__global__ __launch_bounds__(SR_THREADS) void sweep_resident_kernel(SrArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, N = p.N, np = p.plan.np, sd = p.plan.sd, nc = p.nc;
    double *Kg = p.K + (size_t)b * N * N;
    double *Kl = reinterpret_cast<double *>(smem);
    double *Yt = reinterpret_cast<double *>(smem + p.plan.off_y);  // [16][np]: Y transposed
    unsigned char *R = smem + p.plan.off_r;
    double *Zt = reinterpret_cast<double *>(R);  // [16][np], overlays everything below
    double *xs = reinterpret_cast<double *>(R);  // [N][sd]
    uint32_t *codes = reinterpret_cast<uint32_t *>(R + p.plan.off_codes);
    double *aug = reinterpret_cast<double *>(R + p.plan.off_aug);  // [16][SR_AUG_LD]
    double *vsh = reinterpret_cast<double *>(R + p.plan.off_v);
    int *misc = reinterpret_cast<int *>(R + p.plan.off_misc);  // pivot row, singular, decision
    uint4 *ln = reinterpret_cast<uint4 *>(R + p.plan.off_nodes);

    auto kload = [&](int row, int col) -> double {
        if (K_IN_LDS) return Kl[row * np + (col ^ (row & 15))];
        return Kg[(size_t)row * N + col];
    };
    auto kstore = [&](int row, int col, double v) {
        if (K_IN_LDS)
            Kl[row * np + (col ^ (row & 15))] = v;
        else
            Kg[(size_t)row * N + col] = v;
    };
    auto stage_x = [&]() {
        const double *X = p.X;
        for (int e = tid; e < N * p.d; e += SR_THREADS) {
            const int q = e / p.d, c = e - q * p.d;
            xs[q * sd + c] = X[e];
        }
    };

    if (K_IN_LDS)
        for (int e = tid; e < N * N; e += SR_THREADS) {
            const int row = e / N, col = e - row * N;
            Kl[row * np + (col ^ (row & 15))] = Kg[e];
        }
    stage_x();
    const double s = p.s[b];
    double quad = p.state[2 * b], logdet = p.state[2 * b + 1];  // thread 0's copies are the ones written back
    bool latched = false, any_accept = false;

    // thread = (column i, row segment): whole waves share a segment, so a row index is uniform in a wave
    const int npc = (int)((N + 63) / 64) * 64;
    const int col = tid % npc, seg = tid / npc;
    const int segs_all = SR_THREADS / npc;             // >= 2 (N <= 512)
    const int segs_y = segs_all < 8 ? segs_all : 8;    // Y: the segments are summed one barrier apiece
    const bool col_live = col < N && seg < segs_all;

    for (int t = 0; t < p.n_steps; ++t) {
        if (latched) {  // decide_kernel: a chain that met a singular system stays at -1, its K_inv is not touched again
            if (tid == 0) p.accept_out[(size_t)t * nc + b] = -1;
            continue;
        }
        const StepEntry st = step_entry(p.table, t, p.n_steps, nc, b, SR_STRIDE_MAX);
        const int stride = st.stride, max_depth = st.max_depth, r = min(max(st.word3, 2), SR_RMAX), r_old = min(max(st.column, 1), r - 1);
        const uint4 *pair = reinterpret_cast<const uint4 *>(p.packed + st.offset) + (size_t)b * 2 * stride;

        // ---- 1. walk ----
        for (int e = tid; e < 2 * stride; e += SR_THREADS) ln[e] = pair[e];
        __syncthreads();  // nodes, and the X rows staged before the loop or after the last rewrite
        if (tid < N) {
            const double *xrow = xs + tid * sd;
            const uint32_t zo = walk_tree<true>(ln, max_depth, xrow, p.fault).z;
            const uint32_t zn = walk_tree<true>(ln + stride, max_depth, xrow, p.fault).z;
            codes[tid] = (zo < (uint32_t)r ? 1u << zo : 0u) | (zn < (uint32_t)r ? 1u << zn : 0u);
        }
        __syncthreads();

        // ---- 2. Y = K_inv U (column form), then G = U'Y and v = Y'y ----
        auto y_phase = [&](auto rt_c) {
            constexpr int RT = decltype(rt_c)::value;
            double acc[RT];
#pragma unroll
            for (int c = 0; c < RT; ++c) acc[c] = 0.0;
            const int klen = (N + segs_y - 1) / segs_y;
            const int k0 = seg * klen, k1 = min(N, k0 + klen);
            if (col < N && seg < segs_y) {
#pragma unroll 2
                for (int k = k0; k < k1; ++k) {
                    const double kv = kload(k, col);
                    const uint32_t w = codes[k];
#pragma unroll
                    for (int c = 0; c < RT; ++c) acc[c] = fma(kv, ((w >> c) & 1u) ? 1.0 : 0.0, acc[c]);
                }
            }
            for (int sg = 0; sg < segs_y; ++sg) {
                if (col < N && seg == sg) {
#pragma unroll
                    for (int c = 0; c < RT; ++c)
                        if (c < r) {
                            double v = sg ? Yt[c * np + col] + acc[c] : acc[c];
                            if (sg == segs_y - 1) v *= s;
                            Yt[c * np + col] = v;
                        }
                }
                __syncthreads();
            }
            // row a < r of G (a = r: v) by wave a: lanes stride the points, xor butterfly
            for (int a = wave; a <= r; a += SR_WAVES) {
                double g[RT];
#pragma unroll
                for (int c = 0; c < RT; ++c) g[c] = 0.0;
#pragma unroll 1
                for (int i = lane; i < N; i += 64) {
                    const double m = a < r ? (((codes[i] >> a) & 1u) ? s : 0.0) : p.y[i];
#pragma unroll
                    for (int c = 0; c < RT; ++c)
                        if (c < r) g[c] = fma(m, Yt[c * np + i], g[c]);
                }
#pragma unroll
                for (int c = 0; c < RT; ++c)
                    if (c < r) {
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) g[c] += __shfl_xor(g[c], off);
                        if (lane == c) {
                            if (a < r) {
                                aug[a * SR_AUG_LD + c] = g[c] + (a == c ? (a < r_old ? -1.0 : 1.0) : 0.0);
                                aug[a * SR_AUG_LD + r + c] = (a == c) ? 1.0 : 0.0;
                            } else {
                                vsh[c] = g[c];
                            }
                        }
                    }
            }
        };
        if (r <= 8)
            y_phase(std::integral_constant<int, 8>{});
        else
            y_phase(std::integral_constant<int, 16>{});
        __syncthreads();

        // ---- 3. + 4. one wave: Gauss-Jordan with partial pivoting (small_kernel), then the decision ----
        if (wave == 0) {
            double logsum = 0.0;
            bool is_singular = false;  // lane 0's view
            for (int pc = 0; pc < r; ++pc) {
                if (lane == 0) {
                    int best = pc;
                    double bv = fabs(aug[pc * SR_AUG_LD + pc]);
                    for (int a = pc + 1; a < r; ++a)
                        if (fabs(aug[a * SR_AUG_LD + pc]) > bv) {
                            bv = fabs(aug[a * SR_AUG_LD + pc]);
                            best = a;
                        }
                    misc[0] = best;
                    if (bv == 0.0) is_singular = true;
                }
                wave_sync();
                const int pr = misc[0];
                if (pr != pc && lane < 2 * r) {
                    const double tmp = aug[pc * SR_AUG_LD + lane];
                    aug[pc * SR_AUG_LD + lane] = aug[pr * SR_AUG_LD + lane];
                    aug[pr * SR_AUG_LD + lane] = tmp;
                }
                wave_sync();
                const double dv = aug[pc * SR_AUG_LD + pc];
                logsum += log(fabs(dv));
                wave_sync();
                if (lane < 2 * r) aug[pc * SR_AUG_LD + lane] = aug[pc * SR_AUG_LD + lane] / dv;
                wave_sync();
                for (int e = lane; e < r * 2 * r; e += 64) {  // reads column pc and row pc, writes neither
                    const int a = e / (2 * r), cc = e - a * 2 * r;
                    if (a != pc && cc != pc)
                        aug[a * SR_AUG_LD + cc] = fma(-aug[a * SR_AUG_LD + pc], aug[pc * SR_AUG_LD + cc], aug[a * SR_AUG_LD + cc]);
                }
                wave_sync();
                if (lane < r && lane != pc) aug[lane * SR_AUG_LD + pc] = 0.0;
                wave_sync();
            }
            if (lane == 0) {
                double q = 0.0;
                for (int a = 0; a < r; ++a)
                    for (int c = 0; c < r; ++c) q = fma(vsh[a] * aug[a * SR_AUG_LD + r + c], vsh[c], q);
                const size_t at = (size_t)t * nc + b;
                int acc;
                if (is_singular) {
                    acc = -1;
                } else {
                    acc = metropolis_accept(p.log_u[at], p.log_q_prior[at], 0.5 * (q - logsum));
                }
                p.accept_out[at] = acc;
                if (acc > 0) {
                    quad = quad - q;
                    logdet = logdet + logsum;
                }
                misc[2] = acc;
            }
        }
        __syncthreads();
        const int decision = misc[2];
        if (decision < 0) latched = true;
        if (decision <= 0) continue;  // uniform: every thread read the same word
        any_accept = true;

        // ---- 5. rewrite ----
        auto rewrite = [&](auto rt_c) {
            constexpr int RT = decltype(rt_c)::value;
            double Yj[RT], Zj[RT];
#pragma unroll
            for (int c = 0; c < RT; ++c) Yj[c] = Zj[c] = 0.0;
            if (col_live) {
#pragma unroll
                for (int c = 0; c < RT; ++c)
                    if (c < r) Yj[c] = Yt[c * np + col];
                // Z[j] = S Y[j]' with S = (den^-1 + den^-1') / 2.  den is symmetric, its computed inverse only to cond(den) * eps;
                // mirroring sum_c Y[lo][c] Z[hi][c] with the inverse as computed would put Y inv Y' in one triangle and Y inv' Y' in
                // the other, an error that is not of the form Y E Y' and that the next near-singular system amplifies (three
                // accepted 16-leaf steps at N = 512, cond ~ 1e5: 1.2e-11 in K_inv against 6e-13 with the symmetrised inverse)
#pragma unroll
                for (int c = 0; c < RT; ++c)
                    if (c < r) {
                        double z = 0.0;
                        for (int a = 0; a < r; ++a)
                            z = fma(0.5 * (aug[c * SR_AUG_LD + r + a] + aug[a * SR_AUG_LD + r + c]), Yt[a * np + col], z);
                        Zj[c] = z;
                    }
            }
            __syncthreads();  // den^-1, codes, X rows are dead: Z' goes over them
            if (col_live && seg == 0) {
#pragma unroll
                for (int c = 0; c < RT; ++c)
                    if (c < r) Zt[c * np + col] = Zj[c];
            }
            __syncthreads();
            if (col_live) {
                const int rlen = (N + segs_all - 1) / segs_all;
                const int i0 = seg * rlen, i1 = min(N, i0 + rlen);
                const int jw0 = col & ~63;  // this wave's columns: jw0 .. jw0 + 63
#pragma unroll 1
                for (int i = i0; i < i1; ++i) {
                    double d = 0.0;
                    if (i < jw0) {  // i < j in every lane
#pragma unroll
                        for (int c = 0; c < RT; ++c)
                            if (c < r) d = fma(Yt[c * np + i], Zj[c], d);
                    } else if (i > jw0 + 63) {  // i > j in every lane
#pragma unroll
                        for (int c = 0; c < RT; ++c)
                            if (c < r) d = fma(Yj[c], Zt[c * np + i], d);
                    } else {
                        const bool le = i <= col;
#pragma unroll
                        for (int c = 0; c < RT; ++c)
                            if (c < r) d = fma(le ? Yt[c * np + i] : Yj[c], le ? Zj[c] : Zt[c * np + i], d);
                    }
                    kstore(i, col, kload(i, col) - d);
                }
            }
        };
        if (r <= 8)
            rewrite(std::integral_constant<int, 8>{});
        else
            rewrite(std::integral_constant<int, 16>{});
        if (!K_IN_LDS) __threadfence();  // the rewritten entries leave this CU's write path ...
        __syncthreads();
        if (!K_IN_LDS) __threadfence();  // ... and no stale line of K_inv stays in its L1 for the next step's reads
        stage_x();  // Z' went over the X rows; the barrier at the top of the next step covers this
    }

    if (K_IN_LDS && any_accept) {
        __syncthreads();
        for (int e = tid; e < N * N; e += SR_THREADS) {
            const int row = e / N, c2 = e - row * N;
            Kg[e] = Kl[row * np + (c2 ^ (row & 15))];
        }
    }
    if (tid == 0 && any_accept) {
        p.state[2 * b] = quad;
        p.state[2 * b + 1] = logdet;
    }
}

#define SR_USE_OTHER "; use bark_tree_sweep_chains_hip (the multi-launch sweep) for this shape"

// the limits on N, nc and d, and the plan; sets the error message
int sr_check_shape(int64_t N, int64_t nc, int64_t d, SrPlan *plan) {
    if (N < 1 || N > SR_NMAX)
        return fail(BARK_ERR_ARG, "one-launch sweep: N = %lld is outside 1..%d" SR_USE_OTHER, (long long)N, SR_NMAX);
    if (nc < 1 || nc > SAMPLER_MAX_CHAINS)
        return fail(BARK_ERR_ARG, "one-launch sweep: %lld chains are outside 1..%d" SR_USE_OTHER, (long long)nc, SAMPLER_MAX_CHAINS);
    if (d < 1) return fail(BARK_ERR_ARG, "one-launch sweep: d = %lld" SR_USE_OTHER, (long long)d);
    *plan = sr_plan(N, d);
    if (plan->variant == 0)
        return fail(BARK_ERR_ARG, "one-launch sweep: the X rows of N = %lld points with d = %lld features (%lld bytes) do not fit LDS"
                    SR_USE_OTHER, (long long)N, (long long)d, (long long)(N * (d | 1) * 8));
    return BARK_OK;
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

size_t bark_tree_sweep_resident_table_bytes(int64_t n_steps, int64_t nc) {
    if (n_steps < 1 || nc < 1 || nc > SAMPLER_MAX_CHAINS || n_steps > ((int64_t)1 << 32)) return 0;
    return (size_t)(n_steps * (STEP_TABLE_WORDS + nc)) * sizeof(int64_t);
}

int bark_tree_sweep_resident_table(const int64_t *packed_offsets, const bark_pack_info *infos, const int64_t *r_old,
                                   int64_t n_steps, int64_t nc, void *table_host_out) {
    error_buffer()[0] = 0;
    if (!packed_offsets || !infos || !r_old || !table_host_out || n_steps < 1 || n_steps > ((int64_t)1 << 32))
        return fail(BARK_ERR_ARG, "bark_tree_sweep_resident_table: bad argument");
    if (nc < 1 || nc > SAMPLER_MAX_CHAINS)
        return fail(BARK_ERR_ARG, "one-launch sweep: %lld chains are outside 1..%d" SR_USE_OTHER, (long long)nc, SAMPLER_MAX_CHAINS);
    const StepPackRule rule{"one-launch sweep", "one [old, new] pair", " fit LDS" SR_USE_OTHER, 2, SR_STRIDE_MAX, true};
    for (int64_t t = 0; t < n_steps; ++t) {
        const bark_pack_info &in = infos[t];
        if (step_pack_check(rule, t, packed_offsets[t], in, nc)) return BARK_ERR_ARG;
        if (in.max_bits < 2 || in.max_bits > SR_RMAX)
            return fail(BARK_ERR_ARG, "one-launch sweep, step %lld: %lld leaves in a pair are outside 2..%d" SR_USE_OTHER, (long long)t,
                        (long long)in.max_bits, SR_RMAX);
        for (int64_t b = 0; b < nc; ++b)
            if (r_old[t * nc + b] < 1 || r_old[t * nc + b] >= in.max_bits)
                return fail(BARK_ERR_ARG, "step %lld chain %lld: r_old = %lld is not inside (0, %lld)", (long long)t, (long long)b,
                            (long long)r_old[t * nc + b], (long long)in.max_bits);
    }
    step_table_write(static_cast<int64_t *>(table_host_out), packed_offsets, infos, nullptr, r_old, n_steps, nc);
    return BARK_OK;
}

size_t bark_tree_sweep_resident_workspace_bytes(int64_t N, int64_t r_max, int64_t nc) {
    if (N < 1 || N > SR_NMAX || r_max < 2 || r_max > SR_RMAX || nc < 1 || nc > SAMPLER_MAX_CHAINS) return 0;
    return 256;  // everything the kernel needs sits in LDS
}

int bark_tree_sweep_resident_query(int64_t N, int64_t r_max, int64_t d, int64_t max_nodes_bytes, int *variant_out,
                                   int64_t *lds_bytes_out, int *threads_out) {
    error_buffer()[0] = 0;
    if (variant_out) *variant_out = 0;
    if (lds_bytes_out) *lds_bytes_out = 0;
    if (threads_out) *threads_out = 0;
    if (!variant_out) return fail(BARK_ERR_ARG, "bark_tree_sweep_resident_query: null argument");
    if (r_max < 2 || r_max > SR_RMAX)
        return fail(BARK_ERR_ARG, "one-launch sweep: %lld leaves in a pair are outside 2..%d" SR_USE_OTHER, (long long)r_max, SR_RMAX);
    if (max_nodes_bytes < 0) return fail(BARK_ERR_ARG, "bark_tree_sweep_resident_query: max_nodes_bytes < 0");
    if (max_nodes_bytes > SR_NODE_BYTES)
        return fail(BARK_ERR_ARG, "one-launch sweep: a packed pair of %lld bytes, at most %d (64 nodes per tree) fit LDS" SR_USE_OTHER,
                    (long long)max_nodes_bytes, SR_NODE_BYTES);
    SrPlan plan;
    const int rc = sr_check_shape(N, 1, d, &plan);
    if (rc) return rc;
    *variant_out = plan.variant;
    if (lds_bytes_out) *lds_bytes_out = (int64_t)plan.lds;
    if (threads_out) *threads_out = SR_THREADS;
    return BARK_OK;
}

int bark_tree_sweep_resident_hip(bark_ctx *ctx, double *K_inv, int64_t N, int64_t nc, int64_t n_steps, const void *packed,
                                 const void *table_dev, const double *X, int64_t d, const double *s_dev, const double *y,
                                 const double *log_q_prior, const double *log_u, double *state, int32_t *accept_out,
                                 void *workspace, size_t workspace_bytes, void *stream_) {
    error_buffer()[0] = 0;
    {
        const int crc = check_ctx(ctx);
        if (crc) return crc;
    }
    if (!K_inv || !packed || !table_dev || !X || !s_dev || !y || !log_q_prior || !log_u || !state || !accept_out || n_steps < 1 ||
        n_steps > (1 << 30))
        return fail(BARK_ERR_ARG, "bark_tree_sweep_resident_hip: bad argument");
    SrPlan plan;
    int rc = sr_check_shape(N, nc, d, &plan);
    if (rc) return rc;
    if (!workspace || workspace_bytes < bark_tree_sweep_resident_workspace_bytes(N, 2, nc))
        return fail(BARK_ERR_WORKSPACE, "one-launch sweep: workspace too small");
    static const LdsLimit limits[] = {{reinterpret_cast<const void *>(sweep_resident_kernel<true>), SR_LDS_MAX},
                                      {reinterpret_cast<const void *>(sweep_resident_kernel<false>), SR_LDS_MAX}};
    static LdsLimitsOnce once;
    if ((rc = raise_lds_limits(once, limits))) return rc;
    const SrArgs args{K_inv, (int)N, (int)nc, (int)n_steps, (int)d, static_cast<const unsigned char *>(packed),
                      static_cast<const int64_t *>(table_dev), X, s_dev, y, log_q_prior, log_u, state, accept_out, ctx->fault, plan};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (plan.variant == 1)
        hipLaunchKernelGGL(sweep_resident_kernel<true>, dim3((unsigned)nc), dim3(SR_THREADS), plan.lds, stream, args);
    else
        hipLaunchKernelGGL(sweep_resident_kernel<false>, dim3((unsigned)nc), dim3(SR_THREADS), plan.lds, stream, args);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
