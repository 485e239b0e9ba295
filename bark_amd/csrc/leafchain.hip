// Leaf-space sampler chains — the per-tree Metropolis loop of bark_sampler.py:233-264 and its noise/scale half (:266-282) on a
// chain state that is P = M^-1 (R x R), M = I_R + c Z'Z, instead of the N x N inverse (include/bark_hip.h: bark_leafchain_*).
//
// State of a chain (one opaque block): P (Rcap x Rcap), the bit-planes of its leaves (Rcap x Q uint64, Q = ceil(N / 64): bit l of
// planes[a][q] says whether point 64 q + l reaches the leaf in slot a), v = Z'y, the scalars q = v'Pv, log|M|, y'y, noise, scale,
// and the slot map: slots[t][l] = row of P that holds leaf l of tree t (the packer's leaf order), nleaves[t], a stack of free
// slots.  A free slot is an identity row and column of P with a zero plane and v = 0, so every sum may run over all Rcap slots.
//
// Swapping tree t (slots T, r_old of them) for a tree with r_new leaves, planes Z', is a block down-date and a bordering:
//     B = c Z_O'Z' (zero rows on T and on free slots),  D = I + c diag(Z'1),  Y = P B,  g = P v_O
//     QB = Y - P[:,T] P_TT^-1 Y[T],  Qv = g - P[:,T] P_TT^-1 g[T]                 (rows O)
//     S = D - B'QB,  u = Z''y - B'Qv,  q' = v_O'Qv + u'S^-1 u,  log|M'| = log|M| + log|P_TT| + log|S|
//     accept:  P_OO <- P_OO - P_OT P_TT^-1 P_TO + QB S^-1 QB',  P_O,T' = -QB S^-1,  P_T'T' = S^-1
// One workgroup per chain loops over the steps of a sweep; workgroup barriers are its only synchronisation.  The rewrite gives
// entries (i, j) and (j, i) the same bits (both evaluate sum_a E[lo][a] PT[hi][a] with lo = min(i, j), and the two small inverses
// come out of a symmetric elimination), which is what keeps the error of P flat over accepted steps.
// Conditioning: cond(M) ~ N scale / s2; like every leaf-space path this one loses digits as noise -> 0, so it is opt-in.
#include <algorithm>

#include "sampler_step.h"  // -> common.h

namespace bark {
namespace {

constexpr int LC_THREADS = 512, LC_WAVES = LC_THREADS / 64;
constexpr int LC_LCAP = 32;     // leaves per tree; also the row pitch of the Rcap x r scratch matrices
constexpr int LC_RCAP = 1024;   // slots per chain
constexpr int LC_TREES = 64;
constexpr int LC_STRIDE_MAX = 64;  // packed nodes per tree walked from LDS (a tree of 32 leaves has 63)
constexpr int LC_SP = LC_LCAP + 1; // pitch of the small matrices in LDS
typedef unsigned long long u64;

struct LcLayout {
    int Q;
    size_t off_P, off_v, off_planes, off_ints, stride;              // state block of a chain; its first 64 bytes are the scalars
    size_t w_newpl, w_B, w_Y, w_QB, w_PT, w_E, w_F, w_g, w_Qv, w_M, wstride;  // workspace of a chain
};
enum { H_Q = 0, H_LOGM = 1, H_YY = 2, H_NOISE = 3, H_SCALE = 4 };

LcLayout lc_layout(int64_t N, int64_t Rcap, int64_t m, int64_t lcap) {
    LcLayout L{};
    L.Q = (int)((N + 63) / 64);
    size_t o = 64;
    L.off_P = o, o += (size_t)Rcap * Rcap * 8;
    L.off_v = o, o += (size_t)Rcap * 8;
    L.off_planes = o, o += (size_t)Rcap * L.Q * 8;
    L.off_ints = o, o += (size_t)(m * lcap + m + 1 + Rcap) * 4;
    L.stride = (size_t)round_up((int64_t)o, 256);
    const size_t mat = (size_t)Rcap * LC_LCAP * 8;
    o = 0;
    L.w_newpl = o, o += (size_t)LC_LCAP * L.Q * 8;
    L.w_B = o, o += mat;
    L.w_Y = o, o += mat;
    L.w_QB = o, o += mat;
    L.w_PT = o, o += mat;
    L.w_E = o, o += mat;
    L.w_F = o, o += mat;
    L.w_g = o, o += (size_t)Rcap * 8;
    L.w_Qv = o, o += (size_t)Rcap * 8;
    L.w_M = o, o += (size_t)Rcap * Rcap * 8;
    L.wstride = (size_t)round_up((int64_t)o, 256);
    return L;
}

int lc_check_shape(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc, int64_t d) {
    if (nc < 1 || nc > SAMPLER_MAX_CHAINS)
        return fail(BARK_ERR_ARG, "leaf-space chains: %lld chains are outside 1..%d", (long long)nc, SAMPLER_MAX_CHAINS);
    if (m < 1 || m > LC_TREES) return fail(BARK_ERR_ARG, "leaf-space chains: %lld trees are outside 1..%d", (long long)m, LC_TREES);
    if (lcap < 1 || lcap > LC_LCAP)
        return fail(BARK_ERR_ARG, "leaf-space chains: %lld leaves per tree are outside 1..%d", (long long)lcap, LC_LCAP);
    if (Rcap < 1 || Rcap > LC_RCAP)
        return fail(BARK_ERR_ARG, "leaf-space chains: a capacity of %lld slots is outside 1..%d", (long long)Rcap, LC_RCAP);
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(BARK_ERR_ARG, "leaf-space chains: N = %lld is outside 1..2^24", (long long)N);
    if (d < 1 || N * d > ((int64_t)1 << 31)) return fail(BARK_ERR_ARG, "leaf-space chains: d = %lld", (long long)d);
    return BARK_OK;
}

struct LcArgs {
    unsigned char *state, *ws;
    LcLayout L;
    int N, Rcap, m, lcap, nc, d, n_steps;
    const unsigned char *packed;
    const int64_t *table;
    int64_t tree_stride, max_depth;  // init: nodes per tree, walk bound of the forests
    const int32_t *nleaves_in;
    const double *X, *y, *noise, *scale, *log_q_prior, *log_u;
    double *mstate;
    int32_t *accept_out, *fault;
    double *P_out, *v_out;
    int32_t *nleaves_out;
};

struct LcChain {
    double *hdr, *P, *v;
    u64 *planes;
    int32_t *slots, *nleaves, *nfree, *free_;
};
__device__ __forceinline__ LcChain lc_chain(const LcArgs &p, int b) {
    unsigned char *s = p.state + (size_t)b * p.L.stride;
    LcChain c;
    c.hdr = reinterpret_cast<double *>(s);
    c.P = reinterpret_cast<double *>(s + p.L.off_P);
    c.v = reinterpret_cast<double *>(s + p.L.off_v);
    c.planes = reinterpret_cast<u64 *>(s + p.L.off_planes);
    c.slots = reinterpret_cast<int32_t *>(s + p.L.off_ints);
    c.nleaves = c.slots + p.m * p.lcap;
    c.nfree = c.nleaves + p.m;
    c.free_ = c.nfree + 1;
    return c;
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// A (r x r, pitch LC_SP, LDS, symmetric in bits, positive definite) <- A^-1 by the symmetric sweep operator, run by ONE wave;
// returns log|A|, *bad = 1 for a non-positive pivot.  Row k and column k get the same value, and the update of (i, j) and (j, i)
// multiplies the same two numbers, so the inverse is symmetric in bits.
__device__ double lc_small_inverse(double *A, int r, int lane, int *bad) {
    double logdet = 0.0;
    for (int k = 0; k < r; ++k) {
        const double dv = A[k * LC_SP + k];
        if (!(dv > 0.0)) {
            *bad = 1;
            return logdet;
        }
        logdet += log(dv);
        const double dinv = 1.0 / dv;
        for (int e = lane; e < r * r; e += 64) {
            const int i = e / r, j = e - i * r;
            if (i != k && j != k) A[i * LC_SP + j] = A[i * LC_SP + j] - (A[i * LC_SP + k] * A[k * LC_SP + j]) * dinv;
        }
        wave_sync();
        if (lane < r && lane != k) {
            const double val = A[lane * LC_SP + k] * dinv;
            A[lane * LC_SP + k] = val;
            A[k * LC_SP + lane] = val;
        }
        if (lane == 0) A[k * LC_SP + k] = -dinv;
        wave_sync();
    }
    for (int e = lane; e < r * r; e += 64) {
        const int i = e / r, j = e - i * r;
        A[i * LC_SP + j] = -A[i * LC_SP + j];
    }
    wave_sync();
    return logdet;
}

// Shared by init and the noise/scale step (whole workgroup): A (Rcap x Rcap, global) <- (I + coef Z'Z)^-1 from the resident
// planes; slots whose plane is empty are identity rows and are left out of the elimination.  -> log|M|, q = v'A v; *bad as above.
struct LcBig {
    double ck[LC_RCAP];
    int act[LC_RCAP];
    double red[LC_THREADS];
    int n_act, bad;
};
__device__ void lc_build_inverse(double *A, const u64 *planes, const double *v, int Rcap, int Q, double coef, LcBig &sh,
                                 double *logm_out, double *q_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < Rcap * Rcap; e += LC_THREADS) A[e] = (e / Rcap == e % Rcap) ? 1.0 : 0.0;
    for (int a = wave; a < Rcap; a += LC_WAVES) {
        int c = 0;
        for (int q = lane; q < Q; q += 64) c += planes[(size_t)a * Q + q] ? 1 : 0;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (lane == 0) sh.act[a] = c;  // non-empty words of slot a, compacted below
    }
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int a = 0; a < Rcap; ++a)
            if (sh.act[a]) sh.act[n++] = a;
        sh.n_act = n;
    }
    __syncthreads();
    const int n = sh.n_act;
    for (int e = tid; e < n * n; e += LC_THREADS) {
        const int ii = e / n, jj = e - ii * n;
        if (jj < ii) continue;
        const int a = sh.act[ii], c = sh.act[jj];
        unsigned cnt = 0;
        for (int q = 0; q < Q; ++q) cnt += __popcll(planes[(size_t)a * Q + q] & planes[(size_t)c * Q + q]);
        const double val = (a == c ? 1.0 : 0.0) + coef * (double)cnt;
        A[(size_t)a * Rcap + c] = val;
        A[(size_t)c * Rcap + a] = val;
    }
    __syncthreads();
    double logm = 0.0;
    for (int kk = 0; kk < n; ++kk) {
        const int k = sh.act[kk];
        for (int ii = tid; ii < n; ii += LC_THREADS) sh.ck[ii] = A[(size_t)sh.act[ii] * Rcap + k];
        __syncthreads();
        const double dv = sh.ck[kk];
        if (!(dv > 0.0)) {  // uniform
            if (tid == 0) sh.bad = 1;
            break;
        }
        logm += log(dv);
        const double dinv = 1.0 / dv;
        for (int e = tid; e < n * n; e += LC_THREADS) {
            const int ii = e / n, jj = e - ii * n;
            if (ii == kk || jj == kk) continue;
            const size_t at = (size_t)sh.act[ii] * Rcap + sh.act[jj];
            A[at] = A[at] - (sh.ck[ii] * sh.ck[jj]) * dinv;
        }
        for (int ii = tid; ii < n; ii += LC_THREADS) {
            const int i = sh.act[ii];
            const double val = ii == kk ? -dinv : sh.ck[ii] * dinv;
            A[(size_t)i * Rcap + k] = val;
            A[(size_t)k * Rcap + i] = val;
        }
        __syncthreads();
    }
    __syncthreads();
    double part = 0.0;
    if (!sh.bad) {
        for (int e = tid; e < n * n; e += LC_THREADS) {
            const int ii = e / n, jj = e - ii * n;
            const size_t at = (size_t)sh.act[ii] * Rcap + sh.act[jj];
            A[at] = -A[at];
        }
        __syncthreads();
        for (int ii = tid; ii < n; ii += LC_THREADS) {
            const int i = sh.act[ii];
            double s = 0.0;
            for (int jj = 0; jj < n; ++jj) s = fma(A[(size_t)i * Rcap + sh.act[jj]], v[sh.act[jj]], s);
            part = fma(v[i], s, part);
        }
    }
    sh.red[tid] = part;
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (int k = 0; k < LC_THREADS; ++k) q += sh.red[k];
        *q_out = q;
        *logm_out = logm;
    }
    __syncthreads();
}

// mll of quick_inverse.py:37-38 in the two numbers the callers keep: y'K^-1 y and log|K|
__device__ __forceinline__ void lc_state(double q, double logm, double yy, double noise, double scale, int m, int N, double *quad,
                                         double *logdet) {
    const double s2 = 1e-6 + noise;
    const double coef = scale / ((double)m * s2);
    *quad = (yy - coef * q) / s2;
    *logdet = (double)N * log(s2) + logm;
}

__global__ __launch_bounds__(LC_THREADS) void leafchain_init_kernel(LcArgs p) {
    __shared__ LcBig sh;
    __shared__ int base[LC_TREES + 1];
    __shared__ int ok;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int N = p.N, Rcap = p.Rcap, m = p.m, lcap = p.lcap, Q = p.L.Q;
    LcChain c = lc_chain(p, b);
    const int32_t *nl = p.nleaves_in + (size_t)b * m;
    if (tid == 0) {
        int s = 0, good = 1;
        for (int t = 0; t < m; ++t) {
            base[t] = s;
            if (nl[t] < 1 || nl[t] > lcap) good = 0;
            s += good ? nl[t] : 0;
        }
        base[m] = s;
        ok = good && s <= Rcap;
        if (!ok) p.accept_out[b] = -2;  // the host checked the leaf table; never write past the block
    }
    __syncthreads();
    if (!ok) return;
    const int R = base[m];
    for (int e = tid; e < Rcap * Q; e += LC_THREADS) c.planes[e] = 0ull;
    for (int e = tid; e < m * lcap; e += LC_THREADS) {
        const int t = e / lcap, l = e - t * lcap;
        c.slots[e] = l < nl[t] ? base[t] + l : -1;
    }
    for (int e = tid; e < m; e += LC_THREADS) c.nleaves[e] = nl[e];
    for (int e = tid; e < Rcap; e += LC_THREADS) c.free_[e] = e < Rcap - R ? Rcap - 1 - e : -1;  // pops R, R + 1, ...
    if (tid == 0) *c.nfree = Rcap - R;
    __syncthreads();
    const uint4 *forest = reinterpret_cast<const uint4 *>(p.packed) + (size_t)b * m * p.tree_stride;
    for (int q = wave; q < Q; q += LC_WAVES) {
        const int i = 64 * q + lane;
        for (int t = 0; t < m; ++t) {
            uint32_t z = 0xFFFFFFFFu;
            if (i < N) z = walk_tree<false>(forest + (size_t)t * p.tree_stride, (int)p.max_depth, p.X + (size_t)i * p.d, p.fault).z;
            u64 mine = 0;
            for (int l = 0; l < nl[t]; ++l) {
                const u64 mask = __ballot(z == (uint32_t)(base[t] + l));
                if (lane == l) mine = mask;
            }
            if (lane < nl[t]) c.planes[(size_t)(base[t] + lane) * Q + q] = mine;
        }
    }
    __syncthreads();
    for (int a = wave; a < Rcap; a += LC_WAVES) {
        double s = 0.0;
        for (int q = 0; q < Q; ++q) {
            const int i = 64 * q + lane;
            if (((c.planes[(size_t)a * Q + q] >> lane) & 1ull) && i < N) s += p.y[i];
        }
        s = wave_sum(s);
        if (lane == 0) c.v[a] = s;
    }
    double part = 0.0;
    for (int i = tid; i < N; i += LC_THREADS) part = fma(p.y[i], p.y[i], part);
    sh.red[tid] = part;
    __syncthreads();
    if (tid == 0) {
        double yy = 0.0;
        for (int k = 0; k < LC_THREADS; ++k) yy += sh.red[k];
        c.hdr[H_YY] = yy;
        c.hdr[H_NOISE] = p.noise[b];
        c.hdr[H_SCALE] = p.scale[b];
    }
    __syncthreads();
    const double noise = p.noise[b], scale = p.scale[b];
    const double coef = scale / ((double)m * (1e-6 + noise));
    lc_build_inverse(c.P, c.planes, c.v, Rcap, Q, coef, sh, &c.hdr[H_LOGM], &c.hdr[H_Q]);
    if (tid == 0) {
        p.accept_out[b] = sh.bad ? -1 : 0;
        lc_state(c.hdr[H_Q], c.hdr[H_LOGM], c.hdr[H_YY], noise, scale, m, N, &p.mstate[2 * b], &p.mstate[2 * b + 1]);
    }
}

__global__ __launch_bounds__(LC_THREADS) void leafchain_noise_scale_kernel(LcArgs p) {
    __shared__ LcBig sh;
    __shared__ int decision;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = p.N, Rcap = p.Rcap, m = p.m, Q = p.L.Q;
    LcChain c = lc_chain(p, b);
    double *Mi = reinterpret_cast<double *>(p.ws + (size_t)b * p.L.wstride + p.L.w_M);
    double *scal = reinterpret_cast<double *>(p.ws + (size_t)b * p.L.wstride + p.L.w_B);  // q', log|M'|
    const double noise = p.noise[b], scale = p.scale[b];
    if (!(1e-6 + noise > 0.0)) {  // new_mll is NaN: rejected (noise_scale_decide_kernel)
        if (tid == 0) p.accept_out[b] = 0;
        return;
    }
    const double coef = scale / ((double)m * (1e-6 + noise));
    lc_build_inverse(Mi, c.planes, c.v, Rcap, Q, coef, sh, &scal[1], &scal[0]);
    if (tid == 0) {
        int acc;
        double quad = 0.0, logdet = 0.0;
        if (sh.bad) {
            acc = -1;
        } else {
            lc_state(scal[0], scal[1], c.hdr[H_YY], noise, scale, m, N, &quad, &logdet);
            const double new_mll = 0.5 * (-quad - logdet), cur_mll = 0.5 * (-p.mstate[2 * b] - p.mstate[2 * b + 1]);
            acc = metropolis_accept(p.log_u[b], p.log_q_prior[b], new_mll - cur_mll);
        }
        p.accept_out[b] = acc;
        if (acc > 0) {
            c.hdr[H_Q] = scal[0];
            c.hdr[H_LOGM] = scal[1];
            c.hdr[H_NOISE] = noise;
            c.hdr[H_SCALE] = scale;
            p.mstate[2 * b] = quad;
            p.mstate[2 * b + 1] = logdet;
        }
        decision = acc;
    }
    __syncthreads();
    if (decision > 0)
        for (int e = tid; e < Rcap * Rcap; e += LC_THREADS) c.P[e] = Mi[e];
}

// canonical order: tree-major, leaves in the packer's order; rows and columns past the chain's leaves are identity
__global__ __launch_bounds__(LC_THREADS) void leafchain_export_kernel(LcArgs p) {
    __shared__ int map[LC_RCAP];
    __shared__ int total;
    const int tid = threadIdx.x, b = blockIdx.x, Rcap = p.Rcap;
    LcChain c = lc_chain(p, b);
    if (tid == 0) {
        int n = 0;
        for (int t = 0; t < p.m; ++t) {
            const int nl = min(max(c.nleaves[t], 0), p.lcap);
            for (int l = 0; l < nl && n < Rcap; ++l) map[n++] = min(max(c.slots[t * p.lcap + l], 0), Rcap - 1);
            p.nleaves_out[(size_t)b * p.m + t] = c.nleaves[t];
        }
        total = n;
    }
    __syncthreads();
    const int R = total;
    double *Po = p.P_out + (size_t)b * Rcap * Rcap;
    for (int e = tid; e < Rcap * Rcap; e += LC_THREADS) {
        const int i = e / Rcap, j = e - i * Rcap;
        Po[e] = (i < R && j < R) ? c.P[(size_t)map[i] * Rcap + map[j]] : (i == j ? 1.0 : 0.0);
    }
    for (int e = tid; e < Rcap; e += LC_THREADS) p.v_out[(size_t)b * Rcap + e] = e < R ? c.v[map[e]] : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ the sweep ----
__global__ __launch_bounds__(LC_THREADS) void leafchain_sweep_kernel(LcArgs p) {
    __shared__ uint4 ln[LC_STRIDE_MAX];
    __shared__ double PTT[LC_LCAP * LC_SP], Sm[LC_LCAP * LC_SP], W[LC_LCAP * LC_SP];
    __shared__ double vnew[LC_LCAP], dnew[LC_LCAP], wg[LC_LCAP], uu[LC_LCAP], sc[4];
    __shared__ int Tsl[LC_LCAP], newslot[LC_LCAP], misc[4];
    __shared__ signed char inT[LC_RCAP], newidx[LC_RCAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int N = p.N, Rcap = p.Rcap, m = p.m, lcap = p.lcap, Q = p.L.Q, nc = p.nc;
    constexpr int LP = LC_LCAP;
    LcChain c = lc_chain(p, b);
    unsigned char *wsb = p.ws + (size_t)b * p.L.wstride;
    u64 *newpl = reinterpret_cast<u64 *>(wsb + p.L.w_newpl);
    double *Bm = reinterpret_cast<double *>(wsb + p.L.w_B), *Y = reinterpret_cast<double *>(wsb + p.L.w_Y);
    double *QB = reinterpret_cast<double *>(wsb + p.L.w_QB), *PT = reinterpret_cast<double *>(wsb + p.L.w_PT);
    double *E = reinterpret_cast<double *>(wsb + p.L.w_E), *F = reinterpret_cast<double *>(wsb + p.L.w_F);
    double *g = reinterpret_cast<double *>(wsb + p.L.w_g), *Qv = reinterpret_cast<double *>(wsb + p.L.w_Qv);
    double *P = c.P;

    const double noise = c.hdr[H_NOISE], scale = c.hdr[H_SCALE], yy = c.hdr[H_YY];
    const double coef = scale / ((double)m * (1e-6 + noise));
    double logm = c.hdr[H_LOGM];  // the running scalars are thread 0's
    double quad = p.mstate[2 * b], logdet = p.mstate[2 * b + 1];
    bool latched = false;
    for (int e = tid; e < Rcap; e += LC_THREADS) {
        inT[e] = 0;
        newidx[e] = -1;
    }

    for (int t = 0; t < p.n_steps; ++t) {
        if (latched) {  // as decide_kernel: a chain that met a non-positive pivot stays at -1 and is not touched again
            if (tid == 0) p.accept_out[(size_t)t * nc + b] = -1;
            continue;
        }
        const StepEntry st = step_entry(p.table, t, p.n_steps, nc, b, LC_STRIDE_MAX);
        const int stride = st.stride, max_depth = st.max_depth, tree = min(max(st.word3, 0), m - 1), r_new = min(max(st.column, 1), lcap);
        const int r_old = min(max(c.nleaves[tree], 1), lcap);
        const uint4 *nodes = reinterpret_cast<const uint4 *>(p.packed + st.offset) + (size_t)b * stride;
        __syncthreads();  // the slot map, inT / newidx and the state of the previous step
        if (r_new - r_old > *c.nfree) {  // cannot happen after the host's capacity check; never overflow the stack
            latched = true;
            if (tid == 0) p.accept_out[(size_t)t * nc + b] = -1;
            continue;
        }
        for (int e = tid; e < stride; e += LC_THREADS) ln[e] = nodes[e];
        if (tid < r_old) {
            const int s = min(max(c.slots[tree * lcap + tid], 0), Rcap - 1);
            Tsl[tid] = s;
            inT[s] = 1;
        }
        if (tid == 0) misc[0] = 0;  // bad pivot
        __syncthreads();

        // ---- 1. walk the new tree: one wave per 64 points, one ballot per leaf ----
        for (int q = wave; q < Q; q += LC_WAVES) {
            const int i = 64 * q + lane;
            uint32_t z = 0xFFFFFFFFu;
            if (i < N) z = walk_tree<false>(ln, max_depth, p.X + (size_t)i * p.d, p.fault).z;
            u64 mine = 0;
            for (int l = 0; l < r_new; ++l) {
                const u64 mask = __ballot(z == (uint32_t)l);
                if (lane == l) mine = mask;
            }
            if (lane < r_new) newpl[(size_t)lane * Q + q] = mine;
        }
        __syncthreads();

        // ---- 2. v' = Z''y and D (leaf_sums_kernel's order), B = c Z_O'Z' by popcount ----
        for (int l = wave; l < r_new; l += LC_WAVES) {
            double s = 0.0;
            int cnt = 0;
            for (int q = 0; q < Q; ++q) {
                const u64 mask = newpl[(size_t)l * Q + q];
                const int i = 64 * q + lane;
                if (((mask >> lane) & 1ull) && i < N) {
                    s += p.y[i];
                    ++cnt;
                }
            }
            s = wave_sum(s);
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
            if (lane == 0) {
                vnew[l] = s;
                dnew[l] = 1.0 + coef * (double)cnt;
            }
        }
        for (int a = wave; a < Rcap; a += LC_WAVES) {
            unsigned cnt[LP];
#pragma unroll
            for (int l = 0; l < LP; ++l) cnt[l] = 0;
            if (!inT[a])
                for (int q = lane; q < Q; q += 64) {
                    const u64 pa = c.planes[(size_t)a * Q + q];
                    if (pa) {
#pragma unroll
                        for (int l = 0; l < LP; ++l)
                            if (l < r_new) cnt[l] += __popcll(pa & newpl[(size_t)l * Q + q]);
                    }
                }
            unsigned mine = 0;
#pragma unroll
            for (int l = 0; l < LP; ++l)
                if (l < r_new) {
                    unsigned s = cnt[l];
                    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
                    if (lane == l) mine = s;
                }
            if (lane < r_new) Bm[(size_t)a * LP + lane] = coef * (double)mine;
        }
        __syncthreads();

        // ---- 3. Y = P B, g = P v_O (one wave per row of P), and the columns P[:, T] kept for the rewrite ----
        for (int i = wave; i < Rcap; i += LC_WAVES) {
            double acc[LP], ag = 0.0;
#pragma unroll
            for (int l = 0; l < LP; ++l) acc[l] = 0.0;
            const double *row = P + (size_t)i * Rcap;
            for (int a = lane; a < Rcap; a += 64) {
                const double pv = row[a];
                if (pv == 0.0) continue;  // free slots and most of a sparse-ish row: nothing to add
                ag = fma(pv, inT[a] ? 0.0 : c.v[a], ag);
                const double *brow = Bm + (size_t)a * LP;
#pragma unroll
                for (int l = 0; l < LP; ++l)
                    if (l < r_new) acc[l] = fma(pv, brow[l], acc[l]);
            }
            double mine = 0.0;
#pragma unroll
            for (int l = 0; l < LP; ++l)
                if (l < r_new) {
                    const double s = wave_sum(acc[l]);
                    if (lane == l) mine = s;
                }
            ag = wave_sum(ag);
            if (lane < r_new) Y[(size_t)i * LP + lane] = mine;
            if (lane == 0) g[i] = ag;
            if (lane < r_old) PT[(size_t)i * LP + lane] = row[Tsl[lane]];
        }
        for (int e = tid; e < r_old * r_old; e += LC_THREADS) {
            const int a = e / r_old, k = e - a * r_old;
            PTT[a * LC_SP + k] = P[(size_t)Tsl[a] * Rcap + Tsl[k]];
        }
        __syncthreads();

        // ---- 4. P_TT^-1 (one wave), then W = P_TT^-1 Y[T], wg = P_TT^-1 g[T] ----
        if (wave == 0) {
            int bad = 0;
            const double ld = lc_small_inverse(PTT, r_old, lane, &bad);
            if (lane == 0) {
                sc[0] = ld;
                if (bad) misc[0] = 1;
            }
        }
        __syncthreads();
        for (int e = tid; e < r_old * (r_new + 1); e += LC_THREADS) {
            const int a = e / (r_new + 1), l = e - a * (r_new + 1);
            double s = 0.0;
            for (int k = 0; k < r_old; ++k)
                s = fma(PTT[a * LC_SP + k], l < r_new ? Y[(size_t)Tsl[k] * LP + l] : g[Tsl[k]], s);
            if (l < r_new)
                W[a * LC_SP + l] = s;
            else
                wg[a] = s;
        }
        __syncthreads();

        // ---- 5. QB, Qv on the rows O ----
        for (int e = tid; e < Rcap * (r_new + 1); e += LC_THREADS) {
            const int i = e / (r_new + 1), l = e - i * (r_new + 1);
            double s = 0.0;
            if (!inT[i]) {
                s = l < r_new ? Y[(size_t)i * LP + l] : g[i];
                for (int a = 0; a < r_old; ++a) s = fma(-PT[(size_t)i * LP + a], l < r_new ? W[a * LC_SP + l] : wg[a], s);
            }
            if (l < r_new)
                QB[(size_t)i * LP + l] = s;
            else
                Qv[i] = s;
        }
        __syncthreads();

        // ---- 6. S = D - B'QB (symmetrised below), u = v' - B'Qv, v_O'Qv: a thread per entry, slots in order ----
        for (int e = tid; e < r_new * (r_new + 1) + 1; e += LC_THREADS) {
            double s = 0.0;
            if (e == r_new * (r_new + 1)) {
                for (int a = 0; a < Rcap; ++a) s = fma(inT[a] ? 0.0 : c.v[a], Qv[a], s);
                sc[1] = s;
                continue;
            }
            const int l = e / (r_new + 1), k = e - l * (r_new + 1);
            for (int a = 0; a < Rcap; ++a) {
                const double bv = Bm[(size_t)a * LP + l];
                if (bv != 0.0) s = fma(bv, k < r_new ? QB[(size_t)a * LP + k] : Qv[a], s);
            }
            if (k < r_new)
                W[l * LC_SP + k] = s;  // W is free again: B'QB before it is symmetrised
            else
                uu[l] = vnew[l] - s;
        }
        __syncthreads();
        for (int e = tid; e < r_new * r_new; e += LC_THREADS) {
            const int l = e / r_new, k = e - l * r_new;
            Sm[l * LC_SP + k] = (l == k ? dnew[l] : 0.0) - 0.5 * (W[l * LC_SP + k] + W[k * LC_SP + l]);
        }
        __syncthreads();

        // ---- 7. S^-1, the new scalars and the decision (one wave) ----
        if (wave == 0) {
            int bad = misc[0];
            double ldS = 0.0;
            if (!bad) ldS = lc_small_inverse(Sm, r_new, lane, &bad);
            double part = 0.0;
            if (!bad && lane < r_new) {
                double s = 0.0;
                for (int k = 0; k < r_new; ++k) s = fma(Sm[lane * LC_SP + k], uu[k], s);
                part = uu[lane] * s;
            }
            part = wave_sum(part);
            if (lane == 0) {
                const size_t at = (size_t)t * nc + b;
                int acc;
                double nquad = 0.0, nlogdet = 0.0, nq = 0.0, nlogm = 0.0;
                if (bad) {
                    acc = -1;
                } else {
                    nq = sc[1] + part;
                    nlogm = logm + sc[0] + ldS;
                    lc_state(nq, nlogm, yy, noise, scale, m, N, &nquad, &nlogdet);
                    acc = metropolis_accept(p.log_u[at], p.log_q_prior[at], 0.5 * (-nquad - nlogdet) - 0.5 * (-quad - logdet));
                }
                p.accept_out[at] = acc;
                if (acc > 0) {
                    logm = nlogm, quad = nquad, logdet = nlogdet;
                    c.hdr[H_Q] = nq;
                    c.hdr[H_LOGM] = nlogm;
                    p.mstate[2 * b] = nquad;
                    p.mstate[2 * b + 1] = nlogdet;
                }
                misc[1] = acc;
            }
        }
        __syncthreads();
        const int decision = misc[1];
        if (decision < 0) latched = true;
        if (decision <= 0) {
            if (tid < r_old) inT[Tsl[tid]] = 0;
            continue;  // uniform: every thread read the same word
        }

        // ---- 8. rewrite: E = P[:,T] P_TT^-1, F = QB S^-1, then (i, j) and (j, i) from one expression ----
        for (int e = tid; e < Rcap * LP; e += LC_THREADS) {
            const int i = e / LP, l = e - i * LP;
            if (l < r_old) {
                double s = 0.0;
                for (int k = 0; k < r_old; ++k) s = fma(PT[(size_t)i * LP + k], PTT[k * LC_SP + l], s);
                E[e] = s;
            }
            if (l < r_new) {
                double s = 0.0;
                for (int k = 0; k < r_new; ++k) s = fma(QB[(size_t)i * LP + k], Sm[k * LC_SP + l], s);
                F[e] = s;
            }
        }
        __syncthreads();
        for (int e = tid; e < Rcap * Rcap; e += LC_THREADS) {
            const int i = e / Rcap, j = e - i * Rcap;
            const int lo = min(i, j), hi = max(i, j);
            double d1 = 0.0, d2 = 0.0;
            for (int a = 0; a < r_old; ++a) d1 = fma(E[(size_t)lo * LP + a], PT[(size_t)hi * LP + a], d1);
            for (int l = 0; l < r_new; ++l) d2 = fma(F[(size_t)lo * LP + l], QB[(size_t)hi * LP + l], d2);
            P[e] = (P[e] - d1) + d2;
        }
        if (tid == 0) {  // one lane updates the slot map: reuse the old tree's slots, then pop; a shrinking tree pushes
            int nf = *c.nfree;
            for (int l = 0; l < r_new; ++l) {
                const int s = l < r_old ? Tsl[l] : c.free_[--nf];
                newslot[l] = s;
                c.slots[tree * lcap + l] = s;
            }
            for (int a = r_new; a < r_old; ++a) {
                c.free_[nf++] = Tsl[a];
                c.slots[tree * lcap + a] = -1;
            }
            *c.nfree = nf;
            c.nleaves[tree] = r_new;
        }
        __syncthreads();
        if (tid < r_new) newidx[newslot[tid]] = (signed char)tid;
        for (int e = tid; e < r_old * Rcap; e += LC_THREADS) {  // the old tree's slots become free slots ...
            const int a = e / Rcap, i = e - a * Rcap, s = Tsl[a];
            const double val = i == s ? 1.0 : 0.0;
            P[(size_t)s * Rcap + i] = val;
            P[(size_t)i * Rcap + s] = val;
        }
        for (int e = tid; e < r_old * Q; e += LC_THREADS) c.planes[(size_t)Tsl[e / Q] * Q + e % Q] = 0ull;
        if (tid < r_old) c.v[Tsl[tid]] = 0.0;
        __syncthreads();
        for (int e = tid; e < r_new * Rcap; e += LC_THREADS) {  // ... and the new leaves are bordered in
            const int l = e / Rcap, i = e - l * Rcap, s = newslot[l];
            const double val = newidx[i] >= 0 ? Sm[l * LC_SP + newidx[i]] : 0.0 - F[(size_t)i * LP + l];
            P[(size_t)s * Rcap + i] = val;
            P[(size_t)i * Rcap + s] = val;
        }
        for (int e = tid; e < r_new * Q; e += LC_THREADS) c.planes[(size_t)newslot[e / Q] * Q + e % Q] = newpl[e];
        if (tid < r_new) c.v[newslot[tid]] = vnew[tid];
        __syncthreads();
        if (tid < r_old) inT[Tsl[tid]] = 0;
        if (tid < r_new) newidx[newslot[tid]] = -1;
    }
}

int lc_common(const char *who, bark_ctx *ctx, const void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
              int64_t d, const void *workspace, size_t workspace_bytes, LcLayout *L) {
    error_buffer()[0] = 0;
    const int crc = check_ctx(ctx);
    if (crc) return crc;
    const int rc = lc_check_shape(N, Rcap, m, lcap, nc, d);
    if (rc) return rc;
    if (!state) return fail(BARK_ERR_ARG, "%s: null state", who);
    *L = lc_layout(N, Rcap, m, lcap);
    if (!workspace || workspace_bytes < L->wstride * (size_t)nc) return fail(BARK_ERR_WORKSPACE, "%s: workspace too small", who);
    return BARK_OK;
}

}  // namespace
}  // namespace bark

using namespace bark;

extern "C" {

int bark_leafchain_query(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc, int64_t d, bark_leafchain_plan *out) {
    error_buffer()[0] = 0;
    if (!out) return fail(BARK_ERR_ARG, "bark_leafchain_query: null argument");
    *out = bark_leafchain_plan{};
    out->max_chains = SAMPLER_MAX_CHAINS, out->max_trees = LC_TREES, out->max_leaves = LC_LCAP, out->max_slots = LC_RCAP;
    out->max_nodes = LC_STRIDE_MAX;
    const int rc = lc_check_shape(N, Rcap, m, lcap, nc, d);
    if (rc) return rc;
    const LcLayout L = lc_layout(N, Rcap, m, lcap);
    out->chain_bytes = (int64_t)L.stride;
    out->state_bytes = (int64_t)(L.stride * (size_t)nc);
    out->workspace_bytes = (int64_t)(L.wstride * (size_t)nc);
    out->plane_words = L.Q;
    out->workgroups = (int32_t)nc;
    out->threads = LC_THREADS;
    out->launches_per_sweep = 1;
    return BARK_OK;
}

size_t bark_leafchain_bytes(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc) {
    bark_leafchain_plan plan;
    return bark_leafchain_query(N, Rcap, m, lcap, nc, 1, &plan) ? 0 : (size_t)plan.state_bytes;
}

size_t bark_leafchain_workspace_bytes(int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc) {
    bark_leafchain_plan plan;
    return bark_leafchain_query(N, Rcap, m, lcap, nc, 1, &plan) ? 0 : (size_t)plan.workspace_bytes;
}

int bark_leafchain_init_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                            const void *packed, const bark_pack_info *info, const int32_t *nleaves, const double *X, int64_t d,
                            const double *y, const double *noise, const double *scale, double *mstate, int32_t *info_out,
                            void *workspace, size_t workspace_bytes, void *stream) {
    LcLayout L;
    const int rc = lc_common("bark_leafchain_init_hip", ctx, state, N, Rcap, m, lcap, nc, d, workspace, workspace_bytes, &L);
    if (rc) return rc;
    if (!packed || !info || !nleaves || !X || !y || !noise || !scale || !mstate || !info_out)
        return fail(BARK_ERR_ARG, "bark_leafchain_init_hip: null argument");
    if (info->B != nc || info->m != m) return fail(BARK_ERR_ARG, "bark_leafchain_init_hip: pack the nc forests of m trees (B = chains)");
    if (info->max_leaves > lcap)
        return fail(BARK_ERR_ARG, "leaf-space chains: a tree of %lld leaves, at most %lld fit", (long long)info->max_leaves, (long long)lcap);
    if (info->max_bits > Rcap)
        return fail(BARK_ERR_ARG, "leaf-space chains: a forest of %lld leaves, the capacity is %lld slots", (long long)info->max_bits,
                    (long long)Rcap);
    LcArgs a{};
    a.state = static_cast<unsigned char *>(state), a.ws = static_cast<unsigned char *>(workspace), a.L = L;
    a.N = (int)N, a.Rcap = (int)Rcap, a.m = (int)m, a.lcap = (int)lcap, a.nc = (int)nc, a.d = (int)d;
    a.packed = static_cast<const unsigned char *>(packed), a.tree_stride = info->stride, a.max_depth = info->max_depth;
    a.nleaves_in = nleaves, a.X = X, a.y = y, a.noise = noise, a.scale = scale, a.mstate = mstate, a.accept_out = info_out;
    a.fault = ctx->fault;
    hipLaunchKernelGGL(leafchain_init_kernel, dim3((unsigned)nc), dim3(LC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

size_t bark_leafchain_sweep_table_bytes(int64_t n_steps, int64_t nc) {
    if (n_steps < 1 || nc < 1 || nc > SAMPLER_MAX_CHAINS || n_steps > ((int64_t)1 << 30)) return 0;
    return (size_t)(n_steps * (STEP_TABLE_WORDS + nc)) * sizeof(int64_t);
}

int bark_leafchain_sweep_table(const int64_t *packed_offsets, const bark_pack_info *infos, const int64_t *tree_index,
                               const int64_t *r_new, const int32_t *nleaves, int64_t n_steps, int64_t nc, int64_t m, int64_t lcap,
                               int64_t Rcap, void *table_host_out) {
    error_buffer()[0] = 0;
    if (!packed_offsets || !infos || !tree_index || !r_new || !nleaves || !table_host_out || n_steps < 1 ||
        n_steps > ((int64_t)1 << 30))
        return fail(BARK_ERR_ARG, "bark_leafchain_sweep_table: bad argument");
    const int rc = lc_check_shape(1, Rcap, m, lcap, nc, 1);
    if (rc) return rc;
    const StepPackRule rule{"leaf-space chains", "one new tree", "", 1, LC_STRIDE_MAX, false};
    for (int64_t t = 0; t < n_steps; ++t) {
        const bark_pack_info &in = infos[t];
        if (step_pack_check(rule, t, packed_offsets[t], in, nc)) return BARK_ERR_ARG;
        if (tree_index[t] < 0 || tree_index[t] >= m)
            return fail(BARK_ERR_ARG, "step %lld: tree index %lld is outside 0..%lld", (long long)t, (long long)tree_index[t], (long long)m - 1);
        for (int64_t b = 0; b < nc; ++b)
            if (r_new[t * nc + b] < 1 || r_new[t * nc + b] > lcap || r_new[t * nc + b] > in.max_bits)
                return fail(BARK_ERR_ARG, "leaf-space chains, step %lld chain %lld: a new tree of %lld leaves, at most %lld fit", (long long)t,
                            (long long)b, (long long)r_new[t * nc + b], (long long)lcap);
    }
    // capacity in the worst case over the accept masks: tree k of a chain ends a step with its present leaf count or with that of
    // one of its proposals, and a swap first reuses the old tree's slots, so the slots in use never exceed sum_k max(those counts)
    for (int64_t b = 0; b < nc; ++b) {
        int64_t peak[LC_TREES], need = 0;
        for (int64_t k = 0; k < m; ++k) {
            peak[k] = nleaves[b * m + k];
            if (peak[k] < 1 || peak[k] > lcap) return fail(BARK_ERR_ARG, "chain %lld tree %lld: bad leaf count", (long long)b, (long long)k);
        }
        for (int64_t t = 0; t < n_steps; ++t) peak[tree_index[t]] = std::max(peak[tree_index[t]], r_new[t * nc + b]);
        for (int64_t k = 0; k < m; ++k) need += peak[k];
        if (need > Rcap)
            return fail(BARK_ERR_ARG, "leaf-space chains, chain %lld: the sweep may need %lld slots, the capacity is %lld; rebuild the "
                        "chains with a larger capacity", (long long)b, (long long)need, (long long)Rcap);
    }
    step_table_write(static_cast<int64_t *>(table_host_out), packed_offsets, infos, tree_index, r_new, n_steps, nc);
    return BARK_OK;
}

int bark_leafchain_sweep_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                             int64_t n_steps, const void *packed, const void *table_dev, const double *X, int64_t d,
                             const double *y, const double *log_q_prior, const double *log_u, double *mstate,
                             int32_t *accept_out, void *workspace, size_t workspace_bytes, void *stream) {
    LcLayout L;
    const int rc = lc_common("bark_leafchain_sweep_hip", ctx, state, N, Rcap, m, lcap, nc, d, workspace, workspace_bytes, &L);
    if (rc) return rc;
    if (!packed || !table_dev || !X || !y || !log_q_prior || !log_u || !mstate || !accept_out || n_steps < 1 || n_steps > (1 << 30))
        return fail(BARK_ERR_ARG, "bark_leafchain_sweep_hip: bad argument");
    LcArgs a{};
    a.state = static_cast<unsigned char *>(state), a.ws = static_cast<unsigned char *>(workspace), a.L = L;
    a.N = (int)N, a.Rcap = (int)Rcap, a.m = (int)m, a.lcap = (int)lcap, a.nc = (int)nc, a.d = (int)d, a.n_steps = (int)n_steps;
    a.packed = static_cast<const unsigned char *>(packed), a.table = static_cast<const int64_t *>(table_dev);
    a.X = X, a.y = y, a.log_q_prior = log_q_prior, a.log_u = log_u, a.mstate = mstate, a.accept_out = accept_out;
    a.fault = ctx->fault;
    hipLaunchKernelGGL(leafchain_sweep_kernel, dim3((unsigned)nc), dim3(LC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_leafchain_noise_scale_hip(bark_ctx *ctx, void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                                   const double *new_noise, const double *new_scale, const double *log_q_prior,
                                   const double *log_u, double *mstate, int32_t *accept_out, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    LcLayout L;
    const int rc = lc_common("bark_leafchain_noise_scale_hip", ctx, state, N, Rcap, m, lcap, nc, 1, workspace, workspace_bytes, &L);
    if (rc) return rc;
    if (!new_noise || !new_scale || !log_q_prior || !log_u || !mstate || !accept_out)
        return fail(BARK_ERR_ARG, "bark_leafchain_noise_scale_hip: null argument");
    LcArgs a{};
    a.state = static_cast<unsigned char *>(state), a.ws = static_cast<unsigned char *>(workspace), a.L = L;
    a.N = (int)N, a.Rcap = (int)Rcap, a.m = (int)m, a.lcap = (int)lcap, a.nc = (int)nc;
    a.noise = new_noise, a.scale = new_scale, a.log_q_prior = log_q_prior, a.log_u = log_u, a.mstate = mstate;
    a.accept_out = accept_out;
    hipLaunchKernelGGL(leafchain_noise_scale_kernel, dim3((unsigned)nc), dim3(LC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

int bark_leafchain_export_hip(bark_ctx *ctx, const void *state, int64_t N, int64_t Rcap, int64_t m, int64_t lcap, int64_t nc,
                              double *P_out, double *v_out, int32_t *nleaves_out, void *stream) {
    error_buffer()[0] = 0;
    const int crc = check_ctx(ctx);
    if (crc) return crc;
    const int rc = lc_check_shape(N, Rcap, m, lcap, nc, 1);
    if (rc) return rc;
    if (!state || !P_out || !v_out || !nleaves_out) return fail(BARK_ERR_ARG, "bark_leafchain_export_hip: null argument");
    LcArgs a{};
    a.state = static_cast<unsigned char *>(const_cast<void *>(state)), a.L = lc_layout(N, Rcap, m, lcap);
    a.N = (int)N, a.Rcap = (int)Rcap, a.m = (int)m, a.lcap = (int)lcap, a.nc = (int)nc;
    a.P_out = P_out, a.v_out = v_out, a.nleaves_out = nleaves_out;
    hipLaunchKernelGGL(leafchain_export_kernel, dim3((unsigned)nc), dim3(LC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    BARK_LAUNCH_CHECK();
    return BARK_OK;
}

}  // extern "C"
