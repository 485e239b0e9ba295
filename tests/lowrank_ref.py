"""Host reference of the low-rank (Woodbury / determinant-lemma) updates of csrc/lowrank.hip and the case tables of
tests/test_gpu_lowrank.py (numpy only: no GPU, no library).  tests/test_lowrank_reference_cpu.py pins this module to the
oracle and the goldens, every row of the tables to its cell of the dispatch, and the generator to its conditions.

The formulas are those of include/bark_hip.h.  With mul = -1 for `subtract`, else +1:

    update:  K_out = K - (K U) (mul I + U'K U)^-1 (U'K),      logabsdet = log|det(I + mul U'K U)|

K is a general matrix: the right factor U'K is its own product and equals (K U)' only for a symmetric K.  With
U = [U_old U_new], C = diag(-1 (r_old times), +1), Y = K U, G = U'Y and v = Y'y for a symmetric K:

    swap:    dquad = v'(C + G)^-1 v,   dlogdet = log|det(C + G)|,   K_out = K - Y (C + G)^-1 Y'

    Metropolis (bark_sampler.py:256-259):  accept iff  log_u <= min(log_q_prior + 0.5 (dquad - dlogdet), 0)

where `min` is Python's: a NaN on either side of the comparison rejects.

The r x r systems are solved by LU with partial pivoting, as the reference's np.linalg.solve / slogdet do: LAPACK in
float64, an elimination written out below in np.longdouble (numpy has no LAPACK for it)."""
from __future__ import annotations

import zlib
from typing import NamedTuple

import numpy as np

# The bars of tests/test_gpu_parity.py: matrices (test_woodbury_large_against_oracle), the scalars logabsdet / dquad /
# dlogdet (test_fused_tree_swap_matches_reference_chain), several chains against one (test_chain_batch_matches_single_chains)
MAT_RTOL, MAT_ATOL = 1e-9, 1e-11
SCALAR_RTOL, SCALAR_ATOL = 1e-9, 1e-9
BATCH_RTOL, BATCH_ATOL = 1e-12, 1e-12
COND_MAX = 100.0  # of every r x r system the generator hands out
LR_MAX = 64  # lowrank.hip: the largest rank
MAX_CHAINS = 64


def used(got, want, rtol, atol) -> float:
    """The fraction of the bar |got - want| <= atol + rtol |want| that the worst element uses."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


# ------------------------------------------------------------------------------ reference ----
def solve_logdet(den, rhs, dtype=np.float64):
    """den^-1 rhs and log|det den| by LU with partial pivoting; LinAlgError for an exactly zero pivot column."""
    if dtype == np.float64:
        x = np.linalg.solve(den, rhs)
        return x, np.linalg.slogdet(den)[1]
    r = den.shape[0]
    a = np.concatenate([den, rhs], axis=1).astype(dtype)
    logdet = dtype(0)
    for col in range(r):
        p = col + int(np.argmax(np.abs(a[col:, col])))
        if a[p, col] == 0:
            raise np.linalg.LinAlgError("Singular matrix")
        if p != col:
            a[[col, p]] = a[[p, col]]
        logdet += np.log(np.abs(a[col, col]))
        a[col] = a[col] / a[col, col]
        others = np.arange(r) != col
        a[others] = a[others] - np.outer(a[others, col], a[col])
    return a[:, r:], logdet


def update(K, U, subtract, dtype=np.float64):
    """bark_lowrank_update_hip: -> (K_out, logabsdet), the general form with the right factor U'K."""
    K, U = np.asarray(K, dtype=dtype), np.asarray(U, dtype=dtype)
    r = U.shape[1]
    left = K @ U
    right = U.T @ K
    den = (-1 if subtract else 1) * np.eye(r, dtype=dtype) + U.T @ left
    x, logabsdet = solve_logdet(den, right, dtype)
    return K - left @ x, logabsdet


def swap(K, U, r_old, y, dtype=np.float64):
    """bark_lowrank_swap_eval_hip + bark_lowrank_swap_apply_hip for a symmetric K: -> (dquad, dlogdet, K_out)."""
    K, U, y = np.asarray(K, dtype=dtype), np.asarray(U, dtype=dtype), np.asarray(y, dtype=dtype).reshape(-1)
    r = U.shape[1]
    C = np.diag(np.where(np.arange(r) < r_old, -1, 1).astype(dtype))
    Y = K @ U
    v = Y.T @ y
    x, dlogdet = solve_logdet(C + U.T @ Y, np.concatenate([v[:, None], Y.T], axis=1), dtype)
    return v @ x[:, 0], dlogdet, K - Y @ x[:, 1:]


def metropolis(dquad, dlogdet, log_q_prior, log_u, singular=False, latched=False) -> int:
    """decide_kernel: 1 accept, 0 reject, -1 for a singular system or a chain that met one earlier in the sweep."""
    if singular or latched:
        return -1
    log_alpha = log_q_prior + 0.5 * (dquad - dlogdet)  # new_mll - cur_mll = 0.5 (dquad - dlogdet)
    return 1 if (log_u <= log_alpha and log_u <= 0.0) else 0  # a NaN compares false: reject


def gauss_jordan_no_pivot(den):
    """den^-1 by Gauss-Jordan WITHOUT the row swap: what small_kernel would compute if it lost its pivoting.  Only the
    CPU test uses it, to show that the pivot cases need the swap (inf / NaN here, fine with it)."""
    r = den.shape[0]
    a = np.concatenate([np.asarray(den, dtype=np.float64), np.eye(r)], axis=1)
    with np.errstate(all="ignore"):
        for col in range(r):
            a[col] = a[col] / a[col, col]
            others = np.arange(r) != col
            a[others] = a[others] - np.outer(a[others, col], a[col])
    return a[:, r:]


# ------------------------------------------------------------------------------- dispatch ----
def rank_bin(r) -> int:
    return 8 if r <= 8 else 16 if r <= 16 else 32 if r <= 32 else 64


def colsum_usable(N, r) -> bool:
    return N % 2 == 0 and r <= 16


def colsum_segment(N) -> int:
    return 32 if N <= 1024 else 64 if N <= 2048 else 128 * ((N + 4095) // 4096)


class Route(NamedTuple):
    reach: str  # the cell of the dispatch: "col<bin>/seg<rows>" (N even, r <= 16), "vec<bin>" (N even), "scalar<bin>" (N odd)
    left: str  # the kernel that forms K U (and the shares of U'K U)
    right: str | None  # the kernel that forms (U'K)' when K_out is asked for and `symmetric` is 0
    seg: int  # rows per segment of the column form, 0 where no column form runs


def route(N, r, symmetric) -> Route:
    """bark_lowrank_update_hip's choice of kernels, restated (bark_lowrank_swap_eval_hip takes the symmetric one)."""
    b, col, lanes = rank_bin(r), colsum_usable(N, r), "vec" if N % 2 == 0 else "scalar"
    seg = colsum_segment(N) if col else 0
    colsum = f"colsum<{b}>/seg{seg}"
    left = colsum if (symmetric and col) else f"skinny<{b},{lanes}>"
    right = None if symmetric else colsum if col else f"skinny_t<{b}>/{'even' if N % 2 == 0 else 'odd'}"
    return Route(f"col{b}/seg{seg}" if col else f"{lanes}{b}", left, right, seg)


def all_kernel_instances() -> set:
    """Every (kernel instance, N parity, segment regime) the dispatch can reach: UPDATE_CASES must hit each."""
    out = {f"colsum<{b}>/seg{s}" for b in (8, 16) for s in (32, 64, 128, 256)}
    out |= {f"skinny<{b},{lanes}>" for b in (8, 16, 32, 64) for lanes in ("vec", "scalar")}
    out |= {f"skinny_t<{b}>/odd" for b in (8, 16, 32, 64)} | {f"skinny_t<{b}>/even" for b in (32, 64)}
    return out


class UpdateCase(NamedTuple):
    N: int
    r: int
    reach: str
    edge: str


# name: N, r, the cell it is meant to reach (checked against route() by the CPU test), the edge it sits on.
# Every row runs the four (subtract, symmetric) combinations; with symmetric = 0 an even N with r <= 16 runs
# skinny_kernel<VEC> for K U and the column form for K'U, every other N skinny_kernel and skinny_t_kernel.
UPDATE_CASES = {
    # r = min(3, N) over the tile edges: 8 rows per skinny workgroup, 16 per colsum_finish block, 32-row segments, 64-row
    # chunks of skinny_t and 64 x 64 tiles of the rewrite, 128 columns per chunk and per colsum block, the segment regimes
    "n1": UpdateCase(1, 1, "scalar8", "a single element"),
    "n2": UpdateCase(2, 2, "col8/seg32", "one lane live, r = N"),
    "n7": UpdateCase(7, 3, "scalar8", "one row short of a skinny workgroup"),
    "n8": UpdateCase(8, 3, "col8/seg32", "exactly one skinny workgroup"),
    "n9": UpdateCase(9, 3, "scalar8", "one row into the second skinny workgroup"),
    "n30": UpdateCase(30, 3, "col8/seg32", "short of one 32-row segment, two finish blocks"),
    "n34": UpdateCase(34, 3, "col8/seg32", "segments of 32 and 2 rows"),
    "n63": UpdateCase(63, 3, "scalar8", "one short of a 64 tile / skinny_t chunk"),
    "n64": UpdateCase(64, 3, "col8/seg32", "exactly one 64 x 64 tile"),
    "n65": UpdateCase(65, 3, "scalar8", "one into the second tile and skinny_t chunk"),
    "n127": UpdateCase(127, 3, "scalar8", "one short of a 128-column chunk"),
    "n128": UpdateCase(128, 3, "col8/seg32", "exactly one chunk and one colsum block"),
    "n129": UpdateCase(129, 3, "scalar8", "one column into the second chunk (prefetch, wrap-around)"),
    "n130": UpdateCase(130, 3, "col8/seg32", "a colsum block of 2 columns"),
    "n257": UpdateCase(257, 3, "scalar8", "third chunk of one column"),
    "n258": UpdateCase(258, 3, "col8/seg32", "third colsum block of 2 columns, 9 segments"),
    "n1024": UpdateCase(1024, 3, "col8/seg32", "last N of the 32-row regime: 32 full segments"),
    "n1026": UpdateCase(1026, 3, "col8/seg64", "first N of the 64-row regime, last segment of 2 rows"),
    "n2048": UpdateCase(2048, 3, "col8/seg64", "last N of the 64-row regime"),
    "n2050": UpdateCase(2050, 3, "col8/seg128", "first N of the 128-row regime"),
    # the rank bins at an even N (column form up to 16, skinny_kernel<VEC> beyond) ...
    "even_r1": UpdateCase(130, 1, "col8/seg32", "rank 1"),
    "even_r8": UpdateCase(130, 8, "col8/seg32", "last rank of the first bin"),
    "even_r9": UpdateCase(130, 9, "col16/seg32", "first rank of the second bin"),
    "even_r16": UpdateCase(130, 16, "col16/seg32", "last rank of the column form"),
    "even_r17": UpdateCase(130, 17, "vec32", "first rank past the column form"),
    "even_r32": UpdateCase(130, 32, "vec32", "last rank of the third bin"),
    "even_r33": UpdateCase(130, 33, "vec64", "first rank of the last bin"),
    "even_r64": UpdateCase(130, 64, "vec64", "the largest rank (130 KiB of LDS)"),
    # ... and at an odd one (scalar loads, skinny_t_kernel)
    "odd_r1": UpdateCase(129, 1, "scalar8", "rank 1"),
    "odd_r8": UpdateCase(129, 8, "scalar8", "last rank of the first bin"),
    "odd_r9": UpdateCase(129, 9, "scalar16", "first rank of the second bin"),
    "odd_r16": UpdateCase(129, 16, "scalar16", "last rank of the second bin"),
    "odd_r17": UpdateCase(129, 17, "scalar32", "first rank of the third bin"),
    "odd_r32": UpdateCase(129, 32, "scalar32", "last rank of the third bin"),
    "odd_r33": UpdateCase(129, 33, "scalar64", "first rank of the last bin"),
    "odd_r64": UpdateCase(129, 64, "scalar64", "the largest rank"),
    # the second rank bin of the column form in the two middle segment regimes (the rows above reach them with r = 3 only)
    "n1026_r9": UpdateCase(1026, 9, "col16/seg64", "colsum_kernel<16> on 64-row segments"),
    "n2050_r16": UpdateCase(2050, 16, "col16/seg128", "colsum_kernel<16> on 128-row segments"),
    # 256-row segments, 17 partials of which the last has 2 rows: the largest shapes of the table (134 MB per matrix)
    "n4098_r16": UpdateCase(4098, 16, "col16/seg256", "256-row segments, unequal partials"),
    "n4098_r5": UpdateCase(4098, 5, "col8/seg256", "256-row segments, unequal partials"),
}
LARGE_N = 4098  # rows of this size may take longer than the rest together


# ------------------------------------------------------------------------------ generator ----
class Inputs(NamedTuple):
    K: np.ndarray  # general (N, N)
    Ks: np.ndarray  # (K + K') / 2, what a `symmetric = 1` call and the swap are given
    U: np.ndarray  # (N, r)
    y: np.ndarray  # (N,)
    cond: float  # the largest condition number among the r x r systems of this row


def swap_splits(case: UpdateCase):
    """The r_old values a row's swap runs with: r // 2, and the two ends once each at N = 130."""
    return sorted({case.r // 2} | ({0, case.r} if case.N == 130 else set()))


def systems(inp: Inputs, splits):
    """Every r x r matrix that a row's calls factor."""
    r = inp.U.shape[1]
    out = []
    for K in (inp.K, inp.Ks):
        G = inp.U.T @ K @ inp.U
        out += [np.eye(r) + G, -np.eye(r) + G]
    G = inp.U.T @ inp.Ks @ inp.U
    out += [np.diag(np.where(np.arange(r) < r_old, -1.0, 1.0)) + G for r_old in splits]
    return out


def make_inputs(name) -> Inputs:
    """K = I + (0.25 / sqrt N) G (G standard normal: NOT symmetric), U = (0.6 / sqrt N) standard normal — U'K U stays O(1)
    at every N —, y standard normal; seeded by the row's name.  A draw in which some +-I + U'K U (or a swap's C + U'K U) has
    a condition number above COND_MAX is discarded and the next draw of the same seed sequence taken: at small N and at
    r ~ N / 2 an eigenvalue of U'K U falls next to 1 in a fair share of the draws."""
    case = UPDATE_CASES[name]
    N, r = case.N, case.r
    for attempt in range(200):
        rng = np.random.default_rng([zlib.crc32(name.encode()), attempt])
        K = np.eye(N) + (0.25 / np.sqrt(N)) * rng.standard_normal((N, N))
        U = (0.6 / np.sqrt(N)) * rng.standard_normal((N, r))
        y = rng.standard_normal(N)
        inp = Inputs(K, 0.5 * (K + K.T), U, y, 0.0)
        cond = max(float(np.linalg.cond(d)) for d in systems(inp, swap_splits(case)))
        if cond <= COND_MAX:
            return inp._replace(cond=cond)
    raise AssertionError(f"{name}: no well-conditioned draw")


# ------------------------------------------------------------------------------ pivot cases ----
class PivotCase(NamedTuple):
    r: int
    singular: int  # 1-based column of the first exactly zero pivot of -I + U'U, 0: not singular
    swap_at: int  # 1-based column at which partial pivoting must swap rows, 0: never


# K = I, subtract: den = -I + U'U.  The columns of U are 2 e_p (a 3 on the diagonal of den) except where stated; all
# entries are small integers, so every sum on the way to den is exact in any order and the zeros are exact zeros.
PIVOT_CASES = {
    "swap_row0": PivotCase(3, 0, 1),  # den[0][0] = 0, den[0][1] = den[1][0] = 1: regular, row 0 must be swapped
    "swap_col3": PivotCase(9, 0, 3),  # the same 2 x 2 block at columns 3 and 4 of an r = 9 system
    "singular_k1": PivotCase(9, 1, 0),
    "singular_k4": PivotCase(9, 4, 0),
    "singular_kr": PivotCase(9, 9, 0),
}
PIVOT_N = (130, 129)  # column form (with symmetric = 1) and row form


def pivot_U(name, N):
    case = PIVOT_CASES[name]
    r = case.r
    rows = (np.arange(r) * 37 + 5) % N  # distinct rows, spread over several workgroups
    assert len(set(rows.tolist())) == r
    U = np.zeros((N, r))
    U[rows, np.arange(r)] = 2.0
    for k in (case.singular, case.swap_at):
        if k:
            U[rows[k - 1], k - 1] = 1.0  # unit column: a zero on the diagonal of den
    if case.swap_at:
        U[rows[case.swap_at - 1], case.swap_at] = 1.0  # the next column overlaps it: den[k-1][k] = den[k][k-1] = 1
    return U


# ------------------------------------------------------------------------------ chain cases ----
class ChainCase(NamedTuple):
    N: int
    leaves: tuple  # per chain: (leaves of the old tree, leaves of the new tree)
    path: str  # "grid<8>" / "grid<16>": colsum_kernel<RT, true>, the chain a grid dimension; "streams": one stream per chain
    edge: str


def _varied(nc):
    return tuple((1 + b % 5, 1 + (3 * b) % 7) for b in range(nc))  # 2 .. 12 leaves per pair, chain 4: (5, 6) ...


CHAIN_CASES = {
    "grid_nc1": ChainCase(130, ((3, 4),), "grid<8>", "one chain"),
    "grid_nc2": ChainCase(130, ((3, 4), (2, 5)), "grid<8>", "two chains, different r_old"),
    "grid_nc64": ChainCase(130, _varied(64), "grid<16>", "MAX_CHAINS chains, a per-chain r_neg"),
    "streams_odd": ChainCase(129, _varied(5), "streams", "odd N: one stream per chain"),
    "uneven": ChainCase(130, ((8, 8), (1, 1), (3, 2)), "grid<16>", "max_bits leaves beside 2: zero columns"),
    "leaves8": ChainCase(130, ((4, 4), (3, 5)), "grid<8>", "last pair size of colsum_kernel<8, true>"),
    "leaves9": ChainCase(130, ((4, 5), (5, 4)), "grid<16>", "first pair size of colsum_kernel<16, true>"),
    "leaves16": ChainCase(130, ((8, 8), (7, 9)), "grid<16>", "last pair size of the grid path"),
    "leaves17": ChainCase(130, ((8, 9), (9, 8)), "streams", "first pair size of the stream-per-chain path"),
}
CHAIN_D, CHAIN_M = 4, 4  # features of X, trees per forest


def chain_path(N, r) -> str:
    """eval_chains' choice, restated; r = the largest leaf count of a pair."""
    return f"grid<{rank_bin(r)}>" if colsum_usable(N, r) else "streams"


def caterpillar_tree(leaves, feature, node_limit=100):
    """A tree of exactly `leaves` leaves, built by hand: node 2k splits `feature` at (k + 1) / leaves, its left child is a
    leaf and its right child the next split.  On X ~ U[0, 1)^d every leaf is reached once N is a few times `leaves`."""
    from bark_amd.forest import NODE_RECORD_DTYPE

    tree = np.zeros(node_limit, dtype=NODE_RECORD_DTYPE)
    node, parent, depth = 0, 0xFFFFFFFF, 0
    for k in range(leaves - 1):
        left, right = 2 * k + 1, 2 * k + 2
        tree[node] = (0, feature, (k + 1) / leaves, left, right, parent, depth, 1)
        tree[left] = (1, 0, 0, 0, 0, node, depth + 1, 1)
        node, parent, depth = right, node, depth + 1
    tree[node] = (1, 0, 0, 0, 0, parent, depth, 1)
    return tree


class ChainInputs(NamedTuple):
    X: np.ndarray
    y: np.ndarray
    ft: np.ndarray
    forests: np.ndarray  # (nc, m, node_limit); tree 0 of chain b is the old tree of its pair
    new: np.ndarray  # (nc, node_limit) the proposed trees
    noise: np.ndarray
    scale: np.ndarray


def make_chain_inputs(name) -> ChainInputs:
    from bark_amd import synthetic

    case = CHAIN_CASES[name]
    nc, seed = len(case.leaves), zlib.crc32(name.encode()) % 10000
    X, y, bounds, ft = synthetic.unit_cube_problem(case.N, CHAIN_D, seed)
    forests = synthetic.sample_prior_forests(nc, CHAIN_M, bounds, ft, seed=seed)
    new = np.zeros_like(forests[:, 0])
    for b, (l_old, l_new) in enumerate(case.leaves):
        forests[b, 0] = caterpillar_tree(l_old, b % CHAIN_D)
        new[b] = caterpillar_tree(l_new, (b + 1) % CHAIN_D)
    rng = np.random.default_rng(seed)
    return ChainInputs(X, y, ft, forests, new, rng.uniform(0.05, 0.2, nc), rng.uniform(0.7, 1.4, nc))


def chain_reference(inp: ChainInputs, b, dtype=np.float64):
    """Chain b's proposal on the host: K_inv = the dense inverse of its own forest's kernel (bark_sampler.py:153-162), U from
    the oracle's leaf vectors (one column per REACHED leaf) -> (new_mll, K_inv, K_inv after the swap)."""
    from oracle import oracle as orc

    N, m = inp.X.shape[0], inp.forests.shape[1]
    K = inp.scale[b] * orc.forest_gram_matrix(inp.forests[b], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[b]) * np.eye(N)
    K_inv, logdet = np.linalg.inv(K), np.linalg.slogdet(K)[1]
    K_inv = 0.5 * (K_inv + K_inv.T)
    s = np.sqrt(inp.scale[b] / m)
    U_old = s * orc.get_leaf_vectors(inp.forests[b, 0], inp.X, inp.ft)
    U_new = s * orc.get_leaf_vectors(inp.new[b], inp.X, inp.ft)
    y = inp.y.reshape(-1)
    dquad, dlogdet, K_new = swap(K_inv, np.concatenate([U_old, U_new], axis=1), U_old.shape[1], y, dtype)
    quad = y @ K_inv @ y
    return float(0.5 * (-(quad - dquad) - (logdet + dlogdet))), K_inv, K_new
