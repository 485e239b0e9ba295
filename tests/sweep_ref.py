"""Float64 host reference of every output of the dense sweep entry point (bark_mll_batched_hip) with its optional arguments —
`shift` (the no-null kernel), `cov_out`, BARK_MLL_RHS_IDENTITY and a NULL `scale` — the case table of
tests/test_gpu_sweep_options.py, and a direct ctypes wrapper of the entry point.  tests/test_sweep_reference_cpu.py pins the
reference to the goldens and the oracle and asserts that every row of the table reaches the cell it names.  numpy and the oracle
only; the wrapper alone needs a GPU.

K and K_CX are the oracle's bit-exact counts over m.  K_s is formed in the order include/bark_hip.h states, every step rounded
on its own and skipped when its argument is NULL:

    K_s  = [scale_b *] (K [- shift_b]) + (1e-6 + noise_b) I        K_Xx = [scale_b *] (K_Xx [- shift_b])      (no jitter)

and solved with numpy's LU routines, the reference's arithmetic (oracle.batched_mll, oracle.forest_predict):

    mll  = 0.5 (-y' K_s^-1 y - log|K_s| [- N log 2 pi])
    mu   = K_xX K_s^-1 y,   cov = scale_b - K_xX K_s^-1 K_Xx,   var = diag(cov)
    identity mode: K_s^-1,  K_s^-1 y,  diag(K_s^-1),  log|K_s|

route="cholesky" computes the same from K_s = L L' and triangular solves (as oracle.batched_mll(cholesky=True)): the CPU test
holds the two routes to a tenth of each output's tolerance, so that the GPU comparison is not spent on the reference's rounding.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass

import numpy as np

from bark_amd import _lib, synthetic
from bark_amd.forest import create_empty_forest
from leafspace_ref import solve_lower
from oracle import oracle as orc

# the project's existing bars (test_gpu_parity.py, test_gpu_fuzz.py, test_gpu_leafspace.py)
MLL_RTOL, MLL_ATOL = 1e-9, 1e-8
POST_TOL = 1e-9  # mu, var, cov: rtol and atol
INV_RTOL, INV_ATOL = 1e-8, 1e-9  # K_s^-1, K_s^-1 y, diag(K_s^-1)
LOGDET_RTOL = 1e-10
RESID_ATOL = 1e-8  # K_inv @ K_s against I
ROUTE_RTOL = 1e-12  # the same batch through another schedule / chunk size (atol 0)
SAME_V_RTOL = 1e-12  # var_out against the diagonal of cov_out: two reductions of the same V

REP_BYTES8, REP_BYTES7, REP_BITS = 0, 1, 2  # LeafRep (bark_amd/csrc/common.h)
D_CONT = 8  # both problems have 8 continuous columns first: the complete trees split on those


# ------------------------------------------------------------------ the reference arithmetic ----
def no_null_params(forest):
    """(shift, scale factor) per forest, exactly as forest.batched_forest_gram_matrix_no_null computes them (forest.py:102-111):
    shift = n_null / m, factor = m / max(m - n_null, 1); n_null = trees whose root is a leaf."""
    forest = np.asarray(forest)
    num_trees = forest.shape[-2]
    num_null = np.sum(forest[..., 0]["is_leaf"], axis=-1).astype(np.int64)
    return num_null / num_trees, num_trees / np.maximum(num_trees - num_null, 1)


def n_null(forest):
    return np.sum(np.asarray(forest)[..., 0]["is_leaf"], axis=-1).astype(np.int64)


def form(K, shift, scale, noise):
    """[scale *] (K [- shift]) [+ (1e-6 + noise) on the diagonal]: one rounding per step, None skips the step."""
    A = np.array(K, dtype=np.float64)
    if shift is not None:
        A = A - np.float64(shift)
    if scale is not None:
        A = A * np.float64(scale)
    if noise is not None:
        A[np.diag_indices_from(A)] += 1e-6 + np.float64(noise)
    return A


def solve_system(K_s, y, K_Xx=None, prior=None, identity=False, route="lu"):
    """Every output of one forest from its K_s (N, N), y (N,), the candidate block K_Xx (N, C) and the prior variance `prior`
    (the scale handed to the entry point).  mll is without the 2 pi term, mll_2pi with it."""
    N = K_s.shape[0]
    out = {}
    if route == "lu":
        K_inv = np.linalg.inv(K_s)
        logdet = np.linalg.slogdet(K_s)[1]
        K_inv_y = K_inv @ y
        quad = y @ K_inv_y
        if K_Xx is not None:
            half = K_Xx.T @ K_inv
            out["mu"] = half @ y
            out["cov"] = prior - half @ K_Xx
    else:
        L = np.linalg.cholesky(K_s)
        z = solve_lower(L, y[:, None])[:, 0]
        quad = z @ z
        logdet = 2.0 * np.log(np.diag(L)).sum()
        if identity:
            V = solve_lower(L, np.eye(N))
            K_inv = V.T @ V
            K_inv_y = V.T @ z
        if K_Xx is not None:
            G = solve_lower(L, K_Xx)
            out["mu"] = G.T @ z
            out["cov"] = prior - G.T @ G
    if "cov" in out:
        out["var"] = np.diagonal(out["cov"]).copy()
    if identity:
        out["K_inv"], out["K_inv_y"], out["diag"] = K_inv, K_inv_y, np.diagonal(K_inv).copy()
    out["logdet"] = logdet
    out["mll"] = 0.5 * (-quad - logdet)
    out["mll_2pi"] = 0.5 * (-quad - logdet - N * np.log(2 * np.pi))
    return out


def reference_arrays(F, X, y, ft, noise, scale, shift, cand=None, identity=False, route="lu"):
    """The outputs of the forests F (b, m, L) as a list of dicts; noise (b,), scale and shift (b,) or None."""
    F = np.asarray(F)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    K = orc.batched_forest_gram_matrix(F, X, X, ft)
    K_CX = None if cand is None else orc.batched_forest_gram_matrix(F, cand, X, ft)
    outs = []
    for b in range(F.shape[0]):
        sh = None if shift is None else shift[b]
        sc = None if scale is None else scale[b]
        K_s = form(K[b], sh, sc, noise[b])
        K_Xx = None if K_CX is None else form(K_CX[b].T, sh, sc, None)
        out = solve_system(K_s, y, K_Xx, sc, identity, route)
        out["K_s"] = K_s
        outs.append(out)
    return outs


# ------------------------------------------------------------------ the case table ----
@dataclass(frozen=True)
class Case:
    """One call shape.  cell: the row of the table below that it covers; C: candidates, or "identity" (C = N, explicit inverse);
    kind: "prior" (one-hot bit codes), "bytes7" (complete depth-5 trees, 32 leaves: byte codes of at most 128 leaves) or
    "bytes8" (complete depth-8 trees, 256 leaves); problem: "mixed" | "unit".  plan: what bark_mll_plan_query must report for it
    with the case's own leaf words — (schedule, last_schedule, fused_gram, splitk_layout); split: the plan must report
    splitk_steps > 0 (True) / == 0 (False).  other: the second route of the whole-batch check — "timing" (the instrumented
    call takes the multi-launch sweep) or another chunk size."""

    name: str
    cell: str
    N: int
    B: int
    m: int
    C: object
    chunk: object
    kind: str
    problem: str
    plan: tuple
    split: object = None
    other: object = None
    null_scale: str = ""  # generator family for which the row also runs with a NULL scale ("": it does not)
    reseed: int = 0  # another draw of the row's data (a compared forest's MLL moved by less than 100 bars with the shift)

    @property
    def bc(self):
        return min(self.chunk or self.B, self.B)

    @property
    def identity(self):
        return self.C == "identity"

    @property
    def n_cand(self):
        return self.N if self.identity else int(self.C)


CELLS = ("one_block", "two_block", "multi_block", "plain_fused", "plain_fused_ragged_split", "pipelined_fused", "paired_fused",
         "splitk", "splitk_lookahead", "candidates", "identity")

ONE = ("one_block", "one_block", 1, 0)
TWO = ("two_block", "two_block", 1, 0)
MULTI = ("multi_block", "multi_block", 1, 0)
PLAIN = ("plain", "plain", 1, 0)
PIPE = ("pipelined", "pipelined", 1, 0)
PAIRED = ("paired", "paired", 1, 0)


def _c(name, cell, N, B, m, C, chunk, kind, problem, plan, **kw):
    return Case(name, cell, N, B, m, C, chunk, kind, problem, plan, **kw)


CASES = {c.name: c for c in [
    # ---- one launch per chunk, MLL only (chol_diag.h: diag_kernel<true>, two_block_kernel, multi_block_kernel) ----
    _c("one_n1", "one_block", 1, 5, 50, 0, None, "prior", "mixed", ONE, other="timing"),
    _c("one_n100_bytes7", "one_block", 100, 7, 20, 0, 4, "bytes7", "unit", ONE, other="timing"),
    _c("one_n128_b256", "one_block", 128, 256, 50, 0, 96, "prior", "mixed", ONE, other="timing", null_scale="one-launch"),
    _c("one_n100_bytes8", "one_block", 100, 3, 8, 0, None, "bytes8", "unit", ONE, other="timing"),
    _c("two_n129", "two_block", 129, 5, 50, 0, None, "prior", "mixed", TWO, other="timing"),
    _c("two_n200_bytes7", "two_block", 200, 40, 50, 0, 16, "bytes7", "unit", TWO, other="timing"),
    _c("two_n256_b256", "two_block", 256, 256, 50, 0, None, "prior", "unit", TWO, other="timing"),
    _c("two_n200_bytes8", "two_block", 200, 4, 8, 0, None, "bytes8", "mixed", TWO, other="timing"),
    _c("multi_n300", "multi_block", 300, 200, 50, 0, None, "prior", "mixed", MULTI, other="timing"),
    _c("multi_n512", "multi_block", 512, 256, 50, 0, None, "prior", "unit", MULTI, other="timing"),
    _c("multi_n700", "multi_block", 700, 150, 50, 0, None, "prior", "mixed", MULTI, other="timing"),
    # three block rows: 13 byte-code words of 50 trees fit beside the factor image (15 at most); four block rows take 11
    _c("multi_n380_bytes7", "multi_block", 380, 161, 50, 0, 81, "bytes7", "unit", MULTI, other="timing"),
    # ---- fused row kernels (chol_rows.h: form_tile, syrk_tile, panel_reduce_kernel<GEN>) ----
    # (700, 20) and (900, 12) are too few matrices for one workgroup per tile: schedule_plan puts them in the split-K layout
    # (materialised A: the "splitk" cell below has them).  The plain fused schedule needs chunk x block rows >= 600 tiles below
    # 8 block rows and a chunk that multi_block_kernel does not take.
    _c("plain_n700_b110", "plain_fused", 700, 110, 50, 0, None, "prior", "mixed", PLAIN, split=False, other=100,
       null_scale="fused row kernels"),
    _c("plain_n850_bytes7", "plain_fused", 850, 90, 20, 0, None, "bytes7", "unit", PLAIN, split=False, other=88),
    _c("plain_n600_bytes8", "plain_fused", 600, 128, 8, 0, None, "bytes8", "unit", PLAIN, split=False, other=125),
    # the shapes of test_gpu_parity.py::test_many_small_matrices_and_chunk_invariance: no step of theirs splits its last round
    # (ragged_tail below: 288, 192 and 96 matrices do not end a round of 512 workgroups on a tile boundary or leave more than 192)
    _c("plain_n700_b288", "plain_fused", 700, 288, 50, 0, None, "prior", "mixed", PLAIN, split=False, other=192),
    # (chunks of 192 at six block rows are multi_block_kernel's; the remaining 96 take the plain fused schedule)
    _c("plain_n700_b288_c192", "plain_fused", 700, 288, 50, 0, 192, "prior", "mixed", ("multi_block", "plain", 1, 0),
       split=False, other="timing"),
    # The split ragged last round of the plain schedule (Sweep::step -> ragged_tail -> panel_split_kernel + panel_reduce_kernel<GEN>).
    # The layout (split-K or not) is decided from the full chunk, ragged_tail from the chunk that runs: a full chunk of 100 is
    # plain fused (>= 600 tiles), and its short last chunk leaves a last round of at most 192 workgroups that divides 3 ways or
    # more from step 3 on.  ragged_steps() restates the rule on the host (the plan query does not count these steps) and
    # check_cell asserts it for the last chunk; the whole batch in one chunk (no split step) is the other route.  A tail that
    # starts behind whole rounds (tail > 0) does not occur in a fused plain chunk: the CPU test enumerates it.
    _c("ragged_n850_b140_c100", "plain_fused_ragged_split", 850, 140, 20, 0, 100, "bytes7", "unit", PLAIN, split=False, other=140),
    _c("ragged_n700_b110_c100", "plain_fused_ragged_split", 700, 110, 50, 0, 100, "prior", "mixed", PLAIN, split=False, other=110),
    _c("pipe_n1100_b130", "pipelined_fused", 1100, 130, 50, 0, None, "prior", "mixed", PIPE, split=False, other=100),
    _c("pipe_n1300_b200_c120", "pipelined_fused", 1300, 200, 20, 0, 120, "bytes7", "unit", PIPE, split=True, other=100),
    _c("pipe_n2100_b70", "pipelined_fused", 2100, 70, 50, 0, None, "prior", "mixed", PIPE, split=True, other=48, reseed=1),
    _c("pipe_n1000_bytes8", "pipelined_fused", 1000, 80, 8, 0, None, "bytes8", "unit", PIPE, split=True, other=70),
    _c("paired_n2100_b256", "paired_fused", 2100, 256, 50, 0, None, "prior", "mixed", PAIRED, split=False, other=128),
    # ---- materialised A (gram.hip), MLL only ----
    _c("splitk_n2100_b2", "splitk", 2100, 2, 50, 0, None, "prior", "mixed", ("splitk", "splitk", 0, 1), split=True,
       null_scale="gram.hip"),
    _c("splitk_n1500_b9", "splitk", 1500, 9, 50, 0, 5, "bytes7", "unit", ("splitk", "splitk", 0, 1), split=True),
    _c("splitk_n700_b20", "splitk", 700, 20, 50, 0, None, "prior", "mixed", ("splitk", "splitk", 0, 1), split=True),
    _c("splitk_n900_b12", "splitk", 900, 12, 8, 0, None, "bytes8", "unit", ("splitk", "splitk", 0, 1), split=True),
    # the smallest look-ahead shape: see smallest_lookahead_shape() (asserted by the CPU test)
    _c("lookahead_n769_b50", "splitk_lookahead", 769, 50, 50, 0, None, "prior", "mixed",
       ("splitk_lookahead", "splitk_lookahead", 0, 1), split=True),
    # ---- candidates with shift and cov_out (gram.hip both blocks, launch_predict_reduce, vtv_kernel) ----
    # (640, 16) is in the split-K layout whatever C; one workgroup per tile (plain) takes chunks of about 100 at 6 - 8 block columns
    _c("cand_plain_c1", "candidates", 640, 100, 50, 1, None, "prior", "mixed", ("plain", "plain", 0, 0)),
    _c("cand_plain_c127", "candidates", 640, 200, 50, 127, 100, "bytes7", "unit", ("plain", "plain", 0, 0), other=80),
    _c("cand_pipe_c128", "candidates", 1000, 150, 25, 128, None, "prior", "mixed", ("pipelined", "pipelined", 0, 0)),
    _c("cand_pipe_c129", "candidates", 1000, 150, 25, 129, 64, "prior", "mixed", ("pipelined", "pipelined", 0, 0), other=50),
    _c("cand_splitk_c300", "candidates", 1400, 3, 8, 300, None, "bytes8", "unit", ("splitk", "splitk", 0, 1)),
    _c("cand_paired_c130", "candidates", 2100, 256, 50, 130, None, "prior", "mixed", ("paired", "paired", 0, 0)),
    # ---- identity right-hand side with shift (identity_rhs_kernel, vtv_kernel(+1)) ----
    _c("inv_n130", "identity", 130, 7, 50, "identity", 3, "prior", "mixed", ("plain", "plain", 0, 0)),
    _c("inv_n700_bytes7", "identity", 700, 50, 20, "identity", None, "bytes7", "unit", ("plain", "plain", 0, 0)),
    _c("inv_n1100_pipe", "identity", 1100, 40, 30, "identity", None, "prior", "mixed", ("pipelined", "pipelined", 0, 0)),
    # a shorter last chunk on another schedule.  With identity columns a chunk of 256 at N = 1100 is pipelined like its
    # remainder of 44 (9 block rows < 16), and the paired | pipelined pair (N > 1920) would hold 256 inverses of 35 MB;
    # the split-K layout gives the pair at N = 1100: 18 matrices have look-ahead steps, the last single one has none
    _c("inv_n1100_last_chunk", "identity", 1100, 19, 50, "identity", 18, "prior", "mixed", ("splitk_lookahead", "splitk", 0, 1)),
]}

# ragged_tail of chol.hip on the host: the constants it reads (the CPU test compares them with the source)
SPLITK_SLOTS, TAIL_MAX_WGS, SPLITK_MAX = 512, 192, 32


def ragged_tail(nrb, ncb, bc, j):
    """(first tile of the split tail, split factor) of block step j in a chunk of bc matrices that is not in the split-K layout;
    (tiles of the step, 1): nothing is split."""
    n_tiles = (ncb - j - 1) + (1 if j + 1 < nrb else 0)
    if j < 2 or n_tiles <= 0:
        return n_tiles, 1
    rounds = n_tiles * bc // SPLITK_SLOTS
    n_plain = rounds * SPLITK_SLOTS // bc
    m = n_tiles - n_plain
    if n_plain * bc != rounds * SPLITK_SLOTS or m <= 0 or m * bc > TAIL_MAX_WGS:
        return n_tiles, 1
    s = min(SPLITK_SLOTS // (m * bc), j, SPLITK_MAX)
    return (n_plain, s) if s >= 3 else (n_tiles, 1)


def ragged_steps(nrb, ncb, bc):
    """[(step, first tile of the tail, split factor)] of the steps of a plain chunk that split their last round."""
    out = []
    for j in range(1, nrb):
        tail, s = ragged_tail(nrb, ncb, bc, j)
        if s > 1:
            out.append((j, tail, s))
    return out


def smallest_lookahead_shape(m=50, leaf_words=5):
    """(N, B) of the fewest block rows, then the fewest matrices (MLL only, one chunk), for which the plan reports look-ahead
    steps; N is the smallest of its block-row count."""
    from bark_amd.fitting import schedule_plan

    for nrb in range(4, 64):
        for B in range(1, 65):
            if schedule_plan(128 * nrb, B, m=m, leaf_words=leaf_words)["schedule"] == "splitk_lookahead":
                return 128 * (nrb - 1) + 1, B
    raise AssertionError("no look-ahead shape below 64 block rows")


# ------------------------------------------------------------------ inputs ----
def _null_tree(L):
    return create_empty_forest(1, L)[0]


def build_forests(case: Case, bounds, ft, seed):
    """(B, m, node_limit) forests of the case's kind in which every forest has between 1 and m - 1 null trees and the
    counts differ within the batch (so that shift differs per forest)."""
    rng = np.random.default_rng(seed)
    if case.kind == "prior":
        F = synthetic.sample_prior_forests(case.B, case.m, bounds, ft, seed=seed)
    elif case.kind == "bytes7":
        F = synthetic.full_binary_forests(case.B, case.m, D_CONT, 5, rng, node_limit=100)
    elif case.kind == "bytes8":
        F = synthetic.full_binary_forests(case.B, case.m, D_CONT, 8, rng, node_limit=511)
    else:
        raise ValueError(case.kind)
    nn = n_null(F)
    for b in range(case.B):
        if case.kind == "prior":
            want = 2 if nn[b] == 0 else 0  # prior forests have about 5 % null trees; a seed that gives none gets two
        else:
            want = 2 + b % 3
        bushy = [t for t in range(case.m) if not F[b, t, 0]["is_leaf"]]
        for t in bushy[:max(0, min(want, len(bushy) - 1))]:
            F[b, t] = _null_tree(F.shape[2])
    return F


@dataclass
class Inputs:
    case: Case
    F: np.ndarray  # (B, m, node_limit)
    X: np.ndarray
    y: np.ndarray  # (N, 1)
    ft: np.ndarray
    cand: object  # (C, d) or None
    noise: np.ndarray
    scale: np.ndarray  # what the entry point receives: the model's scale times the no-null factor
    shift: np.ndarray
    info: object  # bark_pack_info of the batch
    rep: int
    leaf_words: int

    @property
    def y1(self):
        return self.y[:, 0]


def pack_info(F, ft):
    lib = _lib.lib()
    info = _lib.PackInfo()
    F = np.ascontiguousarray(F)
    ft = np.ascontiguousarray(ft, dtype=np.int64)
    _lib.check(lib.bark_forest_pack_info(_lib.ptr(F), F.shape[0], F.shape[1], F.shape[2], _lib.ptr(ft), ft.shape[0],
                                         ctypes.byref(info)))
    return info


def leaf_rep(info):
    """LeafRep of common.h from the packer's info: bits, or bytes of at most / more than 128 leaves a tree."""
    if int(_lib.lib().bark_leaf_encoding(ctypes.byref(info))) == 1:
        return REP_BITS
    return REP_BYTES7 if info.max_leaves <= 128 else REP_BYTES8


def make_inputs(case: Case) -> Inputs:
    seed = zlib.crc32(case.name.encode()) % 100003 + 101 * case.reseed  # the row's own: the table can change around it
    if case.problem == "mixed":
        X, y, bounds, ft = synthetic.mixed_problem(case.N, seed=seed)
        cand = synthetic.mixed_problem(case.C, seed=seed + 1)[0] if not case.identity and case.C else None
    else:
        X, y, bounds, ft = synthetic.unit_cube_problem(case.N, D_CONT, seed=seed)
        cand = synthetic.unit_cube_problem(case.C, D_CONT, seed=seed + 1)[0] if not case.identity and case.C else None
    F = build_forests(case, bounds, ft, seed + 2)
    rng = np.random.default_rng(seed + 3)
    noise, scale = rng.uniform(0.05, 0.3, case.B), rng.uniform(0.6, 1.5, case.B)
    shift, factor = no_null_params(F)
    if len(set(n_null(F).tolist())) == 1 and case.B > 1:  # the same count everywhere: any shift is a valid input
        shift = shift + 1e-3 * np.arange(case.B) / case.B
    info = pack_info(F, ft)
    return Inputs(case, F, X, y, ft, cand, noise, scale * factor, shift, info, leaf_rep(info),
                  int(_lib.lib().bark_leaf_words(ctypes.byref(info))))


def compared_forests(case: Case):
    """First, middle and last forest of every chunk."""
    pick = set()
    for c0 in range(0, case.B, case.bc):
        n = min(case.bc, case.B - c0)
        pick |= {c0, c0 + n // 2, c0 + n - 1}
    return sorted(pick)


def reference(inp: Inputs, forests, *, shift=True, scale=True, route="lu"):
    """The outputs of the listed forests: a list of dicts (solve_system).  shift / scale False: as a NULL argument (without
    scale the entry point evaluates the MLL only)."""
    idx = list(forests)
    return reference_arrays(inp.F[idx], inp.X, inp.y, inp.ft, inp.noise[idx], inp.scale[idx] if scale else None,
                            inp.shift[idx] if shift else None, inp.cand if scale else None, inp.case.identity and scale, route)


def plan_of(inp: Inputs, chunk="case", timing=False):
    from bark_amd.fitting import schedule_plan

    case = inp.case
    return schedule_plan(case.N, case.B, C=case.n_cand, chunk=case.chunk if chunk == "case" else chunk, m=case.m,
                         leaf_words=inp.leaf_words, timing=timing)


WANT_REP = {"prior": REP_BITS, "bytes7": REP_BYTES7, "bytes8": REP_BYTES8}


def check_cell(inp: Inputs):
    """The row reaches the cell it names: leaf representation, schedule of the full chunks and of the last one, fused Gram,
    split-K layout and (where the row says so) split-K steps — from the plan query the entry point configures itself from."""
    case = inp.case
    assert inp.rep == WANT_REP[case.kind], (case.name, inp.rep, int(inp.info.max_leaves))
    d = plan_of(inp)
    got = (d["schedule"], d["last_schedule"], d["fused_gram"], d["splitk_layout"])
    assert got == case.plan, (case.name, got, d)
    if case.split is not None:
        assert (d["splitk_steps"] > 0) == case.split, (case.name, d)
    one_launch = ("one_block", "two_block", "multi_block")
    if case.cell in one_launch:
        assert case.plan[:2] == (case.cell, case.cell), case.name
    assert (case.other == "timing") == (case.plan[0] in one_launch or case.plan[1] in one_launch), case.name
    if case.other == "timing":
        t = plan_of(inp, timing=True)
        assert t["schedule"] not in one_launch and t["last_schedule"] not in one_launch, (case.name, t)
    elif case.other is not None:
        o = plan_of(inp, chunk=case.other)
        assert o["fused_gram"] == d["fused_gram"] and o["chunk"] != d["chunk"], (case.name, o)
    if case.plan[1] == "plain" and case.plan[2] == 1:  # fused plain chunks: which steps split their ragged last round
        full = ragged_steps(d["nrb"], d["ncb"], d["chunk"]) if case.plan[0] == "plain" else []
        last = ragged_steps(d["nrb"], d["ncb"], d["last_chunk"])
        if case.cell == "plain_fused_ragged_split":
            assert not full and len(last) >= 2 and d["last_chunk"] < d["chunk"], (case.name, full, last)
            assert not ragged_steps(d["nrb"], d["ncb"], case.other), case.name  # the other route has no split step
        else:
            assert not full and not last, (case.name, full, last)
    if case.identity or case.n_cand:
        assert d["fused_gram"] == 0 and d["ncb"] == d["nrb"] + -(-case.n_cand // 128), (case.name, d)
    nn = n_null(inp.F)
    assert (nn >= 1).all() and (nn < case.m).all(), (case.name, nn)
    assert case.B == 1 or len(set(inp.shift.tolist())) > 1, case.name
    return d


# ------------------------------------------------------------------ the entry point, through ctypes ----
INFO_GUARD = -77


class Outputs:
    """Device outputs of one call, each allocated with one extra forest's worth of elements behind it (the guard band) and
    pre-filled with NaN (info_out: INFO_GUARD)."""

    def __init__(self, B, C, want_cov, device):
        import torch

        nan = float("nan")
        self.B, self.C = B, C
        self.mll = torch.full((B + 1,), nan, dtype=torch.float64, device=device)
        self.info = torch.full((B + 1,), INFO_GUARD, dtype=torch.int32, device=device)
        self.mu = self.var = self.cov = None
        if C:
            self.mu = torch.full((B + 1, C), nan, dtype=torch.float64, device=device)
            self.var = torch.full((B + 1, C), nan, dtype=torch.float64, device=device)
            if want_cov:
                self.cov = torch.full((B + 1, C, C), nan, dtype=torch.float64, device=device)
        self.timing = None

    def arrays(self):
        return {k: getattr(self, k) for k in ("mll", "mu", "var", "cov") if getattr(self, k) is not None}

    def host(self, name, forests=None):
        t = getattr(self, name)[:self.B]
        return (t if forests is None else t[list(forests)]).cpu().numpy()

    def guards_intact(self):
        import torch

        ok = bool((self.info[self.B:] == INFO_GUARD).all())
        return ok and all(bool(torch.isnan(t[self.B:]).all()) for t in self.arrays().values())

    def nan_inside(self):
        import torch

        return {k: int(torch.isnan(t[:self.B]).sum()) for k, t in self.arrays().items()}

    def same_bits(self, other):
        import torch

        mine, theirs = self.arrays(), other.arrays()
        return mine.keys() == theirs.keys() and all(
            torch.equal(mine[k].view(torch.int64), theirs[k].view(torch.int64)) for k in mine) and torch.equal(self.info, other.info)


def run(inp: Inputs, *, shift="own", scale="own", two_pi=False, chunk="case", timing=False, want_cov=True):
    """One bark_mll_batched_hip call on the case's inputs (modelled on fitting.mll._run).  shift / scale: "own", an array or
    None (a NULL pointer; without scale the flags drop BARK_MLL_INCLUDE_SCALE, MLL only).  timing: pass a bark_mll_timing."""
    import torch

    from bark_amd.forest import _points, packed_forest

    lib = _lib.lib()
    case = inp.case
    B = case.B
    Xd, _ = _points(inp.X, inp.ft.shape[0])
    N, d = Xd.shape
    dev = Xd.device
    up = lambda a: None if a is None else _lib.to_device(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)))
    yd = up(inp.y)
    noise_d = up(inp.noise)
    scale_d = up(inp.scale if isinstance(scale, str) else scale)
    shift_d = up(inp.shift if isinstance(shift, str) else shift)
    for t in (noise_d, scale_d, shift_d):
        assert t is None or t.shape[0] == B
    flags = (_lib.MLL_INCLUDE_SCALE if scale_d is not None else 0) | (_lib.MLL_INCLUDE_2PI if two_pi else 0)
    C, cand_d = 0, None
    if scale_d is not None:
        if case.identity:
            flags |= _lib.MLL_RHS_IDENTITY
            C = N
        elif case.C:
            cand_d, _ = _points(inp.cand, inp.ft.shape[0])
            C = cand_d.shape[0]
    out = Outputs(B, C, want_cov, dev)
    pf = packed_forest(np.ascontiguousarray(inp.F), inp.ft)
    Bc = min(B, (case.chunk if chunk == "case" else chunk) or B)
    ws = _lib.workspace(int(lib.bark_mll_workspace_bytes(N, C, pf.m, Bc)))
    if timing:
        out.timing = _lib.MllTiming()
    tref = ctypes.byref(out.timing) if timing else None

    def call():
        _lib.check(lib.bark_mll_batched_hip(
            _lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd), _lib.ptr(noise_d), _lib.ptr(scale_d),
            _lib.ptr(shift_d), flags, _lib.ptr(cand_d), C, _lib.ptr(out.mll), _lib.ptr(out.mu), _lib.ptr(out.var),
            _lib.ptr(out.cov), _lib.ptr(out.info), _lib.ptr(ws), ws.numel(), Bc, tref, _lib.stream_ptr()))
        torch.cuda.synchronize()

    call()
    if bool((out.info[:B] == -3).any()):  # the device-side wait timed out (include/bark_hip.h): event joins from now on
        lib.bark_device_wait(0)
        call()
    return out
