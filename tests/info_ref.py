"""Where the first non-positive pivot of a matrix falls: the host side of tests/test_gpu_sweep_info.py, which holds info_out of
the sweep entry points (include/bark_hip.h: LAPACK potrf's info, the 1-based index of the first non-positive pivot) to a pivot
that the test places, per matrix, at the positions where the kernels' index arithmetic changes.  numpy, the oracle and
sweep_ref / leafspace_ref only; tests/test_sweep_info_reference_cpu.py checks everything here without a GPU.

The dense entry point.  `shift` is per matrix and subtracts a rank-one term:

    K_s = scale (K - shift) + s2 I = A - scale shift 11',      A = scale K + s2 I  (positive definite),  s2 = 1e-6 + noise > 0.

With q_k = 1_k' A_k^-1 1_k over the leading k x k block (the running sum of squares of L^-1 1, A = L L'; q_0 = 0) the matrix
determinant lemma gives det (K_s)_k = det A_k (1 - scale shift q_k), so

    pivot_k(K_s) = pivot_k(A) (1 - scale shift q_k) / (1 - scale shift q_{k-1}).

q_k is non-decreasing, so shift = 2 / (scale (q_{p-1} + q_p)) makes pivot p the first non-positive one, and that pivot is
-pivot_p(A) <= -s2.  (p = 1: shift = 2 (scale + s2) / scale, the pivot -(scale + s2).)  place_pivot() returns that shift and
the pivots of the K_s that sweep_ref.form() builds from it — rounded as the header states — from one Cholesky factorisation of
the leading (p - 1) block and one triangular solve.

The margin condition: every preceding pivot > PRE_MIN = 1e-6 and the failing pivot < FAIL_MAX = -1e-3.  Both are more than six
orders above what another summation order of fp64 can move (pivots of matrices with entries of order 1: ~1e-13 at N = 2100), so
the index cannot depend on the kernel's order of operations.  A position that misses the condition is never used.

The leaf-space entry points factor M = I + c Z'Z, c = scale / (m s2), which fails for a negative scale: the leading k x k block
stays positive definite while -1/c > lambda_max((Z'Z)_k).  leafspace_place() looks for a position where that quantity strictly
grows and the same margin condition holds."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np

import sweep_ref as sr
from leafspace_ref import solve_lower
from oracle import oracle as orc

PRE_MIN, FAIL_MAX = 1e-6, -1e-3
NB, SB = 128, 16  # block step of the sweep, sub-block of the diagonal tile (chol_tiles.h)
BAD_NOISE = -1.5  # the "noise" class: every diagonal entry scale (1 - shift) + 1e-6 - 1.5 is negative
MAX_BAD, MAX_BAD_LARGE, LARGE_N = 9, 6, 1500


# ------------------------------------------------------------------ placing a pivot ----
def _running_q(A):
    """(pivots of A, q_1 .. q_n) of a positive definite A."""
    L = np.linalg.cholesky(A)
    t = solve_lower(L, np.ones((A.shape[0], 1)))[:, 0]
    return np.diag(L) ** 2, np.cumsum(t * t)


def _a_matrix(K, scale, s2):
    A = np.float64(scale) * np.asarray(K, dtype=np.float64)
    A[np.diag_indices_from(A)] += s2
    return A


def _form(K, shift, scale, s2):
    """sweep_ref.form with the diagonal term given as s2 = 1e-6 + noise."""
    A = (np.asarray(K, dtype=np.float64) - np.float64(shift)) * np.float64(scale)
    A[np.diag_indices_from(A)] += s2
    return A


def leading_pivots(K_s, p):
    """The first p pivots of the elimination of K_s in order, given that the leading (p - 1) block is positive definite
    (numpy raises LinAlgError otherwise): one Cholesky of that block and one triangular solve for pivot p."""
    piv = np.empty(p)
    if p > 1:
        L = np.linalg.cholesky(K_s[:p - 1, :p - 1])
        piv[:p - 1] = np.diag(L) ** 2
        r = solve_lower(L, K_s[:p - 1, p - 1:p])[:, 0]
        piv[p - 1] = K_s[p - 1, p - 1] - r @ r
    else:
        piv[0] = K_s[0, 0]
    return piv


def place_pivot(K, scale, s2, p):
    """(shift, pivots 1 .. p of K_s = scale (K - shift) + s2 I) such that pivot p is the first non-positive one.  K: the Gram
    matrix (only its leading p x p block is read)."""
    K = np.asarray(K, dtype=np.float64)[:p, :p]
    _, q = _running_q(_a_matrix(K, scale, s2))
    shift = 2.0 / (scale * ((q[p - 2] if p > 1 else 0.0) + q[p - 1]))
    return shift, leading_pivots(_form(K, shift, scale, s2), p)


def predicted_pivots(dA, q, p):
    """The closed form above: pivots 1 .. p of K_s for the shift of place_pivot, from the pivots dA and the q of A."""
    c = 2.0 / ((q[p - 2] if p > 1 else 0.0) + q[p - 1])
    q0 = np.concatenate([[0.0], q[:p - 1]])
    return dA[:p] * (1.0 - c * q[:p]) / (1.0 - c * q0)


def margin_ok(piv):
    return bool(piv[-1] < FAIL_MAX and (len(piv) == 1 or piv[:-1].min() > PRE_MIN))


def eliminate(K_s, replace=False):
    """The plain unblocked elimination, column by column: (pivots, 1-based indices of the non-positive ones).  replace=False
    stops at the first non-positive (or NaN) pivot; replace=True puts 1.0 in its place and goes on, as the kernels do
    (chol_diag.h, block4)."""
    A = np.asarray(K_s, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    piv, bad = np.empty(n), []
    with np.errstate(all="ignore"):
        for k in range(n):
            col = A[k:, k] - L[k:, :k] @ L[k, :k]
            piv[k] = col[0]
            if not col[0] > 0.0:
                bad.append(k + 1)
                if not replace:
                    return piv[:k + 1], bad
                col[0] = 1.0
            L[k:, k] = col / np.sqrt(col[0])
    return piv, bad


def first_bad_pivot(K_s):
    """LAPACK potrf's info of K_s: 0, or the 1-based index of the first non-positive pivot."""
    bad = eliminate(K_s)[1]
    return bad[0] if bad else 0


# ------------------------------------------------------------------ the position classes ----
CLASSES = ("p1", "group", "p17", "p128", "p129", "middle", "last_first", "pN", "noise")


def class_positions(N):
    """class -> the positions it may take at N, nearest to its target first; classes that N has no position for are absent.
    A position is listed once: under its first class in the order of CLASSES.  "noise" has no position of its own (its first
    failure is pivot 1, the later ones are what it is about): it needs a second 16 x 16 sub-block."""
    nrb = -(-N // NB)
    near = lambda lo, hi, t: sorted(range(lo, hi + 1), key=lambda p: (abs(p - t), p))
    out = {"p1": [1]}
    if N >= 5:
        out["group"] = near(5, min(16, N), 10)
    for name, p in (("p17", 17), ("p128", 128), ("p129", 129)):
        if N >= p:
            out[name] = [p]
    if nrb >= 3:
        j = (nrb - 1) // 2  # a block step with steps before and after it
        out["middle"] = near(j * NB + 1, (j + 1) * NB, j * NB + 77)
        out["last_first"] = [NB * (nrb - 1) + 1]
    if N > 1 and all(N not in v for v in out.values()):
        out["pN"] = [N]
    if N > SB:
        out["noise"] = [1]
    return {k: out[k] for k in CLASSES if k in out}


# ------------------------------------------------------------------ which matrices of a row are made bad ----
@dataclass
class Bad:
    b: int  # matrix of the batch
    cls: str
    p: int  # the expected info_out[b]
    shift: float
    noise: float
    pivots: np.ndarray  # pivots 1 .. p of the K_s the kernel is given


@dataclass
class Call:
    """One call of a row: the batch's own noise and shift with those of the bad matrices replaced."""
    bad: list
    noise: np.ndarray
    shift: np.ndarray
    info: np.ndarray  # the expected info_out, (B,) int32

    @property
    def healthy(self):
        return np.flatnonzero(self.info == 0)


def chunks_of(case):
    return [(c0, min(case.bc, case.B - c0)) for c0 in range(0, case.B, case.bc)]


def _positions(n, turn):
    """Positions inside a chunk of n matrices in the order they are made bad.  The first four are the middle and its right
    neighbour (two adjacent ones), the first and the last; `turn` says which pair leads."""
    mid = [n // 2, n // 2 + 1]
    heads = ([*mid, 0, n - 1], [n - 1, 0, *mid], [0, n - 1, *mid[::-1]])
    want = heads[turn % 3] + [1, n - 2, n // 4, 3 * n // 4, n // 4 + 1, 3 * n // 4 + 1] + list(range(n))
    seen, out = set(), []
    for p in want:
        if 0 <= p < n and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def choose_slots(case, want, rot):
    """`want` matrices of the batch (fewer if the chunks do not have them): round robin over the chunks — first, last, middle,
    then the others — each taking its _positions() in turn, led by another pair in every chunk and every call (`rot`); a chunk
    of n matrices gives at most n - 1, so that it keeps a healthy one."""
    chunks = chunks_of(case)
    k = len(chunks)
    order = list(dict.fromkeys([0, k - 1, k // 2] + list(range(k))))
    seqs = []
    for rank, ci in enumerate(order):
        c0, n = chunks[ci]
        seqs.append([c0 + p for p in _positions(n, rank + rot)][:n - 1])
    slots, depth = [], 0
    while len(slots) < want and any(depth < len(s) for s in seqs):
        for s in seqs:
            if depth < len(s) and len(slots) < want:
                slots.append(s[depth])
        depth += 1
    return slots


@dataclass
class RowPlan:
    calls: list
    classes: dict  # class_positions of the row
    unassigned: list = field(default_factory=list)  # classes no matrix of the row had an admissible position for


class _Matrices:
    """Per matrix of the batch, on first use: the Gram matrix K, the pivots of A and its q."""

    def __init__(self, inp):
        self.inp, self.cache = inp, {}

    def __call__(self, b):
        if b not in self.cache:
            inp = self.inp
            K = orc.batched_forest_gram_matrix(inp.F[b:b + 1], inp.X, inp.X, inp.ft)[0]
            s2 = 1e-6 + inp.noise[b]
            self.cache[b] = (K, s2, *_running_q(_a_matrix(K, inp.scale[b], s2)))
        return self.cache[b]


def _try_class(inp, mats, b, cls, positions, tries=12):
    """The Bad of class `cls` at matrix b, or None where no position of the class meets the margin condition there."""
    scale = float(inp.scale[b])
    if cls == "noise":
        s2 = 1e-6 + BAD_NOISE
        piv = np.array([np.float64(scale) * (np.float64(1.0) - np.float64(inp.shift[b])) + s2])  # K[0, 0] = 1: all m trees agree
        return Bad(b, cls, 1, float(inp.shift[b]), BAD_NOISE, piv) if margin_ok(piv) else None
    K, s2, dA, q = mats(b)
    for p in positions[:tries]:
        if not margin_ok(predicted_pivots(dA, q, p)):
            continue
        try:
            shift, piv = place_pivot(K, scale, s2, p)
        except np.linalg.LinAlgError:
            continue
        if margin_ok(piv):
            return Bad(b, cls, p, float(shift), float(inp.noise[b]), piv)
    return None


def plan_row(inp, max_bad=None) -> RowPlan:
    """The calls of one row of sweep_ref.CASES: every class the row's N allows once, at most `max_bad` bad matrices per call
    (default: 9, 6 where N > 1500), as many calls as that takes."""
    case = inp.case
    classes = class_positions(case.N)
    cap = max_bad or (MAX_BAD_LARGE if case.N > LARGE_N else MAX_BAD)
    mats = _Matrices(inp)
    queue, calls = list(classes), []
    for rot in range(2 * len(classes) + 2):
        if not queue:
            break
        bad = []
        for b in choose_slots(case, min(cap, len(queue)), rot):
            for cls in queue:
                hit = _try_class(inp, mats, b, cls, classes[cls])
                if hit is not None:
                    bad.append(hit)
                    queue.remove(cls)
                    break
        if bad:
            noise, shift, info = inp.noise.copy(), inp.shift.copy(), np.zeros(case.B, dtype=np.int32)
            for h in bad:
                noise[h.b], shift[h.b], info[h.b] = h.noise, h.shift, h.p
            calls.append(Call(bad, noise, shift, info))
    return RowPlan(calls, classes, queue)


def with_call(inp, call):
    """The row's inputs with the call's noise (sweep_ref.run takes the shift as an argument)."""
    return dataclasses.replace(inp, noise=call.noise)


def bad_matrix(inp, h: Bad):
    """The K_s of a bad matrix as the kernel forms it (sweep_ref.form)."""
    K = orc.batched_forest_gram_matrix(inp.F[h.b:h.b + 1], inp.X, inp.X, inp.ft)[0]
    return sr.form(K, h.shift, inp.scale[h.b], h.noise)


# ------------------------------------------------------------------ leaf space ----
def leafspace_place(G, lo, hi, fractions=(0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9)):
    """(k, c, pivots 1 .. k of M = I + c G) with lo < k <= hi the first non-positive pivot and the margin condition met, or None.
    G = Z'Z (R, R).  lambda_max of the leading blocks is non-decreasing in k: for a threshold tau between its values at lo and hi
    the first k whose lambda_max exceeds tau is found by bisection, and -1/c is put half way between lambda_max at k - 1 and at k."""
    lam = lambda k: float(np.linalg.eigvalsh(G[:k, :k])[-1]) if k > 0 else 0.0
    l_lo, l_hi = lam(lo), lam(hi)
    if not l_hi > l_lo:
        return None
    for f in fractions:
        tau = l_lo + f * (l_hi - l_lo)
        a, b = lo, hi  # lam(a) <= tau < lam(b)
        while b - a > 1:
            mid = (a + b) // 2
            if lam(mid) > tau:
                b = mid
            else:
                a = mid
        l0, l1 = lam(b - 1), lam(b)
        if not l1 > l0:
            continue
        c = -2.0 / (l0 + l1)
        M = c * G[:b, :b]
        M[np.diag_indices(b)] += 1.0
        try:
            piv = leading_pivots(M, b)
        except np.linalg.LinAlgError:
            continue
        if margin_ok(piv):
            return b, c, piv
    return None


# lo < k <= hi (None: R); "inner": past 256 but not the last leaves, where a null tree's one leaf (every point) makes the jump
LEAF_RANGES = {"first": (0, 128), "second": (128, 256), "past256": (256, None), "inner": (256, 500)}


def _leaf_cases():
    import leafspace_ref as lr

    # (case, {forest: range}): first, two adjacent ones in the middle and the last forest are bad; the others are healthy
    return [
        (lr.Case("info_r323_plain", ((("full", 10, 5), ("null", 3)),), N=300, B=7, shape=(323, 11, 3, "plain"), C=33, S=5, seed=21),
         {0: "first", 3: "second", 4: "past256", 6: "first"}),
        (lr.Case("info_r513_splitk", ((("full", 4, 7), ("null", 1)),), N=300, B=6, shape=(513, 17, 5, "splitk"), C=33, S=5, seed=22),
         {0: "past256", 2: "first", 3: "second", 5: "inner"}),
    ]


@dataclass
class LeafPlan:
    inp: object  # leafspace_ref.Inputs
    scale: np.ndarray  # the batch's scale with the bad forests' replaced by c m s2 < 0
    info: np.ndarray  # expected info_out
    placed: dict  # forest -> (range, k, c, pivots)
    missing: list  # (forest, range) without an admissible position

    @property
    def healthy(self):
        return np.flatnonzero(self.info == 0)


def leaf_plans():
    import leafspace_ref as lr

    plans = []
    for case, which in _leaf_cases():
        inp = lr.make_inputs(case)
        scale, info = inp.scale.copy(), np.zeros(case.B, dtype=np.int32)
        placed, missing = {}, []
        for n, (b, rng) in enumerate(which.items()):
            G = inp.Z[b].T @ inp.Z[b]
            lo, hi = LEAF_RANGES[rng]
            fr = (0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9)
            hit = leafspace_place(G, lo, hi or inp.R, fr[n % 2:] + fr[:n % 2])  # a repeated range starts at another threshold
            if hit is None:
                missing.append((b, rng))
                continue
            k, c, piv = hit
            placed[b] = (rng, k, c, piv)
            scale[b] = c * inp.m * (1e-6 + inp.noise[b])
            info[b] = k
        plans.append(LeafPlan(inp, scale, info, placed, missing))
    return plans


LEAF_GUARD = -77


def leaf_run(inp, entry, scale):
    """One call of a leaf-space entry point — "mll" (bark_mll_leafspace_hip with the candidates: mll, mu, var), "inverse"
    (bark_kernel_inverse_leafspace_hip: mll, kinv, kinv_y) or "draws" (bark_posterior_samples_hip: f) — with the given scale:
    ({name: device tensor}, info tensor), each with one extra forest's worth of elements behind it, pre-filled with NaN
    (info: LEAF_GUARD).  Needs a GPU."""
    import torch

    from bark_amd import _lib
    from bark_amd.forest import _points, packed_forest

    lib = _lib.lib()
    case = inp.case
    B, Bc = case.B, case.bc
    Xd, _ = _points(inp.X, inp.ft.shape[0])
    N, d = Xd.shape
    dev = Xd.device
    cand_d, _ = _points(inp.cand, inp.ft.shape[0])
    C = int(cand_d.shape[0])
    up = lambda a: _lib.to_device(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)))
    yd, noise_d, scale_d = up(inp.y), up(inp.noise), up(scale)
    pf = packed_forest(np.ascontiguousarray(inp.F), inp.ft)
    R, m = int(pf.info.max_bits), pf.m
    full = lambda *shape: torch.full((B + 1, *shape), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((B + 1,), LEAF_GUARD, dtype=torch.int32, device=dev)
    flags = _lib.MLL_INCLUDE_SCALE
    if entry == "mll":
        out = {"mll": full(), "mu": full(C), "var": full(C)}
        ws = _lib.workspace(int(lib.bark_mll_leafspace_workspace_bytes(N, R, m, Bc, C)))
        _lib.check(lib.bark_mll_leafspace_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd),
                                              _lib.ptr(noise_d), _lib.ptr(scale_d), flags, _lib.ptr(cand_d), C, _lib.ptr(out["mll"]),
                                              _lib.ptr(out["mu"]), _lib.ptr(out["var"]), _lib.ptr(info), _lib.ptr(ws), ws.numel(),
                                              Bc, _lib.stream_ptr()))
    elif entry == "inverse":
        out = {"mll": full(), "kinv": full(N, N), "kinv_y": full(N)}
        ws = _lib.workspace(int(lib.bark_kernel_inverse_leafspace_workspace_bytes(N, R, m, Bc)))
        _lib.check(lib.bark_kernel_inverse_leafspace_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d,
                                                         _lib.ptr(yd), _lib.ptr(noise_d), _lib.ptr(scale_d), flags,
                                                         _lib.ptr(out["mll"]), _lib.ptr(out["kinv"]), _lib.ptr(out["kinv_y"]),
                                                         _lib.ptr(info), _lib.ptr(ws), ws.numel(), Bc, _lib.stream_ptr()))
    elif entry == "draws":
        S = case.S
        out = {"f": full(S, C)}
        eps_d = _lib.to_device(np.ascontiguousarray(inp.eps))
        ws = _lib.workspace(int(lib.bark_posterior_samples_workspace_bytes(N, R, m, Bc, C, S)))
        _lib.check(lib.bark_posterior_samples_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd),
                                                  _lib.ptr(noise_d), _lib.ptr(scale_d), _lib.ptr(cand_d), C, _lib.ptr(eps_d), S,
                                                  _lib.SAMPLE_FULL, _lib.ptr(out["f"]), None, None, _lib.ptr(info), _lib.ptr(ws),
                                                  ws.numel(), Bc, _lib.stream_ptr()))
    else:
        raise ValueError(entry)
    torch.cuda.synchronize()
    return out, info
