"""Host reference of the leaf-space sampler chains (csrc/leafchain.hip, bark_amd.fitting.LeafChainBatch) and the case table of
tests/test_gpu_leafchain.py (numpy + the oracle: no GPU, no library).  tests/test_leafchain_reference_cpu.py holds every case to
the decision-margin condition and this module to the dense route.

Notation of include/bark_hip.h: s2 = 1e-6 + noise, c = scale / (m s2), Z the N x R one-hot leaf matrix, M = I + c Z'Z, P = M^-1,
v = Z'y, q = v'Pv;  log|K_s| = N log s2 + log|M|,  y'K_s^-1 y = (y'y - c q) / s2.  Swapping a tree with slots T for one with the
one-hot columns Z' (O = every other slot):

    B = c Z_O'Z' (zero rows on T),  D = I + c diag(Z''1),  Y = P B,  g = P v_O
    QB = Y - P[:,T] P_TT^-1 Y[T],   Qv = g - P[:,T] P_TT^-1 g[T]
    S = D - B'QB,  u = Z''y - B'Qv,  q' = v_O'Qv + u'S^-1 u,  log|M'| = log|M| + log|P_TT| + log|S|
    accept:  P_OO <- Q + QB S^-1 QB'  (Q = P_OO - P_OT P_TT^-1 P_TO),  P_O,T' = -QB S^-1,  P_T'T' = S^-1

with the slot bookkeeping of the device: the new leaves reuse the old tree's slots, then pop the free stack (lowest free slot
first after init), a shrinking tree pushes its leftovers; a free slot is an identity row of P."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import lowrank_ref as lr

MARGIN = 1e-6  # |log_u - log_alpha| of every proposal with finite inputs: a condition on the inputs, never lowered
D = lr.CHAIN_D
# case n4097: largest |P(float64) - P(longdouble)| of the host reference over the sweep, measured 1.18e-10;
# the device, which sums in another order, is allowed 100 x this figure
N4097_P_DEVIATION = 1.2e-10


# ------------------------------------------------------------------------------------ trees ----
def leaf_order(tree):
    """Node indices of the leaves reachable from the root, depth first, left child first: the packer's order."""
    out, stack = [], [0]
    while stack:
        n = stack.pop()
        if tree["is_leaf"][n]:
            out.append(n)
        else:
            stack.append(int(tree["right"][n]))
            stack.append(int(tree["left"][n]))
    return out


def onehot(tree, X, ft):
    """(N, leaves) one-hot columns in the packer's order (a leaf no point reaches is a zero column)."""
    from oracle import oracle as orc

    reached = orc.pass_through_forest(tree[None], X, ft)[:, 0]
    return (reached[:, None] == np.asarray(leaf_order(tree))[None, :]).astype(np.float64)


def unreached_tree(leaves, feature):
    """A caterpillar whose first split sends every point of the unit cube left: leaves - 1 leaves that no point reaches."""
    tree = lr.caterpillar_tree(leaves, feature)
    tree["threshold"][0] = 5.0
    return tree


def spd_inverse(A, dtype):
    """A^-1 and log|A| by the symmetric sweep operator (the device's elimination); LinAlgError for a non-positive pivot."""
    A = np.array(A, dtype=dtype)
    r = A.shape[0]
    logdet = dtype(0)
    for k in range(r):
        d = A[k, k]
        if not d > 0:
            raise np.linalg.LinAlgError("non-positive pivot")
        logdet += np.log(d)
        col = A[:, k].copy()
        A -= np.outer(col, col) / d
        A[:, k] = col / d
        A[k, :] = col / d
        A[k, k] = -1 / d
    return -A, logdet


# ------------------------------------------------------------------------------- reference ----
class RefChain:
    """One chain on the host, carried in `dtype`.  symmetric=False keeps the rewrite as the formulas give it (one triangle from
    S^-1 QB', the other from its transpose as computed): what the CPU test shows to drift."""

    def __init__(self, forest, noise, scale, X, y, ft, capacity, dtype=np.float64, symmetric=True):
        self.dtype, self.symmetric = dtype, symmetric
        self.X, self.ft, self.y = X, ft, np.asarray(y, dtype=dtype).reshape(-1)
        self.N, self.m, self.cap = X.shape[0], forest.shape[0], capacity
        self.noise, self.scale = dtype(noise), dtype(scale)
        self.Z = np.zeros((self.N, capacity))
        self.slots, n = [], 0
        for t in range(self.m):
            Zt = onehot(forest[t], X, ft)
            self.slots.append(list(range(n, n + Zt.shape[1])))
            self.Z[:, n:n + Zt.shape[1]] = Zt
            n += Zt.shape[1]
        assert n <= capacity
        self.free = list(range(capacity - 1, n - 1, -1))  # pop() gives the lowest free slot first
        self.yy = self.y @ self.y
        self.rebuild(self.noise, self.scale)

    @property
    def coef(self):
        return self.scale / (self.dtype(self.m) * (self.dtype(1e-6) + self.noise))

    def system(self, noise, scale):
        c = scale / (self.dtype(self.m) * (self.dtype(1e-6) + noise))
        M = np.eye(self.cap, dtype=self.dtype) + c * (self.Z.T @ self.Z).astype(self.dtype)
        P, logm = spd_inverse(M, self.dtype)
        v = (self.Z.T.astype(self.dtype) @ self.y)
        return P, logm, v @ P @ v

    def rebuild(self, noise, scale):
        self.noise, self.scale = self.dtype(noise), self.dtype(scale)
        self.P, self.logm, self.q = self.system(self.noise, self.scale)
        self.v = self.Z.T.astype(self.dtype) @ self.y

    def state(self, q=None, logm=None, noise=None, scale=None):
        """(y'K^-1 y, log|K|)."""
        q = self.q if q is None else q
        logm = self.logm if logm is None else logm
        noise = self.noise if noise is None else noise
        scale = self.scale if scale is None else scale
        s2 = self.dtype(1e-6) + noise
        c = scale / (self.dtype(self.m) * s2)
        return (self.yy - c * q) / s2, self.dtype(self.N) * np.log(s2) + logm

    @property
    def mll(self):
        quad, logdet = self.state()
        return float(0.5 * (-quad - logdet))

    def propose(self, t, new_tree):
        """-> (new_mll - cur_mll, commit) for swapping tree t; commit() applies it."""
        dt, c = self.dtype, self.coef
        T = self.slots[t]
        Zn = onehot(new_tree, self.X, self.ft)
        r_new = Zn.shape[1]
        if r_new - len(T) > len(self.free):
            raise ValueError("no free slot")
        Zo = self.Z.copy()
        Zo[:, T] = 0.0
        B = c * (Zo.T @ Zn).astype(dt)
        Dm = np.eye(r_new, dtype=dt) + c * np.diag(Zn.sum(axis=0)).astype(dt)
        vn = Zn.T.astype(dt) @ self.y
        vO = self.v.copy()
        vO[T] = 0
        P = self.P
        Y, g = P @ B, P @ vO
        PT = P[:, T]
        if self.symmetric:
            PTTi, ldT = spd_inverse(P[np.ix_(T, T)], dt)
        else:  # LAPACK's LU inverse: symmetric to rounding only
            PTTi, ldT = np.linalg.inv(P[np.ix_(T, T)]), np.linalg.slogdet(P[np.ix_(T, T)])[1]
        QB, Qv = Y - PT @ (PTTi @ Y[T]), g - PT @ (PTTi @ g[T])
        QB[T], Qv[T] = 0, 0
        S = Dm - B.T @ QB
        if self.symmetric:
            S = (S + S.T) / 2
        Si, ldS = spd_inverse(S, dt) if self.symmetric else (np.linalg.inv(S), np.linalg.slogdet(S)[1])
        u = vn - B.T @ Qv
        q_new = vO @ Qv + u @ Si @ u
        logm_new = self.logm + ldT + ldS
        quad, logdet = self.state()
        nquad, nlogdet = self.state(q_new, logm_new)
        delta = float(0.5 * (-nquad - nlogdet) - 0.5 * (-quad - logdet))

        def commit():
            if self.symmetric:
                Pn = P - PT @ PTTi @ PT.T + QB @ Si @ QB.T
                Pn = (Pn + Pn.T) / 2
            else:
                Pn = P - (PT @ PTTi) @ PT.T + QB @ (Si @ QB.T)
            new = [T[l] if l < len(T) else self.free.pop() for l in range(r_new)]
            for s in T[r_new:]:
                self.free.append(s)
            for s in T:
                Pn[s, :], Pn[:, s] = 0, 0
                Pn[s, s] = 1
                self.Z[:, s] = 0
                self.v[s] = 0
            F = QB @ Si
            for l, s in enumerate(new):
                Pn[:, s], Pn[s, :] = -F[:, l], -F[:, l]
            Pn[np.ix_(new, new)] = Si
            self.Z[:, new] = Zn
            self.v[new] = vn
            self.slots[t] = new
            self.P, self.q, self.logm = Pn, q_new, logm_new

        return delta, commit

    def propose_noise_scale(self, noise, scale):
        """-> (new_mll - cur_mll or NaN, commit); LinAlgError for a non-positive pivot."""
        noise, scale = self.dtype(noise), self.dtype(scale)
        if not (1e-6 + noise > 0):
            return float("nan"), None
        P, logm, q = self.system(noise, scale)
        quad, logdet = self.state()
        nquad, nlogdet = self.state(q, logm, noise, scale)

        def commit():
            self.noise, self.scale, self.P, self.logm, self.q = noise, scale, P, logm, q

        return float(0.5 * (-nquad - nlogdet) - 0.5 * (-quad - logdet)), commit

    def export(self):
        """Canonical P (capacity x capacity, identity beyond the leaves), v and the leaf counts."""
        order = [s for t in range(self.m) for s in self.slots[t]]
        P, v = np.eye(self.cap), np.zeros(self.cap)
        R = len(order)
        P[:R, :R] = np.asarray(self.P[np.ix_(order, order)], dtype=np.float64)
        v[:R] = np.asarray(self.v[order], dtype=np.float64)
        return P, v, np.array([len(s) for s in self.slots], dtype=np.int32)


def decide(delta, log_q, log_u) -> int:
    log_alpha = log_q + delta
    return 1 if (log_u <= log_alpha and log_u <= 0.0) else 0  # a NaN compares false: reject


# ----------------------------------------------------------------------------------- cases ----
class Case(NamedTuple):
    N: int
    nc: int
    init: tuple  # the m initial trees: a leaf count (a caterpillar) or (kind, leaves) with the kinds of `steps`
    steps: tuple  # (tree index, kind, leaves[, log_u]): kind "cat" caterpillar, "dead" unreached_tree, "g3" a golden tree; log_u,
    #               one number or one per chain (None: the random draw), replaces the draw: TAKE accepts, REFUSE rejects
    capacity: int
    lcap: int
    noise: float  # centre of the chains' noise levels (>= 1e-2)
    seed: int
    matrix: bool  # exported P is held to the matrix bar (N <= 300, noise 0.1)
    why: str


TAKE, REFUSE = -1e3, 1.0  # forced log_u: below every finite log_alpha of the table / positive, which the rule never accepts
_EDGE = ((0, "cat", 5), (1, "cat", 1), (2, "cat", 4), (0, "cat", 2), (1, "dead", 3))
CASES = {
    "n3": Case(3, 1, (1, 2), ((0, "cat", 2), (1, "cat", 1), (0, "cat", 3)), 8, 4, 0.1, 0, True, "fewer points than lanes, m = 2"),
    "n63": Case(63, 2, (1, 3, 4), _EDGE, 16, 8, 0.1, 0, True, "one point short of a plane word; root-only old and new, pop, push, "
                "the same tree twice, leaves no point reaches"),
    "n64": Case(64, 1, (1, 3, 4), _EDGE, 16, 8, 0.1, 1, True, "exactly one plane word"),
    "n65": Case(65, 2, (1, 3, 4), _EDGE, 16, 8, 0.1, 2, True, "one point into the second plane word"),
    "n129": Case(129, 3, (2, 8, 3), ((0, "cat", 8), (2, "cat", 8), (1, "cat", 1), (1, "cat", 8)), 24, 8, 0.05, 0, True,
                 "r = lcap on both sides; the sweep's worst case uses the capacity exactly (8 + 8 + 8 = 24)"),
    "nc64": Case(64, 64, (2, 3), ((0, "cat", 4), (1, "cat", 2), (0, "cat", 1)), 8, 4, 0.1, 0, True, "the full grid of chains"),
    "g3_n257": Case(257, 2, (), tuple((t, "g3", 0) for t in range(6)), 0, 32, 0.1, 0, True,
                    "mixed cat / int / cont golden forests of 50 trees"),
    "n4097": Case(4097, 4, (3, 5, 2, 4), ((0, "cat", 6), (1, "cat", 2), (0, "cat", 3)), 32, 8, 1.0, 0, False,
                  "65 plane words; the conditioning of a large N"),
    # wide trees and full slot capacity.  Every initial tree of the m = 64 cases has 9 leaves: 576 active slots, more than the
    # 512 threads of a workgroup.  Steps with a forced log_u are the ones tests/test_leafchain_reference_cpu.py
    # (test_table_contains_the_wide_edges) needs taken or refused; the others keep their random draw.
    "m64_cap1024": Case(600, 2, (9,) * 64, (
        (0, "cat", 32, TAKE),  # 9 -> 32: pops 23 slots
        (0, "cat", 32, (TAKE, REFUSE)),  # 32 -> 32 taken by chain 0; chain 1 refuses a 32-leaf proposal (inT reset, nothing written)
        (1, "cat", 23),  # 9 -> 23: steps 4 and 6 one entry past a pass of the workgroup
        (63, "cat", 12, TAKE),  # the last tree
        (2, "dead", 32, TAKE),  # 31 leaves no point reaches
        (0, "cat", 1, TAKE),  # 32 -> 1: pushes 31 slots
        (5, "cat", 32, TAKE),  # 9 -> 32: pops 23 of the pushed slots, last pushed first
        (2, "cat", 5),  # pushes 27 slots with empty planes
        # a 32-leaf proposal taken last: every accepted step computes q' afresh, so only the last one's v_O'Qv — at 32 leaves
        # the entry of step 6 that falls into the workgroup's third pass — reaches the scalars the sweep returns
        (63, "cat", 32, (TAKE, None))), 1024, 32, 0.1, 0, True,
        "m = 64 trees, 1024 slots, 32-leaf trees on both sides, pushes and pops of tens of slots"),
    # the table builder's worst case: 576 + (32 - 9) + (20 - 9) + (30 - 9) + (23 - 9) = 645 slots, odd; chain 0 takes every
    # growing step and runs the free stack empty before tree 3 shrinks
    "m64_tight": Case(600, 2, (9,) * 64, (
        (3, "cat", 32, TAKE), (63, "cat", 20, (TAKE, None)), (10, "cat", 30, (TAKE, None)), (1, "cat", 23, (TAKE, None)),
        (3, "cat", 1, TAKE), (10, "cat", 30)), 645, 32, 0.1, 3, True,
        "the capacity is the sweep's worst case exactly, odd and above 512; no free slot left in chain 0 after step 3"),
    "odd67": Case(130, 2, (5, ("dead", 9), 7, 11), ((0, "cat", 12), (1, "cat", 3), (2, "cat", 13), (3, "cat", 2), (1, "cat", 10)),
                  67, 13, 0.1, 0, True, "ragged tails of the lane- and wave-strided loops (67 slots), r from 9 to 13 = lcap, "
                  "empty-plane slots below active ones at init"),
}


class Inputs(NamedTuple):
    X: np.ndarray
    y: np.ndarray
    ft: np.ndarray
    forests: np.ndarray  # (nc, m, node_limit) initial forests
    old: np.ndarray  # (nc, steps, node_limit) the tree each step replaces if every earlier step were rejected ... see make_inputs
    new: np.ndarray  # (nc, steps, node_limit)
    tree_index: np.ndarray  # (steps,)
    noise: np.ndarray
    scale: np.ndarray
    log_q: np.ndarray  # (nc, steps)
    log_u: np.ndarray
    capacity: int
    lcap: int


def make_inputs(name) -> Inputs:
    from bark_amd import synthetic

    case = CASES[name]
    rng = np.random.default_rng([case.N, case.nc, case.seed, 7])
    steps = len(case.steps)
    tidx = np.array([s[0] for s in case.steps], dtype=np.int64)
    if name == "g3_n257":
        from conftest import load_golden
        from oracle import oracle as orc

        g = load_golden("g3_prior_mixed_n257")
        raw = orc.nodes_from_raw(g["forest"])
        X, y, ft = g["X"], g["y"].reshape(-1), g["feat_types"]
        forests = raw[:case.nc].copy()
        new = np.stack([np.stack([raw[2, (t + 3 * b) % raw.shape[1]] for t in range(steps)]) for b in range(case.nc)])
        leaves = max(len(leaf_order(tr)) for f in raw for tr in f)
        total = max(sum(len(leaf_order(tr)) for tr in f) for f in forests)
        assert leaves <= case.lcap
        capacity = (total + 6 * leaves + 31) // 32 * 32
        noise, scale = g["noise"][:case.nc].copy(), g["scale"][:case.nc].copy()
        noise = np.maximum(noise, 0.05)
    else:
        X, y, _, ft = synthetic.unit_cube_problem(case.N, D, seed=1000 * case.N + case.seed)
        kinds = {"cat": lr.caterpillar_tree, "dead": unreached_tree}
        init = [k if isinstance(k, tuple) else ("cat", k) for k in case.init]
        forests = np.stack([np.stack([kinds[kind](k, (b + t) % D) for t, (kind, k) in enumerate(init)]) for b in range(case.nc)])
        new = np.stack([np.stack([kinds[s[1]](s[2], (b + 2 * t + 1) % D) for t, s in enumerate(case.steps)]) for b in range(case.nc)])
        capacity = case.capacity
        noise = rng.uniform(0.8 * case.noise, 1.6 * case.noise, case.nc)
        scale = rng.uniform(0.7, 1.4, case.nc)
    # old_trees is validation only: the tree a step replaces when no earlier step of the sweep touched it, else the proposal of
    # the latest earlier step on the same tree (what a caller that accepted it would hold)
    old = np.empty_like(new)
    for t in range(steps):
        prev = [u for u in range(t) if tidx[u] == tidx[t]]
        old[:, t] = new[:, prev[-1]] if prev else forests[:, tidx[t]]
    log_q = rng.normal(0.0, 0.5, size=(case.nc, steps))
    log_u = np.log(rng.uniform(size=(case.nc, steps)))
    for t, s in enumerate(case.steps):
        if len(s) > 3:  # a forced log_u, drawn over: the stream of the random ones is the same with and without it
            for b, forced in enumerate(np.broadcast_to(np.array(s[3], dtype=object), (case.nc,))):
                if forced is not None:
                    log_u[b, t] = forced
    return Inputs(X, y, ft, forests, old, new, tidx, noise, scale, log_q, log_u, capacity, case.lcap)


class Trajectory(NamedTuple):
    mask: np.ndarray  # (nc, steps) 0 / 1
    margin: np.ndarray  # (nc, steps)
    quad: np.ndarray  # (nc,) after the sweep
    logdet: np.ndarray
    chains: list  # the RefChain of every chain (None on the dense route)
    final: np.ndarray  # (nc, m, node_limit) forests after the sweep
    init_active: list = None  # per chain the slots with a non-empty plane at init (leaf route)
    log: list = None  # per chain, per step: StepLog (leaf route)


class StepLog(NamedTuple):
    r_old: int
    r_new: int
    accepted: bool
    popped: tuple  # slots the swap took off RefChain's free stack, in the order taken
    pushed: tuple  # slots it put on the stack, in the order put
    free_after: int  # depth of the stack after the step


def leaf_sweep(inp: Inputs, dtype=np.float64, symmetric=True, chains=None) -> Trajectory:
    nc, steps = inp.log_q.shape
    mask, margin = np.zeros((nc, steps), dtype=np.int32), np.full((nc, steps), np.inf)
    quad, logdet, out = np.zeros(nc), np.zeros(nc), [None] * nc
    final = inp.forests.copy()
    active, log = [None] * nc, [None] * nc
    for b in (range(nc) if chains is None else chains):
        ch = RefChain(inp.forests[b], inp.noise[b], inp.scale[b], inp.X, inp.y, inp.ft, inp.capacity, dtype, symmetric)
        active[b], log[b] = np.flatnonzero(ch.Z.any(axis=0)), []
        for t in range(steps):
            k = int(inp.tree_index[t])
            held, stack = list(ch.slots[k]), list(ch.free)
            delta, commit = ch.propose(k, inp.new[b, t])
            if np.isfinite(inp.log_q[b, t] + delta) and np.isfinite(inp.log_u[b, t]):
                margin[b, t] = abs(inp.log_u[b, t] - (inp.log_q[b, t] + delta))
            mask[b, t] = decide(delta, inp.log_q[b, t], inp.log_u[b, t])
            if mask[b, t]:
                commit()
                final[b, inp.tree_index[t]] = inp.new[b, t]
            kept = 0  # a swap pops or pushes, never both: the stack below `kept` is untouched
            while kept < min(len(stack), len(ch.free)) and stack[kept] == ch.free[kept]:
                kept += 1
            log[b].append(StepLog(len(held), len(ch.slots[k]) if mask[b, t] else len(leaf_order(inp.new[b, t])), bool(mask[b, t]),
                                  tuple(stack[kept:][::-1]), tuple(ch.free[kept:]), len(ch.free)))
        q, ld = ch.state()
        quad[b], logdet[b], out[b] = float(q), float(ld), ch
    return Trajectory(mask, margin, quad, logdet, out, final, active, log)


def dense_sweep(inp: Inputs, chains=None) -> Trajectory:
    """The same sweep on the N x N inverse: lowrank_ref.swap + the oracle's leaf vectors — the independent route."""
    from oracle import oracle as orc

    nc, steps = inp.log_q.shape
    N, m = inp.X.shape[0], inp.forests.shape[1]
    y = inp.y.reshape(-1)
    mask, margin = np.zeros((nc, steps), dtype=np.int32), np.full((nc, steps), np.inf)
    quad, logdet = np.zeros(nc), np.zeros(nc)
    final = inp.forests.copy()
    for b in (range(nc) if chains is None else chains):
        K = inp.scale[b] * orc.forest_gram_matrix(final[b], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[b]) * np.eye(N)
        K_inv = np.linalg.inv(K)
        K_inv = 0.5 * (K_inv + K_inv.T)
        ld, q = np.linalg.slogdet(K)[1], y @ K_inv @ y
        s = np.sqrt(inp.scale[b] / m)
        for t in range(steps):
            k = int(inp.tree_index[t])
            U_old = s * orc.get_leaf_vectors(final[b, k], inp.X, inp.ft)
            U_new = s * orc.get_leaf_vectors(inp.new[b, t], inp.X, inp.ft)
            dquad, dlogdet, K_new = lr.swap(K_inv, np.concatenate([U_old, U_new], axis=1), U_old.shape[1], y)
            delta = 0.5 * (float(dquad) - float(dlogdet))
            if np.isfinite(inp.log_q[b, t] + delta) and np.isfinite(inp.log_u[b, t]):
                margin[b, t] = abs(inp.log_u[b, t] - (inp.log_q[b, t] + delta))
            mask[b, t] = decide(delta, inp.log_q[b, t], inp.log_u[b, t])
            if mask[b, t]:
                K_inv, q, ld = 0.5 * (K_new + K_new.T), q - dquad, ld + dlogdet
                final[b, k] = inp.new[b, t]
        quad[b], logdet[b] = float(q), float(ld)
    return Trajectory(mask, margin, quad, logdet, None, final)


def dense_P(forest, noise, scale, X, ft, capacity):
    """inv(M) of a forest in canonical order, identity beyond its leaves (numpy's LAPACK inverse)."""
    Z = np.concatenate([onehot(tr, X, ft) for tr in forest], axis=1)
    R = Z.shape[1]
    c = scale / (forest.shape[0] * (1e-6 + noise))
    P = np.eye(capacity)
    P[:R, :R] = np.linalg.inv(np.eye(R) + c * (Z.T @ Z))
    return P


# ------------------------------------------------------------------------- the g11 trajectory ----
class G11(NamedTuple):
    tree_margin: float  # smallest |log_u - log_alpha| over the tree proposals
    ns_margin: float  # the same over the noise / scale proposals
    accept: np.ndarray  # (chains, steps, m) decisions taken
    ns_accept: np.ndarray  # (chains, steps)
    mll: np.ndarray  # (chains, steps, m) running MLL after every tree proposal
    mll_after: np.ndarray  # (chains, steps) MLL after the noise / scale proposal
    capacity: int
    lcap: int


def g11_replay(dtype=np.float64) -> G11:
    """The reference sampler's recorded steps (tests/golden/g11_sampler_steps: 2 chains x 3 steps of 8 tree proposals and one
    noise / scale proposal, N = 48) replayed through RefChain with the recorded proposals and uniform draws."""
    from conftest import load_golden
    from oracle import oracle as orc

    g = load_golden("g11_sampler_steps")
    X, y, ft = g["X"], g["y"].reshape(-1), g["feat_types"]
    chains, steps, m = g["accept"].shape
    forests = orc.nodes_from_raw(g["start_forest"])
    old, new = orc.nodes_from_raw(g["old"]), orc.nodes_from_raw(g["new"])
    leaves = max(len(leaf_order(tr)) for tr in np.concatenate([forests.reshape(-1, 100), new.reshape(-1, 100)]))
    lcap, capacity = max(leaves, 1), 32 * ((m * leaves + 31) // 32)
    acc, ns_acc = np.zeros((chains, steps, m), dtype=bool), np.zeros((chains, steps), dtype=bool)
    mll, mll_after = np.zeros((chains, steps, m)), np.zeros((chains, steps))
    tree_margin = ns_margin = np.inf
    for b in range(chains):
        ch = RefChain(forests[b], g["start_noise"][b], g["start_scale"][b], X, y, ft, capacity, dtype)
        for s in range(steps):
            for t in range(m):
                delta, commit = ch.propose(t, new[b, s, t])
                lu = np.log(g["u"][b, s, t])
                tree_margin = min(tree_margin, abs(lu - (g["log_q"][b, s, t] + delta)))
                acc[b, s, t] = decide(delta, g["log_q"][b, s, t], lu) == 1
                if acc[b, s, t]:
                    commit()
                mll[b, s, t] = ch.mll
            delta, commit = ch.propose_noise_scale(g["ns_prop"][b, s, 0], g["ns_prop"][b, s, 1])
            lu = np.log(g["ns_u"][b, s])
            ns_margin = min(ns_margin, abs(lu - (g["ns_log_q"][b, s] + delta)))
            ns_acc[b, s] = decide(delta, g["ns_log_q"][b, s], lu) == 1
            if ns_acc[b, s]:
                commit()
            mll_after[b, s] = ch.mll
    return G11(float(tree_margin), float(ns_margin), acc, ns_acc, mll, mll_after, capacity, lcap)
