"""Host restatement of the device's tree proposals (csrc/propose.hip, bark_amd.fitting.tree_proposals) in plain numpy, and the
case table of tests/test_gpu_proposals.py.  No GPU, no library.  Two halves that share nothing:

    decide(draws, tree, bounds, ft, params) -> Decision(kind, node, feature, threshold, status)     what is drawn
    apply(tree, kind, node, feature, threshold, params) -> Applied(new_tree, log_q, log_prior, sum_abs, status)   what it does

tests/test_proposals_cpu.py holds `apply` and `subspace` to the reference's own functions (tests/golden/g12_tree_proposals).

Draw layout (include/bark_hip.h): Philox4x32-10, key = (seed low, seed high), counter = (chain, tree, sweep, block); words
(0, 1) and (2, 3) of a block are one 64-bit draw each, low word first; u = (x >> 11) * 2^-53; draws 0..4 = kind, node, feature,
threshold or mask, accept.  Status: 0 valid, 1 no valid node, 2 invalid discrete split, 3 no two inactive slots, 4 max_leaves."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

NODE = np.dtype([("is_leaf", np.uint8), ("feature_idx", np.uint32), ("threshold", np.float32), ("left", np.uint32),
                 ("right", np.uint32), ("parent", np.uint32), ("depth", np.uint32), ("active", np.uint8)])
CAT, INT, CONT = 0, 1, 2
GROW, PRUNE, CHANGE = 0, 1, 2
N_DRAWS = 5


class Params(NamedTuple):
    alpha: float = 0.95
    beta: float = 2.0
    proposal_weights: tuple = (0.25, 0.25, 0.5)
    max_leaves: int = 100


class Decision(NamedTuple):
    kind: int
    node: int
    feature: int
    threshold: float  # as stored: a float32 value
    status: int


class Applied(NamedTuple):
    new_tree: np.ndarray
    log_q: float
    log_prior: float
    sum_abs: float  # sum of the absolute values of the log / pow terms behind log_q + log_prior
    status: int


# ------------------------------------------------------------------------------------ Philox ----
def philox4x32(key, counter):
    """One block: key (k0, k1), counter (c0, c1, c2, c3), Python integers -> four 32-bit words."""
    k0, k1 = key
    c0, c1, c2, c3 = counter
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draws_of(seed, sweep, chain, tree, n=N_DRAWS):
    """The first n uniforms of the stream (seed, sweep, chain, tree)."""
    out = []
    for block in range((n + 1) // 2):
        w = philox4x32((seed & 0xFFFFFFFF, seed >> 32), (chain, tree, sweep, block))
        for lo, hi in ((w[0], w[1]), (w[2], w[3])):
            out.append(float(((hi << 32 | lo) >> 11)) * 2.0 ** -53)
    return out[:n]


# ------------------------------------------------------------------------------------- trees ----
def terminal(tree):
    return np.flatnonzero(tree["active"] & tree["is_leaf"]).tolist()


def singly_internal(tree):
    """Active decision nodes whose two children are leaves; a child outside the container disqualifies the node."""
    L, leaf = len(tree), tree["is_leaf"]
    l, r = tree["left"].astype(np.int64), tree["right"].astype(np.int64)
    inside = (l < L) & (r < L)
    cond = tree["active"] & (np.uint8(1) - leaf) & leaf[np.where(inside, l, 0)] & leaf[np.where(inside, r, 0)]
    return np.flatnonzero(inside & (cond != 0)).tolist()


def subspace(tree, node, bounds, ft):
    """The part of the domain that reaches `node`, (d, 2) float64, categorical features as [0, mask]."""
    sub = np.array(bounds, dtype=np.float64)
    cur = node
    for _ in range(len(tree)):
        if cur == 0:
            break
        par = int(tree["parent"][cur])
        if par >= len(tree):
            break
        f, thr = int(tree["feature_idx"][par]), float(tree["threshold"][par])
        is_left = cur == int(tree["left"][par])
        if ft[f] == CAT:
            avail = int(sub[f, 1])
            if is_left:
                sub[f, 1] = int(thr) & avail
            else:
                full = 1
                while avail >= full:
                    full <<= 1
                sub[f, 1] = int(full - 1 - thr) & avail
        elif is_left:
            sub[f, 1] = sub[f, 1] if sub[f, 1] < thr else thr
        else:
            bound = thr + (1.0 if ft[f] == INT else 0.0)
            sub[f, 0] = sub[f, 0] if sub[f, 0] > bound else bound
        cur = par
    return sub


def _pick(u, n):
    return min(int(u * float(n)), n - 1)


def spread_mask(avail, draw):
    """The bits of `draw` over the set bits of `avail`, lowest first."""
    out, i = 0, 0
    while avail >> i:
        if avail >> i & 1:
            out |= (draw & 1) << i
            draw >>= 1
        i += 1
    return out


def decide(draws, tree, bounds, ft, params) -> Decision:
    u_kind, u_node, u_feat, u_thr = draws[:4]
    w = np.asarray(params.proposal_weights, dtype=np.float64)
    kind = min(int(np.searchsorted(np.cumsum(w / np.sum(w)), u_kind)), 2)
    valid = terminal(tree) if kind == GROW else singly_internal(tree)
    if not valid:
        return Decision(kind, -1, -1, 0.0, 1)
    node = valid[_pick(u_node, len(valid))]
    if kind == PRUNE:
        return Decision(kind, node, -1, 0.0, 0)
    f = _pick(u_feat, len(ft))
    lo, hi = (float(v) for v in subspace(tree, node, bounds, ft)[f])
    status = 0
    if ft[f] == CAT:
        avail = int(hi)
        k = bin(avail).count("1")
        thr = float(spread_mask(avail, 1 + _pick(u_thr, (1 << k) - 2))) if k >= 2 else 0.0
        status = 2 if thr == 0.0 else 0
    elif ft[f] == INT:
        if lo == hi or int(hi) <= int(lo):
            thr, status = hi, 2
        else:
            thr = float(int(lo) + _pick(u_thr, int(hi) - int(lo)))
    else:
        thr = lo + u_thr * (hi - lo)
    return Decision(kind, node, f, float(np.float32(thr)), status)


def apply(tree, kind, node, feature, threshold, params) -> Applied:
    new = tree.copy()
    depth = int(tree["depth"][node])
    a, b = float(params.alpha), float(params.beta)
    t1, t2, t3 = math.log(a), 2.0 * math.log(1.0 - a / (2.0 + depth) ** b), -math.log((1.0 + depth) ** b - a)
    prior = t1 + t2 + t3
    if kind == CHANGE:
        new["feature_idx"][node], new["threshold"][node] = feature, np.float32(threshold)
        return Applied(new, 0.0, 0.0, 0.0, 0)
    if kind == PRUNE:
        w1, w0 = len(singly_internal(tree)), len(terminal(tree)) - 1
        new["active"][int(tree["left"][node])] = 0
        new["active"][int(tree["right"][node])] = 0
        new["is_leaf"][node] = 1
        la, lb = math.log(w1), math.log(w0)
        return Applied(new, la - lb, -prior, abs(la) + abs(lb) + abs(t1) + abs(t2) + abs(t3), 0)
    idle = np.flatnonzero(tree["active"] == 0).tolist()
    if len(idle) < 2:
        return Applied(new, -math.inf, 0.0, 0.0, 3)
    w0 = len(terminal(tree))
    if w0 + 1 > params.max_leaves:
        return Applied(new, -math.inf, 0.0, 0.0, 4)
    left, right = idle[0], idle[1]
    for child in (left, right):
        new[child] = (1, 0, 0, 0, 0, node, depth + 1, 1)
    new[node] = (0, feature, np.float32(threshold), left, right, tree["parent"][node], depth, 1)
    la, lb = math.log(w0), math.log(len(singly_internal(new)))
    return Applied(new, la - lb, prior, abs(la) + abs(lb) + abs(t1) + abs(t2) + abs(t3), 0)


def propose(draws, tree, bounds, ft, params):
    """decide + apply + the accept draw -> (new_tree, log_q_prior, log_u, detail (4,), sum_abs of log_q_prior, |log_u|)."""
    d = decide(draws, tree, bounds, ft, params)
    log_u = math.log(draws[4]) if draws[4] > 0 else -math.inf
    if d.status:
        return tree.copy(), -math.inf, log_u, (d.kind, d.node, d.feature, d.status), 0.0
    a = apply(tree, d.kind, d.node, d.feature, d.threshold, params)
    if a.status:
        return tree.copy(), -math.inf, log_u, (d.kind, d.node, d.feature, a.status), 0.0
    return a.new_tree, a.log_q + a.log_prior, log_u, (d.kind, d.node, d.feature, 0), a.sum_abs


def propose_forests(forests, bounds, ft, params, seed, sweep, chain_offset=0, tree_offset=0):
    """`propose` for every tree of (chains, m, L) forests -> arrays shaped as the device's outputs, and sum_abs (chains, m)."""
    nc, m, _ = forests.shape
    new = forests.copy()
    lq, lu, sa = np.empty((nc, m)), np.empty((nc, m)), np.empty((nc, m))
    detail = np.empty((nc, m, 4), dtype=np.int32)
    for c in range(nc):
        for t in range(m):
            new[c, t], lq[c, t], lu[c, t], detail[c, t], sa[c, t] = propose(
                draws_of(seed, sweep, chain_offset + c, tree_offset + t), forests[c, t], bounds, ft, params)
    return new, lq, lu, detail, sa


# ------------------------------------------------------------------------------------- cases ----
MIXED_BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 10.0], [0.0, 31.0]])  # 2 continuous, 1 integer, 1 categorical (5 categories)
MIXED_FT = np.array([CONT, CONT, INT, CAT], dtype=np.int64)


def root_tree(L):
    t = np.zeros(L, dtype=NODE)
    t[0] = (1, 0, 0, 0, 0, 0xFFFFFFFF, 0, 1)
    return t


def full_tree(L, depth, ft, bounds, rng):
    """A complete binary tree of 2^(depth + 1) - 1 nodes in slot order (fills a container of that size)."""
    t = np.zeros(L, dtype=NODE)
    n = 2 ** (depth + 1) - 1
    assert n <= L
    for i in range(n):
        dep = int(math.log2(i + 1))
        parent = 0xFFFFFFFF if i == 0 else (i - 1) // 2
        if dep == depth:
            t[i] = (1, 0, 0, 0, 0, parent, dep, 1)
        else:
            f = int(rng.integers(0, len(ft)))
            thr = {CAT: 5.0, INT: float(rng.integers(2, 8)), CONT: float(rng.uniform(0.2, 0.8))}[int(ft[f])]
            t[i] = (0, f, thr, 2 * i + 1, 2 * i + 2, parent, dep, 1)
    return t


def evolved_forests(nc, m, L, bounds, ft, params, seed, sweeps=6):
    """Forests with history: root trees pushed through `sweeps` rounds of this module's proposals (grow-heavy weights), every valid one taken — so
    containers hold pruned records and reused slots (stale fields the copy must keep)."""
    forests = np.stack([np.stack([root_tree(L) for _ in range(m)]) for _ in range(nc)])
    growing = params._replace(proposal_weights=(0.6, 0.15, 0.25))  # mostly grows: trees of several levels within max_leaves
    for s in range(sweeps):
        forests = propose_forests(forests, bounds, ft, growing, seed, 1000 + s)[0]
    return forests


class Case(NamedTuple):
    nc: int
    m: int
    L: int
    bounds: np.ndarray
    ft: np.ndarray
    params: Params
    forests: object  # () -> (nc, m, L) records


def _overflow_forests():
    rng = np.random.default_rng(5)
    f = np.stack([np.stack([full_tree(7, 2, MIXED_FT, MIXED_BOUNDS, rng), root_tree(7), full_tree(7, 1, MIXED_FT, MIXED_BOUNDS, rng)])
                  for _ in range(2)])
    f[1, 1] = full_tree(7, 2, MIXED_FT, MIXED_BOUNDS, rng)
    return f


CASES = {
    "mixed": Case(3, 5, 100, MIXED_BOUNDS, MIXED_FT, Params(max_leaves=6),
                  lambda: evolved_forests(3, 5, 100, MIXED_BOUNDS, MIXED_FT, Params(max_leaves=6), seed=11, sweeps=12)),
    "one": Case(1, 1, 100, np.array([[0.0, 1.0]]), np.array([CONT], dtype=np.int64), Params(),
                lambda: evolved_forests(1, 1, 100, np.array([[0.0, 1.0]]), np.array([CONT], dtype=np.int64), Params(), seed=12, sweeps=9)),
    # 4 096 proposals, more than one round of the CUs: eight evolved chains, repeated (every chain still draws its own stream)
    "wide": Case(64, 64, 100, MIXED_BOUNDS, MIXED_FT, Params(max_leaves=32),
                 lambda: np.tile(evolved_forests(8, 64, 100, MIXED_BOUNDS, MIXED_FT, Params(max_leaves=32), seed=13, sweeps=5), (8, 1, 1))),
    "overflow": Case(2, 3, 7, MIXED_BOUNDS, MIXED_FT, Params(proposal_weights=(0.8, 0.1, 0.1), max_leaves=7), _overflow_forests),
}
