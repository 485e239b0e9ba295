"""Host restatement of the device's tree proposals (csrc/propose.hip, bark_amd.fitting.tree_proposals) in plain numpy, and the
case tables of tests/test_gpu_proposals.py (CASES) and tests/test_gpu_proposals_edges.py (EDGE_CASES, with the builders
that put trees into every ballot word of the kernel).  No GPU, no library.  Two halves that share nothing:

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


# -------------------------------------------------------------------------------- edge cases ----
# Trees in every ballot word of the kernel (slots 0..63, 64..127, 128..191, 192..255) and at the edges of the container: built
# here, held to the conditions that make them meaningful by tests/test_proposals_cpu.py, run on the device by
# tests/test_gpu_proposals_edges.py.  CASES and evolved_forests above are unchanged: other tests depend on their bits.
EDGE_SEED = 0x5EED0123456789
ROOT_PARENT = 0xFFFFFFFF


def random_tree(L, n_leaves, rng, bounds, ft):
    """A root grown by `decide` + `apply`, the kind forced to grow, to n_leaves terminal nodes: slots 0 .. 2 n_leaves - 2 of L."""
    assert 1 <= n_leaves and 2 * n_leaves - 1 <= L
    tree, grow = root_tree(L), Params(proposal_weights=(1.0, 0.0, 0.0), max_leaves=L)
    while len(terminal(tree)) < n_leaves:
        d = decide(rng.random(N_DRAWS).tolist(), tree, bounds, ft, grow)
        if d.status == 0:  # an exhausted discrete feature: draw again
            tree = apply(tree, d.kind, d.node, d.feature, d.threshold, grow).new_tree
    return tree


def move(tree, dest, L):
    """The records of `tree` at slots dest[i] of a new container of L slots (dest[i] < 0: dropped; slots nothing moves to are
    zero).  left, right and parent of the active records follow their targets; one that names a dropped record becomes 0, one
    outside the old container (the root's parent) stays."""
    dest = np.asarray(dest, dtype=np.int64)
    kept = np.flatnonzero(dest >= 0)
    assert len(set(dest[kept].tolist())) == len(kept) and (dest < L).all()
    new = np.zeros(L, dtype=NODE)
    new[dest[kept]] = tree[kept]
    live = dest[kept][tree["active"][kept] != 0]
    for field in ("left", "right", "parent"):
        old = new[field][live].astype(np.int64)
        inside = old < len(tree)
        new[field][live] = np.where(inside, np.maximum(dest[np.where(inside, old, 0)], 0), old).astype(np.uint32)
    return new


def relabel(tree, perm):
    """Slot i moves to perm[i] (a permutation with perm[0] == 0: the kernel's ancestor walk ends at slot 0).  left, right and
    parent of the active records are rewritten; inactive records move unchanged."""
    perm = np.asarray(perm, dtype=np.int64)
    assert perm[0] == 0 and sorted(perm.tolist()) == list(range(len(tree)))
    return move(tree, perm, len(tree))


def place(tree, L, idle, rng=None):
    """A relabel into a container of L slots whose inactive slots are exactly `idle`: the root stays at slot 0, the other active
    nodes fill the remaining slots in ascending order (in random order with `rng`).  Inactive records of `tree` go to the idle
    slots, in order, as far as both last."""
    idle = sorted(int(i) for i in set(np.asarray(idle, dtype=np.int64).tolist()))
    act = np.flatnonzero(tree["active"])
    assert (L - len(idle)) % 2 == 1 and len(act) == L - len(idle) and act[0] == 0 and 0 not in idle and (not idle or idle[-1] < L)
    free = np.array(sorted(set(range(L)) - set(idle)), dtype=np.int64)
    if rng is not None:
        free[1:] = rng.permutation(free[1:])
    dest = np.full(len(tree), -1, dtype=np.int64)
    dest[act] = free
    rest = np.flatnonzero(tree["active"] == 0)[:len(idle)]
    dest[rest] = idle[:len(rest)]
    return move(tree, dest, L)


def caterpillar(L, depth, features, thresholds, side, single_slot=None):
    """A chain of `depth` decision nodes: level j splits features[j] at thresholds[j] and goes on in its left (side[j] = 0) or
    right (1) child; the other child is a leaf.  Scalars serve every level.  Level j's children sit at slots 2 j + 1 and 2 j + 2.
    The deepest decision node is the only singly internal one; single_slot moves it (depth >= 2) to that slot."""
    assert depth >= 1 and 2 * depth + 1 <= L
    f, s = np.broadcast_to(features, (depth,)), np.broadcast_to(side, (depth,))
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (depth,))
    t = np.zeros(L, dtype=NODE)
    cur, parent = 0, ROOT_PARENT
    for j in range(depth):
        left, right = 2 * j + 1, 2 * j + 2
        t[cur] = (0, f[j], thr[j], left, right, parent, j, 1)
        t[left] = t[right] = (1, 0, 0, 0, 0, cur, j + 1, 1)
        parent, cur = cur, (right if s[j] else left)
    if single_slot is not None and single_slot != parent:
        assert parent != 0 and 0 < single_slot < L
        perm = np.arange(L)
        perm[parent], perm[single_slot] = single_slot, parent
        t = relabel(t, perm)
    return t


def stale_fill(tree, rng):
    """Random bits in every field of the inactive slots — what a long chain leaves behind, and the copy must keep bit for bit.
    active stays 0, is_leaf is 0 or 1, left / right / parent lie in 0..L."""
    out, L = tree.copy(), len(tree)
    idle = np.flatnonzero(out["active"] == 0)
    n = len(idle)
    out["is_leaf"][idle] = rng.integers(0, 2, n, dtype=np.uint8)
    out["feature_idx"][idle] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    out["threshold"][idle] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for field in ("left", "right", "parent"):
        out[field][idle] = rng.integers(0, L + 1, n, dtype=np.uint32)
    out["depth"][idle] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return out


def valid_tree(tree):
    """One tree: the root at slot 0, every other active node the left or the right child of its active parent and one level
    below it, children that name their parent, leaves = decisions + 1."""
    L = len(tree)
    act = tree["active"] != 0
    leaf = tree["is_leaf"]
    if L < 1 or not act[0] or tree["depth"][0] != 0 or (tree["active"] > 1).any() or (leaf[act] > 1).any():
        return False
    left, right, parent = (tree[k].astype(np.int64) for k in ("left", "right", "parent"))
    for i in np.flatnonzero(act)[1:]:
        p = parent[i]
        if p >= L or not act[p] or leaf[p] or (left[p] == i) == (right[p] == i) or tree["depth"][i] != tree["depth"][p] + 1:
            return False
    for i in np.flatnonzero(act & (leaf == 0)):
        for ch in (left[i], right[i]):
            if ch >= L or ch == 0 or not act[ch] or parent[ch] != i:
                return False
    return int((act & (leaf == 1)).sum()) == int((act & (leaf == 0)).sum()) + 1


def split_root(L, feature, threshold, left=1, right=2):
    t = root_tree(L)
    t[0] = (0, feature, threshold, left, right, ROOT_PARENT, 0, 1)
    t[left] = t[right] = (1, 0, 0, 0, 0, 0, 1, 1)
    return t


_BUILT = {}


def _once(key, make):
    """Forests shared by several cases are built once (read-only: the tests copy what they hand to the device)."""
    if key not in _BUILT:
        _BUILT[key] = make()
        _BUILT[key].setflags(write=False)
    return _BUILT[key]


def _stack(rows, rng):
    return np.stack([np.stack([stale_fill(t, rng) for t in row]) for row in rows])


def _spread_forests(nc, m, L, seed):
    """m random trees that leave 2 (L odd) or 3 (L even) slots of L inactive; every chain holds them under a random permutation
    of its own, with inactive slots of its own."""
    def make():
        rng = np.random.default_rng([seed, L])
        n_idle = 2 if L % 2 else 3
        base = [random_tree(L, (L - n_idle + 1) // 2, rng, MIXED_BOUNDS, MIXED_FT) for _ in range(m)]
        return _stack([[place(b, L, rng.choice(np.arange(1, L), size=n_idle, replace=False), rng) for b in base] for _ in range(nc)], rng)
    return _once(("spread", nc, m, L, seed), make)


def _full_trees(L, n_leaves, idles, seed, nc, orphans=None):
    """One random tree of n_leaves per entry of `idles`, placed so that exactly that set is inactive; every chain holds the same
    trees (it draws its own stream).  orphans: per tree, an inactive slot turned into an active leaf that no node names."""
    rng = np.random.default_rng([seed, L])
    row = []
    for k, idle in enumerate(idles):
        spare = [] if orphans is None else [orphans[k]]
        t = place(random_tree(L, n_leaves, rng, MIXED_BOUNDS, MIXED_FT), L, list(idle) + spare, rng)
        t = stale_fill(t, rng)
        for s in spare:
            t[s] = (1, 0, 0, 0, 0, 0, 1, 1)
        row.append(t)
    return np.stack([np.stack(row)] * nc)


# the two lowest inactive slots, and a third where the container's parity needs one.  A tree has 2 n - 1 nodes, so no tree
# leaves exactly slots (254, 255) or (5, 255) of 256 inactive: those two pairs stand in IDLE_PAIRS_ODD, on containers that hold
# one active leaf outside the tree (ORPHANS; not valid_tree — the kernel scans slots, not trees), and as the last two slots
# of 255 here.
IDLE_PAIRS = {255: [(63, 64), (191, 192), (253, 254), (5, 254)], 256: [(127, 128, 255), (64, 65, 130), (63, 64, 192)]}
IDLE_PAIRS_ODD = [(254, 255), (5, 255)]
ORPHANS = [131, 100]

# ladders: caterpillars of 12 levels on one feature (index 2 integer, 3 categorical, 0 continuous in MIXED_FT)
_R, _L = 1, 0
_ZIG = [_R, _L] * 6
LADDERS_STOP = {   # the deepest leaves cannot be split on the ladder's feature: status 2
    "int_right": dict(thresholds=[0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], side=_R),          # [10, 10]: lo == hi
    "int_left": dict(thresholds=[9, 9, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], side=_L),           # [0, 0]
    # {0..4} -R{0}-> {1..4} -L{2,3,4}-> {2,3,4} -R{2}-> {3,4} -L{3,4}-> ... -R{3}-> {4} -L{4}-> {4} | {}
    "cat": dict(thresholds=[1, 28, 4, 24, 4, 24, 4, 24, 4, 24, 8, 16], side=_ZIG),
}
LADDERS_OPEN = {   # both bounds tightened again and again, and still a split to draw
    "int_zigzag": dict(thresholds=[0, 9, 1, 8, 2, 7, 2, 7, 2, 7, 3, 6], side=_ZIG),       # [4, 6]
    # {0..4} -R{0,1}-> {2,3,4} -L{1,2,3,4}-> {2,3,4} -R{0}-> ... -L{0,2,3,4}-> {2,3,4}: leaves {0,1} (left), {2} | {3,4}
    "cat": dict(thresholds=[3, 30, 1, 30, 1, 29, 1, 29, 1, 29, 1, 4], side=_ZIG[:11] + [_R]),
    "cat_left": dict(thresholds=[28, 3, 28, 3, 28, 3, 28, 3, 28, 3, 28, 8], side=[_L, _R] * 5 + [_L, _L]),
    "cont": dict(thresholds=[0.1, 0.9, 0.15, 0.85, 0.2, 0.8, 0.25, 0.75, 0.3, 0.7, 0.35, 0.65], side=_ZIG),
}
LADDER_L = 70
_LADDER_FEATURE = {"int": 2, "cat": 3, "cont": 0}


def _ladder_forests(table, kinds, nc, one_feature, seed):
    rng = np.random.default_rng(seed)
    names = [n for n in sorted(table) if n.split("_")[0] in kinds]
    row = [caterpillar(LADDER_L, 12, 0 if one_feature else _LADDER_FEATURE[n.split("_")[0]], table[n]["thresholds"], table[n]["side"],
                       single_slot=(LADDER_L - 1, 64, None)[k % 3]) for k, n in enumerate(names)]
    return _stack([row] * nc, rng)


def _deep_forests(nc, m):
    """Caterpillars of 60 levels on the two continuous features, the interval halved from alternating sides."""
    rng = np.random.default_rng(60)
    thr = [0.5 + (0.4 if j % 2 else -0.4) * 0.93 ** j for j in range(60)]
    rows = [[caterpillar(256, 60, [j % 2 for j in range(60)] if (c + t) % 2 else 0, thr, [(j + 1) % 2 for j in range(60)],
                         single_slot=(255, 128, 191, None, 64)[(c * m + t) % 5]) for t in range(m)] for c in range(nc)]
    return _stack(rows, rng)


def _last_slot_forests(L, nc, m, single):
    rng = np.random.default_rng([7, L, single])
    if single:  # the only singly internal node at slot L - 1
        rows = [[caterpillar(L, 3 + (c + t) % 4, [0, 2, 3, 1, 0, 2][:3 + (c + t) % 4], [0.5, 4, 6, 0.25, 0.75, 7][:3 + (c + t) % 4],
                             [(c + t + j) % 2 for j in range(3 + (c + t) % 4)], single_slot=L - 1) for t in range(m)] for c in range(nc)]
    else:       # a split root with its two leaves at L - 2 and L - 1
        rows = [[split_root(L, (c + t) % 4, (0.5, 0.25, 4.0, 6.0)[(c + t) % 4], L - 2, L - 1) for t in range(m)] for c in range(nc)]
    return _stack(rows, rng)


def _tiny_forests(L, nc, m):
    rng = np.random.default_rng(L)
    return _stack([[split_root(3, 2, 4.0) if L == 3 and (c + t) % 3 == 2 else root_tree(L) for t in range(m)] for c in range(nc)], rng)


GUARDED_L = 70


def _guarded_forests(nc=3, m=5):
    """The records the kernel documents as "not a valid node" (a child or a parent outside the container, a parent cycle), with no
    index above L, on trees that are not the last of the buffer: even a kernel without the guards would read inside it."""
    L = GUARDED_L
    rng = np.random.default_rng(99)
    rows = []
    for c in range(nc):
        base = [place(random_tree(L, 6, rng, MIXED_BOUNDS, MIXED_FT), L, rng.choice(np.arange(1, L), size=L - 11, replace=False), rng)
                for _ in range(m)]
        for k, field in ((0, "left"), (1, "right")):  # a singly internal node loses a child to slot L
            base[k][field][singly_internal(base[k])[-1]] = L
        inner = [i for i in np.flatnonzero(base[2]["active"] & (base[2]["is_leaf"] == 0)).tolist() if i != 0]
        base[2]["parent"][inner[0]] = L               # a decision node below the root: the walk stops there
        inner = [i for i in np.flatnonzero(base[3]["active"] & (base[3]["is_leaf"] == 0)).tolist() if i != 0]
        base[3]["parent"][inner[0]] = base[3]["left"][inner[0]]  # it and its left child name each other: the walk ends after L hops
        rows.append(base)                             # tree 4, the last of every chain and of the buffer, stays a plain tree
    return _stack(rows, rng)


_W = (0.4, 0.3, 0.3)


def _edge(nc, m, L, forests, max_leaves=None, weights=_W, bounds=MIXED_BOUNDS, ft=MIXED_FT):
    return Case(nc, m, L, bounds, ft, Params(proposal_weights=weights, max_leaves=L if max_leaves is None else max_leaves), forests)


_ONE = {"int": (np.array([[0.0, 10.0]]), np.array([INT], dtype=np.int64)), "cat": (np.array([[0.0, 31.0]]), np.array([CAT], dtype=np.int64)),
        "cont": (np.array([[0.0, 1.0]]), np.array([CONT], dtype=np.int64))}

EDGE_CASES = {
    "spread256": _edge(8, 16, 256, lambda: _spread_forests(8, 16, 256, 1)),
    "idle_pairs_255": _edge(5, 4, 255, lambda: _full_trees(255, 127, IDLE_PAIRS[255], 2, 5), weights=(0.8, 0.1, 0.1)),
    "idle_pairs_256": _edge(5, 3, 256, lambda: _full_trees(256, 127, IDLE_PAIRS[256], 2, 5), weights=(0.8, 0.1, 0.1)),
    "idle_pairs_odd": _edge(5, 2, 256, lambda: _full_trees(256, 127, IDLE_PAIRS_ODD, 3, 5, orphans=ORPHANS), weights=(0.8, 0.1, 0.1)),
    "idle_short_one": _edge(5, 3, 256, lambda: _full_trees(256, 128, [(200,)] * 3, 4, 5)),
    "idle_short_none": _edge(5, 3, 255, lambda: _full_trees(255, 128, [()] * 3, 4, 5)),
    "ladders_stop": _edge(3, 3, LADDER_L, lambda: _ladder_forests(LADDERS_STOP, ("int", "cat"), 3, False, 21)),
    "ladders_open": _edge(5, 4, LADDER_L, lambda: _ladder_forests(LADDERS_OPEN, ("int", "cat", "cont"), 5, False, 22)),
    "deep_prior": _edge(3, 7, 256, lambda: _deep_forests(3, 7)),
    "max_leaves_127": _edge(8, 16, 256, lambda: _spread_forests(8, 16, 256, 1), max_leaves=127),
    "max_leaves_128": _edge(8, 16, 256, lambda: _spread_forests(8, 16, 256, 1), max_leaves=128),
    "guarded": _edge(3, 5, GUARDED_L, _guarded_forests),
}
for _Lc in (63, 64, 65, 128, 129, 192, 193, 255):
    EDGE_CASES["spread_%d" % _Lc] = _edge(3, 5, _Lc, lambda L=_Lc: _spread_forests(3, 5, L, 1))
for _Lc in (65, 129, 193, 256):
    EDGE_CASES["last_single_%d" % _Lc] = _edge(3, 5, _Lc, lambda L=_Lc: _last_slot_forests(L, 3, 5, True))
    EDGE_CASES["last_leaf_%d" % _Lc] = _edge(3, 5, _Lc, lambda L=_Lc: _last_slot_forests(L, 3, 5, False))
for _Lc in (1, 2, 3):
    EDGE_CASES["tiny_%d" % _Lc] = _edge(3, 5, _Lc, lambda L=_Lc: _tiny_forests(L, 3, 5))
for _k in ("int", "cat"):  # d = 1: the drawn feature is the ladder's
    EDGE_CASES["ladders_stop_" + _k] = _edge(5, len([n for n in LADDERS_STOP if n.startswith(_k)]), LADDER_L, bounds=_ONE[_k][0], ft=_ONE[_k][1],
                                             forests=lambda k=_k: _ladder_forests(LADDERS_STOP, (k,), 5, True, 23))
for _k in ("int", "cat", "cont"):
    EDGE_CASES["ladders_open_" + _k] = _edge(5, len([n for n in LADDERS_OPEN if n.startswith(_k)]), LADDER_L, bounds=_ONE[_k][0], ft=_ONE[_k][1],
                                             forests=lambda k=_k: _ladder_forests(LADDERS_OPEN, (k,), 5, True, 24))

# the sweep of each case's stream (EDGE_SEED, sweep, chain, tree): 17 unless the conditions of tests/test_proposals_cpu.py — a
# chosen node in every word, a grow on every pair — need another draw
EDGE_SWEEPS = {"spread_65": 21, "spread_129": 29, "spread_193": 34, "spread_255": 18}


def edge_sweep(name):
    return EDGE_SWEEPS.get(name, 17)


_EDGE_REF = {}


def edge_ref(name):
    """(forests, host proposals at (EDGE_SEED, edge_sweep(name))) of an edge case, computed once, shared and read-only."""
    if name not in _EDGE_REF:
        c = EDGE_CASES[name]
        forests = np.array(c.forests())
        assert forests.shape == (c.nc, c.m, c.L) and c.nc * c.m <= 128
        out = propose_forests(forests, c.bounds, c.ft, c.params, EDGE_SEED, edge_sweep(name))
        for a in (forests,) + out:
            a.setflags(write=False)
        _EDGE_REF[name] = (forests, out)
    return _EDGE_REF[name]


def walk_end(tree, node):
    """How the ancestor walk from `node` ends: "root", "outside" (a parent beyond the container) or "cycle" (L hops)."""
    cur = node
    for _ in range(len(tree)):
        if cur == 0:
            return "root"
        cur = int(tree["parent"][cur])
        if cur >= len(tree):
            return "outside"
    return "root" if cur == 0 else "cycle"
