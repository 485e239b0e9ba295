"""Host reference of the acquisition scan conditioned on pending points (numpy and the oracle only, no GPU) and the case
table shared by tests/test_acquisition_pending_cpu.py and tests/test_gpu_acquisition_pending.py.

Written from the formulas of include/bark_hip.h, not from the kernel.  Per forest, with M = I + c Z'Z, w = M^-1 Z'y,
c = scale / (m s2), s2 = 1e-6 + noise, and z the one-hot row of a pending point:
    t = M^-1 z,   q = z't,   M^-1 <- M^-1 - (c / (1 + c q)) t t',   w unchanged
    mu_b(x) = c z_x'w,   var_b(x) = (scale / m) z_x' M^-1 z_x
(a) `leafspace`: that downdate in float64 or np.longdouble (M^-1 by a Gauss-Jordan elimination written here: numpy's
    LAPACK routes do not take longdouble);
(b) `dense`: the oracle's `forest_predict`, as tests/acq_ref.py uses it: mu_b from the original data, var_b from
    scale - k K_s^-1 k' on the training inputs augmented by the pending points (the variance depends on no y);
(c) `greedy`: the loop of `propose_batch_from_candidates` over (b).
The columns of Z are the leaves reached by any of the points involved (training, pending, candidates), tree by tree; a
leaf nobody reaches is an identity row of M and changes nothing."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import acq_ref as ar
from oracle import oracle as orc

KINDS = ar.KINDS
RTOL, ATOL = ar.RTOL, ar.ATOL  # the posterior bar of DESIGN.md section 2
AGREE = 0.01  # (a) in longdouble and (b) agree within this fraction of the bar
MARGIN = 1e-6  # relative gap between the winner and the best value that differs from it
MAX_PENDING = 64


@dataclass(frozen=True)
class PCase:
    """base: the acq_ref.Case of forests, data and candidates; pending: how the pending points are made (`pending_of`);
    q: greedy picks (0: a conditioning case)"""

    name: str
    base: ar.Case
    pending: tuple
    q: int = 0


_N20 = ar.Case("pend_m1_n20", ("full", 1, 3), N=20, B=3, C=300, seed=11)  # R = 8
_N64 = ar.Case("pend_m13_n64", ("leaves", 13, 100), N=64, B=3, C=300, seed=12)
_N257 = ar.Case("pend_prior_n257", ("prior", 50), N=257, B=3, C=300, seed=13)  # R no multiple of 64 (checked on the host)
SLAB_BASE = ar.Case("pend_slab_c70000", ("prior", 2), N=20, B=3, C=70_000, chunk=2, seed=14)

CASES = {c.name: c for c in [
    # conditioning against the dense reference
    PCase("n20_m1_p1", _N20, ("random", 1)),
    PCase("n64_m13_p2", _N64, ("random", 2)),
    PCase("n257_prior_p5", _N257, ("random", 5)),
    # awkward pending sets
    PCase("same_point_twice", _N64, ("twice",)),
    PCase("candidate_and_training_point", _N64, ("cand_and_train", 7, 3)),
    PCase("unreached_leaves", _N64, ("unreached",)),
    PCase("p64", _N64, ("random", 64)),
    # the two orders of one pair
    PCase("pair_ab", _N64, ("pair", 0, 1)),
    PCase("pair_ba", _N64, ("pair", 1, 0)),
    # greedy batches
    PCase("greedy_q4_n64", _N64, ("random", 2), q=4),
    PCase("greedy_q8_n257", _N257, ("random", 1), q=8),
]}
CONDITIONING = ["n20_m1_p1", "n64_m13_p2", "n257_prior_p5"]
AWKWARD = ["same_point_twice", "candidate_and_training_point", "unreached_leaves", "p64"]
GREEDY = ["greedy_q4_n64", "greedy_q8_n257"]
SLAB = PCase("slab_c70000_p2", SLAB_BASE, ("random", 2))
SLAB_STRIDE = 997


def leaves_of(F, X, ft):
    """(B, n, m) leaf node index of every point under every tree"""
    return np.stack([orc.pass_through_forest(F[b], X, ft) for b in range(F.shape[0])]).astype(np.int64)


def unreached_count(inp, pts):
    """(n,) over the points: how many (forest, tree) pairs put the point into a leaf no training point reaches"""
    lx = leaves_of(inp.F, inp.X, inp.ft)
    lp = leaves_of(inp.F, pts, inp.ft)
    return (lp[:, :, None, :] != lx[:, None, :, :]).all(axis=2).sum(axis=(0, 2))


@lru_cache(maxsize=None)
def pending_of(name) -> np.ndarray:
    case = CASES[name] if isinstance(name, str) else name
    inp = ar.make_inputs(case.base)
    how = case.pending
    pool = ar.problem(max(MAX_PENDING, 2), 300 + case.base.seed)[0]
    if how[0] == "random":
        out = pool[:how[1]]
    elif how[0] == "twice":
        out = np.stack([pool[0], pool[0]])
    elif how[0] == "cand_and_train":
        out = np.stack([inp.cand[how[1]], inp.X[how[2]]])
    elif how[0] == "pair":
        out = np.stack([pool[how[1]], pool[how[2]]])
    else:  # the point of a larger pool that lands in the most leaves without a training point, and an ordinary one
        wide = ar.problem(500, 400 + case.base.seed)[0]
        out = np.stack([wide[int(np.argmax(unreached_count(inp, wide)))], pool[0]])
    out = np.ascontiguousarray(out, dtype=np.float64)
    out.setflags(write=False)
    return out


def gauss_jordan_inverse(M):
    """inverse of a symmetric positive definite matrix in M's own dtype (no pivoting needed)"""
    n = M.shape[0]
    A = np.concatenate([M.copy(), np.eye(n, dtype=M.dtype)], axis=1)
    for k in range(n):
        A[k] = A[k] / A[k, k]
        f = A[:, k].copy()
        f[k] = 0
        A -= f[:, None] * A[k][None, :]
    return A[:, n:]


def one_hot(leaves_by_set, b):
    """Z of each point set under forest b: [(n_i, R)], the columns the leaves any of the points reaches, tree by tree"""
    allp = np.concatenate([l[b] for l in leaves_by_set], axis=0)
    cols, off = [], 0
    for t in range(allp.shape[1]):
        ids = np.unique(allp[:, t])
        cols.append((ids, off))
        off += ids.size
    out = []
    for l in leaves_by_set:
        Z = np.zeros((l.shape[1], off))
        for t, (ids, o) in enumerate(cols):
            Z[np.arange(l.shape[1]), o + np.searchsorted(ids, l[b][:, t])] = 1.0
        out.append(Z)
    return out


def leafspace(inp, pending, cand=None, dtype=np.float64):
    """(a) -> mu, var (B, C) and, for the identity test, per forest (w, w recomputed from the augmented system)"""
    cand = inp.cand if cand is None else cand
    P = 0 if pending is None else len(pending)
    sets = [inp.X, cand] + ([pending] if P else [])
    lv = [leaves_of(inp.F, s, inp.ft) for s in sets]
    B, m = inp.F.shape[:2]
    mu, var, ws = [], [], []
    for b in range(B):
        Zs = [z.astype(dtype) for z in one_hot(lv, b)]
        Z, Zc = Zs[0], Zs[1]
        y = inp.y.reshape(-1).astype(dtype)
        s2 = dtype(1e-6) + dtype(inp.noise[b])
        c = dtype(inp.scale[b]) / (dtype(m) * s2)
        R = Z.shape[1]
        Minv = gauss_jordan_inverse(np.eye(R, dtype=dtype) + c * (Z.T @ Z))
        w = Minv @ (Z.T @ y)
        Za, ya = Z, y
        for p in range(P):
            z = Zs[2][p]
            t = Minv @ z
            q = z @ t
            Minv = Minv - (c / (1 + c * q)) * np.outer(t, t)
            Za = np.concatenate([Za, z[None]], axis=0)
            ya = np.concatenate([ya, [c * (z @ w)]])  # the believer's observation: the posterior mean at the point
        w_aug = gauss_jordan_inverse(np.eye(R, dtype=dtype) + c * (Za.T @ Za)) @ (Za.T @ ya) if P else w
        mu.append(c * (Zc @ w))
        var.append(dtype(inp.scale[b]) / dtype(m) * np.einsum("ci,ij,cj->c", Zc, Minv, Zc))
        ws.append((w, w_aug))
    return np.stack(mu), np.stack(var), ws


def dense(inp, pending, cand=None):
    """(b) -> mu, var (B, C) float64"""
    cand = inp.cand if cand is None else cand
    mu, var = [], []
    for i in range(0, len(cand), ar.POSTERIOR_BLOCK):
        blk = cand[i:i + ar.POSTERIOR_BLOCK]
        m0, v0 = orc.forest_predict(inp.model, inp.data, blk, inp.ft)
        if pending is not None and len(pending):
            Xa = np.concatenate([inp.X, pending], axis=0)
            _, v0 = orc.forest_predict(inp.model, (Xa, np.zeros((len(Xa), 1))), blk, inp.ft)
        mu.append(m0)
        var.append(v0)
    return np.concatenate(mu, axis=1), np.concatenate(var, axis=1)


def gap_of(v, skip=()):
    """(arg-min with ties to the lowest index, relative gap to the best value that differs from the winner's)"""
    v = np.asarray(v).copy()
    v[list(skip)] = np.inf
    i = int(np.argmin(v))
    rest = v[v != v[i]]
    gap = float((rest.min() - v[i]) / max(1.0, abs(float(v[i])))) if rest.size else np.inf
    return i, gap


@lru_cache(maxsize=None)
def conditioned(name):
    """-> {kind: (values float64 (C,), arg-min)} of (b) for a conditioning case"""
    case = CASES[name] if isinstance(name, str) else name
    inp = ar.make_inputs(case.base)
    mu, var = dense(inp, pending_of(name))
    out = {}
    for kind in KINDS:
        v = ar.acquisition(mu, var, case.base.kappa, kind)
        v.setflags(write=False)
        out[kind] = (v, gap_of(v)[0])
    return out


@lru_cache(maxsize=None)
def greedy(name, kind):
    """(c) -> (indices (q,), the acquisition vector of every pick [(C,)], the pending set of every pick)"""
    case = CASES[name]
    inp = ar.make_inputs(case.base)
    pend = pending_of(name)
    picks, vecs, pends = [], [], []
    for _ in range(case.q):
        cur = np.concatenate([pend, inp.cand[picks]], axis=0) if picks else pend
        mu, var = dense(inp, cur)
        v = ar.acquisition(mu, var, case.base.kappa, kind)
        pends.append(cur)
        vecs.append(v)
        picks.append(gap_of(v, picks)[0])
    return np.asarray(picks), vecs, pends
