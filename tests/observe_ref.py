"""Host reference of conditioning a fitted leaf-space posterior on points with observed or fantasised values (numpy and the
oracle only, no GPU), shared by tests/test_posterior_observe_cpu.py and tests/test_gpu_posterior_observe.py.

Written from the formulas of include/bark_hip.h (bark_leaf_posterior_observe_hip), not from the kernel.  Per forest, with
M = I + c Z'Z, w = M^-1 Z'y, c = scale / (m s2), s2 = 1e-6 + noise, and z the one-hot row of a point, in the order given:
    t = M^-1 z,  q = z't,  s = z'w,  mu = c s,  v = (scale / m) q + s2
    y* = the given value, or mu + sqrt(v) eps
    w <- w + t (y* - mu) / (1 + c q),   M^-1 <- M^-1 - (c / (1 + c q)) t t',   logpred += -1/2 (log v + (y* - mu)^2 / v)
(a) `sequential`: that update in float64 or np.longdouble, on acq_pending_ref's one-hot columns and Gauss-Jordan inverse;
(b) `dense`: the oracle's `forest_predict` on (X u points, y u values): the reference's own arithmetic on the augmented data;
(c) `logpred_dense`: the log predictive from its definition, point by point through (b); `mll_difference`: the oracle's MLL;
(d) `greedy`: the loop of `propose_batch_from_candidates(fantasy=...)` over (a), `greedy_dense` the constant liar over (b).
Values are deterministic: the y of the generator that made the points (`values_of`), or a constant."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import acq_pending_ref as pr
import acq_ref as ar
from oracle import oracle as orc

RTOL, ATOL, AGREE, MARGIN = pr.RTOL, pr.ATOL, pr.AGREE, pr.MARGIN
LIAR = 0.25  # the constant of the constant-liar cases

# R > 1024: every thread-strided loop of the one-workgroup kernels takes a second trip
WIDE_BASE = ar.Case("obs_m13_r1100", ("leaves", 13, 1100), N=64, B=2, C=300, seed=15)
CHUNK_BASE = ar.Case("obs_prior_b5", ("prior", 8), N=48, B=5, C=300, chunk=2, seed=16)  # chunks of 2, 2 and 1 forests
EXTRA = {c.name: c for c in [pr.PCase("leaves1100_p3", WIDE_BASE, ("random", 3)), pr.PCase("b5_chunk2_p3", CHUNK_BASE, ("random", 3))]}
NAMES = ["n20_m1_p1", "n64_m13_p2", "n257_prior_p5", "same_point_twice", "unreached_leaves", "p64", "leaves1100_p3", "b5_chunk2_p3"]
GREEDY = ["greedy_q4_n64", "greedy_q8_n257"]


def case_of(name):
    return EXTRA[name] if name in EXTRA else pr.CASES[name]


def points_of(name) -> np.ndarray:
    return pr.pending_of(case_of(name))


@lru_cache(maxsize=None)
def values_of(name) -> np.ndarray:
    """(P,): the generator's y at the points of `points_of(name)`, made the way acq_pending_ref.pending_of makes the points"""
    case = case_of(name)
    how = case.pending
    pool = np.asarray(ar.problem(max(pr.MAX_PENDING, 2), 300 + case.base.seed)[1], dtype=np.float64).reshape(-1)
    if how[0] == "random":
        out = pool[:how[1]]
    elif how[0] == "twice":
        out = np.array([pool[0], pool[0] + 0.125])  # two noisy readings of one point
    else:  # "unreached": the widest point of the larger pool, then an ordinary one
        inp = ar.make_inputs(case.base)
        wide_x, wide_y = ar.problem(500, 400 + case.base.seed)[:2]
        out = np.array([np.asarray(wide_y).reshape(-1)[int(np.argmax(pr.unreached_count(inp, wide_x)))], pool[0]])
    assert len(out) == len(points_of(name))
    out = np.ascontiguousarray(out, dtype=np.float64)
    out.setflags(write=False)
    return out


def per_forest(values, B, P):
    """(B, P) from a scalar, (P,) or (B, P)"""
    return np.broadcast_to(np.asarray(values, dtype=np.float64), (B, P))


class Forest:
    """One forest's leaf-space state on the host columns: Minv, w, the constants, and Z of the training, candidate and
    conditioning points; `cols[i]` (n_i, m) are the host columns of point set i, tree by tree."""

    def __init__(self, inp, b, sets, dtype):
        lv = [pr.leaves_of(inp.F, s, inp.ft) for s in sets]
        self.Z = [z.astype(dtype) for z in pr.one_hot(lv, b)]
        m = inp.F.shape[1]
        self.cols = [np.nonzero(z)[1].reshape(z.shape[0], m) for z in self.Z]
        self.dtype, self.m = dtype, m
        self.s2 = dtype(1e-6) + dtype(inp.noise[b])
        self.scale = dtype(inp.scale[b])
        self.c = self.scale / (dtype(m) * self.s2)
        Z, y = self.Z[0], inp.y.reshape(-1).astype(dtype)
        self.Minv = pr.gauss_jordan_inverse(np.eye(Z.shape[1], dtype=dtype) + self.c * (Z.T @ Z))
        self.w = self.Minv @ (Z.T @ y)
        self.logpred = dtype(0)

    def predictive(self, z):
        t = self.Minv @ z
        q = z @ t
        return t, q, self.c * (z @ self.w), self.scale / self.dtype(self.m) * q + self.s2

    def update(self, z, value=None, eps=None):
        """one point; -> the value used"""
        t, q, mu, v = self.predictive(z)
        ys = self.dtype(value) if eps is None else mu + np.sqrt(v) * self.dtype(eps)
        self.w = self.w + t * ((ys - mu) / (1 + self.c * q))
        self.Minv = self.Minv - (self.c / (1 + self.c * q)) * np.outer(t, t)
        self.logpred = self.logpred - (np.log(v) + (ys - mu) ** 2 / v) / 2
        return ys

    def posterior(self, Zc):
        return self.c * (Zc @ self.w), self.scale / self.dtype(self.m) * np.einsum("ci,ij,cj->c", Zc, self.Minv, Zc)


def sequential(inp, points, values=None, eps=None, cand=None, dtype=np.float64):
    """(a) -> dict: mu, var (B, C) at the candidates, values (B, P) used, logpred (B,), forests [Forest] (their Minv and w
    after the update).  values: scalar, (P,) or (B, P); or eps (B, P) for sampled fantasies."""
    cand = inp.cand if cand is None else cand
    B, P = inp.F.shape[0], len(points)
    vals = None if values is None else per_forest(values, B, P)
    mu, var, used, forests = [], [], np.empty((B, P), dtype=dtype), []
    for b in range(B):
        f = Forest(inp, b, [inp.X, cand, points], dtype)
        for p in range(P):
            used[b, p] = f.update(f.Z[2][p], None if vals is None else vals[b, p], None if eps is None else eps[b, p])
        m_, v_ = f.posterior(f.Z[1])
        mu.append(m_), var.append(v_), forests.append(f)
    return dict(mu=np.stack(mu), var=np.stack(var), values=used, logpred=np.array([f.logpred for f in forests]), forests=forests)


def augmented(inp, points, values, b):
    """forest b alone with its own augmented data: (model, data)"""
    vals = per_forest(values, inp.F.shape[0], len(points))[b]
    model = (inp.F[b:b + 1], inp.noise[b:b + 1], inp.scale[b:b + 1])
    return model, (np.concatenate([inp.X, points]), np.concatenate([inp.y.reshape(-1), vals]).reshape(-1, 1))


def dense(inp, points, values, cand=None):
    """(b) -> mu, var (B, C) float64"""
    cand = inp.cand if cand is None else cand
    out = [orc.forest_predict(*augmented(inp, points, values, b), cand, inp.ft) for b in range(inp.F.shape[0])]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def logpred_dense(inp, points, values):
    """(c) -> (B,): sum_p -1/2 (log v_p + (y_p - mu_p)^2 / v_p), (mu_p, v_p - s2) the dense posterior at point p given the
    data and the points before it"""
    B, P = inp.F.shape[0], len(points)
    vals = per_forest(values, B, P)
    out = np.zeros(B)
    for b in range(B):
        for p in range(P):
            model, data = augmented(inp, points[:p], vals[:, :p], b)
            mu, var = orc.forest_predict(model, data, points[p:p + 1], inp.ft)
            v = var[0, 0] + 1e-6 + inp.noise[b]
            out[b] -= 0.5 * (np.log(v) + (vals[b, p] - mu[0, 0]) ** 2 / v)
    return out


def mll_difference(inp, points, values):
    """-> (B,): MLL(data + new) - MLL(data) of the oracle, with the scale and without the 2 pi term"""
    kw = dict(include_scale=True, include_2pi=False)
    out = []
    for b in range(inp.F.shape[0]):
        (F, noise, scale), (Xa, ya) = augmented(inp, points, values, b)
        out.append(orc.batched_mll(F, noise, scale, Xa, ya, inp.ft, **kw)[0] - orc.batched_mll(F, noise, scale, inp.X, inp.y, inp.ft, **kw)[0])
    return np.array(out)


def greedy(inp, pending, q, kind, kappa, fantasy, normals=None, dtype=np.float64):
    """(d) over (a) -> (picks (q,), the smallest gap of the q winners).  fantasy: a float (the constant liar) or "sample" with
    normals(b, draw, P) -> (P,): pick k is fantasised with draw k, the pending points with draw q."""
    B = inp.F.shape[0]
    forests = [Forest(inp, b, [inp.X, inp.cand, inp.cand if pending is None else pending], dtype) for b in range(B)]

    def take(b, z, draw, n, j):
        forests[b].update(z, *((fantasy, None) if fantasy != "sample" else (None, normals(b, draw, n)[j])))

    if pending is not None:
        for b in range(B):
            for p in range(len(pending)):
                take(b, forests[b].Z[2][p], q, len(pending), p)
    picks, gap = [], np.inf
    for k in range(q):
        mu, var = (np.stack(v) for v in zip(*(f.posterior(f.Z[1]) for f in forests)))
        i, g = pr.gap_of(ar.acquisition(mu, var, kappa, kind, dtype).astype(np.float64), picks)
        picks.append(i)
        gap = min(gap, g)
        for b in range(B):
            take(b, forests[b].Z[1][i], k, 1, 0)
    return np.asarray(picks), gap


def greedy_dense(inp, pending, q, kind, kappa, liar):
    """the constant liar over (b) -> (picks (q,), the smallest gap)"""
    picks, gap = [], np.inf
    for _ in range(q):
        cur = inp.cand[picks] if pending is None else np.concatenate([pending, inp.cand[picks]])
        mu, var = dense(inp, cur, liar) if len(cur) else orc.forest_predict(inp.model, inp.data, inp.cand, inp.ft)
        i, g = pr.gap_of(ar.acquisition(mu, var, kappa, kind), picks)
        picks.append(i)
        gap = min(gap, g)
    return np.asarray(picks), gap
