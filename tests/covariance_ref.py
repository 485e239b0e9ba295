"""Host reference of the joint covariance from a fitted posterior (numpy and the oracle only, no GPU), shared by
tests/test_posterior_covariance_cpu.py and tests/test_gpu_posterior_covariance.py.  Written from the formulas of
include/bark_hip.h (bark_leaf_posterior_covariance_hip), not from the kernel.  The cases are those of tests/acq_ref.py; points
are rows of the case's `cand`, named by index arrays or slices i1 and i2.

    truth(name, i1, i2)            (B, C1, C2) per forest by the reference's dense arithmetic: K_s = scale K_XX + (1e-6 + noise) I
                                   from `oracle.batched_forest_gram_matrix`, inverted by np.linalg.inv as the reference inverts,
                                   cov_b = scale K_12 - (scale K_1X) K_s^-1 (scale K_X2).  Nothing of it is in leaf space.
    mixture(w, cov, mu1, mu2)      the law of total covariance in np.longdouble, two passes: mean = sum w mu / sum w, then
                                   sum_b w_b (cov_b + (mu_b1 - mean_1)(mu_b2 - mean_2)') / sum w; mu from `acq_ref.posterior`
    two_stage(name, i1, i2)        the header's order restated in float64 on a host M^-1 = inv(I + c Z'Z): T[i][r] = sum_k
                                   M^-1[a_k][r] with k in tree order from 0.0, cov = (scale / m) sum_l T[i][b_l] with l in tree order
                                   from 0.0.  The leaf of a point under a tree comes from `oracle.get_leaf_vectors`; a point has one
                                   leaf per tree, so "code-bit order" is tree order whatever the columns inside a tree are called.
    mixture_order(w, cov, mu1, mean1, mu2, mean2)   the header's forest-order sum in float64, every operation as written

TI and TJ are the rows and columns of a workgroup's tile in bark_amd/csrc/covariance.hip (COV_TI, COV_TJ); the edge tests
place their shapes around them.

Bars.  The device posterior is held to the bar of DESIGN.md section 2, ATOL + RTOL |value| (acq_ref.ATOL / RTOL), for the
quantities that bar was derived for: mu_b and var_b = scale_b - (scale K_xX) K_s^-1 (scale K_Xx), whose two terms are each of the
size of scale_b.  cov_b[i][j] is the same expression between two points: its first term is scale_b K(x, x') <= scale_b and its
second is bounded by sqrt of the product of the two points' own second terms (Cauchy-Schwarz in the K_s^-1 inner product), each
<= scale_b.  The rounding of either route is relative to those terms, not to their difference, which vanishes for two points
that share no leaf with each other or the data; so per forest
    |d cov_b| <= ATOL + RTOL scale_b                                                                    (`forest_bar`).
mixture[i][j] = sum w_b (cov_b[i][j] + (mu_bi - mean_i)(mu_bj - mean_j)) / sum w has d / d cov_b = w_b and d / d mu_bi =
w_b (mu_bj - mean_j) (the terms through d mean cancel, sum w (mu_b - mean) = 0), likewise for mu_bj.  With spread = max_b
|mu_b - mean| over both points and the posterior bar on mu,
    |d mixture| <= ATOL + RTOL max_b scale_b + 2 spread (ATOL + RTOL max_b |mu_b|)                       (`mixture_bar`),
the shape of `predict_ref.var_bar`.  Two summation orders of the same float64 numbers (the diagonal against predict's variance,
a device result against a host sum of device numbers) are held to rtol = atol = 1e-12 (`ORDER_TOL`), as
tests/test_gpu_posterior_predict.py does between orders: m <= 64 terms of size <= 1 reorder to within m 2^-53 = 7e-15."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import acq_ref as ar
from oracle import oracle as orc

LD = np.longdouble
TI, TJ = 32, 64
ORDER_TOL = 1e-12


# the row and column points of the tests against `truth`, per case: both sides cross a tile edge wherever the case has the
# candidates for it, and the two sets overlap without being equal
CASE_POINTS = {
    "m1_r64": (np.arange(1), np.arange(1)),
    "m2_r65": (np.arange(5), np.array([4, 2, 1])),
    "m13_lds_limit": (np.arange(0, 45), np.arange(30, 130)),
    "m13_past_lds": (np.arange(0, 45), np.arange(30, 130)),
    "m64_r128": (np.arange(0, 40), np.arange(20, 100)),
    "prior_n257_chunks": (np.arange(0, 70), np.arange(60, 257)),
    "prior_n64": (np.arange(0, 2 * TI + 3), np.arange(40, 40 + 2 * TJ + 3)),
}


def points(name, idx):
    return ar.make_inputs(name).cand[idx]


@lru_cache(maxsize=None)
def _dense(name):
    """(K_s^-1 (B, N, N), scale K_XC (B, N, C)) of a case, once"""
    inp = ar.make_inputs(name)
    sc = inp.scale[:, None, None]
    K = sc * orc.batched_forest_gram_matrix(inp.F, inp.X, inp.X, inp.ft)
    K_inv = np.linalg.inv(K + (1e-6 + inp.noise[:, None, None]) * np.eye(inp.X.shape[0]))
    K_Xc = sc * orc.batched_forest_gram_matrix(inp.F, inp.X, inp.cand, inp.ft)
    return K_inv, K_Xc


def truth(name, i1, i2):
    """(B, C1, C2) float64"""
    inp = ar.make_inputs(name)
    K_inv, K_Xc = _dense(name)
    K12 = inp.scale[:, None, None] * orc.batched_forest_gram_matrix(inp.F, inp.cand[i1], inp.cand[i2], inp.ft)
    return K12 - K_Xc[:, :, i1].transpose(0, 2, 1) @ K_inv @ K_Xc[:, :, i2]


def mu_of(name, idx):
    """(B, C) posterior means of the dense route at the points"""
    return ar.posterior(name)[0][:, idx]


def mixture(w, cov, mu1, mu2):
    """np.longdouble (C1, C2); forests of weight 0 take no part"""
    w = np.asarray(w, dtype=LD)
    live = w != 0
    w, cov, mu1, mu2 = w[live], np.asarray(cov, dtype=LD)[live], np.asarray(mu1, dtype=LD)[live], np.asarray(mu2, dtype=LD)[live]
    total = w.sum()
    d1 = mu1 - (w[:, None] * mu1).sum(axis=0) / total
    d2 = mu2 - (w[:, None] * mu2).sum(axis=0) / total
    return (w[:, None, None] * (cov + d1[:, :, None] * d2[:, None, :])).sum(axis=0) / total


def forest_bar(name):
    """(B, 1, 1)"""
    return (ar.ATOL + ar.RTOL * ar.make_inputs(name).scale)[:, None, None]


def mixture_bar(name, w, mu1, mu2):
    """(C1, C2) for the weights w and the reference means mu1 (B, C1), mu2 (B, C2)"""
    w = np.asarray(w, dtype=np.float64)
    live = w != 0
    scale = ar.make_inputs(name).scale[live]
    m1, m2 = np.asarray(mu1)[live], np.asarray(mu2)[live]
    wl = w[live] / w[live].sum()
    s1 = np.abs(m1 - (wl[:, None] * m1).sum(axis=0)).max(axis=0)
    s2 = np.abs(m2 - (wl[:, None] * m2).sum(axis=0)).max(axis=0)
    spread = np.maximum(s1[:, None], s2[None, :])
    big = np.maximum(np.abs(m1).max(axis=0)[:, None], np.abs(m2).max(axis=0)[None, :])
    return ar.ATOL + ar.RTOL * scale.max() + 2 * spread * (ar.ATOL + ar.RTOL * big)


@lru_cache(maxsize=None)
def _leaf_space(name):
    """(leaf ids of the candidates (B, C, m), M^-1 per forest as a list of (R_b, R_b)) on the host"""
    inp = ar.make_inputs(name)
    N, m = inp.X.shape[0], inp.case.m
    pts = np.vstack([inp.X, inp.cand])
    ids, Minv = [], []
    for b in range(inp.case.B):
        cols, off = [], 0
        for t in range(m):
            lv = orc.get_leaf_vectors(inp.F[b, t], pts, inp.ft)
            cols.append(off + lv.argmax(axis=1))
            off += lv.shape[1]
        a = np.stack(cols, axis=1)  # (N + C, m), increasing along a row: tree order
        Z = np.zeros((N, off))
        Z[np.arange(N)[:, None], a[:N]] = 1.0
        c = inp.scale[b] / (m * (1e-6 + inp.noise[b]))
        Minv.append(np.linalg.inv(np.eye(off) + c * (Z.T @ Z)))
        ids.append(a[N:])
    return np.stack(ids), Minv


def two_stage(name, i1, i2):
    """(B, C1, C2) float64 by the header's two stages, in its order"""
    inp = ar.make_inputs(name)
    ids, Minv = _leaf_space(name)
    m, out = inp.case.m, []
    for b in range(inp.case.B):
        A1, A2 = ids[b][i1], ids[b][i2]
        T = np.zeros((A1.shape[0], Minv[b].shape[0]))
        for k in range(m):
            T = T + Minv[b][A1[:, k], :]
        acc = np.zeros((A1.shape[0], A2.shape[0]))
        for l in range(m):
            acc = acc + T[:, A2[:, l]]
        out.append((inp.scale[b] / m) * acc)
    return np.stack(out)


def mixture_order(w, cov, mu1, mean1, mu2, mean2):
    """the header's sum in float64: forests of non-zero weight in order from 0.0, then the division by their W"""
    w = np.asarray(w, dtype=np.float64)
    acc, W = np.zeros(cov.shape[1:]), 0.0
    for b in range(len(w)):
        if w[b] == 0.0:
            continue
        W = W + w[b]
        acc = acc + w[b] * (cov[b] + (mu1[b] - mean1)[:, None] * (mu2[b] - mean2)[None, :])
    return acc / W
