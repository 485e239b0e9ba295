"""Host reference of the predictive scores (numpy and the oracle only, no GPU), shared by tests/test_scores_cpu.py and
tests/test_gpu_scores.py.  The cases are those of tests/acq_ref.py.

Held out: (mu, var) (B, C) is `acq_ref.posterior`, the oracle's dense `forest_predict`; the targets of a case are the y that
`acq_ref.problem(C, 200 + seed)` returns beside the case's candidates.  The scores are the reference's metrics
(src/bark/utils/metrics.py:5-39) per forest, and for the equally weighted mixture of the forests
    log_density_c = log( (1/B) sum_b N(y_c; mu_bc, var_bc) ),   sq_err_c = (y_c - mean_b mu_bc)^2.

Leave one out, two ways: from the oracle's inverse of K_s = scale K + (1e-6 + noise) I,
    mu_i = y_i - [K_s^-1 y]_i / [K_s^-1]_ii,   var_i = 1 / [K_s^-1]_ii,
and by brute force, N refits on N - 1 points with `orc.forest_predict` at the point left out plus the diagonal addend
1e-6 + noise on the variance (the predictive of the observation, not of the latent function).

Every reduction runs in float64 and in np.longdouble; `precheck` asserts that the two agree to 1e-12, that every variance is
at least acq_ref.VAR_FLOOR, and returns the amplification of a posterior error into a log density.

Bars.  The device posterior is held to rtol = acq_ref.RTOL, atol = acq_ref.ATOL.  A log density
l = -0.5 log(2 pi var) - 0.5 (y - mu)^2 / var has dl/dmu = (y - mu) / var and dl/dvar = -1 / (2 var) + (y - mu)^2 / (2 var^2), so
it moves by at most A = max(|y - mu| / var, 1 / (2 var) + (y - mu)^2 / (2 var^2)) per unit of posterior error: the held-out bar
is (RTOL A, ATOL A).  The leave-one-out moments are functions of the posterior (mu_f, var_f) at the training points, with
u = var_f / s2:  mu = y - (y - mu_f) / (1 - u),  var = s2 / (1 - u), whose derivatives are bounded by
    |dmu/dmu_f| = 1 / (1 - u),  |dmu/dvar_f| = |y - mu_f| / (s2 (1 - u)^2),  dvar/dvar_f = 1 / (1 - u)^2;
G = max(1, 1 / (1 - u) + |y - mu_f| / (s2 (1 - u)^2), 1 / (1 - u)^2) carries a posterior error into the leave-one-out
moments, and the leave-one-out bar is (RTOL A G, ATOL A G) with A taken at the leave-one-out moments."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import acq_ref as ar
from oracle import oracle as orc

KEYS = ("nlpd", "mse", "nlpd_mixture", "mse_mixture", "log_density", "sq_err")
GPU_CASES = ("prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit", "m13_past_lds", "m64_r256", ar.SLAB_CASE.name)
LOO_CASES = ("prior_n64", "prior_n257_chunks")
BRUTE_N, BRUTE_B = 24, 2


def case_of(name):
    return ar.SLAB_CASE if name == ar.SLAB_CASE.name else ar.CASES[name]


def inputs(name):
    return ar.make_inputs(case_of(name) if name == ar.SLAB_CASE.name else name)


@lru_cache(maxsize=None)
def targets(name):
    """(C,) test targets of a case"""
    case = case_of(name)
    y = ar.problem(case.C, 200 + case.seed)[1].reshape(-1).copy()
    y.setflags(write=False)
    return y


def scores(mu, var, y, dtype=np.float64):
    """mu, var (B, C), y (C,) -> the dict of `predictive_scores(..., return_values=True)`"""
    mu, var, y = np.asarray(mu, dtype=dtype), np.asarray(var, dtype=dtype), np.asarray(y, dtype=dtype)
    B, C = mu.shape
    sq = (y - mu) ** 2
    ll = -0.5 * np.log(2 * dtype(np.pi) * var) - 0.5 * sq / var  # metrics.py:17
    top = ll.max(axis=0)
    log_density = top + np.log(np.exp(ll - top).sum(axis=0) / dtype(B))
    sq_err = (y - mu.mean(axis=0)) ** 2
    return {"nlpd": -ll.sum(axis=1) / dtype(C), "mse": sq.sum(axis=1) / dtype(C), "nlpd_mixture": -log_density.sum() / dtype(C),
            "mse_mixture": sq_err.sum() / dtype(C), "log_density": log_density, "sq_err": sq_err}


def amplification(mu, var, y):
    r = np.abs(y - mu)
    return float(np.maximum(r / var, 0.5 / var + 0.5 * r**2 / var**2).max())


def heldout(name, dtype=np.float64):
    mu, var = ar.posterior(case_of(name) if name == ar.SLAB_CASE.name else name)
    return scores(mu, var, targets(name), dtype)


def _agree(a, b, what):
    for k in KEYS:
        assert np.allclose(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), rtol=1e-12, atol=1e-12), (what, k)


@lru_cache(maxsize=None)
def precheck(name):
    """-> A of the held-out case"""
    mu, var = ar.posterior(case_of(name) if name == ar.SLAB_CASE.name else name)
    assert var.min() >= ar.VAR_FLOOR, (name, float(var.min()))
    _agree(heldout(name), heldout(name, np.longdouble), name)
    return amplification(mu, var, targets(name))


# ---- leave one out ------------------------------------------------------------------------------------------------
def brute_inputs():
    """N = 24, B = 2: prior_n64's first forests on its first points"""
    inp = ar.make_inputs("prior_n64")
    return ar.Inputs(inp.case, inp.F[:BRUTE_B], inp.X[:BRUTE_N], inp.y[:BRUTE_N], inp.ft, inp.cand, inp.noise[:BRUTE_B],
                     inp.scale[:BRUTE_B])


def loo_inputs(name):
    return brute_inputs() if name == "brute" else ar.make_inputs(name)


@lru_cache(maxsize=None)
def loo_moments(name):
    """(mu, var, G) from the dense inverse: the moments (B, N) and the factor G of the module docstring"""
    inp = loo_inputs(name)
    y = inp.y.reshape(-1)
    mu, var, G = [], [], 1.0
    for b in range(inp.F.shape[0]):
        s2 = 1e-6 + inp.noise[b]
        K = inp.scale[b] * orc.forest_gram_matrix(inp.F[b], inp.X, inp.X, inp.ft)
        K_inv = np.linalg.inv(K + s2 * np.eye(len(y)))
        alpha, kappa = K_inv @ y, np.diagonal(K_inv)
        mu.append(y - alpha / kappa)
        var.append(1.0 / kappa)
        one_minus_u = s2 * kappa
        resid_f = np.abs(s2 * alpha)  # y - mu_f
        G = max(G, float((1 / one_minus_u + resid_f / (s2 * one_minus_u**2)).max()), float((1 / one_minus_u**2).max()))
    return np.stack(mu), np.stack(var), G


@lru_cache(maxsize=None)
def loo_brute():
    """(mu, var) (B, N) of the N refits of brute_inputs()"""
    inp = brute_inputs()
    B, N = inp.F.shape[0], inp.X.shape[0]
    mu, var = np.empty((B, N)), np.empty((B, N))
    for i in range(N):
        keep = np.arange(N) != i
        m_i, v_i = orc.forest_predict(inp.model, (inp.X[keep], inp.y[keep]), inp.X[i:i + 1], inp.ft)
        mu[:, i], var[:, i] = m_i[:, 0], v_i[:, 0] + (1e-6 + inp.noise)
    return mu, var


def loo(name, dtype=np.float64):
    inp = loo_inputs(name)
    mu, var, _ = loo_moments(name)
    return scores(mu, var, inp.y.reshape(-1), dtype)


@lru_cache(maxsize=None)
def loo_precheck(name):
    """-> A G of the leave-one-out case"""
    inp = loo_inputs(name)
    mu, var, G = loo_moments(name)
    assert var.min() >= ar.VAR_FLOOR, (name, float(var.min()))
    _agree(loo(name), loo(name, np.longdouble), name)
    return amplification(mu, var, inp.y.reshape(-1)) * G
