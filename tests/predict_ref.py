"""Host restatement of the predictions from a fitted posterior (numpy and the oracle only, no GPU), shared by
tests/test_posterior_predict_cpu.py and tests/test_gpu_posterior_predict.py.  Written from the formulas of include/bark_hip.h
(bark_leaf_posterior_predict_hip), not from the kernel.  The cases are those of tests/acq_ref.py.

Per forest b and point c, (mu_bc, var_bc) is `acq_ref.posterior`, the oracle's dense `forest_predict`; with `observation`
var_bc + (1e-6 + noise_b).  Under normalised weights w_b:

    west(w, mu, var)        the header's one-pass recurrence in float64, forests in order, weight 0 skipped:
                            W += w; delta = mu - mean; mean += (w / W) delta; S += (w delta)(mu - mean); V += w var
                            -> mean, (V + S) / W
    two_pass(w, mu, var)    the same moments in np.longdouble: mean = sum w mu / sum w, var = sum w (var + (mu - mean)^2) / sum w
    cdf / pdf               F(t) = sum_b w_b Phi((t - mu_b) / sd_b) and its density in np.longdouble; sd = sqrt(max(var, 0)), a
                            forest with sd = 0 is a step at mu
    quantile(p, w, mu, var) the root of F(t) = p by bisection in np.longdouble to the fixed point, from the header's bracket
                            [min_b, max_b] of mu_b + z_p sd_b (F(lo) >= p gives lo, F(hi) < p gives hi)
    scores(w, mu, var, y)   `scores_ref.scores` with the weighted mixture: log sum_b w_b N(y; mu_b, var_b) and
                            (y - sum_b w_b mu_b)^2; per forest as there

Phi in np.longdouble.  math.erfc is a double; here erf(x) = (2 / sqrt pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 ... (2n+1)), a
series of positive terms (no cancellation) summed until a term no longer changes the sum; |x| >= 7 gives -1 / 1 (erfc(7) =
4e-23).  Its absolute error is a few longdouble roundings, 1e-19, far below the 2^-53 = 1.1e-16 the tests resolve.

Bars.  The device posterior is held to |d mu_b| <= e_mu = ATOL + RTOL |mu_b| and |d var_b| <= e_var = ATOL + RTOL |var_b|
(acq_ref.ATOL / RTOL).  mean = sum w mu_b moves by at most sum w e_mu; the tests hold it to ATOL + RTOL
|mean|, which is no wider.  var = sum w var_b + sum w (mu_b - mean)^2 has d var / d var_b = w_b and d var / d mu_b = 2 w_b
(mu_b - mean) (the terms through d mean cancel: sum w (mu_b - mean) = 0), so with spread = max_b |mu_b - mean| and
sum w var_b <= var
    |d var| <= ATOL + RTOL var + 2 spread (ATOL + RTOL max_b |mu_b|)                                    (`var_bar`).
No division by a small variance and no mean^2 enter: the recurrence does not cancel, so the bar needs no amplification by
mean^2 / var, whatever the size of y.  A quantile t solves F(t; mu, var) = p; moving every mu_b by e moves t by e, and moving
var_b by e_var moves the component quantile mu_b + z sd_b by |z| e_var / (2 sd_b) <= |z| e_var / (2 sqrt(VAR_FLOOR)), about 16
|z| e_var at VAR_FLOOR = 1e-3 — the cases' variances are O(1), where the factor is 1/2: the tests use (1 + |z_p|) times the
posterior bar, as the issue that introduced them sets.  The weighted scores move by at most `scores_ref.precheck(name)` (the
amplification A of a posterior error into a log density, derived there) times the posterior bar."""
from __future__ import annotations

import statistics
from functools import lru_cache

import numpy as np

import acq_ref as ar
import scores_ref as sr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def zscore(p: float) -> float:
    return statistics.NormalDist().inv_cdf(float(p))


def forest_moments(name, observation: bool = False):
    """(mu, var) (B, C) float64 of a case; with `observation` the noise 1e-6 + noise_b is added to var"""
    mu, var = ar.posterior(sr.case_of(name) if name == ar.SLAB_CASE.name else name)
    if observation:
        var = var + (1e-6 + sr.inputs(name).noise)[:, None]
    return mu, var


def west(w, mu, var):
    """the header's recurrence, float64, every operation as written -> (mean (C,), var (C,))"""
    w, mu, var = np.asarray(w, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    C = mu.shape[1]
    W, mean, S, V = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    for b in range(mu.shape[0]):
        if w[b] == 0.0:
            continue
        W = W + w[b]
        delta = mu[b] - mean
        mean = mean + (w[b] / W) * delta
        S = S + (w[b] * delta) * (mu[b] - mean)
        V = V + w[b] * var[b]
    return mean, (V + S) / W


def two_pass(w, mu, var):
    """np.longdouble -> (mean, var)"""
    w = np.asarray(w, dtype=LD)[:, None]
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    total = w.sum()
    mean = (w * mu).sum(axis=0) / total
    return mean, (w * (var + (mu - mean) ** 2)).sum(axis=0) / total


def var_bar(w, mu, var):
    """the bar of the mixture variance derived in the module docstring, per point"""
    mean, v = two_pass(w, mu, var)
    live = np.asarray(w) != 0
    spread = np.abs(np.asarray(mu)[live] - mean.astype(np.float64)).max(axis=0)
    return ar.ATOL + ar.RTOL * v.astype(np.float64) + 2 * spread * (ar.ATOL + ar.RTOL * np.abs(np.asarray(mu)[live]).max(axis=0))


def erf_ld(x):
    """erf in np.longdouble, elementwise, by the positive series of the module docstring"""
    x = np.asarray(x, dtype=LD)
    a = np.minimum(np.abs(x), LD(7))
    term = a.copy()
    total = a.copy()
    n = 0
    while True:
        n += 1
        term = term * (2 * a * a) / LD(2 * n + 1)
        new = total + term
        if np.array_equal(new, total):
            break
        total = new
    out = LD(2) / np.sqrt(LD(np.pi)) * np.exp(-a * a) * total
    out = np.where(np.abs(x) >= 7, LD(1), out)
    return np.sign(x) * out


def Phi(x):
    return LD(0.5) * (1 + erf_ld(np.asarray(x, dtype=LD) / np.sqrt(LD(2))))


def cdf(t, w, mu, var):
    """F(t) per point in np.longdouble: t (C,), w (B,), mu / var (B, C)"""
    t, w = np.asarray(t, dtype=LD), np.asarray(w, dtype=LD)
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    sd = np.sqrt(np.maximum(var, 0))
    safe = np.where(sd > 0, sd, 1)
    comp = np.where(sd > 0, Phi((t - mu) / safe), (t >= mu).astype(LD))
    return (w[:, None] * comp).sum(axis=0)


def pdf(t, w, mu, var):
    """the density of the components with sd > 0, per point, np.longdouble"""
    t, w = np.asarray(t, dtype=LD), np.asarray(w, dtype=LD)
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    sd = np.sqrt(np.maximum(var, 0))
    safe = np.where(sd > 0, sd, 1)
    comp = np.where(sd > 0, np.exp(-((t - mu) / safe) ** 2 / 2) / (safe * np.sqrt(2 * LD(np.pi))), 0)
    return (w[:, None] * comp).sum(axis=0)


def quantile(p, w, mu, var):
    """(C,) np.longdouble: bisection to the fixed point inside the header's bracket"""
    w = np.asarray(w, dtype=np.float64)
    live = w != 0
    mu64, var64 = np.asarray(mu, dtype=np.float64)[live], np.asarray(var, dtype=np.float64)[live]
    ends = mu64 + zscore(p) * np.sqrt(np.maximum(var64, 0))
    lo, hi = ends.min(axis=0).astype(LD), ends.max(axis=0).astype(LD)
    wl, p = w[live], LD(p)
    at_lo, at_hi = cdf(lo, wl, mu64, var64) >= p, cdf(hi, wl, mu64, var64) < p
    a, b = lo.copy(), hi.copy()  # F(a) < p <= F(b) where neither end answers
    for _ in range(200):
        mid = a + (b - a) / 2
        if np.all((mid == a) | (mid == b)):
            break
        below = cdf(mid, wl, mu64, var64) < p
        a, b = np.where(below, mid, a), np.where(below, b, mid)
    return np.where(at_lo, lo, np.where(at_hi, hi, b))


def scores(w, mu, var, y, dtype=np.float64):
    """the dict of `scores_ref.scores` with the mixture rows of the weighted mixture; forests of weight 0 take no part in them"""
    out = sr.scores(mu, var, y, dtype)
    w = np.asarray(w, dtype=dtype)
    live = w != 0
    mu, var, y = np.asarray(mu, dtype=dtype)[live], np.asarray(var, dtype=dtype)[live], np.asarray(y, dtype=dtype)
    C = mu.shape[1]
    ll = -0.5 * np.log(2 * dtype(np.pi) * var) - 0.5 * (y - mu) ** 2 / var + np.log(w[live])[:, None]
    top = ll.max(axis=0)
    log_density = top + np.log(np.exp(ll - top).sum(axis=0))
    sq_err = (y - (w[live][:, None] * mu).sum(axis=0)) ** 2
    out.update({"nlpd_mixture": -log_density.sum() / dtype(C), "mse_mixture": sq_err.sum() / dtype(C), "log_density": log_density,
                "sq_err": sq_err})
    return out


@lru_cache(maxsize=None)
def random_weights(B: int, seed: int = 0):
    """normalised random weights (B,), shared and read-only"""
    w = np.random.default_rng(1000 + seed).uniform(0.1, 1.0, size=B)
    w /= w.sum()
    w.setflags(write=False)
    return w
