"""Host restatement of the importance weights of a fitted posterior's forest samples (numpy only, no GPU), shared by
tests/test_posterior_weights_cpu.py and tests/test_gpu_posterior_weights.py:

    update(log_w, inc, info)     the log-sum-exp update of bark_forest_weights_hip: l = log_w + inc (-inf for a dead forest),
                                 M = max l, S = sum exp(l - M), log_w' = l - M - log S, w' = exp(log_w'),
                                 stats = (M + log S, 1 / sum w'^2, max w')
    systematic(w, n, seed)       systematic resampling: positions (u + i) / n looked up in the running sum of w
    combine(w, values)           sum_b w_b v_b accumulated in forest order (the four sum kinds of the scan)
    mixture(w, mu, var, kappa)   the lower confidence bound of the moment-matched weighted mixture, in np.longdouble

The reference's mixture is always equal-weight (tree_gps.py:116-131), so none of this has a counterpart there; with
w = 1 / B `mixture` is acq_ref.acquisition(kind="lcb_mixture")."""
import numpy as np


def _terms(log_w, inc, info, B, dtype):
    lw = np.zeros(B, dtype=dtype) if log_w is None else np.asarray(log_w, dtype=dtype)
    ic = np.zeros(B, dtype=dtype) if inc is None else np.asarray(inc, dtype=dtype)
    dead = ~np.isfinite(ic) | ~np.isfinite(lw)
    if info is not None:
        dead |= np.asarray(info) != 0
    with np.errstate(invalid="ignore"):
        return np.where(dead, -np.inf, lw + ic)


def update(log_w, inc, info=None, dtype=np.float64):
    """-> (log_w' (B,), w' (B,), stats (3,)); all dead: stats[0] = -inf and NaN everywhere else"""
    B = len(next(a for a in (log_w, inc, info) if a is not None))
    term = _terms(log_w, inc, info, B, dtype)
    top = term.max()
    if top == -np.inf:
        nan = np.full(B, np.nan, dtype=dtype)
        return nan, nan.copy(), np.array([-np.inf, np.nan, np.nan], dtype=dtype)
    total = np.exp(term - top).sum()
    log_new = term - top - np.log(total)
    w = np.exp(log_new)
    return log_new, w, np.array([top + np.log(total), 1 / (w * w).sum(), w.max()], dtype=dtype)


def brute_force(log_w, inc, info=None):
    """the same three results without the log-sum-exp shift, in np.longdouble: only for increments whose exp does not
    underflow there"""
    B = len(inc)
    term = _terms(log_w, inc, info, B, np.longdouble)
    raw = np.exp(term)
    w = raw / raw.sum()
    with np.errstate(divide="ignore"):
        return np.log(w), w, np.array([np.log(raw.sum()), 1 / (w * w).sum(), w.max()], dtype=np.longdouble)


def systematic(w, n, seed):
    """-> (n,) int64: for position p the first forest whose running sum of w / sum(w) exceeds p, by a plain loop"""
    w = np.asarray(w, dtype=np.float64)
    u = np.random.default_rng(seed).random()
    cum = np.cumsum(w)
    cum = cum / cum[-1]
    out, b = [], 0
    for i in range(n):
        p = (u + i) / n
        while not cum[b] > p:
            b += 1
        out.append(b)
    return np.asarray(out, dtype=np.int64)


def combine(w, values):
    """sum_b w_b values[b] in forest order from 0.0, skipping weight 0 -> ((C,), sum_b |w_b values[b]| (C,))"""
    acc, mag = np.zeros(values.shape[1]), np.zeros(values.shape[1])
    for b in range(values.shape[0]):
        if w[b] == 0.0:
            continue
        acc = acc + w[b] * values[b]
        mag = mag + np.abs(w[b] * values[b])
    return acc, mag


def mixture(w, mu, var, kappa):
    """mu_mix - kappa sqrt(var_mix), mu_mix = sum_b w_b mu_b, var_mix = sum_b w_b (var_b + mu_b^2) - mu_mix^2"""
    w = np.asarray(w, dtype=np.longdouble)[:, None]
    mu, var = np.asarray(mu, dtype=np.longdouble), np.asarray(var, dtype=np.longdouble)
    mu_y = (w * mu).sum(axis=0)
    var_y = (w * (var + mu ** 2)).sum(axis=0) - mu_y ** 2
    return mu_y - np.longdouble(kappa) * np.sqrt(np.maximum(var_y, 0))
