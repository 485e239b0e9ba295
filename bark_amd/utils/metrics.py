"""Drop-in for `bark.utils.metrics` (reference: src/bark/utils/metrics.py:5-39): scores of Gaussian predictions.

Arrays are (N, batch): N points down the rows, one column per forest sample (the transpose of what `forest_predict`
returns); targets are (N, 1) or (N, batch).  numpy or torch: a torch input is worked on where it lives and gives a tensor
there.  `bark_amd.tree_kernels.predictive_scores` gives the same numbers for a forest model without the (N, batch) arrays."""

from __future__ import annotations

import math

import numpy as np

from ..forest import _is_torch


def gaussian_log_likelihood(mu, var, y):
    """log N(y; mu, var) elementwise -> (N, batch)  (metrics.py:5-17)."""
    resid = y - mu
    log = var.log() if _is_torch(var) else np.log(var)
    return -0.5 * (math.log(2.0 * math.pi) + log) - 0.5 * resid * resid / var


def nlpd(mu, var, test_y, diag=False):
    """Negative log predictive density per column -> (batch,): minus the mean over the N points of the log likelihood
    (metrics.py:20-33).  `diag` is accepted and, as in the reference, has no effect: only the marginal terms enter."""
    return -gaussian_log_likelihood(mu, var, test_y).sum(0) / test_y.shape[0]


def mse(mu, test_y):
    """Mean squared error over all points and columns -> scalar (metrics.py:36-39)."""
    resid = mu - test_y
    return (resid * resid).mean()
