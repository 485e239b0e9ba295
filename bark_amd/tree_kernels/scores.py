"""Predictive scores of a set of forest samples, on the device: how well do they predict targets they were not given?

The reference answers with `bark.utils.metrics` (gaussian_log_likelihood, nlpd, mse; metrics.py:5-39) applied to the
(B, C) arrays of `forest_predict`.  `predictive_scores` gives the same numbers per forest, and those of the equally
weighted mixture of the forests, from one call (bark_predictive_scores_hip) that never forms the (B, C) arrays;
`loo_scores` gives them for the leave-one-out predictives at the training points, the usual check when no test set
exists.  include/bark_hip.h has the formulas.
"""

from __future__ import annotations

import numpy as np

from .. import _lib
from ..fitting.mll import _feat_types_of, _forest3, _leaf_call, _leaf_inputs, _y_vector
from ..forest import _is_torch

VARIANTS = {"auto": 0, "lds": 1, "global": 2}
MAX_TREES, MAX_LEAVES = 64, 8192  # limits of the leaf-space posterior (include/bark_hip.h)


def _entries(v) -> int:
    return int(v.numel()) if _is_torch(v) else int(np.size(v))


def _scores(model, data, points, y_points, domain, mode, return_values, chunk, variant, on_device):
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
    forest, noise, scale = model
    train_x, train_y = data
    nodes3 = _forest3(forest)
    m = int(nodes3.shape[1])
    if m > MAX_TREES:
        raise ValueError(f"predictive scores support at most {MAX_TREES} trees (got {m})")
    C = len(points)
    if C < 1:
        raise ValueError("predictive scores need at least one point")
    if _entries(y_points) != C:
        raise ValueError(f"the targets must have one entry per point ({C}), got {_entries(y_points)}")

    import torch

    from ..optimizer.acquisition import acquisition_plan

    q = _leaf_inputs(nodes3, noise, scale, train_x, train_y, _feat_types_of(domain), points)
    R, dev = q.R, q.device
    if R > MAX_LEAVES:
        raise ValueError(f"predictive scores support at most {MAX_LEAVES} leaves per forest (got {R})")
    acquisition_plan(R, m, variant)  # refuses variant="lds" past the LDS limit before anything is allocated
    yp = _y_vector(y_points, C)
    rows = torch.empty((q.B, 2), dtype=torch.float64, device=dev)
    mix = torch.empty(2, dtype=torch.float64, device=dev)
    values = torch.empty((2, C), dtype=torch.float64, device=dev) if return_values else None
    lib = _lib.lib()
    _leaf_call(q, lib.bark_predictive_scores_hip, lambda k: int(lib.bark_predictive_scores_workspace_bytes(q.N, R, q.pf.m, k, C)),
               chunk, _lib.ptr(q.cand_d), C, _lib.ptr(yp), mode, VARIANTS[variant], _lib.ptr(rows), _lib.ptr(mix), _lib.ptr(values))
    out = {"nlpd": -rows[:, 0] / C, "mse": rows[:, 1] / C, "nlpd_mixture": -mix[0] / C, "mse_mixture": mix[1] / C}
    if return_values:
        out["log_density"], out["sq_err"] = values[0], values[1]
    if on_device:
        return out
    return {k: (float(v.item()) if v.ndim == 0 else v.cpu().numpy()) for k, v in out.items()}


def predictive_scores(model, data, test_x, test_y, domain, *, return_values: bool = False, chunk: int | None = None,
                      variant: str = "auto", posterior=None):
    """Scores of the forest samples' posteriors at C held-out points -> dict:

      "nlpd" (B,)      per forest b, -(1/C) sum_c log N(y_c; mu_bc, var_bc): the column of the reference's
                       `nlpd(mu.T, var.T, test_y)` for (mu, var) = `forest_predict(model, data, test_x, domain)`
      "mse" (B,)       per forest, (1/C) sum_c (y_c - mu_bc)^2
      "nlpd_mixture"   -(1/C) sum_c log( (1/B) sum_b N(y_c; mu_bc, var_bc) ): the predictive density of the equally
                       weighted mixture of the forests (a log-sum-exp over forests per point)
      "mse_mixture"    (1/C) sum_c (y_c - mean_b mu_bc)^2
      with `return_values` also "log_density" (C,) and "sq_err" (C,): the per-point terms of the two mixture scores.

    model: the (forest, noise, scale) triple with leading dims flattened, data: (train_x, train_y), `domain` may be
    feat_types — as `forest_predict` takes them.  var is the latent variance of `forest_predict(diag=True)`; it is not
    clamped, so a variance that rounding made non-positive gives NaN or an infinity.  A NaN in test_y propagates.

    Every sum runs in a fixed order, so the result does not depend on `chunk` or `variant` ("auto", or "lds" / "global"
    as in `acquisition_scan`), bit for bit.  At most 64 trees and 8192 leaves per forest.  Extra device memory is that of
    the acquisition scan, against 16 B C bytes for `forest_predict` plus the formulas of `bark_amd.utils.metrics`.

    Torch test_x gives 0-d and 1-d device tensors; numpy test_x gives floats and numpy arrays.  ValueError when test_y
    does not have C entries, for shapes the entry point refuses and for an invalid categorical value; LinAlgError for a
    forest whose leaf-space system is not positive definite; there is no CPU fallback (RuntimeError without a GPU).

    posterior: a `LeafPosterior` (`fit_posterior`) to score instead of refitting; `model`, `data` and `domain` may then be
    None.  The result is `posterior.scores(test_x, test_y, ...)`: the state as it is now, after every `observe_`, and the
    mixture rows are those of its weighted mixture."""
    if posterior is not None:
        return posterior.scores(test_x, test_y, return_values=return_values, chunk=chunk, variant=variant)
    return _scores(model, data, test_x, test_y, domain, _lib.SCORE_HELDOUT, return_values, chunk, variant, _is_torch(test_x))


def loo_scores(model, data, domain, *, return_values: bool = False, chunk: int | None = None, variant: str = "auto"):
    """Leave-one-out scores at the N training points -> the dict of `predictive_scores`, with (mu_bi, var_bi) the predictive of
    observation i given the other N - 1 under forest b: mu_i = y_i - alpha_i / kappa_i, var_i = 1 / kappa_i with
    alpha = K_s^-1 y and kappa_i = [K_s^-1]_ii of K_s = scale K + (1e-6 + noise) I.  var_i is the variance of the observation
    (it contains the noise), unlike the latent variance of the held-out scores.  Both come from the two leaf-space sums of
    point i (include/bark_hip.h); no N x N matrix is formed and nothing is refitted.

    Torch train_x gives device tensors, numpy train_x floats and numpy arrays.  Errors as in `predictive_scores`."""
    train_x, train_y = data
    return _scores(model, data, train_x, train_y, domain, _lib.SCORE_LOO, return_values, chunk, variant, _is_torch(train_x))
