"""information_based_fidelity.py:16-36, 90-167 on a fitted `LeafPosterior`: which fidelity is worth paying for.

The reference makes the fidelity an input feature (a categorical `TaskInput` column the trees split on like any other), so
forests, walks and the fitted state need nothing new.  Given a proposed x it computes, per fidelity l, the information that
observing f(x, l) gives about the minimum of the target-fidelity function, divides by the cost of l and takes the arg-max.
The target-fidelity half is the scan's kind "mes"; the lower-fidelity half needs the joint posterior of (x, l) and
(x, target), which in leaf space is one more bilinear form in the M^-1 the state holds:
    cov_b(p, q) = (scale_b / m) z_p' M_b^-1 z_q
and a one-dimensional quadrature per (candidate, forest), which runs on the device (bark_fidelity_gain_fitted_hip;
include/bark_hip.h has the formulas, the order contract and the limits).  No multi-task model is involved.

DEVIATION from the reference: it switches to the closed form by `fidelity == 0`; here every forest does, for every pair whose
two points share all their leaves under it — such a forest sees one random variable.  With fidelities[0] as the queried
fidelity the two rules coincide."""

from __future__ import annotations

import math

import numpy as np

from .. import _lib
from ..forest import FeatureTypeEnum, _is_torch, _points

CAT, INT = FeatureTypeEnum.Cat.value, FeatureTypeEnum.Int.value

GRID = (-10.0, 10.0, 100, 0.25, 250)  # (lo, hi, n_a, pad, G): information_based_fidelity.py:138-141, 156
MAX_PAIRS, MAX_TARGETS, MAX_SUPPORT, MAX_QUADRATURE = 65536, 1024, 1024, 4096


def _grid(grid):
    """(lo, hi, n_a, pad, G) checked on the host, by the limits of the entry point"""
    if len(grid) != 5:
        raise ValueError(f"grid must be (lo, hi, n_a, pad, G), got {grid!r}")
    lo, hi, n_a, pad, G = float(grid[0]), float(grid[1]), int(grid[2]), float(grid[3]), int(grid[4])
    if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(pad) and lo < hi and pad >= 0):
        raise ValueError(f"grid needs finite lo < hi and a finite pad >= 0, got {grid!r}")
    if not 2 <= n_a <= MAX_SUPPORT or not 2 <= G <= MAX_QUADRATURE:
        raise ValueError(f"grid needs 2 <= n_a <= {MAX_SUPPORT} and 2 <= G <= {MAX_QUADRATURE}, got {grid!r}")
    return lo, hi, n_a, pad, G


def _targets(targets, B: int):
    """(B, S) targets, numpy or torch as given, checked before a device is needed"""
    if targets is None:
        raise ValueError("the information gain needs targets: draws of the minimum, e.g. from fstar_at_fidelity")
    shape = tuple(targets.shape) if hasattr(targets, "shape") else np.shape(targets)
    if len(shape) != 2 or shape[0] != B:
        raise ValueError(f"targets must be ({B}, S): one row per forest (got shape {shape})")
    if not 1 <= shape[1] <= MAX_TARGETS:
        raise ValueError(f"between 1 and {MAX_TARGETS} targets per forest (got {shape[1]})")
    return targets


def information_gain(posterior, query, target, targets, *, grid=GRID, per_forest: bool = False, chunk: int | None = None,
                     weights="state"):
    """-> gains (C,), and with per_forest also the (B, C) values of the forests: the information that a value at query[c]
    gives about the minimum of the function target[c] lies on, whose draws are targets (B, S), averaged over the forests
    (bark_fidelity_gain_fitted_hip).  query, target: (C, d), 1 <= C <= 65536; targets: (B, S), S <= 1024.  The gain is not
    negated; -inf where the query has no variance, NaN where the quadrature finds no support.  weights: as for
    `LeafPosterior.scan` — "state" honours `log_weights`, a forest of weight 0 is skipped (its per-forest row is NaN).
    numpy inputs give numpy, torch inputs device tensors (decided by `query`).  chunk bounds the workspace and changes no bit.
    ValueError for an invalid categorical value in either array, a bad shape or grid; no CPU fallback."""
    import torch

    lo, hi, n_a, pad, G = _grid(grid)
    tgt = _targets(targets, posterior.B)
    if len(query) < 1 or len(query) != len(target):
        raise ValueError("information_gain needs as many target points as query points, and at least one")
    if len(query) > MAX_PAIRS:
        raise ValueError(f"at most {MAX_PAIRS} pairs per call (got {len(query)})")
    w_d = posterior._scan_weights(weights)
    q_d, t_d = _points(query, posterior.d)[0], _points(target, posterior.d)[0]
    C, S, R, dev = int(q_d.shape[0]), int(tgt.shape[1]), posterior.R, posterior.state.device
    # a copy: the caller's array may be read-only
    tgt_d = _lib.to_device(tgt.detach() if _is_torch(tgt) else np.array(tgt, dtype=np.float64), torch.float64)
    w_d = None if w_d is None else _lib.to_device(w_d, torch.float64)
    gain = torch.empty(C, dtype=torch.float64, device=dev)
    rows = torch.empty((posterior.B, C), dtype=torch.float64, device=dev) if per_forest else None
    lib = _lib.lib()
    posterior._call(lib.bark_fidelity_gain_fitted_hip,
                    lambda k: int(lib.bark_fidelity_gain_fitted_workspace_bytes(R, posterior.m, k, C, S)), chunk,
                    _lib.ptr(posterior.state), posterior.nbytes, _lib.ptr(q_d), _lib.ptr(t_d), C, _lib.ptr(tgt_d), S, _lib.ptr(w_d),
                    lo, hi, n_a, pad, G, _lib.ptr(gain), _lib.ptr(rows), weights=w_d)
    if not _is_torch(query):
        gain, rows = gain.cpu().numpy(), None if rows is None else rows.cpu().numpy()
    return (gain, rows) if per_forest else gain


def _fidelity_value(feat_types, d: int, fidelity_feature, value) -> float:
    j = int(fidelity_feature)
    if not 0 <= j < d:
        raise ValueError(f"fidelity_feature must lie in [0, {d}), got {fidelity_feature}")
    v = float(value)
    kind = None if feat_types is None else int(np.asarray(feat_types)[j])
    if not math.isfinite(v):
        raise ValueError(f"fidelity value must be finite, got {value}")
    if kind == CAT and not (v == int(v) and 0 <= v < 32):
        raise ValueError(f"a categorical fidelity takes an integer code in [0, 32), got {value}")
    if kind == INT and v != int(v):
        raise ValueError(f"an integer fidelity takes an integer, got {value}")
    return v


def with_fidelity(x, fidelity_feature: int, value, feat_types=None):
    """A copy of the rows x (C, d), numpy or torch, with column `fidelity_feature` set to `value`.  With feat_types the value
    is checked against the column's type: ValueError for a categorical code outside [0, 32) or a fraction in an integer
    or categorical column."""
    if len(np.shape(x)) != 2:
        raise ValueError(f"x must be (C, d), got shape {tuple(np.shape(x))}")
    v = _fidelity_value(feat_types, int(x.shape[1]), fidelity_feature, value)
    out = x.clone() if _is_torch(x) else np.array(x, dtype=np.float64)
    out[:, int(fidelity_feature)] = v
    return out


def _check_fidelities(posterior, fidelity_feature, fidelities):
    if len(fidelities) < 1:
        raise ValueError("fidelities must name at least the target fidelity")
    for v in fidelities:
        _fidelity_value(posterior.feat_types, posterior.d, fidelity_feature, v)


def fidelity_information_gain(posterior, x, *, fidelity_feature: int, fidelities, targets, grid=GRID, chunk: int | None = None):
    """-> (T, C): row t the gain about the minimum at fidelities[0], the target fidelity, from evaluating the rows of x at
    fidelities[t]: `information_gain(with_fidelity(x, j, fidelities[t]), with_fidelity(x, j, fidelities[0]), targets)`.
    Row 0 is the scan's "mes" utility.  numpy x gives numpy, torch x a device tensor."""
    _check_fidelities(posterior, fidelity_feature, fidelities)
    ft = posterior.feat_types
    x0 = with_fidelity(x, fidelity_feature, fidelities[0], ft)
    rows = [information_gain(posterior, with_fidelity(x, fidelity_feature, v, ft), x0, targets, grid=grid, chunk=chunk)
            for v in fidelities]
    if _is_torch(x):
        import torch

        return torch.stack(rows)
    return np.stack(rows)


def fstar_at_fidelity(posterior, sites, *, fidelity_feature: int, target, num_samples: int = 100, seed: int = 0):
    """-> (B, num_samples) device float64: draws of the minimum of the target-fidelity function, each the minimum over
    `with_fidelity(sites, fidelity_feature, target)` of one posterior sample path (`posterior.sample_paths(num_samples,
    seed=seed)`, `LeafPaths.minimise`).  The reference's generate_fstar_samples on a fitted state: no model, no data.  The
    limits of `sample_paths` apply."""
    pts = with_fidelity(sites, fidelity_feature, target, posterior.feat_types)
    paths = posterior.sample_paths(int(num_samples), seed=seed)
    values, _ = paths.minimise(_points(pts, posterior.d)[0])
    return values.reshape(posterior.B, int(num_samples))


def _costs(costs, T: int) -> np.ndarray:
    c = np.asarray(costs, dtype=np.float64).reshape(-1)
    if c.shape[0] != T:
        raise ValueError(f"one cost per fidelity: got {c.shape[0]} costs for {T} fidelities")
    if not np.isfinite(c).all() or (c <= 0).any():
        raise ValueError("costs must be positive and finite")
    return c


def best_per_cost(gains, costs) -> np.ndarray:
    """(C,) int64: per column of gains (T, C) the arg-max over t of gains[t] / costs[t], ties to the lowest t; a NaN never
    wins, a column of NaN gives -1.  Host only."""
    g = np.asarray(gains, dtype=np.float64)
    ratio = g / _costs(costs, g.shape[0])[:, None]
    dead = np.isnan(ratio)
    index = np.argmax(np.where(dead, -np.inf, ratio), axis=0).astype(np.int64)
    index[dead.all(axis=0)] = -1
    return index


def propose_fidelity_information_based(posterior, x, costs, *, fidelity_feature: int, fidelities, sites=None, num_samples: int = 100,
                                       seed: int = 0, targets=None, grid=GRID):
    """The reference's function of this name for C points at once -> (index (C,) int64, gains (T, C)): index[c] is the t that
    maximises gains[t, c] / costs[t] (ties: the lowest t; NaN never wins; -1 when every gain is NaN), gains as
    `fidelity_information_gain` returns them.  targets: (B, S) draws of the target-fidelity minimum; without them
    `fstar_at_fidelity(posterior, sites, target=fidelities[0], num_samples=num_samples, seed=seed)` draws them (the
    reference uses 100).  ValueError for costs that are not positive and finite or not one per fidelity, a
    fidelity_feature outside [0, d), or a fidelity value the column's feature type does not admit — all before a device is
    needed.  numpy x gives numpy arrays, torch x device tensors."""
    c = _costs(costs, len(fidelities))
    _check_fidelities(posterior, fidelity_feature, fidelities)
    if targets is None:
        if sites is None:
            raise ValueError("propose_fidelity_information_based needs targets, or sites to draw them at")
        targets = fstar_at_fidelity(posterior, sites, fidelity_feature=fidelity_feature, target=fidelities[0],
                                    num_samples=num_samples, seed=seed)
    gains = fidelity_information_gain(posterior, x, fidelity_feature=fidelity_feature, fidelities=fidelities, targets=targets,
                                      grid=grid)
    index = best_per_cost(gains.cpu().numpy() if _is_torch(gains) else gains, c)
    if _is_torch(x):
        import torch

        return torch.from_numpy(index).to(gains.device), gains
    return index, gains
