"""thompson_sampling.py:10-27 `generate_fstar_samples` on the numpy model triple.

The reference draws joint samples of the latent function at the training inputs from a gpytorch `BARKGP` (which no
longer exists) and keeps the min (or max) of each draw.  Here the draws come from the leaf-space
posterior (`posterior_samples`), whose covariance is the true scale K - K K_s^-1 K, so no non-PD warning needs
silencing, and the reduction over the sample sites runs on the device (`reduce=`).

`propose_thompson_from_candidates` / `propose_thompson_from_domain` are Thompson sampling proper: a batch of q proposals, each
the minimiser of one posterior sample path drawn from a fitted `LeafPosterior` (`sample_paths`)."""

from __future__ import annotations

import math

import numpy as np

from ..forest import _is_torch
from ..tree_kernels.tree_gps import posterior_samples


def generate_fstar_samples(model, data, domain, num_samples: int = 10, maximise: bool = False, generator=None):
    """-> (B, num_samples): the min (max with `maximise`) over the training inputs of each joint posterior draw of each
    forest sample.  model: (forest, noise, scale); data: (train_x, train_y); `domain` may be feat_types; generator: a
    torch.Generator, an int seed or None (see `posterior_samples`).  Torch train_x gives a device tensor, numpy a numpy
    array."""
    train_x, _ = data
    values, _ = posterior_samples(model, data, train_x, domain, num_samples, generator=generator,
                                  reduce="max" if maximise else "min")
    return values


# ---- Thompson sampling from the fitted posterior: one sample path per proposal, each minimised on its own ----

def thompson_forests(B: int, q: int, seed: int = 0, weights=None) -> np.ndarray:
    """The forest of each of the q draws: uniform over the B forest samples, `numpy.random.default_rng(seed)`.  weights: (B,)
    normalised importance weights of the forests (`LeafPosterior.weights`); the draws are then `rng.choice(B, q, p=weights)`,
    so a forest of weight 0 is never drawn.  None is the uniform call, the same array as before.  Host only."""
    q = int(q)
    if q < 1:
        raise ValueError(f"q must be positive, got {q}")
    rng = np.random.default_rng(seed)
    if weights is None:
        return rng.integers(0, int(B), size=q).astype(np.int64)
    p = np.asarray(weights, dtype=np.float64).reshape(-1)
    if p.shape[0] != int(B) or not np.isfinite(p).all() or (p < 0).any() or not p.sum() > 0:
        raise ValueError(f"weights must be ({int(B)},) non-negative finite numbers with a positive sum")
    return rng.choice(int(B), size=q, p=p / p.sum()).astype(np.int64)


def _forest_weights_of(post):
    """the state's weights on the host for `thompson_forests`, None while it has none"""
    return None if post.log_weights is None else post.weights.cpu().numpy()


def _posterior_of(model, data, domain, posterior):
    from ..tree_kernels.posterior import fit_posterior
    from .acquisition import _fitted

    if posterior is not None:
        return _fitted(posterior, domain)
    return fit_posterior(model, data, domain)


def propose_thompson_from_candidates(model, data, candidates, domain, q: int, *, seed: int = 0, posterior=None,
                                     return_info: bool = False):
    """-> indices (q,) int64 into `candidates`: a batch of q Thompson proposals.  Each draw takes a forest sample uniformly,
    or by the state's importance weights when it has them (`thompson_forests(B, q, seed, weights)`), one posterior sample path of it (`LeafPosterior.sample_paths(forests=..., seed=seed)`:
    a repeated forest gets draw numbers 0, 1, ...) and that path's arg-min over the candidates (ties: the lowest index).  No
    outcome is fantasised and the draws do not see each other, so two draws can name the same candidate: duplicates are kept,
    and info["unique"] says how many distinct candidates the batch holds.

    model, data and `domain` mean what they mean to `acquisition_scan`; posterior: a `LeafPosterior` to draw from instead
    of fitting one (it is not modified; `model` / `data` may then be None) — a conditioned one gives paths that respect its
    pending points.  numpy candidates give a numpy array, torch candidates a device tensor.  With return_info: (indices, info),
    info = {"forest", "draw", "value" (one per draw, numpy), "unique"}."""
    post = _posterior_of(model, data, domain, posterior)
    forests = thompson_forests(post.B, q, seed, _forest_weights_of(post))
    paths = post.sample_paths(forests=forests, seed=seed)
    values, index = paths.minimise(candidates)
    if not return_info:
        return index
    host = index.cpu().numpy() if _is_torch(index) else index
    info = {"forest": forests, "draw": paths.draw.astype(np.int64), "unique": int(np.unique(host).shape[0]),
            "value": values.cpu().numpy() if _is_torch(values) else values}
    return index, info


def propose_thompson_from_domain(model, data, bounds, feat_types, q: int, *, seed: int = 0, posterior=None,
                                 exhaustive_limit: int = 2 ** 22, n_candidates: int = 2 ** 18, round_size: int = 2 ** 18,
                                 starts: int = 8, max_sweeps: int = 32, mode: str = "cells", return_info: bool = False):
    """-> X (q, d) numpy float64: a batch of q Thompson proposals over the whole domain `bounds` / `feat_types`.  The forests
    and paths are those of `propose_thompson_from_candidates` with the same seed.  A path depends on one forest only, so it
    is piecewise constant on that forest's own cell grid (`split_table(forest[b:b+1], ...)`), far smaller than the grid of all
    forests.  The draws are grouped by forest: one table and one candidate stream per distinct forest, every evaluation
    covering all its paths.

    A grid of at most `exhaustive_limit` cells is enumerated in rounds of `round_size` rows and each path keeps its first
    minimum in grid order: its exact global minimiser.  A larger grid is searched per path by `local_search` over the path's
    values, with `n_candidates`, `starts`, `max_sweeps`, `mode` and the seed as in `propose_from_domain` (the candidate
    rounds are evaluated once for all paths of the forest).  The result does not depend on `round_size`.  Duplicates are kept.

    posterior: as above.  With return_info: (X, info), info a list of one dict per draw: "forest", "draw", "value",
    "exhaustive", "grid", "sweeps" (0 when exhaustive), "index" (row of the grid, -1 after a search) and, after a search,
    "start_values" / "final_values"."""
    import torch

    from ..fitting.tree_proposals import check_bounds
    from .domain import MAX_NEIGHBOURS, _DeviceTable, domain_plan, local_search, split_table

    n_candidates, round_size, starts, max_sweeps = int(n_candidates), int(round_size), int(starts), int(max_sweeps)
    if round_size < 1 or round_size > MAX_NEIGHBOURS:
        raise ValueError(f"round_size must lie in [1, 2^24] (the scan's candidate limit), got {round_size}")
    if n_candidates < 1 or starts < 1 or max_sweeps < 0:
        raise ValueError("n_candidates and starts must be positive, max_sweeps non-negative")
    if mode not in ("cells", "uniform"):
        raise ValueError(f"unknown mode {mode!r} (use 'cells' or 'uniform')")
    b, ft = check_bounds(bounds, feat_types)
    post = _posterior_of(model, data, ft, posterior)
    forests = thompson_forests(post.B, q, seed, _forest_weights_of(post))
    paths = post.sample_paths(forests=forests, seed=seed)
    X = np.full((int(q), post.d), np.nan)
    info = [None] * int(q)
    for fb in np.unique(forests):
        sel = np.flatnonzero(forests == fb)
        sub = paths.subset(sel)
        table = split_table(post.forest[fb:fb + 1], b, ft)
        plan = domain_plan(table)
        dev = _DeviceTable(table, b, ft)
        grid = plan["grid"]
        if grid <= exhaustive_limit:
            k, device = len(sel), dev.rep.device
            best = torch.full((k,), math.inf, dtype=torch.float64, device=device)
            best_i = torch.full((k,), -1, dtype=torch.int64, device=device)
            best_row = torch.full((k, dev.d), math.nan, dtype=torch.float64, device=device)
            for first in range(0, grid, round_size):
                rows = dev.candidates(min(round_size, grid - first), "grid", 0, 0, first)
                value, index = sub.minimise(rows)
                better = value < best  # rounds run in grid order: equal values keep the lower index; NaN never wins
                best_row = torch.where(better.unsqueeze(1), rows[index.clamp(min=0)], best_row)
                best_i = torch.where(better, index + first, best_i)
                best = torch.where(better, value, best)
            if bool((best_i < 0).any()):
                raise RuntimeError(f"a sample path of forest {int(fb)} is NaN on every cell of its grid")
            rows_h, best_h, at_h = best_row.cpu().numpy(), best.cpu().numpy(), best_i.cpu().numpy()
            for j, i in enumerate(sel):
                X[i] = rows_h[j]
                info[i] = {"forest": int(fb), "draw": int(paths.draw[i]), "value": float(best_h[j]), "exhaustive": True,
                           "grid": grid, "sweeps": 0, "index": int(at_h[j])}
            continue
        if starts * plan["neighbours"] > MAX_NEIGHBOURS:
            raise ValueError(f"{starts} starts x {plan['neighbours']} cells exceed the scan's 2^24 candidates: use fewer starts")
        rounds = {}  # (first, n) -> (rows, values of all the forest's paths at them): one stream, one evaluate per round

        def candidates(first, n):
            if (first, n) not in rounds:
                rows = dev.candidates(n, mode, seed, 0, first)
                rounds[first, n] = (rows, sub.evaluate(rows))
            return rounds[first, n][0]

        for j, i in enumerate(sel):
            one = sub.subset(np.array([j]))

            def acq(rows, j=j, one=one):
                for cached, values in rounds.values():
                    if rows is cached:
                        return values[j]
                return one.evaluate(rows)[0]

            x, found = local_search(acq, candidates, dev.neighbours, n_candidates, round_size, starts, max_sweeps)
            X[i] = x
            info[i] = {"forest": int(fb), "draw": int(paths.draw[i]), "value": found["value"], "exhaustive": False, "grid": grid,
                       "sweeps": found["sweeps"], "index": -1, "start_values": found["start_values"],
                       "final_values": found["final_values"]}
    return (X, info) if return_info else X
