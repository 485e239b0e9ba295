"""The fitted leaf-space posterior as an object: fit once on the device, scan it many times.

Every call of `bark_amd.optimizer.acquisition_scan` packs the forests, walks the N training points, forms and factorises
I + c Z'Z for every forest, solves for w and M^-1, scores the candidates and throws all of that away.  `fit_posterior` does
the part that does not depend on the candidates (bark_leaf_posterior_fit_hip) and returns a `LeafPosterior` that owns the
result; its `scan` is the same scan from that state (bark_acquisition_scan_fitted_hip), `condition` is the step a greedy
batch takes between two picks (bark_leaf_posterior_condition_hip), and `observe` / `fantasise` / `log_predictive` move the
state forward on points with observed or sampled values (bark_leaf_posterior_observe_hip).  include/bark_hip.h has the contract: a scan from the
state returns the bits of the stateless scan that uses the `chunk` the state was fitted with.

The B forests are a sample of the tree posterior given the data of the fit.  After `observe_` they are a sample of the OLD
posterior; the exact correction is one importance weight per forest, w_b <- w_b p_b(y_new | data), and p_b is the log
predictive the observe kernel computes anyway.  `log_weights` holds them (None: equal weights, and then nothing changes a
bit): `observe_(reweight=True)` / `reweight_` update them (bark_forest_weights_hip), `ess` says how many forests still
matter, `resample` / `subset` thin them (bark_leaf_posterior_gather_hip), and `scan` (bark_acquisition_scan_fitted_weighted_hip)
and the Thompson proposals honour them — fit, propose, observe, propose as a sequential Monte Carlo loop.
"""

from __future__ import annotations

import math

import numpy as np

from .. import _lib
from ..fitting.mll import _feat_types_of, _fit_chunk, _forest3, _leaf_call, _leaf_inputs, _raise_on_info
from ..forest import _is_torch, _points, packed_forest

MAX_TREES, MAX_LEAVES = 64, 8192  # limits of the leaf-space posterior (include/bark_hip.h)
MAX_PENDING = 64  # points per call of `condition`, and pending points of a scan
MAX_COV_POINTS = 65536  # points per side of `covariance`


def _align256(n: int) -> int:
    return (n + 255) & ~255


class LeafPosterior:
    """M^-1 (B, R, R), w (B, R) and the sweep's status of B forest samples fitted to (train_x, train_y), in one device
    buffer (`state`, `nbytes` bytes), with what a scan needs beside them: the packed forests on the device (`packed`), the
    forest records on the host (`forest`, for `propose_from_domain`'s cell table), `noise` and `scale` (device, (B,)),
    `feat_types`, and B, m, R, d, N.  `info` is the device int32 status per forest (a view of the state; all zero unless a
    later `condition_` met an invalid categorical value), `train_y_min` the default target of kind "ei" / "pi", `chunk` the
    forests per chunk it was fitted with.  `log_weights`: None (equal weights) or the forests' log importance weights, a
    device float64 (B,) tensor whose log-sum-exp is 0, -inf for a dead forest; treat the tensor as read-only (copies share
    it).  `log_normaliser`: what the last `reweight_` returned.  Made by `fit_posterior`; there is no CPU fallback."""

    def __init__(self, q, state, chunk):
        self.packed, self.forest, self.feat_types = q.pf, q.nodes3, q.ft
        self.noise, self.scale = q.noise_d, q.scale_d
        self.B, self.m, self.R, self.d, self.N = q.B, q.m, q.R, q.d, q.N
        self.state, self.chunk = state, chunk
        self.train_y_min = float(q.yd.min())
        self.log_weights, self.log_normaliser = None, None

    @property
    def weights(self):
        """(B,) device float64: the normalised weights exp(log_weights), all 1 / B while there are none"""
        import torch

        if self.log_weights is None:
            return torch.full((self.B,), 1.0 / self.B, dtype=torch.float64, device=self.state.device)
        return torch.exp(self.log_weights)

    @property
    def ess(self) -> float:
        """the effective sample size 1 / sum_b w_b^2: B for equal weights, 1 when one forest holds all the weight"""
        w = self.weights
        return float(1.0 / (w * w).sum().item())

    @property
    def live_forest(self):
        """the records of the forests whose weight is not zero, in forest order (all of them while there are no weights)"""
        if self.log_weights is None:
            return self.forest
        return self.forest[(self.weights > 0).cpu().numpy()]

    @property
    def nbytes(self) -> int:
        return int(self.state.numel())

    @property
    def info(self):
        import torch

        at = _align256(8 * self.B * self.R * self.R) + _align256(8 * self.B * self.R)
        return self.state[at:at + 4 * self.B].view(torch.int32)

    def _copy(self) -> "LeafPosterior":
        new = object.__new__(LeafPosterior)
        new.__dict__.update(self.__dict__)
        new.state = self.state.clone()
        return new

    def _call(self, fn, need, chunk, *args, weights=None):
        """Run an entry point that starts from the state: args stand between `scale` and `info_out`.  weights: the device
        weights of a weighted scan; the status of a forest of weight 0 raises nothing, as it fails nothing in the call."""
        import torch

        info = torch.empty(self.B, dtype=torch.int32, device=self.state.device)
        Bc = int(chunk) if chunk else _fit_chunk(self.B, need)
        ws = _lib.workspace(need(Bc))
        _lib.check(fn(_lib.ctx(), _lib.ptr(self.packed.packed), self.packed.info_ref, self.d, _lib.ptr(self.noise), _lib.ptr(self.scale),
                      *args, _lib.ptr(info), _lib.ptr(ws), ws.numel(), Bc, _lib.stream_ptr()))
        _raise_on_info(info if weights is None else torch.where(weights == 0, torch.zeros_like(info), info), "leaf-space system")

    def _scan_weights(self, weights):
        """`scan`'s weights=, checked on the host -> None (the equal-weight call), the state's device weights or a normalised
        host array (B,)"""
        if weights is None:
            return None
        if isinstance(weights, str):
            if weights != "state":
                raise ValueError(f"weights must be 'state', None or a ({self.B},) array, got {weights!r}")
            return None if self.log_weights is None else self.weights
        w = np.asarray(weights.detach().cpu() if _is_torch(weights) else weights, dtype=np.float64)
        if w.shape != (self.B,):
            raise ValueError(f"weights must be ({self.B},), got {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError("weights must be non-negative finite numbers with a positive sum")
        return w / w.sum()

    def scan(self, candidates, kappa: float = 1.96, kind: str = "lcb_mean", return_values: bool = False, chunk: int | None = None,
             variant: str = "auto", pending=None, skip=None, targets=None, weights="state"):
        """What `acquisition_scan(model, data, candidates, domain, ...)` returns, by the same numpy / torch conventions and
        with the same errors, from the state: nothing of size N is touched.  The state is not modified; pending points
        condition a scratch copy of M^-1 inside the call.  Bit for bit the stateless result at the `chunk` of the fit; the
        `chunk` given here only bounds this call's workspace.

        weights: "state" (the default) averages the forests with the state's importance weights when it has them
        (`log_weights`), and is the call above when it has none; None forces equal weights; a (B,) array of non-negative
        finite numbers with a positive sum is normalised on the host and used for this call only.  With weights every
        per-forest term is multiplied by its forest's weight instead of 1 / B — `lcb_mixture` gets the weighted moments — and
        a forest of weight exactly 0 is skipped whole: its status fails nothing.  Pending points condition every forest."""
        from ..optimizer.acquisition import KINDS, TARGET_KINDS, VARIANTS, _skip_indices, _target_matrix, acquisition_plan

        if kind not in KINDS:
            raise ValueError(f"unknown kind {kind!r} (use 'lcb_mean', 'lcb_mixture', 'ei', 'pi' or 'mes')")
        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
        kappa = float(kappa)
        if not math.isfinite(kappa):
            raise ValueError(f"kappa must be finite, got {kappa}")
        if len(candidates) < 1:
            raise ValueError("acquisition scan needs at least one candidate")
        tgt = _target_matrix(targets, self.B, kind, np.array([self.train_y_min])) if kind in TARGET_KINDS else None
        w_d = self._scan_weights(weights)

        import torch

        cand_d = _points(candidates, self.d)[0]
        C, R, dev = int(cand_d.shape[0]), self.R, self.state.device
        acquisition_plan(R, self.m, variant)  # refuses variant="lds" past the LDS limit before anything is allocated
        pend_d = None if pending is None or len(pending) == 0 else _points(pending, self.d)[0]
        P = 0 if pend_d is None else int(pend_d.shape[0])
        if P > MAX_PENDING:
            raise ValueError(f"acquisition scan supports at most {MAX_PENDING} pending points (got {P})")
        skip_d = None if skip is None else _skip_indices(skip, C)
        tgt_d = None if tgt is None else _lib.to_device(tgt, torch.float64)
        w_d = None if w_d is None else _lib.to_device(w_d, torch.float64)
        acq = torch.empty(C, dtype=torch.float64, device=dev) if return_values else None
        best = torch.empty((), dtype=torch.float64, device=dev)
        idx = torch.empty((), dtype=torch.int64, device=dev)
        lib = _lib.lib()
        front = (_lib.ptr(self.state), self.nbytes, _lib.ptr(cand_d), C, _lib.ptr(pend_d), P, _lib.ptr(skip_d),
                 0 if skip_d is None else int(skip_d.numel()), _lib.ptr(tgt_d), 0 if tgt_d is None else int(tgt_d.shape[1]), kappa,
                 KINDS[kind], VARIANTS[variant])
        outs = (_lib.ptr(acq), _lib.ptr(best), _lib.ptr(idx))
        if w_d is None:
            self._call(lib.bark_acquisition_scan_fitted_hip,
                       lambda k: int(lib.bark_acquisition_scan_fitted_workspace_bytes(R, self.m, k, C, P, VARIANTS[variant])), chunk,
                       *front, *outs)
        else:
            self._call(lib.bark_acquisition_scan_fitted_weighted_hip,
                       lambda k: int(lib.bark_acquisition_scan_fitted_weighted_workspace_bytes(R, self.m, k, C, P, VARIANTS[variant])),
                       chunk, *front, _lib.ptr(w_d), *outs, weights=w_d)
        if _is_torch(candidates):
            return (best, idx, acq) if return_values else (best, idx)
        out = (float(best.item()), int(idx.item()))
        return (*out, acq.cpu().numpy()) if return_values else out

    def _predict_weights(self, weights):
        """`predict`'s and `scores`' weights=: None is the state's own weights (`scan`'s "state"), "equal" forces equal weights,
        an array is `scan`'s -> None or a float64 device tensor (B,)"""
        import torch

        w = self._scan_weights(None if isinstance(weights, str) and weights == "equal" else "state" if weights is None else weights)
        return None if w is None else _lib.to_device(w, torch.float64)

    def _predict(self, points, w_d, observation, y_d, probs, want_forest, want_values, chunk, variant):
        """One call of bark_leaf_posterior_predict_hip (at most 16 probabilities) -> the device outputs it was asked for"""
        import statistics

        import torch

        from ..optimizer.acquisition import VARIANTS

        pts_d = points
        C, B, R, dev = int(pts_d.shape[0]), self.B, self.R, self.state.device
        Q = len(probs)
        out = {"moments": torch.empty((2, C), dtype=torch.float64, device=dev)}
        if want_forest:
            out["forest"] = torch.empty((2, B, C), dtype=torch.float64, device=dev)
        if Q:
            out["quantiles"] = torch.empty((Q, C), dtype=torch.float64, device=dev)
        if y_d is not None:
            out["rows"] = torch.empty((B, 2), dtype=torch.float64, device=dev)
            out["mix"] = torch.empty(2, dtype=torch.float64, device=dev)
            if want_values:
                out["values"] = torch.empty((2, C), dtype=torch.float64, device=dev)
        p_h = np.asarray(probs, dtype=np.float64)
        z_h = np.asarray([statistics.NormalDist().inv_cdf(float(p)) for p in p_h], dtype=np.float64)
        lib = _lib.lib()
        self._call(lib.bark_leaf_posterior_predict_hip,
                   lambda k: int(lib.bark_leaf_posterior_predict_workspace_bytes(R, self.m, B, k, C, Q, int(want_forest),
                                                                                 int(y_d is not None), VARIANTS[variant])),
                   chunk, _lib.ptr(self.state), self.nbytes, _lib.ptr(pts_d), C, _lib.ptr(w_d), int(bool(observation)), _lib.ptr(y_d),
                   _lib.ptr(p_h if Q else None), _lib.ptr(z_h if Q else None), Q, VARIANTS[variant], _lib.ptr(out["moments"]),
                   _lib.ptr(out.get("forest")), _lib.ptr(out.get("quantiles")), _lib.ptr(out.get("rows")), _lib.ptr(out.get("mix")),
                   _lib.ptr(out.get("values")), weights=w_d)
        return out

    def _predict_args(self, points, variant):
        from ..optimizer.acquisition import VARIANTS, acquisition_plan

        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
        if len(points) < 1:
            raise ValueError("a prediction needs at least one point")
        acquisition_plan(self.R, self.m, variant)  # refuses variant="lds" past the LDS limit before anything is allocated
        return _points(points, self.d)[0]

    def predict(self, points, *, observation: bool = False, per_forest: bool = False, quantiles=None, weights=None,
                chunk: int | None = None, variant: str = "auto"):
        """The predictive of the weighted mixture of the forests at `points` (C, d), from the state
        (bark_leaf_posterior_predict_hip) -> dict:

          "mean", "var" (C,)               the mixture's moments (`mixture_of_gaussians_as_normal` over `forest_predict` for
                                           equal weights), by a one-pass recurrence in forest order that does not cancel
          "forest_mean", "forest_var"      (B, C), with `per_forest`: every forest's own posterior; NaN rows for weight 0
          "quantiles" (Q, C)               with `quantiles=[p, ...]`, each strictly inside (0, 1): the mixture's quantiles (a
                                           credible band is quantiles=[0.025, 0.975]); more than 16 go in calls of 16

        observation: add every forest's noise s2_b to its variance, the predictive of an observation instead of the latent
        function.  weights: None uses the state's own importance weights (equal weights while it has none), "equal" forces
        equal weights, a (B,) array is normalised on the host as in `scan`; a forest of weight exactly 0 is skipped and its
        status fails nothing.  The state is not modified.  No result depends on `chunk` or `variant`, bit for bit.  Torch
        points give device tensors, numpy points numpy arrays.  Errors as in `scan`; ValueError when the per-forest output
        exceeds the memory budget.  No CPU fallback."""
        probs = [] if quantiles is None else [float(p) for p in np.asarray(quantiles, dtype=np.float64).reshape(-1)]
        if any(not (0.0 < p < 1.0) for p in probs):
            raise ValueError(f"quantiles must lie strictly inside (0, 1), got {probs}")
        pts_d = self._predict_args(points, variant)
        C = int(pts_d.shape[0])
        if per_forest:
            from .tree_gps import _check_output_budget

            _check_output_budget(16 * self.B * C, f"predict(per_forest=True): {self.B} forests at {C} points")

        import torch

        w_d = self._predict_weights(weights)
        first = self._predict(pts_d, w_d, observation, None, probs[:16], per_forest, False, chunk, variant)
        out = {"mean": first["moments"][0], "var": first["moments"][1]}
        if per_forest:
            out["forest_mean"], out["forest_var"] = first["forest"][0], first["forest"][1]
        if probs:
            parts = [first["quantiles"]]
            for q0 in range(16, len(probs), 16):
                parts.append(self._predict(pts_d, w_d, observation, None, probs[q0:q0 + 16], False, False, chunk, variant)["quantiles"])
            out["quantiles"] = parts[0] if len(parts) == 1 else torch.cat(parts)
        return out if _is_torch(points) else {k: v.cpu().numpy() for k, v in out.items()}

    def covariance(self, x1, x2=None, *, per_forest: bool = False, observation: bool = False, weights=None,
                   chunk: int | None = None, variant: str = "auto"):
        """The joint posterior covariance of the weighted mixture of the forests between the points `x1` (C1, d) and `x2`
        (C2, d), from the state (bark_leaf_posterior_covariance_hip) -> (C1, C2); with `per_forest` the pair (mixture,
        forest), forest (B, C1, C2) holding every forest's own cov_b(x, x') = (scale_b / m) z(x)' M_b^-1 z(x'), NaN blocks
        for weight 0.  The mixture is the law of total covariance, sum_b w_b (cov_b + (mu_b - mean)(mu_b - mean)'), with
        `predict`'s means.  This is the covariance `sample_paths` draws from; `forest_predict(diag=False)` is not.

        x2=None is the symmetric call on x1: only one triangle is computed and the result equals its transpose in bits; its
        diagonal is `predict`'s variance to rounding.  observation: add every forest's noise s2_b to the diagonal, the
        covariance of observations at x1; only without x2, because two different evaluations share no noise.  weights,
        chunk, variant as in `predict`: the state's own importance weights by default, and no result depends on `chunk` or
        `variant`, bit for bit.  The state is not modified.  At most 65536 points per side.  Torch points give device tensors,
        numpy points numpy arrays.  Errors as in `scan`; ValueError when an output exceeds the memory budget.  No CPU fallback."""
        from ..optimizer.acquisition import VARIANTS
        from .tree_gps import _check_output_budget

        if x2 is not None and observation:
            raise ValueError("observation=True needs the symmetric call (x2=None): two different evaluations share no noise")
        x1_d = self._predict_args(x1, variant)
        if x2 is not None and len(x2) < 1:
            raise ValueError("a covariance needs at least one point on each side")
        x2_d = None if x2 is None else _points(x2, self.d)[0]
        C1 = int(x1_d.shape[0])
        C2 = C1 if x2_d is None else int(x2_d.shape[0])
        if max(C1, C2) > MAX_COV_POINTS:
            raise ValueError(f"covariance takes at most {MAX_COV_POINTS} points per side (got {C1} and {C2})")
        B, R = self.B, self.R
        _check_output_budget(8 * C1 * C2 * (B + 1 if per_forest else 1),
                             f"covariance: {C1} x {C2} points" + (f" for {B} forests" if per_forest else ""))

        import torch

        w_d = self._predict_weights(weights)
        dev = self.state.device
        mix = torch.empty((C1, C2), dtype=torch.float64, device=dev)
        forest = torch.empty((B, C1, C2), dtype=torch.float64, device=dev) if per_forest else None
        lib = _lib.lib()
        sym, var = int(x2_d is None), VARIANTS[variant]
        self._call(lib.bark_leaf_posterior_covariance_hip,
                   lambda k: int(lib.bark_leaf_posterior_covariance_workspace_bytes(R, self.m, B, k, C1, C2, sym, int(per_forest), 1, var)),
                   chunk, _lib.ptr(self.state), self.nbytes, _lib.ptr(x1_d), C1, _lib.ptr(x2_d), C2, _lib.ptr(w_d),
                   int(bool(observation)), var, _lib.ptr(forest), _lib.ptr(mix), weights=w_d)
        if not (_is_torch(x1) or _is_torch(x2)):
            mix, forest = mix.cpu().numpy(), None if forest is None else forest.cpu().numpy()
        return (mix, forest) if per_forest else mix

    def scores(self, points, values, *, observation: bool = False, return_values: bool = False, weights=None,
               chunk: int | None = None, variant: str = "auto"):
        """The dict of `predictive_scores` for targets `values` (C,) at `points` (C, d), from the state
        (bark_leaf_posterior_predict_hip): "nlpd" and "mse" per forest (NaN for a forest of weight 0), and "nlpd_mixture" /
        "mse_mixture" (with `return_values` "log_density" / "sq_err" per point) of the WEIGHTED mixture: the density
        sum_b w_b N(y; mu_b, var_b) and the error against the weighted mean.  weights, observation, chunk, variant as in
        `predict`.  On a freshly fitted state with equal weights and observation=False the result has the bits of
        `predictive_scores(model, data, ...)` at the `chunk` of the fit."""
        from ..fitting.mll import _y_vector

        pts_d = self._predict_args(points, variant)
        C = int(pts_d.shape[0])
        n = int(values.numel()) if _is_torch(values) else int(np.size(values))
        if n != C:
            raise ValueError(f"the targets must have one entry per point ({C}), got {n}")
        got = self._predict(pts_d, self._predict_weights(weights), observation, _y_vector(values, C), [], False, return_values, chunk,
                            variant)
        rows, mix = got["rows"], got["mix"]
        out = {"nlpd": -rows[:, 0] / C, "mse": rows[:, 1] / C, "nlpd_mixture": -mix[0] / C, "mse_mixture": mix[1] / C}
        if return_values:
            out["log_density"], out["sq_err"] = got["values"][0], got["values"][1]
        if _is_torch(points):
            return out
        return {k: (float(v.item()) if v.ndim == 0 else v.cpu().numpy()) for k, v in out.items()}

    def information_gain(self, query, target, targets, **kwargs):
        """-> gains (C,): what a value at query[c] tells about the minimum of the function target[c] lies on, whose draws are
        targets (B, S) — `bark_amd.optimizer.fidelity.information_gain(self, ...)`, which documents grid=, per_forest=, chunk=
        and weights=.  The state is not modified."""
        from ..optimizer.fidelity import information_gain

        return information_gain(self, query, target, targets, **kwargs)

    def condition_(self, points, values=None) -> "LeafPosterior":
        """Condition the state in place on `points` (P <= 64, d), in the order given, as `acquisition_scan(pending=points)`
        conditions its own M^-1: one rank-one downdate per point and forest, w unchanged.  A later `scan()` equals the
        stateless scan with these pending points, bit for bit; conditioning twice equals once on the concatenation.  After a
        ValueError for an invalid categorical value the state is marked failed (`info` = -1).

        values=None is that call, the kriging believer.  Otherwise the points are fantasised at `values` — a float (the
        constant liar), a (P,) array shared by the forests or a (B, P) array — and w moves with them
        (bark_leaf_posterior_observe_hip); M^-1 ends with the same bits either way.  These are fantasies: `N` and
        `train_y_min` stay as they are (`observe_` is the call for data)."""
        if points is None or len(points) == 0:
            return self
        pend_d = _points(points, self.d)[0]
        P = int(pend_d.shape[0])
        if P > MAX_PENDING:
            raise ValueError(f"at most {MAX_PENDING} pending points per call (got {P})")
        if values is not None:
            self._observe(pend_d, self._values(values, P, forests=True))
            return self
        lib = _lib.lib()
        self._call(lib.bark_leaf_posterior_condition_hip,
                   lambda k: int(lib.bark_leaf_posterior_condition_workspace_bytes(self.R, self.m, k, P)), None,
                   _lib.ptr(pend_d), P, _lib.ptr(self.state), self.nbytes)
        return self

    def condition(self, points, values=None) -> "LeafPosterior":
        """A new LeafPosterior conditioned on `points` (`condition_`): it shares the forests and owns a copy of the state."""
        return self._copy().condition_(points, values)

    def _values(self, values, P: int, forests: bool):
        """values of P points as a float64 device tensor: (P,), or with `forests` also a scalar (-> (P,)) or (B, P); with
        `forests` False also (P, 1), and the entries must be finite."""
        import torch

        if forests and np.ndim(values) == 0:  # a float, or a 0-d array or tensor
            values = np.full(P, float(values))
        v = _lib.to_device(values.detach() if _is_torch(values) else np.asarray(values, dtype=np.float64), torch.float64)
        if not forests and v.ndim == 2 and v.shape[1] == 1:
            v = v.reshape(-1)
        ok = tuple(v.shape) == (P,) or (forests and tuple(v.shape) == (self.B, P))
        if not ok:
            want = f"a float, ({P},) or ({self.B}, {P})" if forests else f"({P},) or ({P}, 1)"
            raise ValueError(f"values must be {want}, got {tuple(v.shape)}")
        if not forests and not bool(torch.isfinite(v).all()):
            raise ValueError("observed values must be finite")
        return v

    def _observe(self, pend_d, values_d=None, *, eps_d=None, seed: int = 0, draw: int = 0, values_out=None, logpred_out=None,
                 chunk=None):
        """One call of bark_leaf_posterior_observe_hip on the state: pend_d (P <= 64, d) on the device, with values_d ((P,)
        or (B, P)) or, without them, sampled fantasies (eps_d (B, P) or Philox draws named by seed and draw)."""
        import ctypes

        P = int(pend_d.shape[0])
        lib = _lib.lib()
        stride = 0 if values_d is None or values_d.ndim == 1 else P
        self._call(lib.bark_leaf_posterior_observe_hip,
                   lambda k: int(lib.bark_leaf_posterior_observe_workspace_bytes(self.R, self.m, k, P)), chunk,
                   _lib.ptr(pend_d), P, _lib.ptr(values_d), stride, _lib.OBSERVE_SAMPLE if values_d is None else _lib.OBSERVE_VALUES,
                   _lib.ptr(eps_d), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(draw), _lib.ptr(self.state), self.nbytes,
                   _lib.ptr(values_out), _lib.ptr(logpred_out))

    def observe_(self, points, values, chunk: int | None = None, reweight: bool = False) -> "LeafPosterior":
        """Take in real observations: the state becomes, to rounding, what `fit_posterior` gives on the data plus
        (`points`, `values`), by one rank-one step per point and forest on M^-1 and w instead of a refit
        (bark_leaf_posterior_observe_hip).  values: (P,) or (P, 1), finite, else ValueError.  More than 64 points are applied
        in slices of 64, in order.  Sets N += P and train_y_min = min(train_y_min, values.min()); everything that reads the
        state (`scan`, `sample_paths`, the `propose_*` functions) follows.  Returns self.  After a ValueError for an invalid
        categorical value the state is marked failed (`info` = -1).  chunk: forests per launch; it bounds the workspace and
        changes no bit, here and in `fantasise` and `log_predictive`.

        reweight=True also multiplies every forest's importance weight by its predictive density of the new values: the
        observe calls that update the state write each forest's log predictive (what `log_predictive` returns for the state
        before the update, by the same kernel, slices and sums — no second pass over the state), and the sum goes through
        `reweight_`; `log_normaliser` then holds the log predictive density of the weighted mixture.  A forest that could
        not have produced the data fades out, and `ess` says when to `resample` or to rerun the sampler.  ValueError when
        no forest is left with a weight: state and weights are then put back as they were.  That promise costs a copy of
        the state before the update (one device copy of 8 B R^2 bytes, and as much memory until the call returns); the
        update itself still reads and writes the state once.  The default changes nothing and copies nothing."""
        import torch

        if points is None or len(points) == 0:
            return self
        pend_d = _points(points, self.d)[0]
        P = int(pend_d.shape[0])
        v = self._values(values, P, forests=False)
        if reweight:
            backup = self.state.clone()
            total = torch.zeros(self.B, dtype=torch.float64, device=self.state.device)
            part = torch.empty_like(total)
        for p0 in range(0, P, MAX_PENDING):
            self._observe(pend_d[p0:p0 + MAX_PENDING], v[p0:p0 + MAX_PENDING], chunk=chunk, logpred_out=part if reweight else None)
            if reweight:
                total += part
        if reweight:
            try:
                self.reweight_(total)
            except ValueError:
                self.state.copy_(backup)
                raise
        self.N += P
        self.train_y_min = min(self.train_y_min, float(v.min()))
        return self

    def observe(self, points, values, chunk: int | None = None, reweight: bool = False) -> "LeafPosterior":
        """A new LeafPosterior that has taken in the observations (`observe_`): it shares the forests and owns a copy of the
        state."""
        return self._copy().observe_(points, values, chunk, reweight)

    def reweight_(self, log_increment) -> float:
        """Multiply the forests' weights by exp(log_increment) ((B,), numpy or torch) and renormalise them on the device
        (bark_forest_weights_hip) -> the log normaliser log sum_b w_b exp(inc_b); for a predictive increment that is the log
        predictive density of the weighted mixture.  -inf kills a forest, and so does a non-zero status of the state.
        ValueError, with the weights as they were, for a wrong shape, NaN or +inf in the increment, or when no forest would be
        left with a weight."""
        import torch

        inc = log_increment.detach() if _is_torch(log_increment) else torch.from_numpy(np.asarray(log_increment, dtype=np.float64))
        if tuple(inc.shape) != (self.B,):
            raise ValueError(f"log_increment must be ({self.B},), got {tuple(inc.shape)}")
        if bool((torch.isnan(inc) | (inc == math.inf)).any()):
            raise ValueError("log_increment must not hold NaN or +inf")
        inc = _lib.to_device(inc, torch.float64)
        log_w, _, stats = forest_weights(self.log_weights, inc, self.info)
        if stats[0] == -math.inf:
            raise ValueError("no forest is left with a non-zero weight: the forest samples cannot explain the data (rerun the sampler)")
        self.log_weights, self.log_normaliser = log_w, float(stats[0])
        return self.log_normaliser

    def subset(self, index) -> "LeafPosterior":
        """A new LeafPosterior of the n >= 1 forests `index` (ints in [0, B), repeats and any order allowed): their rows of
        the state copied on the device (bark_leaf_posterior_gather_hip), `noise` and `scale` gathered there, the records
        indexed on the host and packed again.  `log_weights` are gathered and renormalised; None stays None.  ValueError for
        an index out of range or when every chosen forest has weight 0."""
        import torch

        idx = np.asarray(index)
        if idx.ndim != 1 or idx.shape[0] < 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("index must be a non-empty 1-d array of ints")
        if idx.min() < 0 or idx.max() >= self.B:
            raise ValueError(f"index must lie in [0, {self.B})")
        idx = idx.astype(np.int64)
        n = int(idx.shape[0])
        idx_d = _lib.to_device(idx)
        lib = _lib.lib()
        nbytes = int(lib.bark_leaf_posterior_bytes(self.R, self.m, n))
        if nbytes == 0:
            raise ValueError(f"a fitted posterior refuses the shape B = {n}, m = {self.m}, R = {self.R}")
        log_w = None
        if self.log_weights is not None:
            # decided on the host, before anything is launched: the (B,) log weights are read back once
            if not np.isfinite(self.log_weights.cpu().numpy()[idx]).any():
                raise ValueError("every forest of the subset has weight 0")
            log_w = forest_weights(self.log_weights[idx_d], None, None)[0]
        state = torch.empty(nbytes, dtype=torch.uint8, device=self.state.device)
        _lib.check(lib.bark_leaf_posterior_gather_hip(_lib.ptr(self.state), self.B, self.R, _lib.ptr(idx_d), n, _lib.ptr(state),
                                                      _lib.stream_ptr()))
        new = object.__new__(LeafPosterior)
        new.__dict__.update(self.__dict__)
        new.state, new.B, new.chunk, new.log_weights = state, n, min(self.chunk, n), log_w
        new.log_normaliser = None  # it described a reweighting of the source's sample
        new.noise, new.scale = self.noise[idx_d].contiguous(), self.scale[idx_d].contiguous()
        new.forest = np.ascontiguousarray(self.forest[idx])
        new.packed = _PackedAs(packed_forest(new.forest, self.feat_types), self.R)
        return new

    def resample(self, n: int | None = None, seed: int = 0) -> "LeafPosterior":
        """Systematic resampling -> a new LeafPosterior of n (default B) equally weighted forests (`log_weights` None): forest b
        occurs floor(n w_b) or ceil(n w_b) times, a forest of weight 0 never.  The index is host work
        (`systematic_index(weights, n, seed)`: one uniform from `numpy.random.default_rng(seed)`), the copy is `subset`.
        Duplicates are exact copies; nothing rejuvenates them."""
        n = self.B if n is None else int(n)
        new = self.subset(systematic_index(self.weights.cpu().numpy(), n, seed))
        new.log_weights = None
        return new

    def fantasise(self, points, seed: int = 0, draw: int = 0, eps=None, chunk: int | None = None):
        """-> (LeafPosterior, values (B, P)): a copy conditioned on `points` (P <= 64) at values drawn from each forest's own
        predictive, point by point, each draw seeing the ones before it: per forest the P values are one joint draw of the
        noisy observations at the points.  eps: (B, P) standard normals, numpy or torch; without it Philox draws named by
        (`seed`, forest, `draw`, p) alone (fitting/_philox.fantasy_normals restates them), so the same pair gives the same
        fantasy whatever else is asked for; torch's generator is not used.  numpy points give a numpy array of values, torch
        points a device tensor.  `N` and `train_y_min` are those of the original."""
        new = self._copy()
        return new, new._fantasise_(points, seed, draw, eps, chunk)

    def _fantasise_(self, points, seed=0, draw=0, eps=None, chunk=None):
        """`fantasise` in place -> the values (B, P)."""
        import torch

        for name, x in (("seed", seed), ("draw", draw)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
                raise TypeError(f"{name} must be an int, got {type(x).__name__}")
        if not 0 <= int(draw) < 2 ** 32:
            raise ValueError(f"draw must lie in [0, 2^32), got {draw}")
        pend_d = _points(points, self.d)[0]
        P = int(pend_d.shape[0])
        if P < 1 or P > MAX_PENDING:
            raise ValueError(f"between 1 and {MAX_PENDING} points per call (got {P})")
        eps_d = None
        if eps is not None:
            eps_d = _lib.to_device(eps.detach() if _is_torch(eps) else np.asarray(eps, dtype=np.float64), torch.float64)
            if tuple(eps_d.shape) != (self.B, P):
                raise ValueError(f"eps must be ({self.B}, {P}), got {tuple(eps_d.shape)}")
        out = torch.empty((self.B, P), dtype=torch.float64, device=self.state.device)
        self._observe(pend_d, eps_d=eps_d, seed=int(seed), draw=int(draw), values_out=out, chunk=chunk)
        return out if _is_torch(points) else out.cpu().numpy()

    def log_predictive(self, points, values, chunk: int | None = None):
        """-> (B,): per forest the log density of `values` ((P,) or (P, 1), finite) at `points` under the state's predictive,
        one step ahead point by point — log p(y_1) + log p(y_2 | y_1) + ... without the 2 pi terms, which equals
        MLL(data + new) - MLL(data) in the convention of `batched_mll(include_2pi=False)`.  Computed on a scratch copy of
        the state by the update `observe_` applies; the state is not modified.  numpy points give numpy, torch points a device
        tensor."""
        import torch

        total = torch.zeros(self.B, dtype=torch.float64, device=self.state.device)
        if points is not None and len(points) > 0:
            pend_d = _points(points, self.d)[0]
            P = int(pend_d.shape[0])
            v = self._values(values, P, forests=False)
            scratch, part = self._copy(), torch.empty_like(total)
            for p0 in range(0, P, MAX_PENDING):
                scratch._observe(pend_d[p0:p0 + MAX_PENDING], v[p0:p0 + MAX_PENDING], logpred_out=part, chunk=chunk)
                total += part
        return total if _is_torch(points) else total.cpu().numpy()

    def sample_paths(self, num_samples: int = 1, *, forests=None, seed: int = 0, eps=None) -> LeafPaths:
        """Posterior sample paths from the state (bark_leaf_posterior_paths_hip): for path (b, s) the leaf weights
        W = c_b w_b + sqrt(scale_b / m) G_b eps, G_b the lower Cholesky factor of the state's M_b^-1 — of the conditioned matrix
        after `condition`, so the paths then respect the pending points.

        forests=None: `num_samples` paths of every forest, b-major (P = B num_samples).  forests=(P,) ints: one path per entry,
        entry i with the draw number equal to the count of earlier entries naming the same forest; the result is in the caller's
        order.  eps: (P, R) standard normals, numpy or torch, row i for path i; without it the normals are Philox draws named by
        (`seed`, b, s) alone (fitting/_philox.path_normals restates them), so the same seed gives the same path whatever else is
        asked for; torch's generator is not used.  Every forest that occurs is factorised once per 4096 paths.

        A forest whose M^-1 is not positive definite (or whose status is non-zero) gives NaN paths; nothing is raised here.
        ValueError for forests past `paths_plan`'s limit.  No CPU fallback."""
        import ctypes

        import torch

        paths_plan(self.R, self.m)
        if not isinstance(seed, (int, np.integer)):
            raise TypeError(f"seed must be an int, got {type(seed).__name__}")
        forest, draw, order = path_list(forests, self.B, num_samples)
        P, R, dev = int(forest.shape[0]), self.R, self.state.device
        eps_d = None
        if eps is not None:
            eps_d = _lib.to_device(eps.detach() if _is_torch(eps) else np.asarray(eps, dtype=np.float64), torch.float64)
            if tuple(eps_d.shape) != (P, R):
                raise ValueError(f"eps must be ({P}, {R}), got {tuple(eps_d.shape)}")
            eps_d = eps_d[torch.from_numpy(order).to(dev)].contiguous()
        sf, sd = np.ascontiguousarray(forest[order]), np.ascontiguousarray(draw[order])
        W = torch.empty((P, R), dtype=torch.float64, device=dev)
        info = torch.empty(self.B, dtype=torch.int32, device=dev)
        lib = _lib.lib()
        for p0 in range(0, P, MAX_PATHS_PER_CALL):
            n = min(MAX_PATHS_PER_CALL, P - p0)
            ws = _lib.workspace(int(lib.bark_leaf_posterior_paths_workspace_bytes(R, self.m, self.B, n, eps_d is None)))
            _lib.check(lib.bark_leaf_posterior_paths_hip(
                _lib.ctx(), self.packed.info_ref, _lib.ptr(self.noise), _lib.ptr(self.scale), _lib.ptr(self.state), self.nbytes,
                _lib.ptr(sf[p0:p0 + n]), _lib.ptr(sd[p0:p0 + n]), n, _lib.ptr(None if eps_d is None else eps_d[p0:p0 + n]),
                ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _lib.ptr(W[p0:p0 + n]), _lib.ptr(info), _lib.ptr(ws), ws.numel(),
                _lib.stream_ptr()))
        return LeafPaths(self, W, forest, draw, order)



def fit_posterior(model, data, domain, chunk: int | None = None) -> LeafPosterior:
    """The leaf-space posterior of the forest samples `model` = (forest, noise, scale) given `data` = (train_x, train_y), fitted
    on the device and kept there: what every `acquisition_scan` computes before it looks at a candidate.  `domain` may be
    feat_types.  chunk: forests factorised at a time (default: as many as fit the memory budget); a scan from the result
    equals `acquisition_scan(..., chunk=chunk)` bit for bit.

    Limits and errors are those of `acquisition_scan`: at most 64 trees and 8192 leaves per forest, ValueError for an invalid
    categorical value in train_x, LinAlgError for a forest whose leaf-space system is not positive definite, RuntimeError
    without a GPU (no CPU fallback).  Device memory kept: `nbytes` = 8 B (R^2 + R) + 4 B rounded up to 256-byte areas, plus
    the packed forests."""
    forest, noise, scale = model
    train_x, train_y = data
    nodes3 = _forest3(forest)
    m = int(nodes3.shape[1])
    if m > MAX_TREES:
        raise ValueError(f"a fitted posterior supports at most {MAX_TREES} trees (got {m})")
    if scale is None:
        raise ValueError("a fitted posterior needs scale")

    import torch

    q = _leaf_inputs(nodes3, noise, scale, train_x, train_y, _feat_types_of(domain))
    if q.R > MAX_LEAVES:
        raise ValueError(f"a fitted posterior supports at most {MAX_LEAVES} leaves per forest (got {q.R})")
    lib = _lib.lib()
    nbytes = int(lib.bark_leaf_posterior_bytes(q.R, q.pf.m, q.B))
    if nbytes == 0:
        raise ValueError(f"a fitted posterior refuses the shape B = {q.B}, m = {q.pf.m}, R = {q.R}")
    state = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    need = lambda k: int(lib.bark_leaf_posterior_fit_workspace_bytes(q.N, q.R, q.pf.m, k))  # noqa: E731
    Bc = int(chunk) if chunk else _fit_chunk(q.B, need)
    _leaf_call(q, lib.bark_leaf_posterior_fit_hip, need, Bc, _lib.ptr(state), nbytes)
    return LeafPosterior(q, state, Bc)


class _PackedAs:
    """A PackedForest presented with the leaf-space width R of the state it belongs to: a subset's own forests may have
    fewer leaves than the widest forest of the fit, and the state keeps R columns per forest.  The pack is shared (it may sit
    in the pack cache); only the copy of its info says R."""

    def __init__(self, pf, R: int):
        import ctypes

        self.packed, self.B, self.m, self.L = pf.packed, pf.B, pf.m, pf.L
        self.info = _lib.PackInfo()
        ctypes.pointer(self.info)[0] = pf.info
        if int(pf.info.max_bits) > R:
            raise ValueError("the forests have more leaves than the state has columns")
        self.info.max_bits = R

    @property
    def info_ref(self):
        import ctypes

        return ctypes.byref(self.info)


def forest_weights(log_weights, increment, info=None):
    """bark_forest_weights_hip -> (log_w (B,), w (B,), stats (3,) numpy): the weights exp(log_weights + increment)
    normalised on the device, in log form and plain, and {log normaliser, effective sample size, largest weight}.  Either
    input may be None (zeros); info: device int32 status per forest, non-zero kills the forest.  All dead: stats[0] = -inf
    and NaN everywhere else.  Reproducible bit for bit from run to run."""
    import torch

    given = [t for t in (log_weights, increment, info) if t is not None]
    if not given:
        raise ValueError("forest_weights needs log_weights, increment or info")
    B, dev = int(given[0].shape[0]), given[0].device
    log_w = torch.empty(B, dtype=torch.float64, device=dev)
    w = torch.empty_like(log_w)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    args = [None if t is None else t.contiguous() for t in (log_weights, increment, info)]
    _lib.check(_lib.lib().bark_forest_weights_hip(*(_lib.ptr(t) for t in args), B, _lib.ptr(log_w), _lib.ptr(w), _lib.ptr(stats),
                                                  _lib.stream_ptr()))
    return log_w, w, stats.cpu().numpy()


def systematic_index(weights, n: int, seed: int = 0) -> np.ndarray:
    """Systematic resampling, host only -> (n,) int64 forest indices, non-decreasing.  One uniform u from
    `numpy.random.default_rng(seed)`; the positions (u + i) / n, i < n, are looked up in the running sum of `weights` taken in
    forest order and divided by its last entry: position p names the first forest whose running sum exceeds p, so a forest of
    weight 0 is never named and forest b is named floor(n w_b) or ceil(n w_b) times."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be positive, got {n}")
    if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("weights must be non-negative finite numbers with a positive sum")
    cum = np.cumsum(w)
    cum /= cum[-1]
    pos = (np.random.default_rng(seed).random() + np.arange(n)) / n
    return np.searchsorted(cum, pos, side="right").astype(np.int64)


MAX_PATHS_PER_CALL = 4096  # paths per call of the two path entry points (include/bark_hip.h)


def paths_plan(R: int, m: int) -> dict:
    """{"route": the factorisation `sample_paths` takes for forests of R leaves and m trees ("blocked"), "max_leaves": its
    limit}; ValueError for a shape it refuses (bark_leaf_posterior_paths_plan).  Host only."""
    import ctypes

    route, limit = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().bark_leaf_posterior_paths_plan(int(R), int(m), ctypes.byref(route), ctypes.byref(limit)))
    return {"route": {1: "blocked"}[route.value], "max_leaves": int(limit.value)}


def path_list(forests, B: int, num_samples: int = 1):
    """The (forest, draw) pairs `sample_paths` takes, host only -> (forest (P,), draw (P,), order (P,)), int32 / int32 / int64.
    forests=None: num_samples paths of every forest, b-major.  Otherwise one path per entry, entry i taking the draw number
    equal to the count of earlier entries that name the same forest.  `order` sorts the paths by forest, stably: the device
    takes forest[order], and row j of its result is the caller's path order[j]."""
    if forests is None:
        S = int(num_samples)
        if S < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        forest = np.repeat(np.arange(B, dtype=np.int32), S)
        return forest, np.tile(np.arange(S, dtype=np.int32), B), np.arange(B * S, dtype=np.int64)
    f = np.asarray(forests)
    if f.ndim != 1 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("forests must be a non-empty 1-d array of ints")
    if f.min() < 0 or f.max() >= B:
        raise ValueError(f"forests must lie in [0, {B})")
    forest = f.astype(np.int32)
    order = np.argsort(forest, kind="stable").astype(np.int64)
    srt = forest[order]
    start = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
    run = np.repeat(start, np.diff(np.r_[start, srt.shape[0]]))
    draw = np.empty(forest.shape[0], dtype=np.int32)
    draw[order] = np.arange(srt.shape[0]) - run  # stable sort: the rank inside a forest's run is the count of earlier entries
    return forest, draw, order


class LeafPaths:
    """P posterior sample paths of a `LeafPosterior`: `forest` and `draw` (P,) name them, `W` (P, R, device, float64) holds
    their leaf weights in the caller's order, and `posterior` gives the packed forests they are evaluated under.  A path is
    the function f(x) = sum_t W[leaf_t(x)]; `evaluate` and `minimise` take any candidates, any number of times
    (bark_path_scan_hip).  Made by `LeafPosterior.sample_paths`."""

    def __init__(self, posterior, W_sorted, forest, draw, order):
        import torch

        self.posterior, self.forest, self.draw = posterior, forest, draw
        self._W, self._order = W_sorted, order
        self._sorted_forest = np.ascontiguousarray(forest[order])
        self._inverse = torch.from_numpy(np.argsort(order)).to(W_sorted.device)
        self.P = int(forest.shape[0])

    @property
    def W(self):
        return self._W[self._inverse]

    def subset(self, index) -> "LeafPaths":
        """The paths `index` (ints into the caller's order) as a LeafPaths of their own: same posterior, a copy of their rows."""
        import torch

        index = np.asarray(index, dtype=np.int64).reshape(-1)
        forest, draw = self.forest[index], self.draw[index]
        order = np.argsort(forest, kind="stable").astype(np.int64)
        rows = self._inverse[torch.from_numpy(index[order]).to(self._W.device)]
        return LeafPaths(self.posterior, self._W[rows].contiguous(), forest, draw, order)

    def _scan(self, candidates, reduce):
        import torch

        post = self.posterior
        if len(candidates) < 1:
            raise ValueError("a path scan needs at least one candidate")
        cand_d = _points(candidates, post.d)[0]
        C, P, dev = int(cand_d.shape[0]), self.P, self._W.device
        full = reduce == _lib.SAMPLE_FULL
        if full:
            from .tree_gps import _check_output_budget

            _check_output_budget(8 * P * C, f"evaluate: {P} paths at {C} candidates")
        f = torch.empty((P, C), dtype=torch.float64, device=dev) if full else None
        red = None if full else torch.empty(P, dtype=torch.float64, device=dev)
        idx = None if full else torch.empty(P, dtype=torch.int64, device=dev)
        info = torch.empty(post.B, dtype=torch.int32, device=dev)
        lib = _lib.lib()
        bad = np.zeros(post.B, dtype=bool)
        for p0 in range(0, P, MAX_PATHS_PER_CALL):
            n = min(MAX_PATHS_PER_CALL, P - p0)
            need = int(lib.bark_path_scan_workspace_bytes(post.R, post.m, n, C, reduce))
            if need == 0:
                raise ValueError(f"a path scan refuses the shape R = {post.R}, m = {post.m}, P = {n}, C = {C}")
            ws = _lib.workspace(need)
            _lib.check(lib.bark_path_scan_hip(
                _lib.ctx(), _lib.ptr(post.packed.packed), post.packed.info_ref, post.d, _lib.ptr(self._sorted_forest[p0:p0 + n]),
                _lib.ptr(self._W[p0:p0 + n]), n, _lib.ptr(cand_d), C, reduce, _lib.ptr(None if f is None else f[p0:p0 + n]),
                _lib.ptr(None if red is None else red[p0:p0 + n]), _lib.ptr(None if idx is None else idx[p0:p0 + n]),
                _lib.ptr(info), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
            bad |= info.cpu().numpy() != 0
        _raise_on_info(np.where(bad, -1, 0), "leaf-space system")
        inv = self._inverse
        return (f[inv],) if full else (red[inv], idx[inv])

    def evaluate(self, candidates):
        """-> (P, C) float64: every path at every candidate, the trees summed in the order t = 0..m-1 (bit for bit a host
        loop over the leaf weights).  numpy candidates give numpy, torch candidates a device tensor.  A path of a forest
        whose state is not positive definite is a NaN row.  Errors: those of `LeafPosterior.scan`; ValueError when the
        output exceeds the memory budget."""
        (f,) = self._scan(candidates, _lib.SAMPLE_FULL)
        return f if _is_torch(candidates) else f.cpu().numpy()

    def minimise(self, candidates, maximise: bool = False):
        """-> (values (P,), indices (P,) int64): each path's minimum (maximum) over the candidates, the bits `evaluate` gives,
        and its index, the lowest among equals; NaN and -1 for a NaN path.  No (P, C) array is formed."""
        red, idx = self._scan(candidates, _lib.SAMPLE_MAX if maximise else _lib.SAMPLE_MIN)
        return (red, idx) if _is_torch(candidates) else (red.cpu().numpy(), idx.cpu().numpy())
