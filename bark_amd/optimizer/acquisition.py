"""The acquisition of the reference's optimisation step over a candidate set, on the device.

The reference minimises the lower confidence bound of the fitted BARK model with a Gurobi model
(src/bark/optimizer/opt_model.py, proposals.py) and falls back to one random candidate when the solver fails
(bofire_mixed/strategies/tree_kernel.py:49-56).  Its end-to-end test defines the acquisition
(tests/optimization/test_optimality.py:60-63,100-108):

    acqf(x) = mean over forest samples b of ( mu_b(x) - kappa sqrt(var_b(x)) ),   mu, var = forest_predict(...)

and asks that the proposal be no worse than the minimum of acqf over random candidates.  `acquisition_scan` evaluates
acqf over C candidates and returns that minimum and its index from one call (bark_acquisition_scan_hip): the posterior
of every forest sample in leaf space, reduced over the samples in registers, never as (B, C) arrays.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np

from .. import _lib
from ..fitting.mll import _feat_types_of, _forest3, _leaf_call, _leaf_inputs
from ..forest import _is_torch, _points

KINDS = {"lcb_mean": _lib.ACQ_LCB_MEAN, "lcb_mixture": _lib.ACQ_LCB_MIXTURE, "ei": _lib.ACQ_EI, "pi": _lib.ACQ_PI,
         "mes": _lib.ACQ_MES}
TARGET_KINDS = ("ei", "pi", "mes")  # the utilities of (mu_b, sd_b, target): bark_acquisition_scan_targets_hip
VARIANTS = {"auto": 0, "lds": 1, "global": 2}
MAX_TREES, MAX_LEAVES = 64, 8192  # limits of the leaf-space posterior (include/bark_hip.h)
MAX_PENDING = MAX_SKIP = 64  # limits of bark_acquisition_scan_pending_hip
MAX_TARGETS = 1024  # ... of bark_acquisition_scan_targets_hip, per forest


def acquisition_plan(max_bits: int, m: int, variant: str = "auto") -> dict:
    """Which scan kernel a forest shape takes (R = max_bits leaves, m trees): {"variant": "lds" | "global",
    "lds_bytes": dynamic LDS of that launch}.  ValueError for a shape or a variant the entry point refuses.  Host code;
    no GPU needed."""
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
    v, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().bark_acquisition_plan(int(max_bits), int(m), VARIANTS[variant], ctypes.byref(v), ctypes.byref(nbytes)))
    return {"variant": ("lds", "global")[v.value - 1], "lds_bytes": int(nbytes.value)}


def _skip_indices(skip, C: int):
    """-> device int64 vector of the candidates to exclude, or None.  Host values are range-checked here; a device tensor
    is taken as it is (no read-back: entries outside [0, C) have no effect in the kernel)."""
    import torch

    if _is_torch(skip) and skip.is_cuda:
        t = skip.reshape(-1).to(torch.int64)
    else:
        arr = np.asarray(skip.cpu() if _is_torch(skip) else skip).reshape(-1)
        if arr.size and not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"skip must hold integer candidate indices, got dtype {arr.dtype}")
        if arr.size and (arr.min() < 0 or arr.max() >= C):
            raise ValueError(f"skip indices must lie in [0, {C})")
        t = _lib.to_device(arr.astype(np.int64))
    if t.numel() > MAX_SKIP:
        raise ValueError(f"at most {MAX_SKIP} candidates can be skipped (got {t.numel()})")
    return t.contiguous() if t.numel() else None


def _target_matrix(targets, B: int, kind: str, train_y):
    """-> (B, S) float64 targets, numpy or torch as given: a scalar is every forest's one target, (B,) one target per
    forest; None is the incumbent min(train_y) for "ei" / "pi".  Shapes are checked here, before anything needs a device."""
    if targets is None:
        if kind == "mes":
            raise ValueError("kind='mes' needs targets: draws of the minimum, e.g. from generate_fstar_samples")
        targets = train_y.min() if _is_torch(train_y) else np.min(np.asarray(train_y, dtype=np.float64))
    if _is_torch(targets):
        import torch

        t = targets.to(torch.float64)
        t = t.reshape(1, 1).expand(B, 1) if t.ndim == 0 else t.reshape(-1, 1) if t.ndim == 1 else t
    else:
        t = np.array(targets, dtype=np.float64)  # a copy: the caller's array may be read-only
        t = np.broadcast_to(t.reshape(1, 1), (B, 1)) if t.ndim == 0 else t.reshape(-1, 1) if t.ndim == 1 else t
    if t.ndim != 2 or t.shape[0] != B:
        raise ValueError(f"targets must be a scalar, ({B},) or ({B}, S): one row per forest (got shape {tuple(t.shape)})")
    if not 1 <= t.shape[1] <= MAX_TARGETS:
        raise ValueError(f"between 1 and {MAX_TARGETS} targets per forest (got {t.shape[1]})")
    return t


def _fitted(posterior, domain=None):
    """The `posterior=` argument of the functions below, checked: a `tree_kernels.LeafPosterior` (`fit_posterior`), whose
    feature types are those of `domain` when one is given too."""
    from ..tree_kernels.posterior import LeafPosterior

    if not isinstance(posterior, LeafPosterior):
        raise TypeError(f"posterior must be a LeafPosterior (tree_kernels.fit_posterior), got {type(posterior).__name__}")
    if domain is not None and not np.array_equal(_feat_types_of(domain), posterior.feat_types):
        raise ValueError("the domain's feature types are not those the posterior was fitted with")
    return posterior


def acquisition_scan(model, data, candidates, domain, kappa: float = 1.96, kind: str = "lcb_mean",
                     return_values: bool = False, chunk: int | None = None, variant: str = "auto", pending=None, skip=None,
                     targets=None, posterior=None):
    """-> (best_value, best_index[, acq (C,)]): the minimum over the candidates of the acquisition and its index (ties:
    the lowest index); with `return_values` also the acquisition of every candidate.

    model: the (forest, noise, scale) triple with leading dims flattened, data: (train_x, train_y), `domain` may be
    feat_types — as `forest_predict` takes them.  kind="lcb_mean": the reference's acqf above; kind="lcb_mixture":
    mu_mix - kappa sqrt(var_mix) with the moments of `mixture_of_gaussians_as_normal`.  variant: "auto", or "lds" /
    "global" to force the scan kernel that keeps a forest's M^-1 in LDS / reads it from global memory (`acquisition_plan`).

    kind="ei" | "pi" | "mes": expected improvement, probability of improvement and min-value entropy search (the
    reference's `information_gain` at the target fidelity, information_based_fidelity.py:39-87) below `targets`, each the
    mean over forests b and targets s of g(mu_b(x), sd_b(x), t[b][s]); include/bark_hip.h has the formulas.  The call
    returns the negated utility, so the minimum is the utility's maximiser; `kappa` is not used.  targets: a scalar, (B,)
    or (B, S <= 1024), numpy or torch (a device tensor is read where it is); None is the incumbent min(train_y) for "ei" and
    "pi", and refused for "mes", whose targets are draws of the minimum (`generate_fstar_samples`,
    `propose_mes_from_candidates`).  A NaN target gives NaN values and (NaN, -1).  The other kinds ignore `targets`.

    The sums run in a fixed order (a candidate's leaves in tree order, forests 0 .. B-1), so the result does not depend
    on `chunk` or `variant`, bit for bit.  At most 64 trees and 8192 leaves per forest.  Extra device memory is the
    leaf-space workspace of one chunk of forests plus 24 bytes per candidate, against 16 B C bytes of
    `forest_predict(method="leafspace")`.  Measured 3.6x (B = 4, C = 10^4) to 15x (B = 256, C = 10^6) faster than that
    route plus a torch reduction, and not slower at any shape measured; below 65 536 candidates
    the scan does not fill the device (one workgroup per 256 candidates) and the shared leaf-space sweep sets the time.

    pending: (P, d) points, numpy or torch, that are being evaluated already (P <= 64): every forest is conditioned on them
    as if each had been observed at the forest's own posterior mean ("kriging believer"), so mu_b is the mean given the
    real data and var_b the variance given the data and the pending points.  In leaf space that is one symmetric rank-one
    downdate of the R x R matrix M^-1 per point and forest (include/bark_hip.h has the algebra); they are applied in the
    order given, and two orders agree to rounding, not bit for bit.  skip: at most 64 candidate indices (sequence or
    tensor) that keep their value in `acq` but never win the minimum; with every candidate skipped the result is
    (NaN, -1).  With both None the call is the unconditioned scan, exactly as before.

    posterior: a `tree_kernels.LeafPosterior` (`fit_posterior(model, data, domain)`): the call is then its `scan` — the same
    scan from the fitted state, without the walk of the training points and the factorisation, bit for bit the result of this
    function at the `chunk` of the fit — and `model`, `data` and `domain` may be None.  Without it nothing changes.

    Torch candidates give device scalars (0-d tensors) and a device vector, numpy candidates a float, an int and a numpy
    vector.  ValueError for an invalid categorical value, LinAlgError for a forest whose leaf-space system is not positive
    definite; there is no CPU fallback (RuntimeError without a GPU)."""
    if posterior is not None:
        return _fitted(posterior, domain).scan(candidates, kappa=kappa, kind=kind, return_values=return_values, chunk=chunk,
                                               variant=variant, pending=pending, skip=skip, targets=targets)
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r} (use 'lcb_mean', 'lcb_mixture', 'ei', 'pi' or 'mes')")
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
    kappa = float(kappa)
    if not math.isfinite(kappa):
        raise ValueError(f"kappa must be finite, got {kappa}")
    forest, noise, scale = model
    train_x, train_y = data
    nodes3 = _forest3(forest)
    m = int(nodes3.shape[1])
    if m > MAX_TREES:
        raise ValueError(f"acquisition scan supports at most {MAX_TREES} trees (got {m})")
    if len(candidates) < 1:
        raise ValueError("acquisition scan needs at least one candidate")
    tgt = _target_matrix(targets, int(nodes3.shape[0]), kind, train_y) if kind in TARGET_KINDS else None

    import torch

    q = _leaf_inputs(nodes3, noise, scale, train_x, train_y, _feat_types_of(domain), candidates)
    C, R, dev = q.C, q.R, q.device
    if R > MAX_LEAVES:
        raise ValueError(f"acquisition scan supports at most {MAX_LEAVES} leaves per forest (got {R})")
    acquisition_plan(R, m, variant)  # refuses variant="lds" past the LDS limit before anything is allocated
    acq = torch.empty(C, dtype=torch.float64, device=dev) if return_values else None
    best = torch.empty((), dtype=torch.float64, device=dev)
    idx = torch.empty((), dtype=torch.int64, device=dev)
    lib = _lib.lib()
    if pending is None and skip is None and tgt is None:
        _leaf_call(q, lib.bark_acquisition_scan_hip, lambda k: int(lib.bark_acquisition_scan_workspace_bytes(q.N, R, q.pf.m, k, C)),
                   chunk, _lib.ptr(q.cand_d), C, kappa, KINDS[kind], VARIANTS[variant], _lib.ptr(acq), _lib.ptr(best), _lib.ptr(idx))
    else:
        pend_d = None if pending is None or len(pending) == 0 else _points(pending, q.d)[0]
        P = 0 if pend_d is None else int(pend_d.shape[0])
        if P > MAX_PENDING:
            raise ValueError(f"acquisition scan supports at most {MAX_PENDING} pending points (got {P})")
        skip_d = None if skip is None else _skip_indices(skip, C)
        shared = (_lib.ptr(q.cand_d), C, _lib.ptr(pend_d), P, _lib.ptr(skip_d), 0 if skip_d is None else int(skip_d.numel()))
        outs = (kappa, KINDS[kind], VARIANTS[variant], _lib.ptr(acq), _lib.ptr(best), _lib.ptr(idx))
        if tgt is None:
            _leaf_call(q, lib.bark_acquisition_scan_pending_hip,
                       lambda k: int(lib.bark_acquisition_scan_pending_workspace_bytes(q.N, R, q.pf.m, k, C, P)), chunk,
                       *shared, *outs)
        else:
            tgt_d = _lib.to_device(tgt, torch.float64)
            _leaf_call(q, lib.bark_acquisition_scan_targets_hip,
                       lambda k: int(lib.bark_acquisition_scan_targets_workspace_bytes(q.N, R, q.pf.m, k, C, P)), chunk,
                       *shared, _lib.ptr(tgt_d), int(tgt_d.shape[1]), *outs)
    if _is_torch(candidates):
        return (best, idx, acq) if return_values else (best, idx)
    out = (float(best.item()), int(idx.item()))
    return (*out, acq.cpu().numpy()) if return_values else out


def propose_from_candidates(model, data, candidates, domain, kappa: float = 1.96, kind: str = "lcb_mean",
                            chunk: int | None = None, variant: str = "auto", targets=None, posterior=None):
    """The candidate row that minimises the acquisition (`acquisition_scan`): what the reference's `propose` returns when
    its search space is the given candidate set, and a better stand-in than its single random candidate when no solver is
    available.  `targets`: those of kind "ei" / "pi" / "mes"; `posterior`: as in `acquisition_scan`.  Torch candidates give a
    device row (the index is not read back), numpy candidates a numpy row."""
    _, idx = acquisition_scan(model, data, candidates, domain, kappa=kappa, kind=kind, chunk=chunk, variant=variant,
                              targets=targets, posterior=posterior)
    if _is_torch(candidates):
        return candidates.index_select(0, idx.to(candidates.device).reshape(1))[0]
    return np.asarray(candidates)[idx]


def propose_batch_from_candidates(model, data, candidates, domain, q: int, kappa: float = 1.96, kind: str = "lcb_mean",
                                  pending=None, chunk: int | None = None, variant: str = "auto", targets=None, posterior=None,
                                  fantasy="mean", seed: int = 0):
    """-> (rows (q, d), indices (q,)): q distinct candidate rows chosen greedily.  Pick k is the arg-min of the scan
    conditioned on `pending` followed by picks 0 .. k-1 (`acquisition_scan(pending=..., skip=...)`), with those picks
    excluded: a point that is being evaluated no longer attracts the next one, because its variance has collapsed.
    With kind="ei" that is a greedy expected-improvement batch under the kriging believer; `targets` are the same for every pick.

    Without `posterior` a plain loop of q scans with no state kept between the picks, so the cost is q times one scan, and
    pick k replays the P + k downdates before it.  With a `tree_kernels.LeafPosterior` (`model`, `data` and `domain` may be
    None) a private copy of its state is conditioned once on `pending` and once on every pick (`LeafPosterior.condition_`),
    and the scans pass only the picks to skip: nothing is refitted, one downdate per forest and pick, the same rows and indices.
    Torch candidates give device tensors (a pick is gathered with index_select; no index is read back), numpy candidates
    numpy arrays.  ValueError for q < 1, q > C or P + q - 1 > 64 (the scan's limit on pending points), on both routes.

    fantasy: what a point in flight is taken to return.  "mean" (the default, everything above): each forest's own posterior
    mean, the kriging believer.  A float: that constant for every forest, the constant liar (`min(y)` and `mean(y)` are the
    usual ones).  "sample": a draw from each forest's own predictive (`LeafPosterior.fantasise`), pick k with the draw number
    k and the initial `pending` points with the draw number q, all under `seed` — over kind="ei" the usual Monte-Carlo
    batch.  The pending points take the same fantasy as the picks.  The last two move w as well as M^-1, which only a fitted
    state can do: they need `posterior=` (ValueError otherwise)."""
    if isinstance(fantasy, str):
        if fantasy not in ("mean", "sample"):
            raise ValueError(f"unknown fantasy {fantasy!r} (use 'mean', 'sample' or a float)")
    else:
        fantasy = float(fantasy)
        if not math.isfinite(fantasy):
            raise ValueError(f"a constant fantasy must be finite, got {fantasy}")
    if fantasy != "mean" and posterior is None:
        raise ValueError("fantasy other than 'mean' needs a fitted state: pass posterior=fit_posterior(model, data, domain)")
    C = len(candidates)
    q = int(q)
    P = 0 if pending is None else len(pending)
    if q < 1 or q > C:
        raise ValueError(f"q must lie in [1, {C}] (the number of candidates), got {q}")
    if P + q - 1 > MAX_PENDING:
        raise ValueError(f"pending points plus earlier picks exceed {MAX_PENDING} (P = {P}, q = {q})")
    on_device = _is_torch(candidates)
    if on_device:
        import torch

        pend = None if P == 0 else torch.as_tensor(pending, dtype=candidates.dtype, device=candidates.device)
    else:
        candidates = np.asarray(candidates)
        pend = None if P == 0 else np.asarray(pending.cpu() if _is_torch(pending) else pending, dtype=np.float64)
    rows, picks = [], []
    if posterior is not None:
        def fantasised(post, points, draw):
            if fantasy == "sample":
                post._fantasise_(points, seed, draw)
            else:
                post.condition_(points, None if fantasy == "mean" else fantasy)

        post = _fitted(posterior, domain)._copy()  # also when there is nothing to condition on
        if pend is not None:
            fantasised(post, pend, q)
        for k in range(q):
            skip = None if not picks else torch.stack(picks) if on_device else picks
            _, idx = post.scan(candidates, kappa=kappa, kind=kind, chunk=chunk, variant=variant, skip=skip, targets=targets)
            if on_device:
                idx = idx.to(candidates.device)
                rows.append(candidates.index_select(0, idx.reshape(1))[0])
            else:
                rows.append(candidates[idx])
            picks.append(idx)
            if k + 1 < q:
                fantasised(post, rows[-1].reshape(1, -1), k)
        if on_device:
            return torch.stack(rows), torch.stack(picks)
        return np.stack(rows), np.asarray(picks, dtype=np.int64)
    for _ in range(q):
        if on_device:
            cur = pend if not rows else torch.cat(([] if pend is None else [pend]) + [torch.stack(rows)])
            skip = torch.stack(picks) if picks else None
        else:
            cur = pend if not rows else np.concatenate(([] if pend is None else [pend]) + [np.stack(rows)])
            skip = picks or None
        _, idx = acquisition_scan(model, data, candidates, domain, kappa=kappa, kind=kind, chunk=chunk, variant=variant,
                                  pending=cur, skip=skip, targets=targets)
        if on_device:
            idx = idx.to(candidates.device)
            rows.append(candidates.index_select(0, idx.reshape(1))[0])
        else:
            rows.append(candidates[idx])
        picks.append(idx)
    if on_device:
        return torch.stack(rows), torch.stack(picks)
    return np.stack(rows), np.asarray(picks, dtype=np.int64)


def propose_mes_from_candidates(model, data, candidates, domain, num_samples: int = 100, generator=None,
                                chunk: int | None = None, variant: str = "auto", pending=None, skip=None, posterior=None,
                                seed: int = 0, return_info: bool = False):
    """The candidate row with the largest information gain about the minimum value: the workflow of the reference's
    `propose_fidelity_information_based` (information_based_fidelity.py:16-36) with a candidate set in place of its single x.
    `generate_fstar_samples` draws num_samples joint posterior samples per forest at the training inputs and keeps their
    minima, (B, num_samples) on the device; `acquisition_scan(kind="mes", targets=...)` scores every candidate against
    them and returns the arg-min of the negated gain.  generator: a torch.Generator, an int seed or None, as
    `generate_fstar_samples` takes it.  posterior: as in `acquisition_scan`, for the scan.  Torch candidates give a device
    row (the index is not read back), numpy candidates a numpy row.

    With a posterior and model or data None, everything comes from the state: the minima are those of
    `posterior.sample_paths(num_samples, seed=seed)` over the candidates (`LeafPaths.minimise`), (B, num_samples) as
    `fstar_at_fidelity` arranges them, so after `observe_` the draws follow the observations and no model or data is needed.
    A forest of weight 0 whose draws are not finite gets zeros: the scan skips it.  `generator` is not used then.
    return_info: also {"index", "value", "targets"}, the scan's arg-min, its value and the (B, num_samples) minima."""
    import torch

    from .thompson_sampling import generate_fstar_samples

    if model is None or data is None:
        from ..tree_kernels.posterior import LeafPosterior

        if not isinstance(posterior, LeafPosterior):
            raise ValueError("propose_mes_from_candidates draws the minima from model and data, or from a LeafPosterior passed as posterior")
        post = _fitted(posterior, domain)
        values, _ = post.sample_paths(int(num_samples), seed=seed).minimise(_points(candidates, post.d)[0])
        fstar = values.reshape(post.B, int(num_samples))
        if post.log_weights is not None:
            dead = (post.weights == 0)[:, None] & ~torch.isfinite(fstar)
            fstar = torch.where(dead, torch.zeros_like(fstar), fstar)
        value, idx = post.scan(candidates, kind="mes", targets=fstar, chunk=chunk, variant=variant, pending=pending, skip=skip)
        row = candidates.index_select(0, idx.to(candidates.device).reshape(1))[0] if _is_torch(candidates) else np.asarray(candidates)[idx]
        return (row, {"index": idx, "value": value, "targets": fstar}) if return_info else row
    train_x, train_y = data
    # torch inputs keep the minima on the device between the two calls
    site_x = train_x if _is_torch(train_x) else torch.as_tensor(np.asarray(train_x, dtype=np.float64), device=_lib.torch_device())
    fstar = generate_fstar_samples(model, (site_x, train_y), domain, num_samples=num_samples, generator=generator)
    _, idx = acquisition_scan(model, data, candidates, domain, kind="mes", targets=fstar, chunk=chunk, variant=variant,
                              pending=pending, skip=skip, posterior=posterior)
    if _is_torch(candidates):
        return candidates.index_select(0, idx.to(candidates.device).reshape(1))[0]
    return np.asarray(candidates)[idx]
