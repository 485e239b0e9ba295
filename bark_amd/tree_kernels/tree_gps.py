"""Drop-in for the numpy part of `bark.tree_kernels.tree_gps`
(reference: src/bark/tree_kernels/tree_gps.py:80-131).

`forest_predict` runs one fused device sweep per chunk of forest samples: Gram(X,X), Gram(X,cand),
blocked Cholesky with the candidate block appended as extra columns (V = U^-T K_Xx), then
mu = V'z and var = scale - colsumsq(V).  The reference's `diag=False` full (B, C, C) covariance is
formed only on request (scale - V'V, one more MFMA product), from the same V.  The gpytorch `LeafGP`/`LeafMOGP` classes of
the reference are out of scope.

`posterior_samples` draws joint samples of the latent function at candidates from the leaf-space posterior of the
leaf weights (bark_posterior_samples_hip), with the true covariance scale K_CC - K_CX K_s^-1 K_XC.  The reference's
samplers (`bark.optimizer.thompson_sampling`, `nystrom`, `information_based_fidelity`) sit on a gpytorch model that
no longer exists; `bark_amd.optimizer.thompson_sampling` builds on this one.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from .. import _lib
from ..fitting.mll import _feat_types_of, _forest3, _hbm_budget, _leaf_call, _leaf_inputs, _run, _run_leafspace
from ..forest import _feat_types, _is_torch


class BARKModel(NamedTuple):
    """tree_gps.py:14-17 — the (forest, noise, scale) triple `forest_predict` and `mll` take; leading dims
    (chains, samples) of all three are flattened by the callees."""

    forest: np.ndarray
    noise: np.ndarray
    scale: np.ndarray


def forest_predict(model, data, candidates, domain, diag: bool = True, method: str = "dense", posterior=None):
    """tree_gps.py:80-113 -> (mu (B, C), var (B, C) or (B, C, C) if not diag); `domain` may be feat_types.

    method="dense" (default) follows the reference's computation (Gram, factorisation of the N x N matrix);
    method="leafspace" (diag only, <= 64 trees) evaluates the same posterior in closed form over the forest's
    leaves: mu = c sum_{a in L(x)} w_a, var = (scale/m) sum_{a,b in L(x)} (M^-1)_ab — see include/bark_hip.h.

    posterior: a `LeafPosterior` (`fit_posterior`) to read instead of refitting: -> the "forest_mean" and "forest_var" of
    `posterior.predict(candidates, per_forest=True, weights="equal")`, the state as it is now.  `model`, `data` and `domain`
    may then be None; diag=True and the default method only (ValueError otherwise)."""
    if posterior is not None:
        if not diag or method != "dense":
            raise ValueError("forest_predict(posterior=...) provides the diagonal posterior only, by the state's own method")
        out = posterior.predict(candidates, per_forest=True, weights="equal")
        return out["forest_mean"], out["forest_var"]
    forest, noise, scale = model
    train_x, train_y = data
    forest = np.asarray(forest)
    noise = np.asarray(noise, dtype=np.float64).reshape(-1)   # tree_gps.py:88-90 flatten
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    flags = _lib.MLL_INCLUDE_SCALE
    if method == "leafspace":
        if not diag:
            raise ValueError("method='leafspace' provides the diagonal posterior only")
        _, mu, var = _run_leafspace(forest, noise, scale, train_x, train_y, _feat_types_of(domain), flags, cand=candidates)
    elif method != "dense":
        raise ValueError(f"unknown method {method!r} (use 'dense' or 'leafspace')")
    elif diag:
        _, mu, var = _run(forest, noise, scale, train_x, train_y, _feat_types_of(domain), flags, cand=candidates)
    else:  # tree_gps.py:108: full (B, C, C) covariance scale - K_xX K^-1 K_Xx (one extra MFMA V'V product)
        _, mu, _, var = _run(forest, noise, scale, train_x, train_y, _feat_types_of(domain), flags, cand=candidates,
                             want_cov=True)
    if _is_torch(candidates):
        return mu, var
    return mu.cpu().numpy(), var.cpu().numpy()


def mixture_of_gaussians_as_normal(mu, var):
    """tree_gps.py:116-131: moments of the equal-weight mixture over forest samples.
    (B x C elementwise host arithmetic, as in the reference; works on numpy or torch.)"""
    if _is_torch(mu):
        import torch

        # the HIP reduction reads raw contiguous (B, C) float64 pairs; anything else — float32, a full (B, C, C)
        # covariance from diag=False, broadcasting shapes — takes the reference's formula in torch, by dtype and shape
        if (mu.is_cuda and _is_torch(var) and var.is_cuda and mu.dtype == torch.float64 and var.dtype == torch.float64
                and mu.ndim == 2 and var.shape == mu.shape):
            from ..distributed import reduce_mixture

            return reduce_mixture(mu, var, int(mu.shape[0]), group=False)
        mu_y = mu.mean(dim=0)
        var_y = (var + mu**2).mean(dim=0) - mu_y**2
        return mu_y, var_y
    mu_y = np.mean(mu, axis=0)
    var_y = np.mean(var + mu**2, axis=0) - mu_y**2
    return mu_y, var_y


_REDUCE = {None: _lib.SAMPLE_FULL, "max": _lib.SAMPLE_MAX, "min": _lib.SAMPLE_MIN}
MAX_SAMPLE_TREES, MAX_SAMPLE_LEAVES = 64, 8192  # limits of the leaf-space posterior (include/bark_hip.h)


def posterior_sample_dim(forest, domain) -> int:
    """R, the width of the draws' `eps` (B, S, R): max_bits of the packed forest samples (the one-hot leaf-code width).
    Host-side packer query; no GPU needed."""
    nodes3 = _forest3(forest)
    ft = _feat_types(_feat_types_of(domain))
    info = _lib.PackInfo()
    B, m, L = nodes3.shape
    _lib.check(_lib.lib().bark_forest_pack_info(_lib.ptr(nodes3), B, m, L, _lib.ptr(ft), ft.shape[0], ctypes.byref(info)))
    return int(info.max_bits)


def _check_output_budget(nbytes: int, what: str):
    """Refuse outputs larger than the HBM budget `_fit_chunk` works with (`_hbm_budget`): unlike the workspace they
    cannot be chunked."""
    budget = _hbm_budget(nbytes)
    if budget is not None and nbytes > budget:
        raise ValueError(f"{what} needs {nbytes / 2**30:.2f} GiB, more than the {budget / 2**30:.2f} GiB budget: "
                         "use reduce='max' / reduce='min' or fewer draws")


def posterior_samples(model, data, candidates, domain, num_samples, *, generator=None, eps=None, reduce=None, chunk=None):
    """Joint draws of the latent function (no observation noise) at the candidates, per forest sample.

    model: the (forest, noise, scale) triple with leading dims flattened, as in `forest_predict`; `domain` may be
    feat_types.  In leaf space (<= 64 trees, R <= 8192 leaves) the leaf weights have the posterior
    W ~ N(c w, (scale/m) M^-1), so draw s of forest b is  f = c Z_C w + sqrt(scale/m) Z_C U^-1 eps[b, s]  with
    M = U'U (include/bark_hip.h).  Its covariance is scale K_CC - K_CX K_s^-1 K_XC; `forest_predict(diag=False)`
    keeps the reference's formula (scale 11' - ...) for parity and is not this covariance.

    eps: (B, num_samples, R) standard normals (R = `posterior_sample_dim`), or None to draw them with one
    `torch.randn` call on the device from `generator` (a torch.Generator, an int seed, or None: torch's default).
    Returns (B, S, C) float64; with reduce="max" | "min" the pair (values (B, S), indices (B, S) int64) over the
    candidates (ties: the lowest index).  Torch candidates give device tensors, numpy candidates numpy arrays."""
    import torch

    if reduce not in _REDUCE:
        raise ValueError(f"unknown reduce {reduce!r} (use None, 'max' or 'min')")
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    forest, noise, scale = model
    train_x, train_y = data
    nodes3 = _forest3(forest)
    if nodes3.shape[1] > MAX_SAMPLE_TREES:
        raise ValueError(f"leaf-space posterior samples support at most {MAX_SAMPLE_TREES} trees (got {nodes3.shape[1]})")
    q = _leaf_inputs(nodes3, noise, scale, train_x, train_y, _feat_types_of(domain), candidates)
    B, C, R, dev = q.B, q.C, q.R, q.device
    if R > MAX_SAMPLE_LEAVES:
        raise ValueError(f"leaf-space posterior samples support at most {MAX_SAMPLE_LEAVES} leaves per forest (got {R})")
    if eps is not None and tuple(eps.shape) != (B, S, R):
        raise ValueError(f"eps must have shape (B, num_samples, R) = {(B, S, R)}, got {tuple(eps.shape)}")
    code = _REDUCE[reduce]
    out_bytes = 8 * B * S * C if code == _lib.SAMPLE_FULL else 16 * B * S
    _check_output_budget(out_bytes + (8 * B * S * R if eps is None else 0),
                         "the full (B, S, C) output" if code == _lib.SAMPLE_FULL else "eps (B, S, R)")
    if eps is None:
        gen = generator
        if isinstance(generator, (int, np.integer)):
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(generator))
        eps_d = torch.randn((B, S, R), dtype=torch.float64, device=dev, generator=gen)
    else:
        eps_d = _lib.to_device(eps.detach() if _is_torch(eps) else np.asarray(eps, dtype=np.float64)).to(torch.float64)
        eps_d = eps_d.contiguous()
    if code == _lib.SAMPLE_FULL:
        f = torch.empty((B, S, C), dtype=torch.float64, device=dev)
        red = idx = None
    else:
        f = None
        red = torch.empty((B, S), dtype=torch.float64, device=dev)
        idx = torch.empty((B, S), dtype=torch.int64, device=dev)
    lib = _lib.lib()
    _leaf_call(q, lib.bark_posterior_samples_hip,
               lambda k: int(lib.bark_posterior_samples_workspace_bytes(q.N, R, q.pf.m, k, C, S)), chunk,
               _lib.ptr(q.cand_d), C, _lib.ptr(eps_d), S, code, _lib.ptr(f), _lib.ptr(red), _lib.ptr(idx))
    on_device = _is_torch(candidates)
    if code == _lib.SAMPLE_FULL:
        return f if on_device else f.cpu().numpy()
    return (red, idx) if on_device else (red.cpu().numpy(), idx.cpu().numpy())
