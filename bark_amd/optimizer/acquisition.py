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
from ..fitting.mll import _feat_types_of, _fit_chunk, _raise_on_info
from ..forest import _as_nodes, _feat_types, _is_torch, _points, packed_forest

KINDS = {"lcb_mean": _lib.ACQ_LCB_MEAN, "lcb_mixture": _lib.ACQ_LCB_MIXTURE}
VARIANTS = {"auto": 0, "lds": 1, "global": 2}
MAX_TREES, MAX_LEAVES = 64, 8192  # limits of the leaf-space posterior (include/bark_hip.h)


def acquisition_plan(max_bits: int, m: int, variant: str = "auto") -> dict:
    """Which scan kernel a forest shape takes (R = max_bits leaves, m trees): {"variant": "lds" | "global",
    "lds_bytes": dynamic LDS of that launch}.  ValueError for a shape or a variant the entry point refuses.  Host code;
    no GPU needed."""
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
    v, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().bark_acquisition_plan(int(max_bits), int(m), VARIANTS[variant], ctypes.byref(v), ctypes.byref(nbytes)))
    return {"variant": ("lds", "global")[v.value - 1], "lds_bytes": int(nbytes.value)}


def acquisition_scan(model, data, candidates, domain, kappa: float = 1.96, kind: str = "lcb_mean",
                     return_values: bool = False, chunk: int | None = None, variant: str = "auto"):
    """-> (best_value, best_index[, acq (C,)]): the minimum over the candidates of the acquisition and its index (ties:
    the lowest index); with `return_values` also the acquisition of every candidate.

    model: the (forest, noise, scale) triple with leading dims flattened, data: (train_x, train_y), `domain` may be
    feat_types — as `forest_predict` takes them.  kind="lcb_mean": the reference's acqf above; kind="lcb_mixture":
    mu_mix - kappa sqrt(var_mix) with the moments of `mixture_of_gaussians_as_normal`.  variant: "auto", or "lds" /
    "global" to force the scan kernel that keeps a forest's M^-1 in LDS / reads it from global memory (`acquisition_plan`).

    The sums run in a fixed order (a candidate's leaves in tree order, forests 0 .. B-1), so the result does not depend
    on `chunk` or `variant`, bit for bit.  At most 64 trees and 8192 leaves per forest.  Extra device memory is the
    leaf-space workspace of one chunk of forests plus 24 bytes per candidate, against 16 B C bytes of
    `forest_predict(method="leafspace")`.  Measured 3.6x (B = 4, C = 10^4) to 15x (B = 256, C = 10^6) faster than that
    route plus a torch reduction, and not slower at any shape measured; below 65 536 candidates
    the scan does not fill the device (one workgroup per 256 candidates) and the shared leaf-space sweep sets the time.

    Torch candidates give device scalars (0-d tensors) and a device vector, numpy candidates a float, an int and a numpy
    vector.  ValueError for an invalid categorical value, LinAlgError for a forest whose leaf-space system is not positive
    definite; there is no CPU fallback (RuntimeError without a GPU)."""
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r} (use 'lcb_mean' or 'lcb_mixture')")
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (use 'auto', 'lds' or 'global')")
    kappa = float(kappa)
    if not math.isfinite(kappa):
        raise ValueError(f"kappa must be finite, got {kappa}")
    forest, noise, scale = model
    train_x, train_y = data
    nodes = _as_nodes(forest, 2)
    nodes3 = nodes.reshape(-1, *nodes.shape[-2:])
    ft = _feat_types(_feat_types_of(domain))
    B, m = int(nodes3.shape[0]), int(nodes3.shape[1])
    if m > MAX_TREES:
        raise ValueError(f"acquisition scan supports at most {MAX_TREES} trees (got {m})")
    noise = np.ascontiguousarray(np.asarray(noise, dtype=np.float64).reshape(-1))
    scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
    if noise.shape[0] != B or scale.shape[0] != B:
        raise ValueError(f"noise/scale must have one entry per forest ({B})")
    if len(candidates) < 1:
        raise ValueError("acquisition scan needs at least one candidate")

    import torch

    lib = _lib.lib()
    _lib.torch_device()  # RuntimeError without a GPU: no CPU fallback
    Xd, _ = _points(train_x, ft.shape[0])
    N, d = Xd.shape
    dev = Xd.device
    yd = _lib.to_device(train_y.detach() if _is_torch(train_y) else np.asarray(train_y, dtype=np.float64))
    yd = yd.to(torch.float64).reshape(-1).contiguous()
    if yd.shape[0] != N:
        raise ValueError(f"y has {yd.shape[0]} rows, X has {N}")
    cand_d, _ = _points(candidates, ft.shape[0])
    C = int(cand_d.shape[0])
    pf = packed_forest(nodes3, ft)
    R = int(pf.info.max_bits)
    if R > MAX_LEAVES:
        raise ValueError(f"acquisition scan supports at most {MAX_LEAVES} leaves per forest (got {R})")
    acquisition_plan(R, m, variant)  # refuses variant="lds" past the LDS limit before anything is allocated
    noise_d, scale_d = _lib.to_device(noise), _lib.to_device(scale)
    acq = torch.empty(C, dtype=torch.float64, device=dev) if return_values else None
    best = torch.empty((), dtype=torch.float64, device=dev)
    idx = torch.empty((), dtype=torch.int64, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    need = lambda k: int(lib.bark_acquisition_scan_workspace_bytes(N, R, pf.m, k, C))  # noqa: E731
    Bc = int(chunk) if chunk else _fit_chunk(B, need)
    ws = _lib.workspace(need(Bc))
    _lib.check(lib.bark_acquisition_scan_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), N, d, _lib.ptr(yd),
                                             _lib.ptr(noise_d), _lib.ptr(scale_d), _lib.ptr(cand_d), C, kappa, KINDS[kind],
                                             VARIANTS[variant], _lib.ptr(acq), _lib.ptr(best), _lib.ptr(idx), _lib.ptr(info),
                                             _lib.ptr(ws), ws.numel(), Bc, _lib.stream_ptr()))
    _raise_on_info(info, "leaf-space system")
    if _is_torch(candidates):
        return (best, idx, acq) if return_values else (best, idx)
    out = (float(best.item()), int(idx.item()))
    return (*out, acq.cpu().numpy()) if return_values else out


def propose_from_candidates(model, data, candidates, domain, kappa: float = 1.96, kind: str = "lcb_mean",
                            chunk: int | None = None, variant: str = "auto"):
    """The candidate row that minimises the acquisition (`acquisition_scan`): what the reference's `propose` returns when
    its search space is the given candidate set, and a better stand-in than its single random candidate when no solver is
    available.  Torch candidates give a device row (the index is not read back), numpy candidates a numpy row."""
    _, idx = acquisition_scan(model, data, candidates, domain, kappa=kappa, kind=kind, chunk=chunk, variant=variant)
    if _is_torch(candidates):
        return candidates.index_select(0, idx.to(candidates.device).reshape(1))[0]
    return np.asarray(candidates)[idx]
