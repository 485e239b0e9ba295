"""Tree proposals of the sampler on the device (reference: src/bark/fitting/tree_proposals.py:187-256 `get_tree_proposal`).

`propose_trees` draws a grow / prune / change proposal for every tree of every chain in ONE launch (csrc/propose.hip) and
returns what `ChainBatch.sweep_trees` / `LeafChainBatch.sweep_trees` take.  The random stream is Philox4x32-10 addressed by
(seed, sweep, chain, tree) — include/bark_hip.h has the draw layout — so a proposal does not depend on the batch it is drawn in.
Not the reference's stream: numba's generator state cannot be addressed that way.

Deviations from the reference: a container without two inactive slots (the reference raises
OverflowError) and a grow beyond `max_leaves` are rejected proposals (status 3 and 4), i.e. the chain samples the depth prior
truncated to the container and to max_leaves.  No CPU path: outside its limits the call raises ValueError."""

from __future__ import annotations

import ctypes
from enum import Enum

import numpy as np

from .. import _lib
from ..forest import NODE_RECORD_DTYPE, FeatureTypeEnum, _as_nodes, _feat_types, _is_torch

STATUS = ("valid", "no valid node", "invalid discrete split", "no two inactive slots", "max_leaves")


class TreeProposalEnum(Enum):  # tree_proposals.py:39-42
    Grow = 0
    Prune = 1
    Change = 2


class ProposalParams(ctypes.Structure):
    """bark_proposal_params (include/bark_hip.h)."""
    _fields_ = [("alpha", ctypes.c_double), ("beta", ctypes.c_double), ("weights", ctypes.c_double * 3),
                ("max_leaves", ctypes.c_int64), ("chain_offset", ctypes.c_int64), ("tree_offset", ctypes.c_int64)]


class TreeProposalsPlan(ctypes.Structure):
    """bark_tree_proposals_plan (include/bark_hip.h)."""
    _fields_ = [("nodes_bytes", ctypes.c_int64)] + [
        (n, ctypes.c_int32) for n in ("max_slots", "max_features", "max_proposals", "threads", "workgroups")]


def tree_proposals_plan(L: int, d: int, max_leaves: int, nc: int, m: int) -> dict:
    """`bark_tree_proposals_query`: the limits ("max_slots" 256, "max_features" 2^20, "max_proposals" 2^22 per launch), the launch
    shape and "reason": "" or why the shape is refused.  No GPU needed."""
    plan = TreeProposalsPlan()
    lib = _lib.lib()
    rc = lib.bark_tree_proposals_query(L, d, max_leaves, nc, m, ctypes.byref(plan))
    out = {name: int(getattr(plan, name)) for name, _ in TreeProposalsPlan._fields_}
    out["reason"] = "" if rc == 0 else lib.bark_last_error().decode(errors="replace")
    return out


def check_bounds(bounds, feat_types):
    """bounds (d, 2) float64 in the reference's bitmask encoding, feat_types (d,) int64.  Integer bounds and category masks must
    be exact in float32 (|value| <= 2^24): thresholds are stored as float32."""
    ft = _feat_types(feat_types)
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64))
    if b.shape != (ft.shape[0], 2):
        raise ValueError(f"bounds must be ({ft.shape[0]}, 2), got {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError("bounds must be finite")
    if not np.isin(ft, [e.value for e in FeatureTypeEnum]).all():
        raise ValueError("feat_types must hold FeatureTypeEnum values")
    discrete = ft != FeatureTypeEnum.Cont.value
    if (np.abs(b[discrete]) > 2.0 ** 24).any() or (b[discrete] != np.trunc(b[discrete])).any():
        raise ValueError("integer bounds and category masks must be whole numbers of at most 2^24")
    if (b[ft == FeatureTypeEnum.Cat.value] < 0).any():
        raise ValueError("a category mask is negative")
    if (b[:, 0] > b[:, 1])[ft != FeatureTypeEnum.Cat.value].any():
        raise ValueError("a lower bound exceeds its upper bound")
    return b, ft


def proposal_params(params, max_leaves: int, chain_offset: int = 0, tree_offset: int = 0) -> ProposalParams:
    """The C struct from any object with alpha, beta and proposal_weights (`BARKTrainParams`)."""
    w = np.asarray(params.proposal_weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != 3:
        raise ValueError("proposal_weights must hold three weights: grow, prune, change")
    return ProposalParams(float(params.alpha), float(params.beta), (ctypes.c_double * 3)(*w), int(max_leaves), int(chain_offset),
                          int(tree_offset))


def records_to_device(forests):
    """(chains, m, node_limit) records -> their bytes as a (chains, m, node_limit * 26) uint8 device tensor."""
    nodes = _as_nodes(forests, 3)
    if nodes.ndim != 3:
        raise ValueError(f"forests must be (chains, m, node_limit) records, got {nodes.shape}")
    return _lib.to_device(nodes.view(np.uint8).reshape(nodes.shape[0], nodes.shape[1], -1))


def records_from_device(t) -> np.ndarray:
    """The inverse of `records_to_device` (one read-back)."""
    a = t.cpu().numpy()
    return np.ascontiguousarray(a).view(NODE_RECORD_DTYPE).reshape(a.shape[0], a.shape[1], -1)


def propose_trees_device(nodes_d, bounds_d, ft_d, cparams: ProposalParams, seed: int, sweep: int):
    """The launch alone, device tensors in and out: nodes_d (chains, m, node_limit * 26) uint8 -> (new_nodes, log_q_prior,
    log_u, detail).  Allocates its outputs; enqueues on the current stream without synchronising."""
    import torch

    nc, m, nbytes = (int(v) for v in nodes_d.shape)
    L = nbytes // 26
    if nodes_d.dtype != torch.uint8 or nbytes != 26 * L or not nodes_d.is_contiguous():
        raise ValueError("nodes must be a contiguous (chains, m, node_limit * 26) uint8 tensor")
    dev = nodes_d.device
    new_d = torch.empty_like(nodes_d)
    lq = torch.empty((nc, m), dtype=torch.float64, device=dev)
    lu = torch.empty((nc, m), dtype=torch.float64, device=dev)
    detail = torch.empty((nc, m, 4), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().bark_tree_proposals_hip(_lib.ctx(), _lib.ptr(nodes_d), nc, m, L, _lib.ptr(bounds_d), _lib.ptr(ft_d),
                                                  int(ft_d.shape[0]), ctypes.byref(cparams), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                  int(sweep), _lib.ptr(new_d), _lib.ptr(lq), _lib.ptr(lu), _lib.ptr(detail),
                                                  _lib.stream_ptr()))
    return new_d, lq, lu, detail


def commit_trees_device(nodes_d, new_d, accept_d, tree_index_d):
    """nodes[c, tree_index[t]] <- new_nodes[c, tree_index[t]] wherever accept[t, c] > 0, on the device: accept_d is the (steps,
    chains) int32 tensor a sweep wrote, tree_index_d (steps,) int64."""
    nc, m, nbytes = (int(v) for v in nodes_d.shape)
    _lib.check(_lib.lib().bark_tree_proposals_commit_hip(_lib.ptr(nodes_d), _lib.ptr(new_d), _lib.ptr(accept_d), _lib.ptr(tree_index_d),
                                                         int(tree_index_d.shape[0]), nc, m, nbytes // 26, _lib.stream_ptr()))


def propose_trees(forests, bounds, feat_types, params, *, seed: int, sweep: int, max_leaves=None, return_device: bool = False,
                  chain_offset: int = 0, tree_offset: int = 0):
    """A proposal for every tree: forests (chains, m, node_limit) records (numpy, or their bytes as a (chains, m, node_limit * 26)
    uint8 device tensor), bounds (d, 2) in the reference's bitmask encoding, params with alpha, beta and proposal_weights
    -> (new_trees (chains, m, node_limit) records, log_q_prior (chains, m), log_u (chains, m), detail (chains, m, 4) int32:
    kind, node, feature, status — `STATUS`).  Pass the first three to `sweep_trees` with old_trees = forests.  max_leaves: a grow
    beyond it is rejected (default: the container admits any).  chain_offset / tree_offset shift the stream's address, so a
    slice of a batch draws what the whole batch draws.  return_device=True returns the four device tensors (new_trees as
    bytes) without a read-back."""
    b, ft = check_bounds(bounds, feat_types)
    nodes_d = forests if _is_torch(forests) else records_to_device(forests)
    if nodes_d.ndim != 3:
        raise ValueError("forests must be (chains, m, node_limit)")
    nc, m, L = int(nodes_d.shape[0]), int(nodes_d.shape[1]), int(nodes_d.shape[2]) // 26
    max_leaves = L if max_leaves is None else int(max_leaves)
    plan = tree_proposals_plan(L, ft.shape[0], max_leaves, nc, m)
    if plan["reason"]:
        raise ValueError(plan["reason"])
    cparams = proposal_params(params, max_leaves, chain_offset, tree_offset)
    out = propose_trees_device(nodes_d, _lib.to_device(b), _lib.to_device(ft), cparams, seed, sweep)
    if return_device:
        return out
    new_d, lq, lu, detail = out
    return records_from_device(new_d), lq.cpu().numpy(), lu.cpu().numpy(), detail.cpu().numpy()
