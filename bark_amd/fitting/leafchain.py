"""Leaf-space sampler chains (reference: src/bark/fitting/bark_sampler.py:217-282, `_step_bark_sampler`).

`ChainBatch` keeps the explicit N x N inverse of every chain; a tree proposal is a pass over it.  `LeafChainBatch` keeps
P = M^-1 instead, M = I_R + c Z'Z over the R leaves of the chain's forest (include/bark_hip.h, "Leaf-space sampler chains"):
swapping a tree removes its rows and columns of M and borders in those of the proposal, so a proposal costs
O(R^2 r + R r N / 64) and a chain holds about 8 Rcap^2 + Rcap N / 8 bytes whatever N is.  Same decision rule, same state
convention and the same `sweep_trees` signature as `ChainBatch`, so a caller switches classes.

Opt-in: cond(M) ~ N scale / (1e-6 + noise); the path loses digits as noise -> 0 like every leaf-space route (DESIGN.md
section 7).  Outside its limits it raises ValueError — it never reroutes to another path."""

from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from ..forest import _as_nodes, _feat_types, _points, _raise_on_categorical_fault, packed_forest
from . import _chains


class LeafChainPlan(ctypes.Structure):
    """bark_leafchain_plan (include/bark_hip.h)."""
    _fields_ = [("state_bytes", ctypes.c_int64), ("chain_bytes", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)] + [
        (n, ctypes.c_int32) for n in ("plane_words", "workgroups", "threads", "launches_per_sweep", "max_chains", "max_trees",
                                      "max_leaves", "max_slots", "max_nodes")]


def leafchain_plan(N: int, capacity: int, m: int, lcap: int, *, nc: int = 1, d: int = 1) -> dict:
    """`bark_leafchain_query` for a shape: N points, `capacity` slots (rows of P) per chain, m trees of at most lcap leaves, nc
    chains, d features -> the limits ("max_chains" 64, "max_trees" 64, "max_leaves" 32, "max_slots" 1024, "max_nodes" 64), the
    resident "chain_bytes" / "state_bytes", the "workspace_bytes" of a call, the launch shape, and "reason": "" or why the
    shape is refused (the byte counts are 0 then).  No GPU needed."""
    plan = LeafChainPlan()
    lib = _lib.lib()
    rc = lib.bark_leafchain_query(N, capacity, m, lcap, nc, d, ctypes.byref(plan))
    out = {name: int(getattr(plan, name)) for name, _ in LeafChainPlan._fields_}
    out["reason"] = "" if rc == 0 else lib.bark_last_error().decode(errors="replace")
    return out


class LeafChainBatch:
    """P = M^-1 (capacity x capacity), the leaves' bit-planes, v = Z'y and the slot map of several independent chains of the
    sampler (bark_sampler.py:147), resident in HBM.  `sweep_trees` runs a sweep over the trees in ONE launch with the
    Metropolis decision on the device, `step_noise_scale` the noise/scale proposal; one read-back each."""

    def __init__(self):
        raise TypeError("use LeafChainBatch.from_forests")

    @classmethod
    def from_forests(cls, forests, noise, scale, X, y, feat_types, capacity=None, lcap=None):
        """Initial state of every chain (bark_sampler.py:153-162): forests (chains, m, node_limit), noise / scale (chains,).
        capacity: slots per chain.  A sweep is refused unless the capacity covers its worst case over the accept masks — the sum over
        the trees of the largest leaf count a tree can take in the sweep —, so the default is generous: twice the leaves of the
        largest forest plus lcap, rounded up to 32, at most 1024 (a full sweep in which every tree may double fits).  A caller
        that knows its proposals passes sum_t max(leaves(old_t), leaves(new_t)) or more; memory is 8 capacity^2 + capacity N / 8
        bytes per chain.  lcap: most leaves a tree may have during the chain's life (default 32, the limit)."""
        import torch

        self = cls.__new__(cls)
        lib = _lib.lib()
        ft = _feat_types(feat_types)
        nodes = _as_nodes(forests, 3)
        if nodes.ndim != 3:
            raise ValueError(f"forests must be (chains, m, node_limit) records, got {nodes.shape}")
        self.nc, self.m = int(nodes.shape[0]), int(nodes.shape[1])
        Xd, _ = _points(X, ft.shape[0])
        self._X_seen = (X, Xd)
        self.N = int(Xd.shape[0])
        self.y = _lib.to_device(np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1)))
        if self.y.shape[0] != self.N:
            raise ValueError(f"y has {self.y.shape[0]} rows, X has {self.N}")
        self.lcap = 32 if lcap is None else int(lcap)
        limits = leafchain_plan(1, 1, 1, 1)
        if not 1 <= self.nc <= limits["max_chains"]:
            raise ValueError(f"1 to {limits['max_chains']} chains")
        if self.m > limits["max_trees"]:
            raise ValueError(f"LeafChainBatch supports at most {limits['max_trees']} trees (got {self.m})")
        self.nleaves = _chains.leaf_counts(nodes, ft).astype(np.int32)  # host mirror of the device's leaf counts
        if int(self.nleaves.max()) > self.lcap:
            raise ValueError(f"a tree has {int(self.nleaves.max())} leaves, lcap is {self.lcap}")
        total = int(self.nleaves.sum(axis=1).max())
        self.capacity = min(limits["max_slots"], (2 * total + self.lcap + 31) // 32 * 32) if capacity is None else int(capacity)
        if total > self.capacity:
            raise ValueError(f"a forest has {total} leaves, the capacity is {self.capacity} slots")
        plan = leafchain_plan(self.N, self.capacity, self.m, self.lcap, nc=self.nc, d=int(Xd.shape[1]))
        if plan["reason"]:
            raise ValueError(plan["reason"])
        self.plan = plan
        dev = Xd.device
        self.state = torch.zeros(plan["state_bytes"], dtype=torch.uint8, device=dev)
        self._ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=dev)
        self._mstate = torch.empty((self.nc, 2), dtype=torch.float64, device=dev)
        pf = packed_forest(nodes, ft)
        self.noise, self.scale = (_chains.broadcast_scale(v, self.nc).copy() for v in (noise, scale))
        info = torch.empty(self.nc, dtype=torch.int32, device=dev)
        nl_d, noise_d, scale_d = _lib.to_device(self.nleaves), _lib.to_device(self.noise), _lib.to_device(self.scale)  # alive until the read-back
        _lib.check(lib.bark_leafchain_init_hip(_lib.ctx(), _lib.ptr(self.state), *self._shape(), _lib.ptr(pf.packed), pf.info_ref,
                                               _lib.ptr(nl_d), _lib.ptr(Xd), Xd.shape[1], _lib.ptr(self.y),
                                               _lib.ptr(noise_d), _lib.ptr(scale_d),
                                               _lib.ptr(self._mstate), _lib.ptr(info), _lib.ptr(self._ws), self._ws.numel(),
                                               _lib.stream_ptr()))
        code = info.cpu().numpy()
        self._take_state()
        _raise_on_categorical_fault(ft)
        if (code != 0).any():
            b = int(np.flatnonzero(code != 0)[0])
            raise np.linalg.LinAlgError(f"leaf-space system of chain {b} is not positive definite (code {int(code[b])})")
        return self

    def _shape(self):
        return self.N, self.capacity, self.m, self.lcap, self.nc

    def _take_state(self):
        st = self._mstate.cpu().numpy()
        self.quad, self.logdet = st[:, 0].copy(), st[:, 1].copy()

    @property
    def mll(self) -> np.ndarray:
        """quick_inverse.py:37-38 for every chain (the convention of `ChainBatch.mll`)."""
        return 0.5 * (-self.quad - self.logdet)

    @property
    def free_slots(self) -> np.ndarray:
        return self.capacity - self.nleaves.sum(axis=1)

    def sweep_plan(self) -> dict:
        """The query for this batch's shape (`leafchain_plan`)."""
        return dict(self.plan)

    def _prepare_sweep(self, old_trees, new_trees, log_q_prior, log_u, X, feat_types, scale, m, tree_index):
        """Validate, pack and upload a sweep -> (enqueue, accept tensor, tree indices, r_new, feat_types)."""
        lib = _lib.lib()
        ft = _feat_types(feat_types)
        Xd = _chains.points_of(self, X, ft, "chains have")
        old, new = _chains.check_step_trees(old_trees, new_trees, self.nc)
        steps = old.shape[1]
        if int(m) != self.m:
            raise ValueError(f"m = {m}, the chains have {self.m} trees")
        if not np.array_equal(_chains.broadcast_scale(scale, self.nc), self.scale):
            raise ValueError("scale differs from the chains' own (step_noise_scale changes it)")
        tidx = np.arange(steps, dtype=np.int64) if tree_index is None else np.ascontiguousarray(tree_index, dtype=np.int64).reshape(-1)
        if tidx.shape[0] != steps or (tidx < 0).any() or (tidx >= self.m).any():
            raise ValueError(f"tree_index must hold {steps} indices in 0..{self.m - 1}")
        lq, lu = _chains.steps_major(log_q_prior, self.nc, steps), _chains.steps_major(log_u, self.nc, steps)
        r_old = _chains.leaf_counts(old, ft)
        first = {}
        for t in range(steps):
            first.setdefault(int(tidx[t]), t)
        for k, t in first.items():
            if not np.array_equal(r_old[:, t], self.nleaves[:, k]):
                raise ValueError(f"old_trees[:, {t}] is not tree {k} of the chains (leaf counts {r_old[:, t]} against {self.nleaves[:, k]})")
        r_new = np.ascontiguousarray(_chains.leaf_counts(new, ft).T)  # (steps, chains)
        infos, offsets, _, host = _chains.pack_steps_host([new[:, t][:, None] for t in range(steps)], ft)
        table = np.empty(int(lib.bark_leafchain_sweep_table_bytes(steps, self.nc)) // 8, dtype=np.int64)
        _lib.check(lib.bark_leafchain_sweep_table(_lib.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), _lib.ptr(tidx), _lib.ptr(r_new),
                                                  _lib.ptr(np.ascontiguousarray(self.nleaves)), steps, self.nc, self.m, self.lcap,
                                                  self.capacity, _lib.ptr(table)))
        packed, lq_d, lu_d, accept = _chains.upload_sweep(host, lq, lu)
        table_d = _lib.to_device(table)
        shape = self._shape()

        def enqueue():  # only enqueues: capturable in a graph; the closure keeps the step's device buffers alive
            _lib.check(lib.bark_leafchain_sweep_hip(_lib.ctx(), _lib.ptr(self.state), *shape, steps, _lib.ptr(packed),
                                                    _lib.ptr(table_d), _lib.ptr(Xd), Xd.shape[1], _lib.ptr(self.y), _lib.ptr(lq_d),
                                                    _lib.ptr(lu_d), _lib.ptr(self._mstate), _lib.ptr(accept), _lib.ptr(self._ws),
                                                    self._ws.numel(), _lib.stream_ptr()))

        return enqueue, accept, tidx, r_new, ft

    def sweep_trees(self, old_trees, new_trees, log_q_prior, log_u, X, feat_types, scale, m: int, tree_index=None) -> np.ndarray:
        """One sweep of the per-tree loop of `_step_bark_sampler` (bark_sampler.py:233-264) for every chain, as
        `ChainBatch.sweep_trees`: old_trees / new_trees (chains, steps, node_limit), log_q_prior / log_u (chains, steps)
        -> the (chains, steps) boolean accept mask after ONE read-back.  Step t swaps tree tree_index[t] (default
        arange(steps), the reference's loop order; a tree may appear more than once).  old_trees is used for validation
        only — the chain knows its trees' slots —: the first swap of a tree must name a tree with the leaf count the chain
        holds.  scale and m must be the chain's own.  ValueError before any launch when a tree has more than lcap leaves or
        the free slots do not cover the sweep in the worst case (rebuild with a larger capacity)."""
        enqueue, accept, tidx, r_new, ft = self._prepare_sweep(old_trees, new_trees, log_q_prior, log_u, X, feat_types, scale, m,
                                                               tree_index)
        enqueue()
        return self._finish_sweep(accept, tidx, r_new, ft)

    def _finish_sweep(self, accept, tidx, r_new, ft) -> np.ndarray:
        acc, self.quad, self.logdet = _chains.read_decisions(accept, self._mstate)
        for t in range(acc.shape[0]):
            took = acc[t] > 0
            self.nleaves[took, tidx[t]] = r_new[t, took]
        self.last_accept = acc.T.copy()
        self.last_accept_device = accept  # (steps, chains) int32, as the device wrote it: the sampler's commit reads it there
        _raise_on_categorical_fault(ft)
        if (acc < 0).any():
            raise np.linalg.LinAlgError("non-positive pivot in a leaf-space tree swap")
        return acc.T > 0

    def step_noise_scale(self, new_noise, new_scale, log_q_prior, log_u) -> np.ndarray:
        """The noise/scale proposal of `_step_bark_sampler` (bark_sampler.py:266-282) for every chain, decided on the device from
        the resident planes (no forests, no walk): -> the (chains,) boolean accept mask after ONE read-back.  The batch keeps
        noise and scale of its chains itself (`.noise`, `.scale`)."""
        import torch

        vecs = _chains.noise_scale_vectors(new_noise, new_scale, log_q_prior, log_u, self.nc)
        dev = [_lib.to_device(v) for v in vecs]
        accept = torch.empty(self.nc, dtype=torch.int32, device=self.state.device)
        _lib.check(_lib.lib().bark_leafchain_noise_scale_hip(_lib.ctx(), _lib.ptr(self.state), *self._shape(), *(_lib.ptr(v) for v in dev),
                                                             _lib.ptr(self._mstate), _lib.ptr(accept), _lib.ptr(self._ws),
                                                             self._ws.numel(), _lib.stream_ptr()))
        acc, self.quad, self.logdet = _chains.read_decisions(accept, self._mstate)
        took = acc > 0
        self.noise, self.scale = np.where(took, vecs[0], self.noise), np.where(took, vecs[1], self.scale)
        if (acc < 0).any():
            b = int(np.flatnonzero(acc < 0)[0])
            raise np.linalg.LinAlgError(f"leaf-space system of chain {b} is not positive definite at the proposed noise / scale")
        return took

    def raw(self) -> dict:
        """The resident block as it is, slot order (debugging and tests; one read-back): {"P": (chains, capacity, capacity),
        "v": (chains, capacity), "planes": (chains, capacity, plane_words) uint64, "slots": (chains, m, lcap) int32 (-1: no such
        leaf), "nleaves": (chains, m), "free": per chain the free-slot stack, bottom first}."""
        R, Q, stride = self.capacity, self.plan["plane_words"], self.plan["chain_bytes"]
        blocks = self.state.cpu().numpy().reshape(self.nc, stride)
        out = {"P": [], "v": [], "planes": [], "slots": [], "nleaves": [], "free": []}
        for blk in blocks:  # the layout of lc_layout (csrc/leafchain.hip): 64 bytes of scalars, P, v, planes, the slot map
            o = 64
            out["P"].append(blk[o:o + 8 * R * R].view(np.float64).reshape(R, R))
            o += 8 * R * R
            out["v"].append(blk[o:o + 8 * R].view(np.float64))
            o += 8 * R
            out["planes"].append(blk[o:o + 8 * R * Q].view(np.uint64).reshape(R, Q))
            o += 8 * R * Q
            ints = blk[o:o + 4 * (self.m * self.lcap + self.m + 1 + R)].view(np.int32)
            out["slots"].append(ints[:self.m * self.lcap].reshape(self.m, self.lcap))
            out["nleaves"].append(ints[self.m * self.lcap:self.m * self.lcap + self.m])
            nfree = int(ints[self.m * self.lcap + self.m])
            out["free"].append(ints[self.m * self.lcap + self.m + 1:][:nfree].copy())
        return {k: (np.stack(v) if k != "free" else v) for k, v in out.items()}

    def export(self) -> dict:
        """Canonical view (tree-major, leaves in the packer's order): {"P": (chains, capacity, capacity) = M^-1 of each chain's
        leaves, identity beyond them, "v": (chains, capacity) = Z'y, "nleaves": (chains, m)} as numpy arrays."""
        import torch

        dev = self.state.device
        P = torch.empty((self.nc, self.capacity, self.capacity), dtype=torch.float64, device=dev)
        v = torch.empty((self.nc, self.capacity), dtype=torch.float64, device=dev)
        nl = torch.empty((self.nc, self.m), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().bark_leafchain_export_hip(_lib.ctx(), _lib.ptr(self.state), *self._shape(), _lib.ptr(P), _lib.ptr(v),
                                                        _lib.ptr(nl), _lib.stream_ptr()))
        return {"P": P.cpu().numpy(), "v": v.cpu().numpy(), "nleaves": nl.cpu().numpy()}
