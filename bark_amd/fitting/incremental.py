"""Device-resident state for the sampler's per-tree Metropolis step (reference:
src/bark/fitting/bark_sampler.py:217-264, `_step_bark_sampler`).

The reference keeps `cur_K_inv`, `cur_K_logdet`, `cur_mll` per chain and, for every tree proposal, chains

    low_rank_inv_update(subtract old leaf vectors) -> low_rank_det_update -> low_rank_inv_update(add new)
    -> low_rank_det_update -> mll                                     (bark_sampler.py:242-257)

i.e. about nine passes over the N x N inverse before the accept/reject.  `ChainState.propose` gets the same
`new_mll` from ONE pass (Y = K_inv [U_old U_new]) plus (r_old + r_new)^2 algebra, and `accept` rewrites
K_inv only for accepted proposals (one read + write pass).  `ChainBatch.sweep_trees` runs a whole sweep over the
trees of several chains with the accept/reject decided on the device (one read-back per sweep).  Proposals, RNG and
the forest container stay on the host, exactly as in the reference; only the linear algebra lives on the GPU.
This is an additive API (the drop-in functions of `quick_inverse` remain available)."""

from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib
from ..forest import _as_nodes, _feat_types, _is_torch, _raise_on_categorical_fault, leaf_vectors_device, packed_forest
from . import _chains
from .mll import _run_leafspace, batched_kernel_inverse

MAX_RANK = 64  # leaf vectors one fused update can carry (lowrank.hip LR_MAX)


def _dev64(a):
    import torch

    t = _lib.to_device(a.detach() if _is_torch(a) else np.asarray(a, dtype=np.float64))
    return t.to(torch.float64).contiguous()


def _quadform(K_inv, y) -> float:
    """y' K_inv y (quick_inverse.py:38) -> host float."""
    import torch

    q = torch.empty(1, dtype=torch.float64, device=K_inv.device)
    _lib.check(_lib.lib().bark_quadform_hip(_lib.ptr(K_inv), _lib.ptr(y), int(y.shape[0]), _lib.ptr(q), _lib.stream_ptr()))
    return float(q.item())


def _raise_if_singular(ws, N: int, r: int):
    flag = ctypes.c_int32(0)
    _lib.check(_lib.lib().bark_lowrank_status_hip(_lib.ptr(ws), N, r, ctypes.byref(flag), _lib.stream_ptr()))
    if flag.value:
        raise np.linalg.LinAlgError(f"Singular matrix in the rank-{r} update (pivot {flag.value})")  # quick_inverse.py:19,31


def _tree_leaves(nodes1, Xd, ft):
    """(N,) device leaf indices of one tree (forest.py:50-55)."""
    import torch

    pf = packed_forest(nodes1[None, None], ft)
    out = torch.empty((1, Xd.shape[0], 1), dtype=torch.int32, device=Xd.device)
    _lib.check(_lib.lib().bark_leaf_indices_hip(_lib.ctx(), _lib.ptr(pf.packed), pf.info_ref, _lib.ptr(Xd), Xd.shape[0],
                                                Xd.shape[1], _lib.ptr(out), _lib.stream_ptr()))
    return out.reshape(-1)


def _reached_leaf_vectors(old, new, Xd, ft, s: float):
    """The scaled leaf vectors of bark_sampler.py:233-236 with one column per REACHED leaf (get_leaf_vectors,
    forest.py:70-75): -> (U, None, r_old, r_new) with U = [U_old U_new] in one (N, r_old + r_new) buffer when that fits
    one fused update, else (U_old, U_new, r_old, r_new) as two matrices."""
    import torch

    lo, ln = _tree_leaves(old, Xd, ft), _tree_leaves(new, Xd, ft)
    _raise_on_categorical_fault(ft)
    r_old = int(np.unique(lo.cpu().numpy()).shape[0])
    r_new = int(np.unique(ln.cpu().numpy()).shape[0])
    if r_old + r_new <= MAX_RANK:
        U = torch.empty((Xd.shape[0], r_old + r_new), dtype=torch.float64, device=Xd.device)
        leaf_vectors_device(lo, s, out=U, col0=0)
        leaf_vectors_device(ln, s, out=U, col0=r_old)
        return U, None, r_old, r_new
    return leaf_vectors_device(lo, s), leaf_vectors_device(ln, s), r_old, r_new


def _copy2d(dst, col0: int, src):
    """dst[:, col0 : col0 + src.shape[1]] = src for row-major float64 device matrices (strided DMA copy)."""
    _lib.check(_lib.lib().bark_copy2d_hip(ctypes.c_void_p(dst.data_ptr() + 8 * col0), int(dst.stride(0)), _lib.ptr(src),
                                          int(src.stride(0)), int(src.shape[0]), int(src.shape[1]), _lib.stream_ptr()))


def sweep_plan(N: int, r_max: int, d: int, *, nc: int = 1, max_nodes_bytes: int = 0) -> dict:
    """Which instance of the one-launch sweep (`ChainBatch.sweep_trees(method="resident")`) a shape takes —
    `bark_tree_sweep_resident_query`, the function the entry point itself launches from.  N points, at most r_max leaves per
    [old, new] pair, d features, nc chains, max_nodes_bytes = packed bytes of the largest pair (2 * stride * 16; 0 = unknown)
    -> {"variant": 0 unsupported | 1 K_inv in LDS | 2 K_inv through global memory (L2), "lds_bytes", "threads", "d_max": the
    largest d whose X rows still fit LDS at this N (0 if unsupported for another reason), "reason": why not, else ""}.
    Limits: N <= 512, 2 <= r_max <= 16, nc <= 64, max_nodes_bytes <= 2048 (64 packed nodes per tree).  The launch is sized for 16
    leaves, so the variant depends on N and d only: 1 up to N = 128 (d <= 9 there), 2 beyond.
    Measured against method="launches" on the MI355X (DESIGN.md section 8(1), 50 proposals, 1 and 4 chains): "resident" wins
    1.1-1.4x only at N <= 128 with at most 8 leaves per pair; it LOSES with 9-16 leaves at every N (0.8-0.95x) and everywhere
    beyond N = 128 (0.4-0.5x at N = 256, 0.16-0.23x at N = 512).  Keep the default outside N <= 128, <= 8 leaves.
    No GPU needed."""
    lib = _lib.lib()

    def ask(dd):
        v, lds, th = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0)
        rc = lib.bark_tree_sweep_resident_query(N, r_max, dd, max_nodes_bytes, ctypes.byref(v), ctypes.byref(lds), ctypes.byref(th))
        return rc, v.value, lds.value, th.value, ("" if rc == 0 else lib.bark_last_error().decode(errors="replace"))

    rc, variant, lds, threads, reason = ask(d)
    if rc == 0 and not 1 <= nc <= 64:
        variant, lds, threads, reason = 0, 0, 0, f"one-launch sweep: {nc} chains are outside 1..64"
    d_max = 0
    if ask(1)[0] == 0:  # supported at all at this N and r_max: bisect the d bound
        lo, hi = 1, 1 << 16
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if ask(mid)[0] == 0 else (lo, mid - 1)
        d_max = lo
    return {"variant": variant, "lds_bytes": lds, "threads": threads, "d_max": d_max, "reason": reason}


class ChainState:
    """K_inv (N, N), log|K|, y'K_inv y and the targets y of one chain, resident in HBM."""

    def __init__(self, K_inv, K_logdet, y):
        import torch

        K_inv, y = _dev64(K_inv), _dev64(y).reshape(-1).contiguous()
        N = y.shape[0]
        if K_inv.shape != (N, N):
            raise ValueError(f"K_inv is {tuple(K_inv.shape)}, y has {N} rows")
        self._setup(K_inv, y, N, _quadform(K_inv, y), float(K_logdet), None,
                    torch.empty(2, dtype=torch.float64, device=K_inv.device))

    def _setup(self, K_inv, y, N, quad, logdet, X_seen, scalars):
        """Every field of a state: `__init__` and `_view_of_chain` both end here."""
        self.K_inv, self.y, self.N = K_inv, y, N
        self.quad, self.logdet = quad, logdet
        self._pending = None
        self._ws = {}  # rank -> workspace tensor, reused across proposals
        self._X_seen = X_seen  # (caller's X object, device tensor) of the last propose_tree
        self._scalars = scalars

    @classmethod
    def _view_of_chain(cls, K_inv, y, N, quad, logdet, Xd, scalars):
        """A state that is a VIEW of one chain of a `ChainBatch`: its slice of K_inv and of the scalars, the batch's y and
        device X, and the quad / logdet the batch already holds (nothing is recomputed, nothing is copied)."""
        st = cls.__new__(cls)
        st._setup(K_inv, y, N, quad, logdet, (Xd, Xd), scalars)
        return st

    def _workspace(self, r: int):  # the tree-swap layout is >= the plain low-rank one: it serves both
        return _chains.workspace(self._ws, r, lambda: _lib.lib().bark_tree_swap_workspace_bytes(self.N, r), self.K_inv.device)

    @classmethod
    def from_forest(cls, forest, noise, scale, X, y, feat_types):
        """Initial state of a chain: bark_sampler.py:153-162 (scale * K + (1e-6 + noise) I, inverse, logdet)."""
        nodes = np.asarray(forest)
        K_inv, _, logdet = batched_kernel_inverse(nodes[None], [noise], [scale], X, y, feat_types, no_null=False,
                                                  return_device=True)
        return cls(K_inv[0], float(logdet[0].item()), y)

    def propose_noise_scale(self, forest, new_noise: float, new_scale: float, X, feat_types) -> float:
        """MLL the chain would have with the proposed (noise, scale) — the second half of `_step_bark_sampler`
        (bark_sampler.py:266-272), where the reference rebuilds inv + slogdet of the N x N matrix.  Evaluated in
        leaf space (R x R system, include/bark_hip.h) without touching K_inv; `accept()` rebuilds the resident
        inverse, also in leaf space.  `forest` is the chain's current (m, node_limit) forest."""
        nodes = np.asarray(forest)
        val = _run_leafspace(nodes[None], [new_noise], [new_scale], X, self.y, feat_types, _lib.MLL_INCLUDE_SCALE)
        self._pending = ("noise_scale", nodes, float(new_noise), float(new_scale), X, feat_types)
        return float(val[0].item())

    @property
    def mll(self) -> float:
        """quick_inverse.py:37-38."""
        return 0.5 * (-self.quad - self.logdet)

    def _eval_explicit(self, U, r_old: int, r_new: int) -> float:
        lib = _lib.lib()
        r = r_old + r_new
        ws, scalars = self._workspace(r), self._scalars
        _lib.check(lib.bark_lowrank_swap_eval_hip(_lib.ptr(self.K_inv), self.N, _lib.ptr(U), r_old, r_new,
                                                  _lib.ptr(self.y), _lib.ptr(scalars), _lib.ptr(ws), ws.numel(),
                                                  _lib.stream_ptr()))
        return self._finish_eval(ws, r)

    def _finish_eval(self, ws, r: int) -> float:
        dquad, dlogdet = (float(v) for v in self._scalars.cpu().numpy())
        if not (np.isfinite(dquad) and np.isfinite(dlogdet)):
            _raise_if_singular(ws, self.N, r)
        self._pending = ("swap", ws, r, self.quad - dquad, self.logdet + dlogdet)
        return 0.5 * (-(self.quad - dquad) - (self.logdet + dlogdet))

    def propose(self, cur_leaf_vectors, new_leaf_vectors) -> float:
        """MLL the chain would have after swapping the old tree's (scaled) leaf vectors for the new tree's
        (bark_sampler.py:238-256).  Does not modify the state; call `accept()` to commit."""
        import torch

        U_old, U_new = _dev64(cur_leaf_vectors), _dev64(new_leaf_vectors)
        if U_old.shape[0] != self.N or U_new.shape[0] != self.N:
            raise ValueError("leaf vectors must have N rows")
        r_old, r_new = U_old.shape[1], U_new.shape[1]
        if max(r_old, r_new) > MAX_RANK:
            raise ValueError(f"a tree contributes at most {MAX_RANK} leaf vectors (got {r_old} and {r_new})")
        if r_old + r_new > MAX_RANK:
            return self._propose_sequential(U_old, U_new)
        U = torch.empty((self.N, r_old + r_new), dtype=torch.float64, device=self.K_inv.device)
        _copy2d(U, 0, U_old)
        _copy2d(U, r_old, U_new)
        return self._eval_explicit(U, r_old, r_new)

    def _propose_sequential(self, U_old, U_new) -> float:
        """More than 64 leaf vectors in total (two bushy trees: the default container allows 50 leaves each): the
        reference's own chain, subtract then add (bark_sampler.py:242-255), on a copy of K_inv."""
        import torch

        lib = _lib.lib()
        K_new = torch.empty_like(self.K_inv)
        dets = torch.empty(2, dtype=torch.float64, device=self.K_inv.device)
        src = self.K_inv
        for i, (U, subtract) in enumerate(((U_old, 1), (U_new, 0))):
            r = int(U.shape[1])
            ws = self._workspace(r)
            _lib.check(lib.bark_lowrank_update_hip(_lib.ptr(src), self.N, _lib.ptr(U), r, subtract, 1, _lib.ptr(K_new),
                                                   ctypes.c_void_p(dets.data_ptr() + 8 * i), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr()))
            _raise_if_singular(ws, self.N, r)
            src = K_new
        d1, d2 = (float(v) for v in dets.cpu().numpy())
        quad = _quadform(K_new, self.y)
        logdet = self.logdet + d1 + d2
        self._pending = ("replace", K_new, quad, logdet)
        return 0.5 * (-quad - logdet)

    def accept(self) -> None:
        """Commit the last proposal: K_inv <- K_inv - Y (C+G)^-1 Y' (bark_sampler.py:259-264)."""
        import torch

        if self._pending is None:
            raise RuntimeError("accept() without a pending propose()")
        kind = self._pending[0]
        if kind == "noise_scale":
            _, nodes, noise, scale, X, feat_types = self._pending
            K_inv, K_inv_y, logdet = batched_kernel_inverse(nodes[None], [noise], [scale], X, self.y, feat_types,
                                                            no_null=False, return_device=True, method="leafspace")
            self.K_inv = K_inv[0]
            q = torch.empty(1, dtype=torch.float64, device=self.K_inv.device)
            _lib.check(_lib.lib().bark_rowdot_hip(_lib.ptr(K_inv_y), 1, self.N, self.N, _lib.ptr(self.y), 1.0, None, 0.0,
                                                  _lib.ptr(q), _lib.stream_ptr()))
            self.quad = float(q.item())
            self.logdet = float(logdet[0].item())
        elif kind == "replace":
            _, self.K_inv, self.quad, self.logdet = self._pending
        else:
            _, ws, r, quad, logdet = self._pending
            _lib.check(_lib.lib().bark_lowrank_swap_apply_hip(_lib.ptr(self.K_inv), self.N, r, _lib.ptr(ws),
                                                              _lib.ptr(self.K_inv), _lib.stream_ptr()))
            self.quad, self.logdet = quad, logdet
        self._pending = None

    def propose_tree(self, old_nodes, new_nodes, X, feat_types, scale: float, m: int) -> float:
        """bark_sampler.py:233-256 from the two trees themselves: both are walked on the GPU and their one-hot
        leaf code, scaled by s_sqrtm = sqrt(scale / m), is the [U_old U_new] of `propose` (one column per leaf;
        leaves no point reaches give zero columns, which change nothing).  Pairs with more than 64 leaves in total
        go through the reached-leaf vectors (and, if those still exceed 64, the subtract-then-add chain of the
        reference).  `accept()` commits as usual."""
        lib = _lib.lib()
        ft = _feat_types(feat_types)
        Xd = _chains.points_of(self, X, ft, "chain has")
        old, new = _as_nodes(old_nodes, 1), _as_nodes(new_nodes, 1)
        if old.ndim != 1 or new.ndim != 1 or old.shape != new.shape:
            raise ValueError(f"trees must be (node_limit,) records of one container, got {old.shape} and {new.shape}")
        s = float(np.sqrt(scale / m))
        r_old = int(_chains.leaf_counts(old, ft))
        pf = packed_forest(np.stack([old, new])[None], ft)
        r = int(pf.info.max_bits)
        if r > MAX_RANK:
            U, U_new, r_old, r_new = _reached_leaf_vectors(old, new, Xd, ft, s)
            if U_new is None:
                return self._eval_explicit(U, r_old, r_new)
            return self._propose_sequential(U, U_new)
        ws, scalars = self._workspace(r), self._scalars
        _lib.check(lib.bark_tree_swap_eval_hip(_lib.ctx(), _lib.ptr(self.K_inv), self.N, _lib.ptr(pf.packed), pf.info_ref,
                                               _lib.ptr(Xd), Xd.shape[1], r_old, s, _lib.ptr(self.y),
                                               _lib.ptr(scalars), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        val = self._finish_eval(ws, r)
        _raise_on_categorical_fault(ft)
        return val


class ChainBatch:
    """`ChainState` for several independent chains of the sampler (bark_sampler.py:147): K_inv (nc, N, N) resident,
    the per-tree proposals of all chains evaluated by ONE library call — the chain index is a grid dimension of
    every kernel, so the call costs one launch sequence.  `sweep_trees` runs a whole sweep over the trees with the
    Metropolis decision on the device: one read-back per sweep instead of one per tree; `step_noise_scale` does the same
    for the noise/scale proposal that ends a step.  The chains share X and y (as in the reference)."""

    def __init__(self, K_inv, K_logdet, y):
        import torch

        self.K_inv = _dev64(K_inv)
        if self.K_inv.ndim != 3 or self.K_inv.shape[1] != self.K_inv.shape[2]:
            raise ValueError(f"K_inv must be (chains, N, N), got {tuple(self.K_inv.shape)}")
        self.nc, self.N = int(self.K_inv.shape[0]), int(self.K_inv.shape[1])
        if not 1 <= self.nc <= 64:
            raise ValueError("1 to 64 chains")
        self.y = _dev64(y).reshape(-1).contiguous()
        if self.y.shape[0] != self.N:
            raise ValueError(f"y has {self.y.shape[0]} rows, K_inv is {self.N} x {self.N}")
        self.logdet = np.asarray(K_logdet, dtype=np.float64).reshape(-1).copy()
        if self.logdet.shape[0] != self.nc:
            raise ValueError("one log-determinant per chain")
        self.quad = np.array([_quadform(self.K_inv[b], self.y) for b in range(self.nc)])
        self._scalars = torch.empty((self.nc, 2), dtype=torch.float64, device=self.K_inv.device)
        self._ws = {}
        self._pending = None
        self._X_seen = None

    @classmethod
    def from_forests(cls, forests, noise, scale, X, y, feat_types, method: str = "dense"):
        """Initial state of every chain (bark_sampler.py:153-162); forests (chains, m, node_limit)."""
        nodes = np.asarray(forests)
        K_inv, _, logdet = batched_kernel_inverse(nodes, noise, scale, X, y, feat_types, no_null=False,
                                                  return_device=True, method=method)
        return cls(K_inv, logdet.cpu().numpy(), y)

    @property
    def mll(self) -> np.ndarray:
        """quick_inverse.py:37-38 for every chain."""
        return 0.5 * (-self.quad - self.logdet)

    def _workspace(self, r: int, extra: int = 0):
        query = lambda: int(_lib.lib().bark_tree_swap_chains_workspace_bytes(self.N, r, self.nc, None)) + extra
        return _chains.workspace(self._ws, (r, extra), query, self.K_inv.device)

    def propose_trees(self, old_trees, new_trees, X, feat_types, scale, m: int) -> np.ndarray:
        """bark_sampler.py:233-256 for one tree per chain: old_trees / new_trees (chains, node_limit) records,
        scale (chains,) -> the (chains,) MLL values the chains would have.  `accept(mask)` commits."""
        lib = _lib.lib()
        ft = _feat_types(feat_types)
        Xd = _chains.points_of(self, X, ft, "chains have")
        old, new = _as_nodes(old_trees, 2), _as_nodes(new_trees, 2)
        if old.shape != new.shape or old.ndim != 2 or old.shape[0] != self.nc:
            raise ValueError(f"trees must be (chains, node_limit) records, got {old.shape} and {new.shape}")
        scale = _chains.broadcast_scale(scale, self.nc)
        r_old = _chains.leaf_counts(old, ft)  # leaves of each old tree alone = the split between removed and added columns
        pf = packed_forest(np.stack([old, new], axis=1), ft)  # (chains, 2, L): one [old, new] pair per chain
        r = int(pf.info.max_bits)
        if r > MAX_RANK:
            return self._propose_trees_one_by_one(old, new, Xd, ft, scale, m)
        ws = self._workspace(r)
        s_sqrtm = np.ascontiguousarray(np.sqrt(scale / m))
        _lib.check(lib.bark_tree_swap_eval_chains_hip(_lib.ctx(), _lib.ptr(self.K_inv), self.N, self.nc, _lib.ptr(pf.packed),
                                                      pf.info_ref, _lib.ptr(Xd), Xd.shape[1], _lib.ptr(r_old),
                                                      _lib.ptr(s_sqrtm), _lib.ptr(self.y), _lib.ptr(self._scalars), _lib.ptr(ws),
                                                      ws.numel(), _lib.stream_ptr()))
        sc = self._scalars.cpu().numpy()
        _raise_on_categorical_fault(ft)
        if not np.isfinite(sc).all():
            raise np.linalg.LinAlgError("Singular matrix in a tree-swap update")
        quad, logdet = self.quad - sc[:, 0], self.logdet + sc[:, 1]
        self._pending = ("swap", ws, r, quad, logdet)
        return 0.5 * (-quad - logdet)

    def _propose_trees_one_by_one(self, old, new, Xd, ft, scale, m):
        """A pair with more than 64 leaves in total somewhere: every chain goes through `ChainState`'s fallback
        (reached-leaf vectors, then the reference's subtract-then-add chain) on its own slice of K_inv."""
        states, vals = [], np.empty(self.nc)
        for b in range(self.nc):
            st = ChainState._view_of_chain(self.K_inv[b], self.y, self.N, float(self.quad[b]), float(self.logdet[b]), Xd,
                                           self._scalars[b])
            vals[b] = st.propose_tree(old[b], new[b], Xd, ft, float(scale[b]), m)
            states.append(st)
        self._pending = ("states", states)
        return vals

    def accept(self, mask) -> None:
        """Commit the pending proposals of the chains where `mask` is true (bark_sampler.py:259-264)."""
        if self._pending is None:
            raise RuntimeError("accept() without a pending propose_trees()")
        mask = np.ascontiguousarray(np.broadcast_to(np.asarray(mask).reshape(-1), (self.nc,)), dtype=np.int32)
        if self._pending[0] == "states":
            for b, st in enumerate(self._pending[1]):
                if mask[b]:
                    st.accept()
                    if st.K_inv.data_ptr() != self.K_inv[b].data_ptr():  # the sequential chain built a new matrix
                        self.K_inv[b].copy_(st.K_inv)
                    self.quad[b], self.logdet[b] = st.quad, st.logdet
            self._pending = None
            return
        _, ws, r, quad, logdet = self._pending
        _lib.check(_lib.lib().bark_lowrank_swap_apply_chains_hip(_lib.ptr(self.K_inv), self.N, self.nc, r, _lib.ptr(mask),
                                                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        keep = mask != 0
        self.quad = np.where(keep, quad, self.quad)
        self.logdet = np.where(keep, logdet, self.logdet)
        self._pending = None

    def sweep_trees(self, old_trees, new_trees, log_q_prior, log_u, X, feat_types, scale, m: int,
                    method: str = "launches") -> np.ndarray:
        """One sweep of the per-tree loop of `_step_bark_sampler` (bark_sampler.py:233-264) for every chain, decided on
        the device: old_trees / new_trees (chains, steps, node_limit) — the tree of step t and its proposal, which the
        host can draw up front because a proposal only depends on the tree it replaces (tree_proposals.py) —,
        log_q_prior and log_u (chains, steps): the proposal ratio and log of the uniform draw of bark_sampler.py:258.
        Per step the device evaluates all chains, accepts where log_u <= min(log_q_prior + new_mll - cur_mll, 0) and
        rewrites those chains' K_inv.  Returns the (chains, steps) boolean accept mask — the caller copies the accepted
        trees into its forest, as bark_sampler.py:264 does — after ONE read-back for the whole sweep.

        method="launches" (default): five or six launches per step, any N, up to 64 leaves per pair.  method="resident": the
        whole sweep in ONE launch, one workgroup per chain with K_inv in LDS or L2 (`sweep_plan` has the limits: N <= 512,
        <= 16 leaves per pair); same state, same decision rule, K_inv equal to rounding (it sums in another order).  It
        reads K_inv by columns and updates (i, j) and (j, i) by the same amount, so K_inv must be exactly symmetric on entry — it
        is after `from_forests`, it need not be after a method="launches" sweep or `step_noise_scale` — and then stays so.  Outside its limits it raises ValueError — it never falls back."""
        if method not in ("launches", "resident"):
            raise ValueError(f"unknown method {method!r} (use 'launches' or 'resident')")
        ft = _feat_types(feat_types)
        Xd = _chains.points_of(self, X, ft, "chains have")
        old, new = _chains.check_step_trees(old_trees, new_trees, self.nc)
        steps = old.shape[1]
        lq, lu = _chains.steps_major(log_q_prior, self.nc, steps), _chains.steps_major(log_u, self.nc, steps)
        scale = _chains.broadcast_scale(scale, self.nc)
        infos, offsets, _, host = _chains.pack_steps_host([np.stack([old[:, t], new[:, t]], axis=1) for t in range(steps)], ft)
        r_old = np.ascontiguousarray(_chains.leaf_counts(old, ft).T)  # (steps, chains): the split between removed and added columns
        r_max = max(int(info.max_bits) for info in infos)
        if method == "resident":
            plan = sweep_plan(self.N, r_max, int(Xd.shape[1]), nc=self.nc,
                              max_nodes_bytes=max(2 * int(info.stride) * 16 for info in infos))
            if not plan["variant"]:
                raise ValueError(f"sweep_trees(method=\"resident\"): {plan['reason']}; use method=\"launches\"")
        if r_max > MAX_RANK:
            raise ValueError(f"sweep_trees supports at most {MAX_RANK} leaves per [old, new] pair (got {r_max}); "
                             "use propose_trees / accept for this sweep")
        packed, lq_d, lu_d, accept = _chains.upload_sweep(host, lq, lu)
        state = _lib.to_device(np.ascontiguousarray(np.stack([self.quad, self.logdet], axis=1)))
        s_sqrtm = np.ascontiguousarray(np.sqrt(scale / m))
        launch = self._sweep_resident if method == "resident" else self._sweep_launches
        return launch(steps, infos, offsets, r_old, r_max, s_sqrtm, Xd, packed, lq_d, lu_d, state, accept, ft)

    def _sweep_launches(self, steps, infos, offsets, r_old, r_max, s_sqrtm, Xd, packed, lq_d, lu_d, state, accept, ft):
        ws = self._workspace(r_max, extra=16 * self.nc)
        _lib.check(_lib.lib().bark_tree_sweep_chains_hip(_lib.ctx(), _lib.ptr(self.K_inv), self.N, self.nc, steps, _lib.ptr(packed),
                                                         _lib.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), _lib.ptr(Xd),
                                                         Xd.shape[1], _lib.ptr(r_old), _lib.ptr(s_sqrtm), _lib.ptr(self.y),
                                                         _lib.ptr(lq_d), _lib.ptr(lu_d), _lib.ptr(state), _lib.ptr(accept),
                                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return self._finish_sweep(accept, state, ft)

    def _sweep_resident(self, steps, infos, offsets, r_old, r_max, s_sqrtm, Xd, packed, lq_d, lu_d, state, accept, ft):
        lib = _lib.lib()
        table = np.empty(int(lib.bark_tree_sweep_resident_table_bytes(steps, self.nc)) // 8, dtype=np.int64)
        _lib.check(lib.bark_tree_sweep_resident_table(_lib.ptr(offsets), ctypes.cast(infos, ctypes.c_void_p), _lib.ptr(r_old),
                                                      steps, self.nc, _lib.ptr(table)))
        table_d, s_d = _lib.to_device(table), _lib.to_device(s_sqrtm)
        ws = _chains.workspace(self._ws, ("resident", r_max),
                               lambda: lib.bark_tree_sweep_resident_workspace_bytes(self.N, r_max, self.nc), self.K_inv.device)
        _lib.check(lib.bark_tree_sweep_resident_hip(_lib.ctx(), _lib.ptr(self.K_inv), self.N, self.nc, steps, _lib.ptr(packed),
                                                    _lib.ptr(table_d), _lib.ptr(Xd), Xd.shape[1], _lib.ptr(s_d),
                                                    _lib.ptr(self.y), _lib.ptr(lq_d), _lib.ptr(lu_d), _lib.ptr(state),
                                                    _lib.ptr(accept), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return self._finish_sweep(accept, state, ft)

    def _finish_sweep(self, accept, state, ft) -> np.ndarray:
        # a singular chain is latched at -1 by decide_kernel and stays at the state after its last accepted step
        acc, self.quad, self.logdet = _chains.read_decisions(accept, state)
        self._pending = None
        self.last_accept = acc.T.copy()
        self.last_accept_device = accept  # (steps, chains) int32, as the device wrote it: the sampler's commit reads it there
        _raise_on_categorical_fault(ft)
        if (acc < 0).any():
            raise np.linalg.LinAlgError("Singular matrix in a tree-swap update")
        return (acc.T > 0)

    def step_noise_scale(self, forests, new_noise, new_scale, log_q_prior, log_u, X, feat_types) -> np.ndarray:
        """The noise/scale proposal of `_step_bark_sampler` (bark_sampler.py:266-282) for every chain, decided on the
        device: forests (chains, m, node_limit) — the chains' current forests, i.e. after the caller applied the mask of
        `sweep_trees` —, new_noise, new_scale, log_q_prior, log_u (chains,).  The MLL at the proposed values comes from the
        R x R leaf-space system of each forest; the device accepts where log_u <= min(log_q_prior + new_mll - cur_mll, 0)
        and rebuilds K_inv of those chains only, in place.  Returns the (chains,) boolean accept mask after ONE
        read-back; the caller keeps noise and scale and applies the mask, as bark_sampler.py:281-282 does."""
        import torch

        lib = _lib.lib()
        ft = _feat_types(feat_types)
        Xd = _chains.points_of(self, X, ft, "chains have")
        nodes = _as_nodes(forests, 3)
        if nodes.ndim != 3 or nodes.shape[0] != self.nc:
            raise ValueError(f"forests must be (chains, m, node_limit) records of {self.nc} chains, got {nodes.shape}")
        if nodes.shape[1] > 1280:
            raise ValueError(f"step_noise_scale supports at most 1280 trees (got {nodes.shape[1]})")
        vecs = [_lib.to_device(v) for v in _chains.noise_scale_vectors(new_noise, new_scale, log_q_prior, log_u, self.nc)]
        pf = packed_forest(nodes, ft)
        state = _lib.to_device(np.ascontiguousarray(np.stack([self.quad, self.logdet], axis=1)))
        accept = torch.empty(self.nc, dtype=torch.int32, device=self.K_inv.device)
        ws = _lib.workspace(int(lib.bark_noise_scale_step_chains_workspace_bytes(self.N, int(pf.info.max_bits), pf.m, self.nc)))
        _lib.check(lib.bark_noise_scale_step_chains_hip(_lib.ctx(), _lib.ptr(self.K_inv), self.N, self.nc, _lib.ptr(pf.packed),
                                                        pf.info_ref, _lib.ptr(Xd), Xd.shape[1], _lib.ptr(self.y),
                                                        *(_lib.ptr(v) for v in vecs), _lib.ptr(state), _lib.ptr(accept),
                                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        acc, self.quad, self.logdet = _chains.read_decisions(accept, state)
        self._pending = None
        if (acc == -2).any():
            _lib.check_categorical_fault()  # reads and clears the context's flag, whatever feat_types says, and raises
            raise ValueError("categorical feature value is negative, NaN or inf")
        if (acc < 0).any():
            b = int(np.flatnonzero(acc < 0)[0])
            raise np.linalg.LinAlgError(f"leaf-space system of chain {b} is not positive definite at the proposed noise / scale")
        return acc > 0
