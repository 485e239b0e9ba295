"""Host-side steps the sampler's chain containers share (`ChainState`, `ChainBatch`, `LeafChainBatch`): input checks,
leaf counts, the packing of a sweep's steps into one upload, workspace caching and the read-back of the decisions.
Private: no public names, nothing here launches."""

import ctypes

import numpy as np

from .. import _lib
from ..forest import _as_nodes, _points


def points_of(owner, X, ft, noun: str):
    """Device copy of the caller's X, reused while the caller passes the same object (owner._X_seen), with owner.N rows;
    noun: "chain has" / "chains have"."""
    if owner._X_seen is None or owner._X_seen[0] is not X:
        Xd, _ = _points(X, ft.shape[0])
        owner._X_seen = (X, Xd)
    Xd = owner._X_seen[1]
    if Xd.shape[0] != owner.N:
        raise ValueError(f"X has {Xd.shape[0]} rows, the {noun} {owner.N} points")
    return Xd


def workspace(cache: dict, key, nbytes, device):
    """cache[key]: a uint8 device tensor of nbytes() bytes (a library query), allocated on first use."""
    import torch

    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty(int(nbytes()), dtype=torch.uint8, device=device)
    return ws


def leaf_counts(trees, ft) -> np.ndarray:
    """Leaves of every tree of `trees` (..., node_limit), in the packer's sense (reachable from the root)."""
    lib = _lib.lib()
    flat = trees.reshape(-1, trees.shape[-1])
    out = np.empty(flat.shape[0], dtype=np.int64)
    info = _lib.PackInfo()
    for k in range(flat.shape[0]):
        _lib.check(lib.bark_forest_pack_info(_lib.ptr(np.ascontiguousarray(flat[k])), 1, 1, flat.shape[1], _lib.ptr(ft), ft.shape[0],
                                             ctypes.byref(info)))
        out[k] = info.max_bits
    return out.reshape(trees.shape[:-1])


def steps_major(a, nc: int, steps: int) -> np.ndarray:
    """(chains, steps) values of a sweep -> contiguous float64 (steps, chains)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(nc, steps).T)


def per_chain(name: str, v, nc: int) -> np.ndarray:
    """One value per chain -> contiguous float64 (chains,)."""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if v.shape[0] != nc:
        raise ValueError(f"{name} has {v.shape[0]} entries for {nc} chains")
    return v


def noise_scale_vectors(new_noise, new_scale, log_q_prior, log_u, nc: int) -> list:
    """The four per-chain inputs of a noise/scale step, in the order the entry points take them."""
    return [per_chain(name, v, nc)
            for name, v in (("new_noise", new_noise), ("new_scale", new_scale), ("log_q_prior", log_q_prior), ("log_u", log_u))]


def broadcast_scale(scale, nc: int) -> np.ndarray:
    """A scalar or one value per chain -> float64 (chains,) (read-only view)."""
    return np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (nc,))


def check_step_trees(old_trees, new_trees, nc: int):
    """The trees of a sweep and their proposals as two contiguous (chains, steps, node_limit) record arrays."""
    old, new = _as_nodes(old_trees, 3), _as_nodes(new_trees, 3)
    if old.shape != new.shape or old.ndim != 3 or old.shape[0] != nc:
        raise ValueError(f"trees must be (chains, steps, node_limit) records, got {old.shape} and {new.shape}")
    return old, new


def pack_steps_host(per_step_forests, ft):
    """Pack every step's (chains, k, node_limit) forests — k = 2: [old, new] pairs, k = 1: the proposal alone — into ONE host
    buffer, step t at offsets[t] (256-byte aligned) -> (infos: PackInfo array, offsets int64 (steps,), sizes, uint8 buffer)."""
    lib = _lib.lib()
    forests = [np.ascontiguousarray(f) for f in per_step_forests]
    steps = len(forests)
    infos = (_lib.PackInfo * steps)()
    for t, f in enumerate(forests):
        _lib.check(lib.bark_forest_pack_info(_lib.ptr(f), f.shape[0], f.shape[1], f.shape[2], _lib.ptr(ft), ft.shape[0],
                                             ctypes.byref(infos[t])))
    sizes = [int(info.packed_bytes) for info in infos]
    offsets = np.zeros(steps, dtype=np.int64)
    offsets[1:] = np.cumsum([(sz + 255) // 256 * 256 for sz in sizes[:-1]])
    host = np.empty(int(offsets[-1]) + sizes[-1], dtype=np.uint8)
    for t, f in enumerate(forests):
        _lib.check(lib.bark_forest_pack(_lib.ptr(f), _lib.ptr(ft), ft.shape[0], ctypes.byref(infos[t]),
                                        ctypes.c_void_p(host.ctypes.data + int(offsets[t]))))
    return infos, offsets, sizes, host


def upload_sweep(host, lq, lu):
    """The upload half: -> (packed steps, log_q_prior, log_u, the (steps, chains) int32 accept tensor), all on the device."""
    import torch

    return _lib.to_device(host), _lib.to_device(lq), _lib.to_device(lu), torch.empty(lq.shape, dtype=torch.int32, device=_lib.torch_device())


def read_decisions(accept, state):
    """The decisions and the (chains, 2) running [quad, logdet] the device left -> host (acc, quad, logdet); the first copy is
    the call's one synchronisation.  The device has already rewritten the accepted chains' matrices, so the caller takes quad /
    logdet and updates its mirrors BEFORE it raises on a code in acc: a caller that catches the error keeps a consistent batch."""
    acc = accept.cpu().numpy()
    st = state.cpu().numpy()
    return acc, st[:, 0].copy(), st[:, 1].copy()
