"""LeafChainBatch.sweep_trees (leaf-space chain state, one launch per sweep) beside ChainBatch.sweep_trees(method="launches")
(N x N state, five or six launches per step), same process, same inputs: 50 proposals at N = 128 / 512 / 4096 / 16384 for 1, 4
and 64 chains (the dense state only where it fits: 8 N^2 bytes per chain), pairs of 4-8 and 12-16 leaves, and the resident bytes
per chain of both.
   python tools/time_leafchain.py [reps]
Timed: the library call alone (hipEvents recorded around bark_leafchain_sweep_hip / bark_tree_sweep_chains_hip, so the host's
packing is outside and the host's launch gaps of the multi-launch path are inside), median of `reps` sweeps after two warm-up
sweeps, each from a fresh batch.  Every shape is a child process of its own under `timeout -k 10 300`, so a kernel that hangs
ends its region, and the parent — which never opens the GPU — stops at the first child that fails."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REGION_LIMIT_S = 300
m, d = 50, 8
DENSE_BUDGET = 10e9  # bytes of K_inv (all chains) the dense path is given
HEADER = (f"{'N':>6} {'chains':>6} {'leaves':>6} {'launches ms':>12} {'leafchain ms':>12} {'ratio':>6} {'accepted':>8} "
          f"{'dense B/chain':>14} {'leaf B/chain':>13}")

if len(sys.argv) < 4:  # parent
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    print(HEADER, flush=True)
    for N in (128, 512, 4096, 16384):
        for nc in (1, 4, 64):
            rc = subprocess.run(["timeout", "-k", "10", str(REGION_LIMIT_S), sys.executable, os.path.abspath(__file__), reps, str(N),
                                 str(nc)]).returncode
            if rc:
                raise SystemExit(f"N = {N}, {nc} chains: the child ended with status {rc}; nothing more is started")
    raise SystemExit(0)

import torch

import bark_amd.fitting as fit
from bark_amd import _lib
from bark_amd import synthetic as syn
from bark_amd.forest import NODE_RECORD_DTYPE

reps, N, nc = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
handle = _lib.lib()
spans = []


def timed(name):
    fn = getattr(handle, name)

    def wrapper(*args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        spans.append((a, b))
        return rc

    setattr(handle, name, wrapper)


timed("bark_tree_sweep_chains_hip")
timed("bark_leafchain_sweep_hip")


def caterpillar_tree(leaves, feature, node_limit=100):
    """A tree of exactly `leaves` leaves: node 2k splits `feature` at (k + 1) / leaves, left child a leaf, right child the next split."""
    tree = np.zeros(node_limit, dtype=NODE_RECORD_DTYPE)
    node, parent, depth = 0, 0xFFFFFFFF, 0
    for k in range(leaves - 1):
        left, right = 2 * k + 1, 2 * k + 2
        tree[node] = (0, feature, (k + 1) / leaves, left, right, parent, depth, 1)
        tree[left] = (1, 0, 0, 0, 0, node, depth + 1, 1)
        node, parent, depth = right, node, depth + 1
    tree[node] = (1, 0, 0, 0, 0, parent, depth, 1)
    return tree


def caterpillars(nc, leaves_of, feature_of):
    return np.stack([np.stack([caterpillar_tree(leaves_of(b, t), feature_of(b, t)) for t in range(m)]) for b in range(nc)])


X, y, bounds, ft = syn.unit_cube_problem(N, d, seed=N)
Xd = torch.from_numpy(X).cuda()
dense_fits = 8.0 * N * N * nc <= DENSE_BUDGET
for tag, lo, hi in (("4-8", 2, 4), ("12-16", 6, 8)):
    cur = caterpillars(nc, lambda b, t: lo + (b + t) % (hi - lo + 1), lambda b, t: (b + t) % d)
    prop = caterpillars(nc, lambda b, t: lo + (2 * b + t + 1) % (hi - lo + 1), lambda b, t: (b + 3 * t + 1) % d)
    noise, scale = np.full(nc, 0.1), np.ones(nc)
    need = max(sum(max(lo + (b + t) % (hi - lo + 1), lo + (2 * b + t + 1) % (hi - lo + 1)) for t in range(m)) for b in range(nc))
    capacity = (need + 31) // 32 * 32  # the sweep's worst case over the accept masks
    rng = np.random.default_rng(5)
    log_q, log_u = rng.normal(0.0, 0.5, size=(nc, m)), np.log(rng.uniform(size=(nc, m)))
    med, masks, leaf_bytes = {}, {}, 0
    for method in ("launches", "leafchain"):
        if method == "launches" and not dense_fits:
            continue
        del spans[:]
        for _ in range(reps + 2):
            if method == "launches":
                cb = fit.ChainBatch.from_forests(cur, noise, scale, Xd, y, ft)
                masks[method] = cb.sweep_trees(cur, prop, log_q, log_u, Xd, ft, scale, m)
            else:
                cb = fit.LeafChainBatch.from_forests(cur, noise, scale, Xd, y, ft, capacity=capacity, lcap=8)
                leaf_bytes = cb.sweep_plan()["chain_bytes"]
                masks[method] = cb.sweep_trees(cur, prop, log_q, log_u, Xd, ft, scale, m)
            del cb
        torch.cuda.synchronize()
        med[method] = float(np.median([a.elapsed_time(b) for a, b in spans[2:]]))
    dense = f"{med['launches']:>12.3f}" if dense_fits else f"{'-':>12}"
    ratio = f"{med['launches'] / med['leafchain']:>6.2f}" if dense_fits else f"{'-':>6}"
    same = not dense_fits or np.array_equal(masks["launches"], masks["leafchain"])
    print(f"{N:>6} {nc:>6} {tag:>6} {dense} {med['leafchain']:>12.3f} {ratio} {int(masks['leafchain'].sum()):>5}/{m * nc:<3}"
          f"{'' if same else ' MASKS DIFFER'} {8 * N * N:>14} {leaf_bytes:>13}", flush=True)
