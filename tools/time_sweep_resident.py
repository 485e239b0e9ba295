"""ChainBatch.sweep_trees: method="resident" (one launch per sweep) beside method="launches" (five or six per step), same process,
same inputs: 50 proposals at N = 64 / 128 / 256 / 512 for 1 and 4 chains, and the numpy oracle's step on the host.
   python tools/time_sweep_resident.py [reps]
Timed: the library call alone (hipEvents recorded around bark_tree_sweep_*_hip, so the host's packing is outside and the host's
launch gaps of the multi-launch path are inside), median of `reps` sweeps after two warm-up sweeps, each from a fresh batch.
Every shape (one N, one chain count: both methods, both leaf ranges) is a child process of its own under `timeout -k 10 90`, so a
kernel that hangs ends its region, and the parent — which never opens the GPU — stops at the first child that fails."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REGION_LIMIT_S = 90
m, d = 50, 8
HEADER = f"{'N':>4} {'chains':>6} {'leaves':>6} {'launches ms':>12} {'resident ms':>12} {'ratio':>6} {'accepted':>8} {'oracle ms/step':>14}"

if len(sys.argv) < 4:  # parent
    reps = sys.argv[1] if len(sys.argv) > 1 else "7"
    print(HEADER, flush=True)
    for N in (64, 128, 256, 512):
        for nc in (1, 4):
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
timed("bark_tree_sweep_resident_hip")


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


def oracle_step_ms(N):
    """One proposal of the reference's chain on the host in numpy (the swap of tests/lowrank_ref.py: Y = K U, LAPACK solve and
    slogdet of C + U'Y, K - Y x) on an N x N inverse, 3 + 3 leaves."""
    rng = np.random.default_rng(N)
    A = rng.standard_normal((N, N))
    K = np.linalg.inv(A @ A.T / N + np.eye(N))
    U = np.zeros((N, 6))
    U[np.arange(N), rng.integers(0, 3, N)] = 0.1
    U[np.arange(N), 3 + rng.integers(0, 3, N)] = 0.1
    y = rng.standard_normal(N)
    C = np.diag([-1.0] * 3 + [1.0] * 3)
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        Y = K @ U
        v = Y.T @ y
        den = C + U.T @ Y
        x = np.linalg.solve(den, np.concatenate([v[:, None], Y.T], axis=1))
        _ = v @ x[:, 0], np.linalg.slogdet(den)[1], K - Y @ x[:, 1:]
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


X, y, bounds, ft = syn.unit_cube_problem(N, d, seed=N)
Xd = torch.from_numpy(X).cuda()
host_ms = oracle_step_ms(N)
for tag, lo, hi in (("4-8", 2, 4), ("12-16", 6, 8)):
    cur = caterpillars(nc, lambda b, t: lo + (b + t) % (hi - lo + 1), lambda b, t: (b + t) % d)
    prop = caterpillars(nc, lambda b, t: lo + (2 * b + t + 1) % (hi - lo + 1), lambda b, t: (b + 3 * t + 1) % d)
    noise, scale = np.full(nc, 0.1), np.ones(nc)
    rng = np.random.default_rng(5)
    log_q, log_u = rng.normal(0.0, 0.5, size=(nc, m)), np.log(rng.uniform(size=(nc, m)))
    med, masks = {}, {}
    for method in ("launches", "resident"):
        del spans[:]
        for _ in range(reps + 2):
            cb = fit.ChainBatch.from_forests(cur, noise, scale, Xd, y, ft)
            masks[method] = cb.sweep_trees(cur, prop, log_q, log_u, Xd, ft, scale, m, method=method)
        torch.cuda.synchronize()
        med[method] = float(np.median([a.elapsed_time(b) for a, b in spans[2:]]))
    same = np.array_equal(masks["launches"], masks["resident"])
    print(f"{N:>4} {nc:>6} {tag:>6} {med['launches']:>12.3f} {med['resident']:>12.3f} {med['launches'] / med['resident']:>6.2f} "
          f"{int(masks['resident'].sum()):>5}/{m * nc:<3}{'' if same else ' MASKS DIFFER'} {host_ms:>13.3f}", flush=True)
