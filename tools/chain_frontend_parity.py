"""Bit-parity record and host-marshalling time of the sampler's chain front end (ChainState, ChainBatch, LeafChainBatch), through
public names only, so the same file runs on any two commits of the tree it sits in:
   python tools/chain_frontend_parity.py OUT.json          SHA-256 of every case's raw result bytes, from fixed seeds
   python tools/chain_frontend_parity.py OUT.json --time   also: wall ms per sweep_trees call, median of 20 after 3 warm-ups
Two commits compute the same iff their OUT.json are identical (profiles/r10/ holds one pair).  Each case is the smallest shape
that takes a distinct path of the front end; the timed shapes are the host-bound ones of DESIGN.md section 8.
The dense classes take their first y'K_inv y from a reduction that ends in atomic adds, whose last bits vary from run to run of
ONE commit; K_inv does not, so every dense case restarts `quad` from the host's sum over the same K_inv (`host_quad`) before the
step it records.  The subtract-then-add fallback for pairs above 64 reached leaves ends in the same reduction, so chain 0 of the
one-by-one case records its MLL and quad to 12 significant digits instead of as a digest.  With that the record is reproducible."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bark_amd.fitting as fit
from bark_amd import synthetic as syn
from bark_amd.forest import NODE_RECORD_DTYPE

D = 8


def caterpillar(leaves, feature, node_limit=100):
    """A tree of exactly `leaves` leaves: node 2k splits `feature` at (k + 1) / leaves, left child a leaf, right the next split."""
    tree = np.zeros(node_limit, dtype=NODE_RECORD_DTYPE)
    node, parent, depth = 0, 0xFFFFFFFF, 0
    for k in range(leaves - 1):
        left, right = 2 * k + 1, 2 * k + 2
        tree[node] = (0, feature, (k + 1) / leaves, left, right, parent, depth, 1)
        tree[left] = (1, 0, 0, 0, 0, node, depth + 1, 1)
        node, parent, depth = right, node, depth + 1
    tree[node] = (1, 0, 0, 0, 0, parent, depth, 1)
    return tree


def trees(nc, steps, leaves_of, feature_of):
    return np.stack([np.stack([caterpillar(leaves_of(b, t), feature_of(b, t)) for t in range(steps)]) for b in range(nc)])


def digest(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def host_quad(K_inv, y):
    """y'K_inv y of one (N, N) device matrix, summed on the host in a fixed order."""
    K, yv = K_inv.cpu().numpy(), np.asarray(y, dtype=np.float64).reshape(-1)
    return float(((K * yv[None, :]).sum(axis=1) * yv).sum())


def dense_batch(forests, noise, scale, X, y, ft):
    cb = fit.ChainBatch.from_forests(forests, noise, scale, X, y, ft)
    cb.quad = np.array([host_quad(cb.K_inv[b], y) for b in range(cb.nc)])
    return cb


def problem(N, nc, steps, seed):
    X, y, _, ft = syn.unit_cube_problem(N, D, seed=N)
    rng = np.random.default_rng(seed)
    noise, scale = 0.05 + 0.1 * rng.uniform(size=nc), 0.8 + 0.4 * rng.uniform(size=nc)
    log_q, log_u = rng.normal(0.0, 0.5, size=(nc, steps)), np.log(rng.uniform(size=(nc, steps)))
    return X, y, ft, noise, scale, log_q, log_u


def dense_sweep(N, nc, steps, lo, hi, method, big=None, seed=1):
    """ChainBatch.sweep_trees over the chains' own trees; pairs of 2 lo .. 2 hi leaves; big = (chain, step, leaves of each tree)."""
    X, y, ft, noise, scale, log_q, log_u = problem(N, nc, steps, seed)
    span = hi - lo + 1
    old_n = lambda b, t: big[2] if big and (b, t) == big[:2] else lo + (b + t) % span
    new_n = lambda b, t: big[2] if big and (b, t) == big[:2] else lo + (2 * b + t + 1) % span
    old, new = trees(nc, steps, old_n, lambda b, t: (b + t) % D), trees(nc, steps, new_n, lambda b, t: (b + 3 * t + 1) % D)
    cb = dense_batch(old, noise, scale, X, y, ft)
    mask = cb.sweep_trees(old, new, log_q, log_u, X, ft, scale, steps, method=method)
    return {"accept": digest(mask), "last_accept": digest(cb.last_accept), "quad": digest(cb.quad), "logdet": digest(cb.logdet),
            "K_inv": digest(cb.K_inv), "accepted": int(mask.sum())}


def one_by_one():
    """propose_trees / accept with a pair above 64 leaves in chain 0: every chain goes through a ChainState on its slice."""
    N, nc, m = 96, 2, 2
    X, y, ft, noise, scale, _, _ = problem(N, nc, 1, 2)
    forests = trees(nc, m, lambda b, t: (40 if b == 0 else 3) if t == 0 else 2, lambda b, t: (b + t) % D)
    new = np.stack([caterpillar(40, 5), caterpillar(4, 6)])
    cb = dense_batch(forests, noise, scale, X, y, ft)
    out = {}
    for rnd, (old, mask) in enumerate(((forests[:, 0], [True, False]), (np.stack([new[0], forests[1, 0]]), [False, True]))):
        mll = cb.propose_trees(old, new, X, ft, scale, m)
        cb.accept(mask)
        out.update({f"mll_{rnd}_chain1": digest(mll[1]), f"quad_{rnd}_chain1": digest(cb.quad[1]), f"logdet_{rnd}": digest(cb.logdet),
                    f"K_inv_{rnd}": digest(cb.K_inv), f"mll_{rnd}_chain0_12_digits": float(f"{mll[0]:.12g}"),
                    f"quad_{rnd}_chain0_12_digits": float(f"{cb.quad[0]:.12g}")})
        new = np.stack([caterpillar(38, 2), caterpillar(5, 1)])
    return out


def dense_noise_scale():
    N, nc, m = 96, 3, 5
    X, y, ft, noise, scale, log_q, log_u = problem(N, nc, 1, 3)
    forests = trees(nc, m, lambda b, t: 2 + (b + t) % 5, lambda b, t: (b + 2 * t) % D)
    cb = dense_batch(forests, noise, scale, X, y, ft)
    mask = cb.step_noise_scale(forests, noise * np.array([1.2, 0.7, 1.05]), scale * np.array([0.9, 1.3, 1.0]), log_q[:, 0], log_u[:, 0], X, ft)
    return {"accept": digest(mask), "quad": digest(cb.quad), "logdet": digest(cb.logdet), "K_inv": digest(cb.K_inv)}


def leaf_chain():
    N, nc, m, steps = 200, 3, 4, 4
    X, y, ft, noise, scale, log_q, log_u = problem(N, nc, steps, 4)
    forests = trees(nc, m, lambda b, t: 2 + (b + t) % 5, lambda b, t: (b + t) % D)
    tidx = np.array([0, 1, 0, 2])
    new = trees(nc, steps, lambda b, t: 2 + (2 * b + t + 1) % 6, lambda b, t: (b + 3 * t + 1) % D)
    old = forests[:, tidx].copy()
    old[:, 2] = new[:, 0]  # the second swap of tree 0 (only the first is checked against the chain)
    cb = fit.LeafChainBatch.from_forests(forests, noise, scale, X, y, ft, capacity=64)
    out = {"quad_0": digest(cb.quad), "logdet_0": digest(cb.logdet)}
    mask = cb.sweep_trees(old, new, log_q, log_u, X, ft, scale, m, tree_index=tidx)
    out.update({"accept": digest(mask), "last_accept": digest(cb.last_accept), "quad_1": digest(cb.quad), "logdet_1": digest(cb.logdet),
                "nleaves_1": digest(cb.nleaves), "accepted": int(mask.sum())})
    mask = cb.step_noise_scale(noise * np.array([1.2, 0.7, 1.05]), scale * np.array([0.9, 1.3, 1.0]), log_q[:, 0], log_u[:, 0])
    ex = cb.export()
    out.update({"accept_ns": digest(mask), "quad_2": digest(cb.quad), "logdet_2": digest(cb.logdet), "noise": digest(cb.noise),
                "scale": digest(cb.scale), "P": digest(ex["P"]), "v": digest(ex["v"]), "nleaves": digest(ex["nleaves"])})
    return out


def single_chain():
    N, m = 96, 3
    X, y, ft, noise, scale, _, _ = problem(N, 1, 1, 5)
    forest = trees(1, m, lambda b, t: 3 + t, lambda b, t: t)[0]
    st = fit.ChainState.from_forest(forest, noise[0], scale[0], X, y, ft)
    st.quad = host_quad(st.K_inv, y)
    val = st.propose_tree(forest[1], caterpillar(6, 7), X, ft, scale[0], m)
    st.accept()
    return {"mll": digest(np.float64(val)), "quad": digest(np.float64(st.quad)), "logdet": digest(np.float64(st.logdet)),
            "K_inv": digest(st.K_inv)}


CASES = {
    "launches N=128 3 chains 4 steps <=16 leaves (one sequence)": lambda: dense_sweep(128, 3, 4, 2, 8, "launches"),
    "launches N=129 (per-chain streams: odd N)": lambda: dense_sweep(129, 3, 4, 2, 8, "launches"),
    "launches N=128 one pair of 20 leaves (per-chain streams: r > 16)": lambda: dense_sweep(128, 3, 4, 2, 8, "launches", big=(1, 2, 10)),
    "resident N=64 2 chains 4 steps <=8 leaves": lambda: dense_sweep(64, 2, 4, 2, 4, "resident"),
    "propose_trees + accept, a pair above 64 leaves, N=96 2 chains": one_by_one,
    "ChainBatch.step_noise_scale N=96 3 chains m=5": dense_noise_scale,
    "LeafChainBatch from_forests, sweep_trees, step_noise_scale N=200 3 chains m=4 capacity 64": leaf_chain,
    "ChainState.propose_tree + accept N=96": single_chain,
}


def time_sweeps(reps=20, warm=3):
    """Wall ms per sweep_trees call (it ends in its read-back, so the device has finished), each on a fresh batch built outside."""
    nc, m = 4, 50
    out = {}
    for name, N in (("ChainBatch.sweep_trees N=128 4 chains 50 steps", 128), ("LeafChainBatch.sweep_trees N=256 4 chains m=50 50 steps", 256)):
        X, y, ft, noise, scale, log_q, log_u = problem(N, nc, m, 6)
        old = trees(nc, m, lambda b, t: 2 + (b + t) % 3, lambda b, t: (b + t) % D)
        new = trees(nc, m, lambda b, t: 2 + (2 * b + t + 1) % 3, lambda b, t: (b + 3 * t + 1) % D)
        Xd = torch.from_numpy(X).cuda()
        ms = []
        for _ in range(warm + reps):
            if name.startswith("Leaf"):
                cb = fit.LeafChainBatch.from_forests(old, noise, scale, Xd, y, ft, capacity=(4 * m + 31) // 32 * 32, lcap=8)
            else:
                cb = fit.ChainBatch.from_forests(old, noise, scale, Xd, y, ft)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cb.sweep_trees(old, new, log_q, log_u, Xd, ft, scale, m)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = np.array(ms[warm:])
        out[name] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs an MI355X"
    result = {name: case() for name, case in CASES.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, r in result.items():
        print(name, {k: (v[:12] if isinstance(v, str) else v) for k, v in r.items()}, flush=True)
    if "--time" in sys.argv[2:]:
        print("TIME", json.dumps(time_sweeps()), flush=True)
