#!/usr/bin/env python3
"""Generate tests/golden/g12_tree_proposals.npz by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_golden_proposals.py

Every expected value is produced by the reference's own functions, imported through `_ref_shim.py` (identity-njit):
`get_node_subspace`, `terminal_nodes`, `singly_internal_nodes` (tree_traversal.py), `grow` / `prune` / `change`,
`tree_q_ratio`, `tree_prior_ratio` (tree_proposals.py), `sample_binary_mask` (bit_operations.py) and
`get_noise_scale_proposal` (noise_scale_proposals.py).  Only the INPUTS are chosen here: about 40 trees (prior draws over a
mixed d = 4 domain, root-only trees, a full 7-slot container) and, per tree, one explicit decision of each kind.  Trees are
stored as raw bytes of the packed 26-byte records, as in make_golden.py.
"""

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim  # noqa: E402

ref = _ref_shim.reference_modules()
TP, TT, DT = ref.tree_proposals, ref.tree_traversal, ref.forest.NODE_RECORD_DTYPE
import bark.fitting.noise_scale_proposals as NS  # noqa: E402
import bark.utils.bit_operations as BITS  # noqa: E402

CAT, INT, CONT = 0, 1, 2
BOUNDS = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 10.0], [0.0, 31.0]])  # 2 continuous, 1 integer, 1 categorical (5 categories)
FT = np.array([CONT, CONT, INT, CAT], dtype=np.int64)
ALPHA, BETA = 0.95, 2.0
PARAMS = types.SimpleNamespace(alpha=ALPHA, beta=BETA)
L = 100


def raw(nodes):
    nodes = np.ascontiguousarray(nodes)
    return nodes.view(np.uint8).reshape(*nodes.shape, DT.itemsize).copy()


def pad(ids, n):
    out = np.full(n, -1, dtype=np.int64)
    out[:len(ids)] = ids
    return out


def full_container():
    t = np.zeros(7, dtype=DT)
    for i in range(7):
        parent = 0xFFFFFFFF if i == 0 else (i - 1) // 2
        t[i] = (1, 0, 0, 0, 0, parent, 2, 1) if i >= 3 else (0, i % 2, 0.25 + 0.25 * i, 2 * i + 1, 2 * i + 2, parent, int(np.log2(i + 1)), 1)
    return t


def threshold_for(sub, f, k):
    """A rule value inside the node's subspace (an input of the fixture, not a reference draw)."""
    lo, hi = sub[f]
    if FT[f] == CAT:
        mask = int(hi)
        return float(mask & -mask) if mask else 1.0  # lowest available category
    if FT[f] == INT:
        return float(int(lo))
    return float(np.float32(lo + (0.25 + 0.1 * (k % 5)) * (hi - lo)))


def main():
    np.random.seed(12)
    forest = ref.prior._sample_single_forest(36, BOUNDS, FT, ALPHA, BETA, np.random.default_rng(12))
    trees = [forest[j] for j in range(36)] + [ref.empty_forest(1, L)[0] for _ in range(2)]
    # pruned records: prune a node of the first six trees that have one, then keep the result as a tree of its own
    for t in list(trees[:36]):
        si = TT.singly_internal_nodes(t)
        if len(si) and len(trees) < 44:
            prop = TP.NodeProposal()
            prop.node_idx = int(si[0])
            trees.append(TP.prune(t.copy(), prop))
    trees = np.stack(trees)
    T = trees.shape[0]
    rows = []  # one row per decision
    term = np.stack([pad(TT.terminal_nodes(t), L) for t in trees])
    single = np.stack([pad(TT.singly_internal_nodes(t), L) for t in trees])
    for k, t in enumerate(trees):
        for kind, kind_enum in ((0, TP.TreeProposalEnum.Grow), (1, TP.TreeProposalEnum.Prune), (2, TP.TreeProposalEnum.Change)):
            valid = TT.terminal_nodes(t) if kind == 0 else TT.singly_internal_nodes(t)
            if len(valid) == 0:
                continue
            node = int(valid[k % len(valid)])
            f = k % 4
            sub = TT.get_node_subspace(t, node, BOUNDS, FT)
            thr = threshold_for(sub, f, k)
            prop = TP.NodeProposal()
            prop.node_idx, prop.new_feature_idx, prop.new_threshold = node, f, thr
            log_q = TP.tree_q_ratio(t, kind_enum, prop)
            prop.node_idx = node
            log_prior = TP.tree_prior_ratio(t, kind_enum, prop, PARAMS)
            new = [TP.grow, TP.prune, TP.change][kind](t.copy(), prop)
            rows.append((k, kind, node, f, thr, float(log_q), float(log_prior), raw(new), np.asarray(sub, dtype=np.float64)))
    full = full_container()
    prop = TP.NodeProposal()
    prop.node_idx, prop.new_feature_idx, prop.new_threshold = 3, 0, 0.1
    try:
        TP.grow(full.copy(), prop)
        overflow = 0
    except OverflowError:
        overflow = 1

    # sample_binary_mask: the reference's map from its integer draw to a mask, the draw handed in through np.random.randint
    masks, real_randint = [], np.random.randint
    try:
        for avail in (0b11111, 0b10110, 0b00011, 0b01000, 0, 0b11001):
            k = bin(avail).count("1")
            for draw in range(1, max((1 << k) - 1, 1)):
                np.random.randint = lambda lo, hi, _d=draw: _d  # noqa: E731
                masks.append((avail, draw if k >= 2 else 0, BITS.sample_binary_mask(avail), (1 << k) - 1 if k >= 2 else 0))
    finally:
        np.random.randint = real_randint

    # get_noise_scale_proposal on seeded inputs, the three parameter branches: (use_softplus_transform, sample_scale)
    ns = []
    for branch, (softplus, sample_scale) in enumerate(((True, False), (True, True), (False, True))):
        p = types.SimpleNamespace(use_softplus_transform=softplus, sample_scale=sample_scale, gamma_prior_shape=2.5,
                                  gamma_prior_rate=9.0)
        for j, (noise, scale) in enumerate(((0.1, 1.0), (0.5, 0.7), (0.02, 2.5), (1.5, 1.2))):
            np.random.seed(100 * branch + j)
            z = np.random.normal(size=2)  # the normals the call below draws, in its order: noise, then scale
            np.random.seed(100 * branch + j)
            (new_noise, new_scale), lqp = NS.get_noise_scale_proposal(noise, scale, p)
            ns.append((branch, int(softplus), int(sample_scale), noise, scale, z[0], z[1], float(new_noise), float(new_scale), float(lqp)))

    meta = {"src": "bark.fitting.tree_proposals / tree_traversal / noise_scale_proposals, bark.utils.bit_operations (reference, via _ref_shim)",
            "alpha": ALPHA, "beta": BETA, "L": L,
            "rows": "tree, kind, node, feature", "ns": "branch, use_softplus, sample_scale, noise, scale, z_noise, z_scale, new_noise, new_scale, log_q_prior",
            "masks": "available, draw, mask, randint upper bound (exclusive)"}
    path = os.path.join(HERE, "g12_tree_proposals.npz")
    np.savez_compressed(
        path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), bounds=BOUNDS, feat_types=FT, trees=raw(trees),
        terminal=term, singly_internal=single,
        rows=np.array([r[:4] for r in rows], dtype=np.int64), thresholds=np.array([r[4] for r in rows], dtype=np.float64),
        log_q=np.array([r[5] for r in rows]), log_prior=np.array([r[6] for r in rows]), new_trees=np.stack([r[7] for r in rows]),
        subspaces=np.stack([r[8] for r in rows]), full_container=raw(full), full_container_overflows=np.array(overflow),
        masks=np.array(masks, dtype=np.int64), noise_scale=np.array(ns, dtype=np.float64))
    print(f"wrote {path} ({os.path.getsize(path)} B): {T} trees, {len(rows)} decisions, {len(masks)} masks, {len(ns)} noise/scale rows")


if __name__ == "__main__":
    main()
