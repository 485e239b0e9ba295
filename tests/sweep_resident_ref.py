"""Cases of the one-launch tree sweep (csrc/sweep_resident.hip, ChainBatch.sweep_trees(method="resident")) and their host
trajectory (numpy + the oracle: no GPU, no library).  tests/test_sweep_resident_cpu.py holds every case to the decision-margin
condition; tests/test_gpu_sweep_resident.py runs them on the device.

A case is a sweep of `steps` trees for `nc` chains on N points: step t swaps tree t of every chain's forest (m = steps trees)
for a proposal.  Trees are lowrank_ref.caterpillar_tree, so the leaf counts of a pair are exact."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import lowrank_ref as lr

MARGIN = 1e-6  # |log_u - log_alpha| of every ordinary proposal: a condition on the inputs, never lowered


class Case(NamedTuple):
    N: int
    nc: int
    steps: int
    leaves: tuple  # leaves[b][t] = (leaves of the old tree, leaves of the new tree)
    seed: int
    why: str


def _rows(nc, per_step):
    return tuple(tuple(per_step[(b + t) % len(per_step)] for t in range(len(per_step))) for b in range(nc))


def _varied_rows(nc, steps):
    base = lr.CHAIN_CASES["grid_nc64"].leaves  # lowrank_ref._varied(64): 2 .. 12 leaves per pair, a per-chain r_old
    return tuple(tuple(base[(b + 7 * t) % len(base)] for t in range(steps)) for b in range(nc))


CASES = {
    "n3": Case(3, 1, 2, (((1, 1), (1, 2)),), 0, "fewer points than threads; single-leaf trees"),
    "n64": Case(64, 2, 4, _rows(2, ((1, 1), (2, 3), (3, 4), (4, 4))), 0, "inside the LDS variant, 2 .. 8 leaves"),
    "n127": Case(127, 3, 4, _rows(3, ((4, 4), (4, 5), (5, 4), (3, 5))), 0, "odd N in LDS; both sides of the 8 / 9 rank boundary"),
    "n128": Case(128, 64, 3, _varied_rows(64, 3), 0, "LDS limit; full grid; per-chain r_old"),
    "n129": Case(129, 3, 4, _rows(3, ((7, 8), (8, 8), (8, 7), (9, 7))), 0, "first global-variant N; odd; largest rank"),
    "n256": Case(256, 2, 4, _rows(2, ((3, 3), (2, 4), (4, 2), (3, 3))), 0, "several row segments per column"),
    "n511": Case(511, 1, 3, _rows(1, ((3, 3), (2, 4), (4, 2))), 1, "odd, near the limit"),
    "n512": Case(512, 2, 3, _rows(2, ((8, 8), (7, 9), (9, 7))), 0, "the limit, 16 leaves"),
}


class Inputs(NamedTuple):
    X: np.ndarray
    y: np.ndarray
    ft: np.ndarray
    cur: np.ndarray  # (nc, steps, node_limit) the forests; tree t is replaced at step t
    prop: np.ndarray  # (nc, steps, node_limit)
    noise: np.ndarray
    scale: np.ndarray
    log_q: np.ndarray  # (nc, steps)
    log_u: np.ndarray


def make_inputs(name, seed=None) -> Inputs:
    from bark_amd import synthetic

    case = CASES[name]
    seed = case.seed if seed is None else seed
    X, y, _, ft = synthetic.unit_cube_problem(case.N, lr.CHAIN_D, seed=1000 * case.N + seed)
    cur = np.stack([np.stack([lr.caterpillar_tree(case.leaves[b][t][0], (b + t) % lr.CHAIN_D) for t in range(case.steps)])
                    for b in range(case.nc)])
    prop = np.stack([np.stack([lr.caterpillar_tree(case.leaves[b][t][1], (b + 2 * t + 1) % lr.CHAIN_D) for t in range(case.steps)])
                     for b in range(case.nc)])
    rng = np.random.default_rng([case.N, case.nc, seed])
    noise, scale = rng.uniform(0.05, 0.2, case.nc), rng.uniform(0.7, 1.4, case.nc)
    log_q = rng.normal(0.0, 0.5, size=(case.nc, case.steps))
    log_u = np.log(rng.uniform(size=(case.nc, case.steps)))
    return Inputs(X, y, ft, cur, prop, noise, scale, log_q, log_u)


class Trajectory(NamedTuple):
    mask: np.ndarray  # (nc, steps) 0 / 1
    margin: np.ndarray  # (nc, steps) |log_u - log_alpha|, inf where either is not finite
    quad: np.ndarray  # (nc,) after the sweep
    logdet: np.ndarray


def host_sweep(inp: Inputs, dtype=np.float64, chains=None) -> Trajectory:
    """The sweep on the host: lowrank_ref.swap + lowrank_ref.metropolis per proposal, K_inv carried in `dtype`."""
    from oracle import oracle as orc

    nc, steps = inp.log_q.shape
    N = inp.X.shape[0]
    y = inp.y.reshape(-1)
    mask = np.zeros((nc, steps), dtype=np.int32)
    margin = np.full((nc, steps), np.inf)
    quad, logdet = np.zeros(nc), np.zeros(nc)
    for b in (range(nc) if chains is None else chains):
        K = inp.scale[b] * orc.forest_gram_matrix(inp.cur[b], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[b]) * np.eye(N)
        K_inv = np.linalg.inv(K)
        K_inv = (0.5 * (K_inv + K_inv.T)).astype(dtype)
        ld = dtype(np.linalg.slogdet(K)[1])
        q = (y.astype(dtype) @ K_inv @ y.astype(dtype))
        s = np.sqrt(inp.scale[b] / steps)
        for t in range(steps):
            U_old = s * orc.get_leaf_vectors(inp.cur[b, t], inp.X, inp.ft)
            U_new = s * orc.get_leaf_vectors(inp.prop[b, t], inp.X, inp.ft)
            dquad, dlogdet, K_new = lr.swap(K_inv, np.concatenate([U_old, U_new], axis=1), U_old.shape[1], y, dtype)
            log_alpha = inp.log_q[b, t] + 0.5 * (float(dquad) - float(dlogdet))
            if np.isfinite(log_alpha) and np.isfinite(inp.log_u[b, t]):
                margin[b, t] = abs(inp.log_u[b, t] - log_alpha)
            mask[b, t] = lr.metropolis(float(dquad), float(dlogdet), inp.log_q[b, t], inp.log_u[b, t])
            if mask[b, t] == 1:
                K_inv, q, ld = K_new, q - dquad, ld + dlogdet
        quad[b], logdet[b] = float(q), float(ld)
    return Trajectory(mask, margin, quad, logdet)


def nan_inputs(N) -> Inputs:
    """The inputs of test_gpu_lowrank.test_device_decision_rejects_nan at another N: 3 chains x 4 steps, one NaN log_u and one
    NaN log_q_prior."""
    from bark_amd import synthetic

    nc, steps = 3, 4
    X, y, _, ft = synthetic.unit_cube_problem(N, lr.CHAIN_D, seed=N)
    cur = np.stack([np.stack([lr.caterpillar_tree(2 + (b + t) % 4, (b + t) % lr.CHAIN_D) for t in range(steps)]) for b in range(nc)])
    prop = np.stack([np.stack([lr.caterpillar_tree(1 + (2 * b + t) % 5, (b + 2 * t + 1) % lr.CHAIN_D) for t in range(steps)])
                     for b in range(nc)])
    noise, scale = np.array([0.1, 0.07, 0.2]), np.array([1.0, 0.8, 1.2])
    rng = np.random.default_rng(11)
    log_q = rng.normal(0.0, 0.5, size=(nc, steps))
    log_u = np.log(rng.uniform(size=(nc, steps)))
    log_u[0, 1] = np.nan
    log_q[1, 2] = np.nan
    return Inputs(X, y, ft, cur, prop, noise, scale, log_q, log_u)
