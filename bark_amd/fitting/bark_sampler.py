"""The BARK sampler (reference: src/bark/fitting/bark_sampler.py, `run_bark_sampler`), all chains in lock step.

Per step: ONE launch draws the proposals of every tree of every chain (`tree_proposals`), the existing sweep of
`LeafChainBatch` or `ChainBatch` decides them on the device, a second launch copies the accepted trees over the forests, which
stay resident in HBM between steps, and the noise / scale half follows (`noise_scale_proposals`, `step_noise_scale`).  The
proposals come back to the host once per step because the sweeps' packer and step tables are host code; a step loop that never
returns to the host and the BoFire glue (domain objects) are not part of this module.  Multi-fidelity problems need no sampler
of their own: the fidelity is an input column the trees split on like any other, and which fidelity to evaluate is chosen from
the fitted posterior (`bark_amd.optimizer.propose_fidelity_information_based`).

Random numbers are Philox4x32-10 addressed by (seed, step, chain, tree): a run is a function of its seed, and is not the
reference's numba stream."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .. import _lib
from ..forest import _as_nodes, _feat_types
from . import _chains, noise_scale_proposals as nsp, tree_proposals as tp
from .incremental import MAX_RANK, ChainBatch
from .leafchain import LeafChainBatch, leafchain_plan

DENSE_MAX_LEAVES = 8  # default of method="dense": 16 leaves per [old, new] pair


@dataclass
class BARKTrainParams:  # bark_sampler.py:17-46
    # MCMC run parameters
    warmup_steps: int = 50
    num_samples: int = 5
    steps_per_sample: int = 10

    # noise and scale proposal parameters
    use_softplus_transform: bool = True
    sample_scale: bool = False
    gamma_prior_shape: float = 2.5
    gamma_prior_rate: float = 9.0

    # node depth prior
    alpha: float = 0.95
    beta: float = 2.0

    # transition type probabilities
    grow_prune_weight: float = 0.5
    change_weight: float = 1.0

    num_chains: int = 1
    verbose: bool = False

    @property
    def proposal_weights(self):
        p = np.array([self.grow_prune_weight, self.grow_prune_weight, self.change_weight])
        return p / np.sum(p)


class _Run:
    """Everything `run_bark_sampler` checks and builds before the first step; `step()` is one step of every chain."""

    def __init__(self, model, data, bounds, params, feat_types, seed, method, max_leaves):
        import torch

        if method not in ("leafspace", "dense"):
            raise ValueError(f"unknown method {method!r} (use 'leafspace' or 'dense')")
        if feat_types is None:
            raise TypeError("run_bark_sampler takes the (d, 2) bounds array in the reference's bitmask encoding together with "
                            "feat_types; domain objects are not supported")
        forest, noise, scale = model
        self.X, y = data
        self.bounds, self.ft = tp.check_bounds(bounds, feat_types)
        self.forest = _as_nodes(forest, 3).copy()
        if self.forest.ndim != 3:
            raise ValueError(f"model forest must be (chains, m, node_limit) records, got {self.forest.shape}")
        self.nc, self.m, self.L = (int(v) for v in self.forest.shape)
        self.params, self.seed, self.method = params, int(seed), method
        if int(params.num_chains) != self.nc:
            raise ValueError(f"params.num_chains = {params.num_chains}, the model holds {self.nc} chains")
        if min(int(params.warmup_steps), int(params.steps_per_sample)) < 0 or int(params.num_samples) < 1 or (
                int(params.steps_per_sample) < 1):
            raise ValueError("warmup_steps >= 0, num_samples >= 1 and steps_per_sample >= 1")
        self.n_steps = int(params.warmup_steps) + int(params.num_samples) * int(params.steps_per_sample)
        if self.n_steps > 2 ** 32 - 1:
            raise ValueError("more than 2^32 - 1 steps")
        nsp._check(params)
        self.noise = _chains.per_chain("noise", noise, self.nc).copy()
        self.scale = _chains.per_chain("scale", scale, self.nc).copy()
        leaves = int(_chains.leaf_counts(self.forest, self.ft).max())
        if method == "leafspace":
            limits = leafchain_plan(1, 1, 1, 1)
            lcap = limits["max_leaves"] if max_leaves is None else int(max_leaves)
            if not 1 <= lcap <= limits["max_leaves"]:
                raise ValueError(f"method='leafspace': max_leaves must be 1..{limits['max_leaves']} (got {lcap})")
            if self.m > limits["max_trees"]:
                raise ValueError(f"method='leafspace' supports at most {limits['max_trees']} trees (got {self.m})")
            if self.m * lcap > limits["max_slots"]:  # the largest capacity the plan allows, with the max_leaves that matches it
                if max_leaves is not None:
                    raise ValueError(f"method='leafspace': {self.m} trees of {lcap} leaves need {self.m * lcap} slots, at most "
                                     f"{limits['max_slots']}; pass max_leaves <= {limits['max_slots'] // self.m}")
                lcap = limits["max_slots"] // self.m
            capacity = min(limits["max_slots"], (self.m * lcap + 31) // 32 * 32)
            self.max_leaves = lcap
        else:
            self.max_leaves = DENSE_MAX_LEAVES if max_leaves is None else int(max_leaves)
            if not 1 <= self.max_leaves <= MAX_RANK // 2:
                raise ValueError(f"method='dense': max_leaves must be 1..{MAX_RANK // 2} (got {self.max_leaves})")
        if leaves > self.max_leaves:
            raise ValueError(f"a tree of the model has {leaves} leaves, max_leaves is {self.max_leaves}")
        plan = tp.tree_proposals_plan(self.L, self.ft.shape[0], self.max_leaves, self.nc, self.m)
        if plan["reason"]:
            raise ValueError(plan["reason"])
        self.cparams = tp.proposal_params(params, self.max_leaves)
        if not 0.0 < float(params.alpha) < 1.0:
            raise ValueError(f"alpha = {params.alpha} is outside (0, 1)")
        w = np.asarray(params.proposal_weights, dtype=np.float64)
        if not (np.isfinite(w).all() and (w >= 0).all() and w.sum() > 0):
            raise ValueError("proposal_weights must be non-negative with a positive sum")
        if method == "leafspace":
            self.batch = LeafChainBatch.from_forests(self.forest, self.noise, self.scale, self.X, y, self.ft, capacity=capacity,
                                                     lcap=self.max_leaves)
        else:
            self.batch = ChainBatch.from_forests(self.forest, self.noise, self.scale, self.X, y, self.ft)
        self.nodes_d = tp.records_to_device(self.forest)
        self.bounds_d, self.ft_d = _lib.to_device(self.bounds), _lib.to_device(self.ft)
        self.tidx_d = torch.arange(self.m, dtype=torch.int64, device=self.nodes_d.device)
        self.step_index = 0
        self.log = None  # a list: step() appends what it fed the sweeps (tests replay it)

    def step(self):
        s = self.step_index
        new_d, lq_d, lu_d, _ = tp.propose_trees_device(self.nodes_d, self.bounds_d, self.ft_d, self.cparams, self.seed, s)
        new, lq, lu = tp.records_from_device(new_d), lq_d.cpu().numpy(), lu_d.cpu().numpy()
        if self.method == "leafspace":
            acc = self.batch.sweep_trees(self.forest, new, lq, lu, self.X, self.ft, self.batch.scale, self.m)
        else:
            acc = self.batch.sweep_trees(self.forest, new, lq, lu, self.X, self.ft, self.scale, self.m)
        tp.commit_trees_device(self.nodes_d, new_d, self.batch.last_accept_device, self.tidx_d)
        old = self.forest.copy() if self.log is not None else None
        self.forest[acc] = new[acc]  # bark_sampler.py:264, the host mirror of the commit
        z, ns_lu = nsp.draw_normals(self.seed, s, self.nc)
        (new_noise, new_scale), ns_lq = nsp.get_noise_scale_proposal(self.noise, self.scale, self.params, z)
        if self.method == "leafspace":
            took = self.batch.step_noise_scale(new_noise, new_scale, ns_lq, ns_lu)
        else:
            took = self.batch.step_noise_scale(self.forest, new_noise, new_scale, ns_lq, ns_lu, self.X, self.ft)
        if self.log is not None:
            self.log.append(dict(old=old, new=new, log_q_prior=lq, log_u=lu, accept=acc.copy(), noise=self.noise.copy(),
                                 scale=self.scale.copy(), new_noise=new_noise, new_scale=new_scale, ns_log_q_prior=ns_lq,
                                 ns_log_u=ns_lu, ns_accept=took.copy()))
        self.noise, self.scale = np.where(took, new_noise, self.noise), np.where(took, new_scale, self.scale)
        self.step_index += 1

    def run(self):
        p = self.params
        node_samples = np.empty((self.nc, int(p.num_samples), self.m, self.L), dtype=self.forest.dtype)
        noise_samples = np.empty((self.nc, int(p.num_samples)), dtype=np.float64)
        scale_samples = np.empty((self.nc, int(p.num_samples)), dtype=np.float64)
        for _ in range(int(p.warmup_steps)):
            self.step()
        for itr in range(int(p.num_samples)):
            for _ in range(int(p.steps_per_sample)):
                self.step()
            node_samples[:, itr] = self.forest
            noise_samples[:, itr], scale_samples[:, itr] = self.noise, self.scale
        return node_samples, noise_samples, scale_samples


def run_bark_sampler(model, data, domain_or_bounds, params, *, feat_types=None, seed: int = 0, method: str = "leafspace",
                     max_leaves=None):
    """Samples of the BARK posterior (bark_sampler.py:95-213): model = (forest (chains, m, node_limit) records, noise (chains,),
    scale (chains,)), data = (train_x (N, d), train_y), domain_or_bounds the (d, 2) bounds in the reference's bitmask encoding with
    feat_types (d,), params a `BARKTrainParams` -> (node_samples (chains, num_samples, m, node_limit), noise_samples (chains,
    num_samples), scale_samples (chains, num_samples)), the reference's return value.

    method="leafspace" (default) keeps the chains in leaf space (`LeafChainBatch`), method="dense" keeps their N x N inverses
    (`ChainBatch`).  max_leaves bounds every tree (a grow beyond it is a rejected proposal): default 32 in leaf space — less
    when m * max_leaves would exceed the 1024 slots of a chain — and 8 for the dense chains.  Every limit is checked before the
    first step (ValueError with the reason); nothing is refused in the middle of a run."""
    return _Run(model, data, domain_or_bounds, params, feat_types, seed, method, max_leaves).run()
