"""Host reference of the acquisition scan (numpy and the oracle only, no GPU) and the case table shared by
tests/test_acquisition_cpu.py and tests/test_gpu_acquisition.py.

The reference's end-to-end test defines the acquisition (tests/optimization/test_optimality.py:60-63):
    lcb_mean(x)    = mean_b ( mu_b(x) - kappa sqrt(var_b(x)) )
    lcb_mixture(x) = mu_mix(x) - kappa sqrt(var_mix(x)),  (mu_mix, var_mix) = mixture_of_gaussians_as_normal(mu, var)
with mu, var (B, C) from `forest_predict`.  Here they come from the oracle's dense `forest_predict` (LU inverse of the
N x N matrix) and are reduced in float64 and in np.longdouble.

Every GPU case is pre-checked on the host (`precheck`): both precisions agree on the arg-min, the best value is at
least MARGIN below every other candidate's (so the device index has to be identical, not close), and every var_b(x)
is at least VAR_FLOOR (so the square root does not amplify the posterior's error bar)."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from bark_amd import synthetic
from bark_amd.forest import create_empty_forest
from bark_amd.optimizer import acquisition_plan
from oracle import oracle as orc

KINDS = ("lcb_mean", "lcb_mixture")
RTOL, ATOL = 1e-9, 1e-8  # the posterior bar of DESIGN.md section 2
MARGIN = 1e-6
VAR_FLOOR = 1e-3
TILE = 256  # candidates per workgroup of acq_scan_kernel (bark_amd/csrc/acquire.hip)
NODE_LIMIT = 255
POSTERIOR_BLOCK = 2048  # candidates per call of the oracle (every case of CASES: one call)
D_CONT = 4  # mixed_problem(d_cont=4, n_int=2, n_cat=2): d = 8; the complete trees split on the continuous columns


def acquisition(mu, var, kappa, kind, dtype=np.float64):
    mu, var = np.asarray(mu, dtype=dtype), np.asarray(var, dtype=dtype)
    kappa = dtype(kappa)
    if kind == "lcb_mean":
        return np.mean(mu - kappa * np.sqrt(np.maximum(var, 0)), axis=0)
    mu_y = np.mean(mu, axis=0)
    var_y = np.mean(var + mu**2, axis=0) - mu_y**2
    return mu_y - kappa * np.sqrt(np.maximum(var_y, 0))


@lru_cache(maxsize=None)
def lds_limit(m: int) -> int:
    """Largest R whose table the scan keeps in LDS at m trees, from the plan query."""
    lo, hi = 1, 8192
    assert acquisition_plan(lo, m)["variant"] == "lds" and acquisition_plan(hi, m)["variant"] == "global"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if acquisition_plan(mid, m)["variant"] == "lds" else (lo, mid)
    return lo


def depths_for(R: int, m: int):
    """m complete trees of depth <= 7 with R leaves in total: greedy, the largest trees first."""
    left, out = R - m, []
    for t in range(m):
        d = 7
        while (1 << d) - 1 > left:
            d -= 1
        out.append(d)
        left -= (1 << d) - 1
    assert left == 0, (R, m)
    return out


@dataclass(frozen=True)
class Case:
    """forest: ("prior", m), ("full", m, depth) (complete trees: R = m 2^depth) or ("leaves", m, R) (complete trees of
    decreasing depth, then null trees) with R an int or "lds_limit" / "lds_limit+1" (resolved from the plan query);
    chunk: forests per chunk (None: all)."""

    name: str
    forest: tuple
    N: int
    B: int
    C: int
    chunk: int | None = None
    kappa: float = 1.96
    seed: int = 0

    @property
    def m(self):
        return self.forest[1]


CASES = {c.name: c for c in [
    # prior-sized forests (R about 140: the LDS variant), a few tiles and a ragged tail
    Case("prior_n64", ("prior", 50), N=64, B=3, C=4 * TILE + 77, seed=1),
    # three chunks (2 + 2 + 1 forests), one candidate past the tile
    Case("prior_n257_chunks", ("prior", 50), N=257, B=5, C=TILE + 1, chunk=2, seed=2),
    # one tree, two code words exactly; a single candidate
    Case("m1_r64", ("leaves", 1, 64), N=64, B=1, C=1, seed=3),
    # one leaf past the code-word edge (three words)
    Case("m2_r65", ("leaves", 2, 65), N=64, B=3, C=5, seed=4),
    # the largest table the LDS holds at 13 trees, and one leaf more (global variant); one below / at the tile
    Case("m13_lds_limit", ("leaves", 13, "lds_limit"), N=257, B=3, C=TILE - 1, seed=5),
    Case("m13_past_lds", ("leaves", 13, "lds_limit+1"), N=64, B=1, C=TILE, seed=6),
    # the tree limit, LDS variant (R = 128) and global variant (R = 256)
    Case("m64_r128", ("full", 64, 1), N=64, B=3, C=300, kappa=0.5, seed=7),
    Case("m64_r256", ("full", 64, 2), N=257, B=1, C=64, seed=8),
]}


# Two passes of the scan's candidate slab loop (65 536 candidates per slab) over two chunks of forests.  Not in CASES: among
# so many candidates under 2-tree forests many share all their leaves, so no arg-min is MARGIN apart (precheck).
SLAB_CASE = Case("slab_c65537", ("prior", 2), N=20, B=3, C=(1 << 16) + 1, chunk=2, seed=9)


def resolve_R(case: Case):
    if case.forest[0] == "prior":
        return None
    if case.forest[0] == "full":
        return case.m << case.forest[2]
    R = case.forest[2]
    if R == "lds_limit":
        return lds_limit(case.m)
    if R == "lds_limit+1":
        return lds_limit(case.m) + 1
    return R


@dataclass
class Inputs:
    case: Case
    F: np.ndarray
    X: np.ndarray
    y: np.ndarray
    ft: np.ndarray
    cand: np.ndarray
    noise: np.ndarray
    scale: np.ndarray

    @property
    def model(self):
        return self.F, self.noise, self.scale

    @property
    def data(self):
        return self.X, self.y


def problem(N, seed):
    return synthetic.mixed_problem(N, seed=seed, d_cont=D_CONT, n_int=2, n_cat=2)


@lru_cache(maxsize=None)
def make_inputs(name) -> Inputs:
    """of a case of CASES by name, or of a Case"""
    case = CASES[name] if isinstance(name, str) else name
    X, y, bounds, ft = problem(case.N, 100 + case.seed)
    cand, _, _, _ = problem(case.C, 200 + case.seed)
    rng = np.random.default_rng(case.seed)
    forests = []
    for _ in range(case.B):
        if case.forest[0] == "prior":
            forests.append(synthetic.sample_prior_forest(case.m, bounds, ft, rng, node_limit=NODE_LIMIT))
        elif case.forest[0] == "full":
            forests.append(synthetic.full_binary_forest(case.m, D_CONT, case.forest[2], rng, node_limit=NODE_LIMIT))
        else:
            parts = [synthetic.full_binary_forest(1, D_CONT, dep, rng, node_limit=NODE_LIMIT) if dep
                     else create_empty_forest(1, NODE_LIMIT) for dep in depths_for(resolve_R(case), case.m)]
            forests.append(np.concatenate(parts, axis=0))
    noise = np.linspace(0.1, 0.3, case.B)
    scale = np.linspace(0.8, 1.3, case.B)
    return Inputs(case, np.stack(forests), X, y, ft, cand, noise, scale)


@lru_cache(maxsize=None)
def posterior(name):
    """(mu, var) (B, C) of the oracle's dense route; computed once per case and shared"""
    inp = make_inputs(name)
    # the oracle forms the full (B, C, C) covariance before it takes the diagonal: blocks of candidates bound it (a
    # candidate's posterior does not depend on the other candidates)
    parts = [orc.forest_predict(inp.model, inp.data, inp.cand[i:i + POSTERIOR_BLOCK], inp.ft)
             for i in range(0, inp.case.C, POSTERIOR_BLOCK)]
    mu = np.concatenate([p[0] for p in parts], axis=1)
    var = np.concatenate([p[1] for p in parts], axis=1)
    mu.setflags(write=False)
    var.setflags(write=False)
    return mu, var


def reference(name, kind: str, dtype=np.float64):
    mu, var = posterior(name)
    return acquisition(mu, var, make_inputs(name).case.kappa, kind, dtype)


def precheck(name: str):
    """-> {kind: (values float64 (C,), arg-min)}; raises AssertionError where a case is unfit for an exact index test."""
    mu, var = posterior(name)
    assert var.min() >= VAR_FLOOR, (name, float(var.min()))
    out = {}
    for kind in KINDS:
        v64 = reference(name, kind)
        vld = reference(name, kind, np.longdouble)
        i = int(np.argmin(v64))
        assert i == int(np.argmin(vld)), (name, kind)
        assert np.allclose(v64, vld.astype(np.float64), rtol=1e-12, atol=1e-12), (name, kind)
        if v64.size > 1:
            gap = float(np.delete(v64, i).min() - v64[i])
            assert gap >= MARGIN, (name, kind, gap)
        out[kind] = (v64, i)
    return out
