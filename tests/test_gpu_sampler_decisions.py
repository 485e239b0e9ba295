"""The Metropolis decision of every device path of the sampler on the same edge inputs: the multi-launch sweep, the one-launch
sweep and the leaf-space sweep (ChainBatch.sweep_trees with both methods, LeafChainBatch.sweep_trees), and the two noise/scale steps.
They all decide through metropolis_accept (csrc/sampler_step.h; tests/test_sampler_step_cpu.py holds the function itself to
Python's rule), so on a NaN, on +-inf and at log_u just above zero every path must return the same flags.  The MLL differences of
this small, well-conditioned problem are finite, so the expected flags follow from the rule alone: no tolerance is involved."""
import math

import numpy as np
import pytest

import lowrank_ref as lr

pytestmark = pytest.mark.gpu

N, D, M, NC, STEPS = 24, 2, 2, 4, 2
# one edge per chain:  log_q_prior, log_u, accepted?
EDGES = ((math.nan, math.log(0.5), 0), (math.inf, 0.0, 1), (math.inf, 5e-324, 0), (-math.inf, -1.0, 0))
LOG_Q = np.array([e[0] for e in EDGES])
LOG_U = np.array([e[1] for e in EDGES])
WANT = np.array([e[2] for e in EDGES], dtype=bool)


@pytest.fixture(scope="module")
def problem():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd import synthetic

    X, y, _, ft = synthetic.unit_cube_problem(N, D, seed=24002)
    forests = np.stack([np.stack([lr.caterpillar_tree(2 + (b + t) % 2, (b + t) % D) for t in range(M)]) for b in range(NC)])
    # the proposal of a tree splits the other feature, so two accepted steps do not give the initial forest back
    new = np.stack([np.stack([lr.caterpillar_tree(2 + (b + t) % 2, (b + t + 1) % D) for t in range(STEPS)]) for b in range(NC)])
    noise, scale = np.array([0.1, 0.12, 0.09, 0.11]), np.array([1.0, 0.9, 1.1, 1.2])
    return dict(X=X, y=y.reshape(-1), ft=ft, forests=forests, new=new, noise=noise, scale=scale)


def _batch(kind, p):
    import bark_amd.fitting as fit

    if kind == "leaf":
        return fit.LeafChainBatch.from_forests(p["forests"], p["noise"], p["scale"], p["X"], p["y"], p["ft"], capacity=32, lcap=4)
    return fit.ChainBatch.from_forests(p["forests"], p["noise"], p["scale"], p["X"], p["y"], p["ft"])


def _check(path, cb, before, mask):
    quad, logdet = before
    assert np.isfinite(quad).all() and np.isfinite(logdet).all()
    want = WANT if mask.ndim == 1 else np.repeat(WANT[:, None], mask.shape[1], axis=1)
    assert np.array_equal(mask, want), (path, mask)
    rejected = ~WANT
    assert cb.quad[rejected].tobytes() == quad[rejected].tobytes() and cb.logdet[rejected].tobytes() == logdet[rejected].tobytes(), path
    assert np.isfinite(cb.quad).all() and np.isfinite(cb.logdet).all(), path  # the accepted chain moved to a finite state
    assert cb.quad[WANT].tobytes() != quad[WANT].tobytes(), path


@pytest.mark.parametrize("path", ["launches", "resident", "leaf"])
def test_tree_sweeps_decide_the_edges_alike(problem, path):
    p = problem
    cb = _batch(path, p)
    before = cb.quad.copy(), cb.logdet.copy()
    lq, lu = np.repeat(LOG_Q[:, None], STEPS, axis=1), np.repeat(LOG_U[:, None], STEPS, axis=1)
    args = (p["forests"][:, :STEPS], p["new"], lq, lu, p["X"], p["ft"], p["scale"], M)  # step t swaps tree t
    mask = cb.sweep_trees(*args) if path == "leaf" else cb.sweep_trees(*args, method=path)
    _check(path, cb, before, mask)
    assert np.array_equal(cb.last_accept, np.repeat(WANT[:, None].astype(np.int32), STEPS, axis=1))  # 0, never -1


@pytest.mark.parametrize("path", ["dense", "leaf"])
def test_noise_scale_steps_decide_the_edges_alike(problem, path):
    p = problem
    cb = _batch(path, p)
    before = cb.quad.copy(), cb.logdet.copy()
    new_noise, new_scale = 1.25 * p["noise"], 0.8 * p["scale"]
    if path == "leaf":
        mask = cb.step_noise_scale(new_noise, new_scale, LOG_Q, LOG_U)
    else:
        mask = cb.step_noise_scale(p["forests"], new_noise, new_scale, LOG_Q, LOG_U, p["X"], p["ft"])
    _check(path, cb, before, mask)
