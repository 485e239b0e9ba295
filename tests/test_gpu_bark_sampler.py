"""`bark_amd.fitting.run_bark_sampler` on the device, both methods: N = 48, d = 4 mixed, 2 chains, m = 8, warm-up 2, 2 samples,
2 steps per sample, noise 0.1.

The run replays on the host: the proposals the device returned go through `leafchain_ref.RefChain` / `decide` and must give the
same accept masks and final forests.  That only says something if no decision is a coin toss between two roundings, so the
first test — no GPU — runs the whole trajectory on the host (proposals from tests/proposals_ref.py at the same seed, which are
the device's bit for bit in structure) in float64 and in longdouble and holds every decision margin to 1e-6, as
test_g11_trajectory_passes_the_precheck does for the recorded steps.  SEED is chosen so that it passes."""
import ctypes

import numpy as np
import pytest

import leafchain_ref as lc
import proposals_ref as pr

SEED = 3
N, NC, M, L, MAX_LEAVES = 48, 2, 8, 100, 8
STEPS = 2 + 2 * 2
_HOST = {}


def problem():
    rng = np.random.default_rng(48)
    X = np.stack([rng.uniform(size=N), rng.uniform(size=N), rng.integers(0, 11, size=N).astype(np.float64),
                  rng.integers(0, 5, size=N).astype(np.float64)], axis=1)
    y = rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    forests = pr.evolved_forests(NC, M, L, pr.MIXED_BOUNDS, pr.MIXED_FT, pr.Params(max_leaves=MAX_LEAVES), seed=21, sweeps=3)
    return X, y, forests, np.full(NC, 0.1), np.full(NC, 1.0)


def train_params():
    from bark_amd.fitting import BARKTrainParams

    return BARKTrainParams(warmup_steps=2, num_samples=2, steps_per_sample=2, num_chains=NC)


def replay(steps, dtype):
    """Feed per-step proposals through RefChain: steps[s] = (new (nc, m, L), log_q_prior, log_u, new_noise, new_scale, ns_log_q,
    ns_log_u) or a callable (s, forests, noise, scale) -> that tuple.  -> (accept (steps, nc, m), ns_accept (steps, nc), final
    forests, noise, scale, mll (nc,), smallest margin over the proposals with finite inputs)."""
    X, y, forests, noise, scale = problem()
    forests, noise, scale = forests.copy(), noise.copy(), scale.copy()
    chains = [lc.RefChain(forests[b], noise[b], scale[b], X, y, pr.MIXED_FT, M * MAX_LEAVES, dtype) for b in range(NC)]
    acc, ns_acc, margin = np.zeros((len(steps), NC, M), dtype=bool), np.zeros((len(steps), NC), dtype=bool), np.inf
    for s, step in enumerate(steps):
        new, lq, lu, new_noise, new_scale, ns_lq, ns_lu = step(s, forests, noise, scale) if callable(step) else step
        for b, ch in enumerate(chains):
            for t in range(M):
                delta, commit = ch.propose(t, new[b, t])
                if np.isfinite(lq[b, t]) and np.isfinite(lu[b, t]):
                    margin = min(margin, abs(lu[b, t] - (lq[b, t] + delta)))
                acc[s, b, t] = lc.decide(delta, lq[b, t], lu[b, t]) == 1
                if acc[s, b, t]:
                    commit()
                    forests[b, t] = new[b, t]
            delta, commit = ch.propose_noise_scale(new_noise[b], new_scale[b])
            margin = min(margin, abs(ns_lu[b] - (ns_lq[b] + delta)))
            ns_acc[s, b] = lc.decide(delta, ns_lq[b], ns_lu[b]) == 1
            if ns_acc[s, b]:
                commit()
                noise[b], scale[b] = new_noise[b], new_scale[b]
    return acc, ns_acc, forests, noise, scale, np.array([ch.mll for ch in chains]), float(margin)


def host_step(s, forests, noise, scale):
    """One step's proposals drawn on the host: the trees by proposals_ref, noise / scale by the product's host module."""
    from bark_amd.fitting import noise_scale_proposals as nsp

    p = train_params()
    new, lq, lu, _, _ = pr.propose_forests(forests, pr.MIXED_BOUNDS, pr.MIXED_FT, pr.Params(p.alpha, p.beta, tuple(p.proposal_weights), MAX_LEAVES),
                                           SEED, s)
    z, ns_lu = nsp.draw_normals(SEED, s, NC)
    (new_noise, new_scale), ns_lq = nsp.get_noise_scale_proposal(noise, scale, p, z)
    return new, lq, lu, new_noise, new_scale, ns_lq, ns_lu


def host(dtype=np.float64):
    if dtype not in _HOST:
        _HOST[dtype] = replay([host_step] * STEPS, dtype)
    return _HOST[dtype]


def test_host_trajectory_passes_the_precheck():
    """No GPU.  Every decision of the run at SEED has a margin of at least 1e-6 in float64 and in longdouble, and both make the
    same decisions: the device, whose sums differ by rounding, cannot legitimately decide otherwise."""
    f64, ext = host(np.float64), host(np.longdouble)
    print("margins: float64 %.3g, longdouble %.3g; accepted trees %d of %d, noise/scale %d of %d"
          % (f64[6], ext[6], f64[0].sum(), f64[0].size, f64[1].sum(), f64[1].size))
    assert f64[6] >= lc.MARGIN and ext[6] >= lc.MARGIN
    assert np.array_equal(f64[0], ext[0]) and np.array_equal(f64[1], ext[1]) and f64[2].tobytes() == ext[2].tobytes()
    assert 0 < f64[0].sum() < f64[0].size  # the run accepts and rejects


@pytest.fixture(scope="module")
def G():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bark_amd.fitting as fit
    from bark_amd import _lib
    from bark_amd.fitting import bark_sampler

    class NS:
        pass

    ns = NS()
    ns.fit, ns.L, ns.bs = fit, _lib, bark_sampler
    return ns


def run(G, method, seed=SEED):
    X, y, forests, noise, scale = problem()
    return G.fit.run_bark_sampler((forests.view(G.fit.tree_proposals.NODE_RECORD_DTYPE), noise, scale), (X, y), pr.MIXED_BOUNDS,
                                  train_params(), feat_types=pr.MIXED_FT, seed=seed, method=method, max_leaves=MAX_LEAVES)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["leafspace", "dense"])
def test_run_replays_on_the_host(G, method):
    X, y, forests, noise, scale = problem()
    r = G.bs._Run((forests.view(G.fit.tree_proposals.NODE_RECORD_DTYPE), noise, scale), (X, y), pr.MIXED_BOUNDS, train_params(),
                  pr.MIXED_FT, SEED, method, MAX_LEAVES)
    r.log = []
    nodes, noise_s, scale_s = r.run()
    assert len(r.log) == STEPS
    # the device's proposals through the host chains: same decisions, same forests
    steps = [(e["new"], e["log_q_prior"], e["log_u"], e["new_noise"], e["new_scale"], e["ns_log_q_prior"], e["ns_log_u"]) for e in r.log]
    acc, ns_acc, final, fnoise, fscale, mll, margin = replay(steps, np.float64)
    assert margin >= lc.MARGIN
    assert np.array_equal(acc, np.stack([e["accept"] for e in r.log])) and np.array_equal(ns_acc, np.stack([e["ns_accept"] for e in r.log]))
    assert final.tobytes() == r.forest.tobytes() and final.tobytes() == nodes[:, -1].tobytes()
    assert np.array_equal(fnoise, r.noise) and np.array_equal(fscale, r.scale)
    # ... which are the host's own trajectory (structure bit for bit, the logs within their bar: the margin covers them)
    want = host()
    assert np.array_equal(acc, want[0]) and np.array_equal(ns_acc, want[1]) and final.tobytes() == want[2].tobytes()
    before = forests.copy()
    for e in r.log:  # every sweep started from the forests the previous one left
        assert e["old"].tobytes() == before.tobytes()
        before[e["accept"]] = e["new"][e["accept"]]
    # the resident forests are the host mirror
    assert G.fit.tree_proposals.records_from_device(r.nodes_d).tobytes() == r.forest.tobytes()
    # MLL parity: the chains' resident state against a fresh evaluation of the final forests
    fresh = G.fit.batched_mll(r.forest, r.noise, r.scale, X, y.reshape(-1, 1), pr.MIXED_FT, include_scale=True, include_2pi=False)
    assert np.allclose(r.batch.mll, fresh, rtol=1e-9, atol=0), (r.batch.mll, fresh)
    assert np.allclose(r.batch.mll, mll, rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["leafspace", "dense"])
def test_samples_are_valid_deterministic_and_shaped(G, method):
    nodes, noise_s, scale_s = run(G, method)
    assert nodes.shape == (NC, 2, M, L) and nodes.dtype == G.fit.tree_proposals.NODE_RECORD_DTYPE
    assert noise_s.shape == (NC, 2) and scale_s.shape == (NC, 2) and noise_s.dtype == np.float64 and scale_s.dtype == np.float64
    assert (noise_s > 0).all() and (scale_s == 1.0).all()  # sample_scale is off
    info = G.L.PackInfo()
    for c in range(NC):
        for k in range(2):
            f = np.ascontiguousarray(nodes[c, k])
            assert G.L.lib().bark_forest_pack_info(G.L.ptr(f), 1, M, L, G.L.ptr(pr.MIXED_FT), 4, ctypes.byref(info)) == 0
            assert info.max_leaves <= MAX_LEAVES
    again = run(G, method)
    for a, b in zip((nodes, noise_s, scale_s), again):
        assert a.tobytes() == b.tobytes()
    other = run(G, method, seed=SEED + 1)
    assert other[0].tobytes() != nodes.tobytes()
    # the two methods decide alike at this seed (the pre-check's margin)
    assert nodes[:, -1].tobytes() == host()[2].tobytes()


@pytest.mark.gpu
def test_limits_are_refused_up_front(G):
    X, y, forests, noise, scale = problem()
    model = (forests.view(G.fit.tree_proposals.NODE_RECORD_DTYPE), noise, scale)
    p = train_params()
    call = lambda **kw: G.fit.run_bark_sampler(model, (X, y), pr.MIXED_BOUNDS, kw.pop("params", p), **{"feat_types": pr.MIXED_FT, **kw})  # noqa: E731
    with pytest.raises(ValueError, match="method"):
        call(method="host")
    with pytest.raises(ValueError, match="max_leaves"):
        call(max_leaves=33)
    with pytest.raises(ValueError, match="max_leaves"):
        call(method="dense", max_leaves=33)
    with pytest.raises(ValueError, match="leaves"):
        call(max_leaves=1)  # the model's trees are larger
    with pytest.raises(ValueError, match="num_chains"):
        call(params=G.fit.BARKTrainParams(num_chains=3))
    with pytest.raises(TypeError, match="feat_types"):
        G.fit.run_bark_sampler(model, (X, y), pr.MIXED_BOUNDS, p)
