"""The calls that start from a fitted posterior across a slab boundary.  The host drivers walk and scan the points in slabs of
65536; C = 65537 makes two slabs, the second of one point.  Every output below is per point, so whatever a slab boundary did
to it would show as a bit that differs from the same call on the two pieces, or from the stateless scan, whose own slab
handling is tested against the reference in tests/test_gpu_acquisition.py.

Shapes: N = 32, d = 4, B = 3 prior forests of m = 2 trees, fitted with chunk = 2 (chunks of 2 and 1 forests), 2 pending
points.  The weighted scan is run at equal weights; it multiplies every forest's terms by 1/3 where the plain scan divides the
sum by 3, so it is held against its own two pieces and not against the stateless scan."""
import numpy as np
import pytest

from bark_amd import synthetic

pytestmark = pytest.mark.gpu

N, B, M, CHUNK, SLAB = 32, 3, 2, 2, 65536
C = SLAB + 1


class Fixture:
    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        kw = dict(d_cont=2, n_int=1, n_cat=1)
        self.X, self.y, bounds, self.ft = synthetic.mixed_problem(N, seed=31, **kw)
        self.points = synthetic.mixed_problem(C, seed=32, **kw)[0]
        self.pend = synthetic.mixed_problem(2, seed=33, **kw)[0]
        self.values = np.random.default_rng(34).normal(float(self.y.mean()), 1.0, size=C)
        F = synthetic.sample_prior_forests(B, M, bounds, self.ft, seed=35)
        self.model = (F, np.full(B, 0.1), np.linspace(0.8, 1.3, B))
        self.post = fit_posterior(self.model, (self.X, self.y), self.ft, chunk=CHUNK)
        self.pieces = (self.points[:SLAB], self.points[SLAB:])


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_shape(fx):
    assert (fx.post.B, fx.post.m, fx.post.chunk) == (B, M, CHUNK) and fx.points.shape == (C, 4) and fx.pieces[1].shape == (1, 4)


@pytest.mark.parametrize("variant", ["lds", "global"])
def test_scan_from_the_state_is_the_stateless_scan(fx, variant):
    from bark_amd.optimizer import acquisition_scan

    want = acquisition_scan(fx.model, (fx.X, fx.y), fx.points, fx.ft, chunk=CHUNK, return_values=True, pending=fx.pend, variant=variant)
    assert want[2].shape == (C,) and np.isfinite(want[2]).all()
    for weights in (None, "state"):  # the state has no importance weights: both are the equal-weight scan
        got = fx.post.scan(fx.points, return_values=True, pending=fx.pend, variant=variant, weights=weights)
        assert got[0] == want[0] and got[1] == want[1] and same_bits(got[2], want[2]), (variant, weights)


@pytest.mark.parametrize("variant", ["lds", "global"])
def test_weighted_scan_is_its_two_pieces(fx, variant):
    kw = dict(return_values=True, pending=fx.pend, variant=variant, weights=np.full(B, 1.0 / B))
    best, idx, values = fx.post.scan(fx.points, **kw)
    parts = [fx.post.scan(p, **kw) for p in fx.pieces]
    want = np.concatenate([p[2] for p in parts])
    assert np.isfinite(values).all() and same_bits(values, want)
    assert best == want.min() == want[idx]


@pytest.mark.parametrize("per_forest", [True, False])
def test_predict_is_its_two_pieces(fx, per_forest):
    kw = dict(per_forest=per_forest, quantiles=[0.1, 0.9])
    got = fx.post.predict(fx.points, **kw)
    parts = [fx.post.predict(p, **kw) for p in fx.pieces]
    assert sorted(got) == sorted(["mean", "var", "quantiles"] + (["forest_mean", "forest_var"] if per_forest else []))
    for key, value in got.items():
        want = np.concatenate([p[key] for p in parts], axis=-1)
        assert value.shape[-1] == C and np.isfinite(value).all() and same_bits(value, want), key


def test_scores_are_their_two_pieces(fx):
    got = fx.post.scores(fx.points, fx.values, return_values=True)
    parts = [fx.post.scores(p, v, return_values=True) for p, v in zip(fx.pieces, (fx.values[:SLAB], fx.values[SLAB:]))]
    for key in ("log_density", "sq_err"):
        want = np.concatenate([p[key] for p in parts])
        assert got[key].shape == (C,) and np.isfinite(got[key]).all() and same_bits(got[key], want), key
