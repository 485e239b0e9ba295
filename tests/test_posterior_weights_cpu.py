"""The host side of the weighted forest samples (LeafPosterior.log_weights): tests/weights_ref.py against brute force, the
systematic resampling index, `thompson_forests(weights=)` and the refusals that need no device.  No GPU."""
import numpy as np
import pytest

import weights_ref as wr
from bark_amd.optimizer.thompson_sampling import thompson_forests
from bark_amd.tree_kernels import LeafPosterior, systematic_index


@pytest.mark.parametrize("B", [1, 5, 1000])
def test_restatement_against_brute_force(B):
    """increments down to -60: exp(-60) is far from the underflow of either format, so the unshifted sum is exact enough to
    judge the shifted one.  Bound: a handful of roundings each, 16 ulp of the largest weight / of the normaliser."""
    rng = np.random.default_rng(B)
    inc = rng.uniform(-60.0, 0.0, size=B)
    log_w = None if B == 1 else np.log(rng.dirichlet(np.ones(B)))
    info = np.zeros(B, dtype=np.int32)
    if B > 1:
        info[1] = 3
        inc[B // 2] = -np.inf
    got_l, got_w, got_s = wr.update(log_w, inc, info)
    want_l, want_w, want_s = wr.brute_force(log_w, inc, info)
    eps = np.finfo(np.float64).eps
    assert np.abs(got_w - want_w).max() <= 16 * eps * float(want_w.max())
    assert np.abs(got_s - want_s).max() <= 16 * eps * float(np.abs(want_s).max())
    alive = np.isfinite(want_l)
    assert np.array_equal(alive, np.isfinite(got_l)) and (got_w[~alive] == 0).all()
    assert np.abs(got_l[alive] - want_l[alive]).max() <= 16 * eps * max(1.0, float(np.abs(want_l[alive]).max()))
    assert abs(float(got_w.sum()) - 1.0) <= 4 * B * eps
    if B > 1:
        assert got_w[1] == 0 and got_w[B // 2] == 0


def test_restatement_all_dead_and_underflow():
    log_w, w, stats = wr.update(None, np.array([-np.inf, 0.0]), np.array([0, 7]))
    assert np.isnan(log_w).all() and np.isnan(w).all() and stats[0] == -np.inf and np.isnan(stats[1:]).all()
    log_w, w, stats = wr.update(None, np.array([0.0, -800.0, -1.0]))
    assert w[1] == 0.0 and np.isfinite(log_w[1]) and stats[2] == w[0]  # underflow to 0 is allowed; the log weight survives


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 7, 64])
def test_systematic_resampling(n, seed):
    rng = np.random.default_rng(10 * n + seed)
    w = rng.dirichlet(np.full(9, 0.4))
    w[[2, 8]] = 0.0
    w /= w.sum()
    index = systematic_index(w, n, seed)
    assert index.dtype == np.int64 and index.shape == (n,) and (np.diff(index) >= 0).all()
    assert np.array_equal(index, wr.systematic(w, n, seed)) and np.array_equal(index, systematic_index(w, n, seed))
    counts = np.bincount(index, minlength=9)
    assert counts[2] == 0 and counts[8] == 0
    # a count one ulp of n w_b off an integer may land on either side of it
    slack = 1e-12
    assert (counts >= np.floor(n * w - slack)).all() and (counts <= np.ceil(n * w + slack)).all(), (counts, n * w)
    # unnormalised weights name the same forests
    assert np.array_equal(index, systematic_index(3.0 * w, n, seed))


def test_systematic_resampling_refusals():
    for bad in ([0.0, 0.0], [0.5, -0.5, 1.0], [np.nan, 1.0], [np.inf, 1.0]):
        with pytest.raises(ValueError, match="weights must be"):
            systematic_index(bad, 3)
    with pytest.raises(ValueError, match="n must be positive"):
        systematic_index([1.0], 0)


@pytest.mark.parametrize("B,q,seed", [(1, 1, 0), (5, 3, 0), (64, 8, 7), (1000, 17, 123)])
def test_thompson_forests_without_weights_is_todays_array(B, q, seed):
    today = np.random.default_rng(seed).integers(0, B, size=q).astype(np.int64)
    assert np.array_equal(thompson_forests(B, q, seed), today)
    assert np.array_equal(thompson_forests(B, q, seed, weights=None), today)


def test_thompson_forests_with_weights():
    for k in (0, 3, 4):
        got = thompson_forests(5, 6, seed=k, weights=np.eye(5)[k])
        assert got.dtype == np.int64 and got.tolist() == [k] * 6
    w = np.array([0.5, 0.0, 0.25, 0.25, 0.0])
    got = thompson_forests(5, 200, seed=1, weights=w)
    assert set(got.tolist()) == {0, 2, 3}
    assert np.array_equal(got, np.random.default_rng(1).choice(5, size=200, p=w))
    for bad in (np.ones(4), -np.eye(5)[0], np.zeros(5), np.full(5, np.nan)):
        with pytest.raises(ValueError, match="weights must be"):
            thompson_forests(5, 2, 0, weights=bad)
    with pytest.raises(ValueError, match="q must be positive"):
        thompson_forests(5, 0, 0, weights=w)


def bare_posterior(B=4):
    """a LeafPosterior without a device: enough for the checks that come before anything is launched"""
    post = object.__new__(LeafPosterior)
    post.B, post.m, post.R, post.d, post.train_y_min = B, 3, 8, 2, 0.0
    post.log_weights = post.log_normaliser = None
    return post


def test_python_refusals_need_no_device():
    post = bare_posterior()
    for bad in (np.zeros(3), np.zeros((4, 1)), 0.0):
        with pytest.raises(ValueError, match="log_increment must be"):
            post.reweight_(bad)
    for bad in ([0.0, np.nan, 0.0, 0.0], [0.0, np.inf, 0.0, 0.0]):
        with pytest.raises(ValueError, match="NaN or \\+inf"):
            post.reweight_(np.array(bad))
    assert post.log_weights is None and post.log_normaliser is None
    for bad in ([], [4], [-1, 0], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="index must"):
            post.subset(np.array(bad))
    cand = np.zeros((2, 2))
    for bad in (np.ones(3), -np.ones(4), np.zeros(4), [1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], "equal"):
        with pytest.raises(ValueError, match="weights must be"):
            post.scan(cand, weights=bad)
