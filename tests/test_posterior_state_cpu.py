"""Host side of the fitted leaf-space posterior (include/bark_hip.h): the byte queries of the state and of the calls that start
from it, and the Python argument checks that raise before a device is touched.  No GPU."""
import numpy as np
import pytest

from bark_amd import _lib, synthetic


def align(n):
    return (n + 255) & ~255


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.mark.parametrize("R, m, B", [(1, 1, 1), (37, 8, 5), (141, 50, 64), (8192, 64, 3), (33, 64, 1000)])
def test_state_bytes(lib, R, m, B):
    want = align(8 * B * R * R) + align(8 * B * R) + align(4 * B)
    assert lib.bark_leaf_posterior_bytes(R, m, B) == want
    assert want % 256 == 0 and want >= B * (R * R + R) * 8 + 4 * B


@pytest.mark.parametrize("R, m, B", [(0, 8, 5), (8193, 8, 5), (37, 0, 5), (37, 65, 5), (37, 8, 0), (-1, -1, -1)])
def test_state_bytes_of_refused_shapes(lib, R, m, B):
    assert lib.bark_leaf_posterior_bytes(R, m, B) == 0


def test_workspace_queries(lib):
    R, m, Bc, C, P = 141, 50, 8, 70000, 3
    fitted = lambda **kw: lib.bark_acquisition_scan_fitted_workspace_bytes(*[{**dict(R=R, m=m, Bc=Bc, C=C, P=P, variant=0), **kw}[k] for k in ("R", "m", "Bc", "C", "P", "variant")])  # noqa: E731
    W, slab = (R + 31) // 32, 65536
    tiles = (C + 255) // 256
    table = align(8 * Bc * (R * (R + 1) // 2 + R))
    base = align(4 * Bc * W * slab) + align(8 * 3 * C) + 2 * align(8 * tiles)
    assert fitted(P=0, variant=2) == base
    assert fitted(P=0) == fitted(P=0, variant=1) == base + table  # auto takes the LDS variant at this shape
    assert fitted(variant=2) == base + align(4 * Bc * W * 128) + align(8 * Bc * R * R)
    # nothing of size N: the stateless scan's workspace grows with N, this one has no N to grow with and is smaller
    small, large = (lib.bark_acquisition_scan_targets_workspace_bytes(N, R, m, Bc, C, P) for N in (512, 1 << 20))
    assert fitted() < small < large
    # the fit carries no candidate, scan or pending areas
    for N in (64, 5000):
        assert 0 < lib.bark_leaf_posterior_fit_workspace_bytes(N, R, m, Bc) < lib.bark_acquisition_scan_workspace_bytes(N, R, m, Bc, 1)
    assert lib.bark_leaf_posterior_condition_workspace_bytes(R, m, Bc, P) == align(4 * Bc * W * 128)
    assert lib.bark_leaf_posterior_condition_workspace_bytes(R, m, Bc, 0) == 0
    # refused shapes
    assert fitted(P=65) == fitted(P=-1) == fitted(C=0) == fitted(C=(1 << 24) + 1) == fitted(Bc=0) == fitted(m=65) == fitted(R=8193) == 0
    assert fitted(variant=3) == 0 and fitted(R=8000, m=8, variant=1) == 0 and fitted(R=8000, m=8) > 0
    assert lib.bark_leaf_posterior_condition_workspace_bytes(R, m, Bc, 65) == 0
    assert lib.bark_leaf_posterior_fit_workspace_bytes(0, R, m, Bc) == lib.bark_leaf_posterior_fit_workspace_bytes(64, R, 65, Bc) == 0


def test_python_checks_before_the_device():
    from bark_amd.optimizer import (acquisition_scan, propose_batch_from_candidates, propose_from_candidates, propose_from_domain,
                                    propose_mes_from_candidates)
    from bark_amd.tree_kernels import LeafPosterior, fit_posterior

    X, y, bounds, ft = synthetic.mixed_problem(16, seed=1, d_cont=2, n_int=1, n_cat=1)
    F = synthetic.sample_prior_forests(2, 65, bounds, ft, seed=2)
    with pytest.raises(ValueError, match="at most 64 trees"):
        fit_posterior((F, np.full(2, 0.1), np.ones(2)), (X, y), ft)
    with pytest.raises(ValueError, match="needs scale"):
        fit_posterior((F[:, :8], np.full(2, 0.1), None), (X, y), ft)
    for call in (lambda p: acquisition_scan(None, None, X, None, posterior=p),
                 lambda p: propose_from_candidates(None, None, X, None, posterior=p),
                 lambda p: propose_batch_from_candidates(None, None, X, None, 2, posterior=p),
                 lambda p: propose_from_domain(None, None, bounds, ft, posterior=p)):
        with pytest.raises(TypeError, match="LeafPosterior"):
            call("not a posterior")
    with pytest.raises(ValueError, match="model and data"):
        propose_mes_from_candidates(None, None, X, ft, posterior="anything")
    # the checks of LeafPosterior.scan that come before any device work, on an object without a state
    p = object.__new__(LeafPosterior)
    p.B, p.train_y_min = 2, 0.0
    for kw, message in ((dict(kind="ucb"), "unknown kind"), (dict(variant="fast"), "unknown variant"), (dict(kappa=np.inf), "finite"),
                        (dict(kind="mes"), "needs targets"), (dict(kind="ei", targets=np.zeros((3, 2))), "one row per forest")):
        with pytest.raises(ValueError, match=message):
            p.scan(X, **kw)
    with pytest.raises(ValueError, match="at least one candidate"):
        p.scan(X[:0])
