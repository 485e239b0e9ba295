"""The leaf-space host reference (tests/leafspace_ref.py) against the oracle's N-space route — the LU inverse of
scale K + s2 I built from the oracle's Gram matrices, as the reference computes — at every shape of
tests/test_gpu_leafspace.py.  At each shape the two agree to 1/100 of the tolerance the GPU test applies to that output,
so that the GPU test measures the kernels and not the reference; a shape that misses this is too ill-conditioned for the
table and is replaced, the tolerance stays.  No GPU."""
import numpy as np
import pytest

import leafspace_ref as lr
from oracle import oracle as orc

# the GPU test's tolerances (test_gpu_leafspace.py) / 100
MLL_RTOL, MLL_ATOL = 1e-11, 1e-10
POST_TOL = 1e-11
INV_RTOL, INV_ATOL = 1e-10, 1e-11
LOGDET_RTOL = 1e-12
DRAW_TOL = 1e-11


def test_leaf_matrix_follows_the_packed_walk():
    """Z's columns (fancy indexing over the oracle's leaves and the packed leaf records) are the bits the emulated device
    walk sets, for a chunk of three forests with different leaf counts."""
    inp = lr.make_inputs(lr.CASES["mixed_chunk"])
    info, packed = lr.host_pack(inp.F, inp.ft)
    for b in range(inp.case.B):
        for i in range(0, inp.case.N, 29):
            bits = sorted(lr.walk_packed(packed[b, t], inp.X[i], info.max_depth)[2] for t in range(inp.m))
            assert np.flatnonzero(inp.Z[b][i]).tolist() == bits


def test_triangular_solves():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((700, 700))
    L = np.linalg.cholesky(A @ A.T + 700 * np.eye(700))
    B = rng.standard_normal((700, 9))
    assert np.allclose(L @ lr.solve_lower(L, B), B, rtol=0, atol=1e-12)
    assert np.allclose(L.T @ lr.solve_lower(L, B, trans=True), B, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(lr.CASES))
def test_reference_agrees_with_the_oracle(name):
    inp = lr.make_inputs(lr.CASES[name])
    lr.check_shape(inp)
    X, y, cand, ft = inp.X, inp.y, inp.cand, inp.ft
    N = X.shape[0]
    worst = {}
    for b in range(inp.case.B):
        ref = lr.reference(inp, b)
        one = (inp.F[b:b + 1], inp.noise[b:b + 1], inp.scale[b:b + 1])
        s2, sc = 1e-6 + inp.noise[b], inp.scale[b]
        K = orc.forest_gram_matrix(inp.F[b], X, X, ft)
        K_s = sc * K + s2 * np.eye(N)
        K_inv0 = np.linalg.inv(K_s)
        K_cx = orc.forest_gram_matrix(inp.F[b], cand, X, ft)
        K_cc = orc.forest_gram_matrix(inp.F[b], cand, cand, ft)
        mu0, var0 = orc.forest_predict(one, (X, y), cand, ft)
        pairs = {
            "mll": (ref.mll(), orc.batched_mll(*one, X, y, ft, include_scale=True, include_2pi=False)[0], MLL_RTOL, MLL_ATOL),
            "mu": (ref.posterior(inp.Zc[b])[0], mu0[0], POST_TOL, POST_TOL),
            "var": (ref.posterior(inp.Zc[b])[1], var0[0], POST_TOL, POST_TOL),
            "K_inv": (ref.inverse()[0], K_inv0, INV_RTOL, INV_ATOL),
            "K_inv_y": (ref.inverse()[1], K_inv0 @ y[:, 0], INV_RTOL, INV_ATOL),
            "logdet": (ref.logdet(), np.linalg.slogdet(K_s)[1], LOGDET_RTOL, 0.0),
            # the draws' covariance: scale K_CC - K_CX K_s^-1 K_XC with K_CX = scale (1/m) Z_C Z'
            "draw_cov": (ref.draw_cov(inp.Zc[b]), sc * K_cc - sc * sc * (K_cx @ K_inv0 @ K_cx.T), DRAW_TOL, DRAW_TOL),
        }
        for key, (got, want, rtol, atol) in pairs.items():
            err = np.abs(np.asarray(got) - want) / (atol + rtol * np.abs(want))
            worst[key] = max(worst.get(key, 0.0), float(err.max()))
    print(name, {k: "%.2g" % v for k, v in worst.items()})  # fraction of the allowed error used
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("m", [512, 513, 1280, 1281])
def test_reference_inverse_at_the_tree_limit(m):
    """the shapes of test_gpu_leafspace.py's tree-limit tests: the inverse, its K_inv y and logdet"""
    inp = lr.make_inputs(lr.limit_case(m), node_limit=3)
    assert inp.m == m and inp.R == m + m // 2
    ref = lr.reference(inp, 0)
    K_s = inp.scale[0] * orc.forest_gram_matrix(inp.F[0], inp.X, inp.X, inp.ft) + (1e-6 + inp.noise[0]) * np.eye(inp.case.N)
    want = np.linalg.inv(K_s)
    K_inv, K_inv_y = ref.inverse()
    assert np.allclose(K_inv, want, rtol=INV_RTOL, atol=INV_ATOL)
    assert np.allclose(K_inv_y, want @ inp.y[:, 0], rtol=INV_RTOL, atol=INV_ATOL)
    assert np.isclose(ref.logdet(), np.linalg.slogdet(K_s)[1], rtol=LOGDET_RTOL, atol=0.0)
    want_mll = orc.batched_mll(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False)[0]
    assert np.isclose(ref.mll(), want_mll, rtol=MLL_RTOL, atol=MLL_ATOL)
