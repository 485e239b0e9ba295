"""Host side of the fidelity information gain: the reference's own fitness (the cap on surviving cases), its closed-form
limits, the pure-host refusals of the entry point and of the Python layer.  No GPU."""
import ctypes

import numpy as np
import pytest

import acq_targets_ref as atr
import fidelity_ref as fr
from bark_amd import _lib, synthetic


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_enough_cases_survive_the_precheck():
    alive = fr.survivors()
    assert len(alive) >= fr.MIN_SURVIVORS, alive
    assert alive == fr.GPU_CASES  # what the GPU tests run


def test_zero_covariance_is_the_independent_case():
    """cov = 0: u(f) = mu_0 whatever f, so Psi_s(f) = Phi((t_s - mu_0) / (sd_0 + 1e-9)) phi(.) and g = H1 + mean_s I_s with
    a one-dimensional integrand; Z_s Psi_s is then the density of f(query) to 1e-9, so the gain is zero to the trapezoid's error"""
    mu_m, var_m, mu_0, var_0 = 0.3, 0.49, -0.2, 0.81
    t = np.array([-1.0, -0.4, 0.1])
    g, _ = fr.low_fidelity([mu_m], [var_m], [mu_0], [var_0], [0.0], t)
    lo, hi, n_a, pad, G = fr.GRID
    sd_m, sd_0 = np.sqrt(var_m), np.sqrt(var_0)
    c = fr.Phi((t - mu_0) / (sd_0 + 1e-9))
    Z = 1.0 / (c * sd_m + 1e-10)
    fk = lo + np.arange(n_a) * (hi - lo) / (n_a - 1)
    live = fk[np.array([np.abs(c * fr.phi((f - mu_m) / (sd_m + 1e-9))).sum() > 1e-8 for f in fk])]
    f = np.linspace(live.min() - pad, live.max() + pad, G)
    total = 0.0
    for s in range(3):
        z = Z[s] * c[s] * fr.phi((f - mu_m) / (sd_m + 1e-9))
        yv = np.where(z == 0, 0.0, z * np.log(np.where(z == 0, 1.0, z)))
        total += (f[1] - f[0]) * (yv.sum() - 0.5 * (yv[0] + yv[-1]))
    want = np.log(sd_m * fr.SQRT_2PI_E) + total / 3
    assert abs(g[0] - want) <= 1e-12
    assert abs(g[0]) <= 1e-6


def test_equal_leaves_are_the_mes_utility():
    rng = np.random.default_rng(0)
    mom = {k: rng.uniform(0.2, 1.0, size=(2, 5)) for k in fr.MOMENTS}
    t = rng.normal(size=(2, 4))
    g = fr.per_forest_gain(mom, np.ones((2, 5), dtype=bool), t)
    want = atr.utility(mom["mu_m"][:, :, None], np.sqrt(mom["var_m"])[:, :, None], t[:, None, :], "mes").mean(axis=2)
    assert np.array_equal(g, want)
    assert np.array_equal(-g.mean(axis=0), atr.acquisition(mom["mu_m"], mom["var_m"], t, "mes"))
    mom["var_m"][0, 0] = 0.0  # no variance: -inf whatever the leaves
    assert fr.per_forest_gain(mom, np.zeros((2, 5), dtype=bool), t)[0, 0] == -np.inf


def align(n):
    return (n + 255) & ~255


def test_workspace_query(lib):
    q = lib.bark_fidelity_gain_fitted_workspace_bytes
    R, m, Bc, C, S = 141, 50, 8, 300, 100
    W, cpad = (R + 31) // 32, 384
    assert q(R, m, Bc, C, S) == 2 * align(4 * Bc * W * cpad) + align(8 * Bc * 6 * C) + align(8 * Bc * C) + align(8 * C)
    # each limit at its edge and one past it
    assert q(8192, 64, 1, 65536, 1024) > 0
    for bad in ((8193, 64, 1, 1, 1), (8192, 65, 1, 1, 1), (141, 50, 1, 65537, 1), (141, 50, 1, 0, 1), (141, 50, 1, 1, 1025),
                (141, 50, 1, 1, 0), (141, 50, 0, 1, 1), (0, 50, 1, 1, 1), (141, 0, 1, 1, 1)):
        assert q(*bad) == 0, bad
    # monotone in Bc, C and S (S adds nothing: the targets stay with the caller)
    assert q(R, m, 1, C, S) < q(R, m, 2, C, S) < q(R, m, 9, C, S)
    assert q(R, m, Bc, 1, S) <= q(R, m, Bc, 128, S) < q(R, m, Bc, 129, S) < q(R, m, Bc, 65536, S)
    assert q(R, m, Bc, C, 1) <= q(R, m, Bc, C, 2) <= q(R, m, Bc, C, 1024)


def _raw_call(lib, *, R=141, m=50, C=4, S=3, lo=-10.0, hi=10.0, n_a=100, pad=0.25, G=250, null=None):
    """the entry point without a context: every refusal of its own comes before the context is looked at"""
    info = _lib.PackInfo(B=2, m=m, L=100, stride=100, max_leaves=8, max_depth=4, packed_bytes=0, max_bits=R)
    buf = np.zeros(64)
    p = {k: _lib.ptr(buf) for k in ("query", "target", "targets", "gain")}
    if null:
        p[null] = _lib.ptr(None)
    rc = lib.bark_fidelity_gain_fitted_hip(None, _lib.ptr(buf), ctypes.byref(info), 4, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 0,
                                           p["query"], p["target"], C, p["targets"], S, None, lo, hi, n_a, pad, G, p["gain"], None,
                                           _lib.ptr(buf), _lib.ptr(buf), 0, 1, None)
    return rc, lib.bark_last_error().decode()


@pytest.mark.parametrize("kw, message", [
    (dict(m=65), "at most 64 trees"), (dict(R=8193), "8192 leaves"), (dict(C=0), "pairs"), (dict(C=65537), "pairs"),
    (dict(S=0), "targets per forest"), (dict(S=1025), "targets per forest"), (dict(n_a=1), "support points"),
    (dict(n_a=1025), "support points"), (dict(G=1), "quadrature points"), (dict(G=4097), "quadrature points"),
    (dict(lo=1.0, hi=1.0), "lo < hi"), (dict(lo=2.0, hi=1.0), "lo < hi"), (dict(hi=np.inf), "lo < hi"), (dict(lo=np.nan), "lo < hi"),
    (dict(pad=-1e-300), "pad"), (dict(pad=np.inf), "pad"), (dict(null="query"), "null argument"),
    (dict(null="target"), "null argument"), (dict(null="targets"), "null argument"), (dict(null="gain"), "null argument")])
def test_refusals_need_no_device(lib, kw, message):
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and message in text, (rc, text)


@pytest.mark.parametrize("kw", [dict(m=64, R=8192), dict(C=1), dict(C=65536), dict(S=1), dict(S=1024), dict(n_a=2), dict(n_a=1024),
                                dict(G=2), dict(G=4096), dict(pad=0.0), dict(lo=0.0, hi=5e-324)])
def test_edges_pass_the_checks(lib, kw):
    """at the edge the call gets as far as the context, which this test does not give it"""
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and "null bark_ctx" in text, (rc, text)


def test_python_checks_before_the_device():
    from bark_amd.optimizer import (fidelity_information_gain, information_gain, propose_fidelity_information_based,
                                    with_fidelity)
    from bark_amd.optimizer.fidelity import best_per_cost
    from bark_amd.tree_kernels import LeafPosterior

    p = object.__new__(LeafPosterior)  # no state: everything below raises before one is needed
    p.B, p.d, p.R, p.m = 2, 4, 8, 2
    p.feat_types = np.array([synthetic.CONT] * 3 + [synthetic.CAT])
    x = np.random.default_rng(0).uniform(size=(3, 4))
    t = np.zeros((2, 3))
    kw = dict(fidelity_feature=3, fidelities=[0, 1, 2], targets=t)
    for costs, message in (([1.0, 2.0], "one cost per fidelity"), ([1.0, 0.0, 1.0], "positive and finite"),
                           ([1.0, -1.0, 1.0], "positive and finite"), ([1.0, np.inf, 1.0], "positive and finite"),
                           ([1.0, np.nan, 1.0], "positive and finite")):
        with pytest.raises(ValueError, match=message):
            propose_fidelity_information_based(p, x, costs, **kw)
    for j in (-1, 4):
        with pytest.raises(ValueError, match="fidelity_feature"):
            propose_fidelity_information_based(p, x, [1.0, 1.0, 1.0], **{**kw, "fidelity_feature": j})
    for bad in (32, -1, 1.5, np.nan):
        with pytest.raises(ValueError, match="fidelity"):
            propose_fidelity_information_based(p, x, [1.0, 1.0, 1.0], **{**kw, "fidelities": [0, 1, bad]})
        with pytest.raises(ValueError, match="fidelity"):
            fidelity_information_gain(p, x, **{**kw, "fidelities": [0, bad]})
    with pytest.raises(ValueError, match="targets, or sites"):
        propose_fidelity_information_based(p, x, [1.0, 1.0, 1.0], **{**kw, "targets": None})
    for targets, message in ((None, "needs targets"), (np.zeros((3, 3)), "one row per forest"), (np.zeros((2, 1025)), "targets per forest"),
                             (np.zeros(2), "one row per forest")):
        with pytest.raises(ValueError, match=message):
            information_gain(p, x, x, targets)
    with pytest.raises(ValueError, match="as many target points"):
        information_gain(p, x, x[:2], t)
    for grid in ((0.0, 0.0, 100, 0.25, 250), (-10, 10, 1, 0.25, 250), (-10, 10, 100, -1.0, 250), (-10, 10, 100, 0.25, 4097), (-10, 10, 100)):
        with pytest.raises(ValueError, match="grid"):
            information_gain(p, x, x, t, grid=grid)
    # with_fidelity copies; an Int column takes whole numbers only
    y = with_fidelity(x, 3, 2)
    assert y is not x and np.array_equal(y[:, :3], x[:, :3]) and (y[:, 3] == 2).all() and not (x[:, 3] == 2).any()
    with pytest.raises(ValueError, match="integer"):
        with_fidelity(x, 3, 0.5, np.array([synthetic.CONT] * 3 + [synthetic.INT]))
    assert (with_fidelity(x, 0, 0.5, p.feat_types)[:, 0] == 0.5).all()
    # the arg-max per cost: ties to the lowest t, NaN never wins, all NaN gives -1
    gains = np.array([[1.0, 1.0, np.nan, np.nan], [2.0, 1.0, 0.1, np.nan], [4.0, np.nan, -np.inf, np.nan]])
    assert best_per_cost(gains, [1.0, 2.0, 4.0]).tolist() == [0, 0, 1, -1]
    assert best_per_cost(gains, [1.0, 1.0, 1.0]).tolist() == [2, 0, 1, -1]
