"""Host side of the predictions from a fitted posterior (include/bark_hip.h, bark_leaf_posterior_predict_hip): the exported
symbols, the pure-host refusals of the entry point, its workspace query, the reference's own fitness and the Python argument
errors.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import acq_ref as ar
import predict_ref as pr
from bark_amd import _lib

LD = np.longdouble
NAMES = ("bark_leaf_posterior_predict_hip", "bark_leaf_posterior_predict_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_symbols_are_exported(lib):
    assert set(NAMES) <= set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None and getattr(lib, name) is not None


def _raw_call(lib, *, R=141, m=50, C=4, Q=2, probs=(0.025, 0.975), z="given", variant=0, observation=0, state_offset=0,
              state_bytes=None, null=(), scores=(), quantiles_out="auto"):
    """the entry point without a context: every refusal of its own comes before the context is looked at"""
    B = 2
    info = _lib.PackInfo(B=B, m=m, L=100, stride=100, max_leaves=8, max_depth=4, packed_bytes=0, max_bits=R)
    buf = np.zeros(64)
    need = int(lib.bark_leaf_posterior_bytes(min(R, 8192), min(m, 64), B))
    raw = np.zeros(need + 512, dtype=np.uint8)
    base = raw.ctypes.data
    state = ctypes.c_void_p(((base + 255) & ~255) + state_offset)
    p = {k: _lib.ptr(buf) for k in ("points", "moments", "info")}
    for k in null:
        p[k] = _lib.ptr(None)
    sc = {k: (_lib.ptr(buf) if k in scores else _lib.ptr(None)) for k in ("y", "rows", "mix", "values")}
    p_h = np.asarray(probs, dtype=np.float64)
    z_h = np.zeros(max(len(p_h), 1))
    qout = _lib.ptr(buf if (Q > 0 if quantiles_out == "auto" else quantiles_out) else None)
    rc = lib.bark_leaf_posterior_predict_hip(None, _lib.ptr(buf), None if "info" in null else ctypes.byref(info), 4, _lib.ptr(buf),
                                             _lib.ptr(buf), state, need if state_bytes is None else state_bytes, p["points"], C, None,
                                             observation, sc["y"], _lib.ptr(p_h if len(p_h) else None),
                                             _lib.ptr(z_h if z == "given" else None), Q, variant, p["moments"], None, qout, sc["rows"],
                                             sc["mix"], sc["values"], _lib.ptr(buf), _lib.ptr(buf), 0, 1, None)
    del raw
    return rc, lib.bark_last_error().decode()


def past_lds(m=13):
    return ar.lds_limit(m) + 1


@pytest.mark.parametrize("kw, message", [
    (dict(Q=17, probs=(0.5,) * 17), "probabilities per call"), (dict(Q=-1), "probabilities per call"),
    (dict(Q=1, probs=(0.0,)), "strictly inside"), (dict(Q=1, probs=(1.0,)), "strictly inside"),
    (dict(Q=1, probs=(math.nan,)), "strictly inside"), (dict(Q=1, probs=(math.inf,)), "strictly inside"),
    (dict(Q=2, probs=(0.5, -0.1)), "strictly inside"), (dict(z=None), "probs and zscores"),
    (dict(Q=2, quantiles_out=False), "exactly when Q > 0"), (dict(Q=0, probs=(), quantiles_out=True), "exactly when Q > 0"),
    (dict(scores=("y",)), "together or not at all"), (dict(scores=("y", "rows")), "together or not at all"),
    (dict(scores=("rows", "mix")), "together or not at all"), (dict(scores=("mix",)), "together or not at all"),
    (dict(scores=("values",)), "values_out needs"), (dict(observation=2), "observation is 0 or 1"),
    (dict(observation=-1), "observation is 0 or 1"), (dict(C=0), "bad shape C"), (dict(C=(1 << 24) + 1), "bad shape C"),
    (dict(state_offset=128), "256-byte aligned"), (dict(state_bytes=1024), "state buffer too small"),
    (dict(m=65), "at most 64 trees"), (dict(R=8193), "8192 leaves"), (dict(variant=3), "unknown variant"),
    (dict(null=("points",)), "null argument"), (dict(null=("moments",)), "null argument"), (dict(null=("info",)), "null argument")])
def test_refusals_need_no_device(lib, kw, message):
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and message in text, (rc, text)


def test_lds_variant_past_the_limit_is_refused(lib):
    rc, text = _raw_call(lib, m=13, R=past_lds(), variant=1)
    assert rc == _lib.BARK_ERR_ARG and "LDS variant" in text, (rc, text)
    rc, text = _raw_call(lib, m=13, R=past_lds(), variant=2)
    assert rc == _lib.BARK_ERR_ARG and "null bark_ctx" in text, (rc, text)


@pytest.mark.parametrize("kw", [dict(Q=0, probs=()), dict(Q=16, probs=(0.5,) * 16), dict(Q=1, probs=(5e-324,)),
                                dict(Q=1, probs=(1 - 2.0 ** -53,)), dict(C=1), dict(C=1 << 24), dict(m=64, R=8192),
                                dict(scores=("y", "rows", "mix")), dict(scores=("y", "rows", "mix", "values")), dict(observation=1),
                                dict(m=13, R=past_lds() - 1, variant=1)])
def test_edges_pass_the_checks(lib, kw):
    """at the edge the call gets as far as the context, which this test does not give it"""
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and "null bark_ctx" in text, (rc, text)


def align(n):
    return (n + 255) & ~255


def test_workspace_query(lib):
    q = lib.bark_leaf_posterior_predict_workspace_bytes
    R, m, B, Bc, C = 141, 50, 8, 4, 300
    W, cpad, tiles = (R + 31) // 32, 384, 2
    tab = align(8 * Bc * (R * (R + 1) // 2 + R))
    base = align(4 * Bc * W * cpad) + align(8 * 4 * C) + 256
    assert q(R, m, B, Bc, C, 0, 0, 0, 2) == base
    assert q(R, m, B, Bc, C, 0, 0, 0, 1) == base + tab == q(R, m, B, Bc, C, 0, 0, 0, 0)
    score = align(8 * 3 * C) + align(8 * 2 * tiles) + align(8 * B * 2 * tiles)
    assert q(R, m, B, Bc, C, 0, 0, 1, 2) == base + score
    assert q(R, m, B, Bc, C, 3, 0, 0, 2) == base + align(8 * 2 * B * C)
    # refused shapes: each limit one past its edge
    for bad in ((8193, 64, 1, 1, 1, 0), (141, 65, 1, 1, 1, 0), (0, 50, 1, 1, 1, 0), (141, 0, 1, 1, 1, 0), (141, 50, 0, 1, 1, 0),
                (141, 50, 1, 0, 1, 0), (141, 50, 1, 1, 0, 0), (141, 50, 1, 1, (1 << 24) + 1, 0), (141, 50, 1, 1, 1, 17),
                (141, 50, 1, 1, 1, -1)):
        assert q(*bad, 0, 0, 0) == 0, bad
    assert q(past_lds(), 13, 1, 1, 1, 0, 0, 0, 1) == 0 and q(past_lds(), 13, 1, 1, 1, 0, 0, 0, 2) > 0
    assert q(8192, 64, 1, 1, 1 << 24, 16, 1, 1, 0) > 0
    assert lib.bark_last_error() == b""  # a query reports through its value only
    # it grows with want_scores and with Q; Q adds the slab of per-forest rows only while no forest_out holds them, so
    # want_forest adds nothing of its own (the per-forest arrays are the caller's) and takes that slab away
    for wf in (0, 1):
        for Q in (0, 1, 16):
            assert q(R, m, B, Bc, C, Q, wf, 0, 0) < q(R, m, B, Bc, C, Q, wf, 1, 0)
    assert q(R, m, B, Bc, C, 0, 0, 0, 0) < q(R, m, B, Bc, C, 1, 0, 0, 0) == q(R, m, B, Bc, C, 16, 0, 0, 0)
    assert q(R, m, B, Bc, C, 0, 1, 0, 0) == q(R, m, B, Bc, C, 16, 1, 0, 0) == q(R, m, B, Bc, C, 0, 0, 0, 0)
    assert q(R, m, B, 1, C, 2, 0, 1, 0) < q(R, m, B, 2, C, 2, 0, 1, 0) < q(R, m, B, 8, C, 2, 0, 1, 0) == q(R, m, B, 99, C, 2, 0, 1, 0)
    assert q(R, m, B, Bc, 1, 2, 0, 1, 0) < q(R, m, B, Bc, 1000, 2, 0, 1, 0) < q(R, m, B, Bc, 1 << 17, 2, 0, 1, 0)


# ---- the reference checks itself -----------------------------------------------------------------------------------
CASES = ("prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit", "m13_past_lds", "m64_r256")


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


@pytest.mark.parametrize("name", CASES)
def test_west_equals_two_pass(name):
    mu, var = pr.forest_moments(name)
    B = mu.shape[0]
    for w in (np.full(B, 1.0 / B), pr.random_weights(B)):
        mean, v = pr.west(w, mu, var)
        mean_ld, v_ld = pr.two_pass(w, mu, var)
        assert (np.abs(v - v_ld.astype(np.float64)) <= 4 * ulp(v_ld)).all(), name
        assert (np.abs(mean - mean_ld.astype(np.float64)) <= 4 * ulp(np.abs(mu).max(axis=0))).all(), name
    # one forest holds all the weight: its own moments, exactly
    hot = np.zeros(B)
    hot[B - 1] = 1.0
    mean, v = pr.west(hot, mu, var)
    assert np.array_equal(mean, mu[B - 1]) and np.array_equal(v, var[B - 1])


def test_erf_series_against_math():
    x = np.concatenate([np.linspace(-8, 8, 321), [1e-300, 1e-10, 0.0, 6.99, 7.0, 40.0]])
    want = np.array([math.erf(v) for v in x])
    got = pr.erf_ld(x)
    assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp(want)).all()
    assert pr.Phi(0.0) == LD(0.5) and abs(float(pr.Phi(1.0)) - 0.8413447460685429) <= 2e-16


@pytest.mark.parametrize("name", ("prior_n64", "prior_n257_chunks", "m2_r65"))
def test_bisected_quantiles(name):
    mu, var = pr.forest_moments(name)
    mu, var = mu[:, :64], var[:, :64]
    B = mu.shape[0]
    w = pr.random_weights(B)
    last = None
    for p in (0.025, 0.5, 0.975):
        t = pr.quantile(p, w, mu, var)
        assert (np.abs(pr.cdf(t, w, mu, var) - LD(p)) <= LD(2.0) ** -50).all(), (name, p)
        assert last is None or (t >= last).all()
        last = t


def test_one_forest_quantile_is_its_own():
    mu, var = pr.forest_moments("m1_r64")
    hot = np.array([1.0])
    for p in (0.025, 0.5, 0.975):
        t = pr.quantile(p, hot, mu, var).astype(np.float64)
        assert np.array_equal(t, mu[0] + pr.zscore(p) * np.sqrt(var[0]))
    # ... and among several forests, the others at weight 0
    mu, var = pr.forest_moments("m2_r65")
    hot = np.array([0.0, 1.0, 0.0])
    t = pr.quantile(0.975, hot, mu, var).astype(np.float64)
    assert np.array_equal(t, mu[1] + pr.zscore(0.975) * np.sqrt(var[1]))
    # a component without variance is a step
    t = pr.quantile(0.5, np.array([0.5, 0.5]), np.array([[0.0], [1.0]]), np.array([[0.0], [0.0]]))
    assert float(t[0]) == 0.0


def test_weighted_scores_reduce_to_the_equal_weight_ones():
    import scores_ref as sr

    name = "prior_n64"
    mu, var = pr.forest_moments(name)
    B = mu.shape[0]
    got, want = pr.scores(np.full(B, 1.0 / B), mu, var, sr.targets(name), LD), sr.heldout(name, LD)
    for k in sr.KEYS:
        assert np.allclose(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), rtol=1e-14, atol=1e-14), k


# ---- Python argument errors ----------------------------------------------------------------------------------------
def test_python_checks_before_the_device():
    from bark_amd.tree_kernels import LeafPosterior, forest_predict

    p = object.__new__(LeafPosterior)  # no state: everything below raises before one is needed
    p.B, p.d, p.R, p.m, p.log_weights = 2, 4, 8, 2, None
    x = np.random.default_rng(0).uniform(size=(3, 4))
    with pytest.raises(ValueError, match="unknown variant"):
        p.predict(x, variant="fast")
    with pytest.raises(ValueError, match="unknown variant"):
        p.scores(x, np.zeros(3), variant="fast")
    for bad in ([0.0], [1.0], [0.5, 1.5], [-0.1], [math.nan]):
        with pytest.raises(ValueError, match="strictly inside"):
            p.predict(x, quantiles=bad)
    with pytest.raises(ValueError, match="at least one point"):
        p.predict(x[:0])
    with pytest.raises(ValueError, match="diagonal posterior only"):
        forest_predict(None, None, x, None, diag=False, posterior=p)
    with pytest.raises(ValueError, match="diagonal posterior only"):
        forest_predict(None, None, x, None, method="leafspace", posterior=p)
