"""Host side of the joint covariance from a fitted posterior (include/bark_hip.h, bark_leaf_posterior_covariance_hip): the
exported symbols, the workspace query, the pure-host refusals of the entry point, the reference's own fitness
(tests/covariance_ref.py) and the Python argument errors.  No GPU."""
import ctypes

import numpy as np
import pytest

import acq_ref as ar
import covariance_ref as cr
import predict_ref as pr
from bark_amd import _lib

NAMES = ("bark_leaf_posterior_covariance_hip", "bark_leaf_posterior_covariance_workspace_bytes")
CASES = tuple(cr.CASE_POINTS)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_symbols_are_exported(lib):
    assert set(NAMES) <= set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None and getattr(lib, name) is not None


def align(n):
    return (n + 255) & ~255


def past_lds(m=13):
    return ar.lds_limit(m) + 1


def test_workspace_query(lib):
    q = lib.bark_leaf_posterior_covariance_workspace_bytes
    R, m, B, Bc, C1, C2 = 141, 50, 8, 4, 300, 70
    W = (R + 31) // 32
    codes = lambda C: align(4 * Bc * W * ((C + 127) // 128 * 128))  # noqa: E731
    means = lambda C: align(8 * 4 * C) + align(8 * 2 * B * C)  # noqa: E731
    # (symmetric, want_forest, want_mixture)
    assert q(R, m, B, Bc, C1, C2, 0, 1, 0, 0) == codes(C1) + codes(C2) + 256
    assert q(R, m, B, Bc, C1, C2, 1, 1, 0, 0) == codes(C1) + 256 == q(R, m, B, Bc, C1, 12345678, 1, 1, 0, 0)
    assert q(R, m, B, Bc, C1, C2, 0, 1, 1, 0) == codes(C1) + codes(C2) + means(C1) + means(C2) + 256
    assert q(R, m, B, Bc, C1, C2, 0, 0, 1, 0) == codes(C1) + codes(C2) + means(C1) + means(C2) + 256 + align(8 * Bc * C1 * C2)
    assert q(R, m, B, Bc, C1, C2, 1, 0, 1, 0) == codes(C1) + means(C1) + 256 + align(8 * Bc * C1 * C1)
    # no T in the workspace: the variant changes nothing where both run
    assert q(R, m, B, Bc, C1, C2, 0, 1, 1, 1) == q(R, m, B, Bc, C1, C2, 0, 1, 1, 2) == q(R, m, B, Bc, C1, C2, 0, 1, 1, 0)
    # refused shapes: each limit one past its edge -> 0
    ok = dict(R=141, m=50, B=2, Bc=1, C1=3, C2=4, sym=0, wf=1, wm=1, variant=0)
    assert q(*ok.values()) > 0
    for bad in (dict(R=8193, m=64), dict(m=65), dict(R=0), dict(m=0), dict(B=0), dict(Bc=0), dict(C1=0), dict(C2=0), dict(C1=65537),
                dict(C2=65537), dict(C1=0, sym=1), dict(C1=65537, sym=1), dict(wf=0, wm=0), dict(variant=3), dict(variant=-1),
                dict(R=past_lds(), m=13, variant=1)):
        assert q(*{**ok, **bad}.values()) == 0, bad
    assert q(*{**ok, **dict(R=past_lds(), m=13, variant=2)}.values()) > 0
    assert q(8192, 64, 1, 1, 65536, 65536, 0, 1, 1, 0) > 0 and q(8192, 64, 1, 1, 65536, 0, 1, 1, 1, 0) > 0
    assert lib.bark_last_error() == b""  # a query reports through its value only
    # monotone in C1, C2 and Bc, whatever is asked for; Bc past B adds nothing
    for sym, wf, wm in ((0, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 1), (1, 1, 1)):
        size = lambda C1=C1, C2=C2, Bc=Bc: q(R, m, B, Bc, C1, C2, sym, wf, wm, 0)  # noqa: E731
        assert size(C1=1) < size(C1=129) < size(C1=1000) < size(C1=65536), (sym, wf, wm)
        if not sym:
            assert size(C2=1) < size(C2=129) < size(C2=1000) < size(C2=65536), (sym, wf, wm)
        assert size(Bc=1) < size(Bc=2) < size(Bc=8) == size(Bc=99), (sym, wf, wm)


def _raw_call(lib, *, R=141, m=50, C1=4, C2=3, x2=True, observation=0, variant=0, state_offset=0, state_bytes=None, null=(),
              outputs=("forest", "mixture")):
    """the entry point without a context: every refusal of its own comes before the context is looked at"""
    B = 2
    info = _lib.PackInfo(B=B, m=m, L=100, stride=100, max_leaves=8, max_depth=4, packed_bytes=0, max_bits=R)
    buf = np.zeros(64)
    need = int(lib.bark_leaf_posterior_bytes(min(R, 8192), min(m, 64), B))
    raw = np.zeros(need + 512, dtype=np.uint8)
    state = ctypes.c_void_p(((raw.ctypes.data + 255) & ~255) + state_offset)
    p = lambda k, given=True: _lib.ptr(buf if given and k not in null else None)  # noqa: E731
    rc = lib.bark_leaf_posterior_covariance_hip(None, _lib.ptr(buf), None if "info" in null else ctypes.byref(info), 4, _lib.ptr(buf),
                                                _lib.ptr(buf), state, need if state_bytes is None else state_bytes, p("x1"), C1,
                                                p("x2", x2), C2, None, observation, variant, p("forest", "forest" in outputs),
                                                p("mixture", "mixture" in outputs), p("info_out"), _lib.ptr(buf), 0, 1, None)
    del raw
    return rc, lib.bark_last_error().decode()


@pytest.mark.parametrize("kw, message", [
    (dict(C1=0), "points per side"), (dict(C1=65537), "points per side"), (dict(C2=0), "points per side"),
    (dict(C2=65537), "points per side"), (dict(C1=0, x2=False), "points per side"), (dict(outputs=()), "or both must be given"),
    (dict(observation=2), "observation is 0 or 1"), (dict(observation=-1), "observation is 0 or 1"),
    (dict(observation=1), "share none"), (dict(null=("x1",)), "null argument"), (dict(null=("info",)), "null argument"),
    (dict(null=("info_out",)), "null argument"), (dict(m=65), "at most 64 trees"), (dict(R=8193), "8192 leaves"),
    (dict(variant=3), "unknown variant"), (dict(state_offset=128), "256-byte aligned"), (dict(state_bytes=1024), "state buffer too small"),
    (dict(m=13, R=past_lds(), variant=1), "LDS variant")])
def test_refusals_need_no_device(lib, kw, message):
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and message in text, (rc, text)


@pytest.mark.parametrize("kw", [dict(C1=1, C2=1), dict(C1=65536, C2=65536), dict(x2=False, observation=1), dict(x2=False, C2=-5),
                                dict(outputs=("forest",)), dict(outputs=("mixture",)), dict(m=64, R=8192),
                                dict(m=13, R=past_lds(), variant=2), dict(m=13, R=past_lds() - 1, variant=1)])
def test_edges_pass_the_checks(lib, kw):
    """at the edge the call gets as far as the context, which this test does not give it"""
    rc, text = _raw_call(lib, **kw)
    assert rc == _lib.BARK_ERR_ARG and "null bark_ctx" in text, (rc, text)


# ---- the reference checks itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_two_stage_order_agrees_with_the_dense_truth(name):
    i1, i2 = cr.CASE_POINTS[name]
    want, got = cr.truth(name, i1, i2), cr.two_stage(name, i1, i2)
    used = float((np.abs(got - want) / cr.forest_bar(name)).max())
    print(f"{name}: the two-stage restatement uses {used:.3g} of the per-forest bar")
    assert used <= 1.0, (name, used)
    # and through the mixture, equal and random weights
    B = want.shape[0]
    mu1, mu2 = cr.mu_of(name, i1), cr.mu_of(name, i2)
    for w in (np.full(B, 1.0 / B), pr.random_weights(B)):
        mean1, mean2 = pr.west(w, mu1, mu1)[0], pr.west(w, mu2, mu2)[0]
        mix = cr.mixture_order(w, got, mu1, mean1, mu2, mean2)
        ref = cr.mixture(w, want, mu1, mu2).astype(np.float64)
        used = float((np.abs(mix - ref) / cr.mixture_bar(name, w, mu1, mu2)).max())
        print(f"{name}: the mixture in forest order uses {used:.3g} of the mixture bar")
        assert used <= 1.0, (name, used)
    # one forest holds all the weight: its own block, exactly
    hot = np.zeros(B)
    hot[B - 1] = 1.0
    assert np.array_equal(cr.mixture_order(hot, got, mu1, pr.west(hot, mu1, mu1)[0], mu2, pr.west(hot, mu2, mu2)[0]), got[B - 1])


@pytest.mark.parametrize("name", CASES)
def test_truth_is_symmetric_and_positive_semidefinite(name):
    i1, i2 = cr.CASE_POINTS[name]
    idx = np.union1d(i1, i2)
    cov = cr.truth(name, idx, idx)
    bar = cr.forest_bar(name)
    assert (np.abs(cov - cov.transpose(0, 2, 1)) <= bar).all()
    # the block between the two sets is the transpose of the block between them the other way round
    assert (np.abs(cr.truth(name, i1, i2) - cr.truth(name, i2, i1).transpose(0, 2, 1)) <= bar).all()
    C = len(idx)
    for b in range(cov.shape[0]):
        low = float(np.linalg.eigvalsh((cov[b] + cov[b].T) / 2).min())
        assert low >= -float(bar[b, 0, 0]) * C, (name, b, low)
    # its diagonal is the oracle's posterior variance
    var = ar.posterior(name)[1][:, idx]
    assert (np.abs(np.diagonal(cov, axis1=1, axis2=2) - var) <= bar[:, :, 0]).all()
    # the mixture of a symmetric block is symmetric and positive semi-definite too
    B = cov.shape[0]
    w = pr.random_weights(B)
    mu = cr.mu_of(name, idx)
    mix = cr.mixture(w, cov, mu, mu).astype(np.float64)
    mbar = cr.mixture_bar(name, w, mu, mu)
    assert (np.abs(mix - mix.T) <= mbar).all()
    assert float(np.linalg.eigvalsh((mix + mix.T) / 2).min()) >= -float(mbar.max()) * C


# ---- Python argument errors ----------------------------------------------------------------------------------------
def test_python_checks_before_the_device():
    from bark_amd.tree_kernels import LeafPosterior

    p = object.__new__(LeafPosterior)  # no state: everything below raises before one is needed
    p.B, p.d, p.R, p.m, p.log_weights = 2, 4, 8, 2, None
    x = np.random.default_rng(0).uniform(size=(3, 4))
    with pytest.raises(ValueError, match="unknown variant"):
        p.covariance(x, variant="fast")
    with pytest.raises(ValueError, match="at least one point"):
        p.covariance(x[:0])
    with pytest.raises(ValueError, match="share no noise"):
        p.covariance(x, x, observation=True)
