"""Predictive scores, the part that needs no GPU: `bark_amd.utils.metrics` against closed forms, the host reference of
tests/scores_ref.py against itself (both precisions, both leave-one-out routes), the prechecks of every GPU case, and the
argument checks of the Python entry points that come before any device use."""
import math
import os
import re

import numpy as np
import pytest
import torch

import acq_ref as ar
import scores_ref as sr

from conftest import ROOT


# ---------------------------------------------------------------------------------------------- utils.metrics ----
def test_metrics_module_and_exports():
    import bark_amd.utils.metrics as metrics
    from bark_amd import tree_kernels as tk

    assert all(callable(getattr(metrics, f)) for f in ("gaussian_log_likelihood", "nlpd", "mse"))
    assert callable(tk.predictive_scores) and callable(tk.loo_scores)


def test_gaussian_log_likelihood_closed_forms():
    from bark_amd.utils.metrics import gaussian_log_likelihood

    # standard normal at 0 and at 1; variance 4 at two standard deviations
    mu, var, y = np.array([[0.0, 0.0], [1.0, 3.0]]), np.array([[1.0, 1.0], [4.0, 4.0]]), np.array([[0.0, 1.0], [5.0, -1.0]])
    want = np.array([[-0.5 * math.log(2 * math.pi), -0.5 * math.log(2 * math.pi) - 0.5],
                     [-0.5 * math.log(8 * math.pi) - 2.0, -0.5 * math.log(8 * math.pi) - 2.0]])
    got = gaussian_log_likelihood(mu, var, y)
    assert got.shape == (2, 2) and np.allclose(got, want, rtol=1e-15, atol=1e-15)


def test_nlpd_is_the_mean_negative_log_likelihood():
    from bark_amd.utils.metrics import gaussian_log_likelihood, nlpd

    rng = np.random.default_rng(0)
    mu, var, y = rng.standard_normal((7, 3)), rng.uniform(0.5, 2.0, (7, 3)), rng.standard_normal((7, 1))
    got = nlpd(mu, var, y)
    assert got.shape == (3,)
    assert np.array_equal(got, -gaussian_log_likelihood(mu, var, y).sum(0) / 7)
    assert np.array_equal(got, nlpd(mu, var, y, diag=True))


def test_mse_worked_by_hand():
    from bark_amd.utils.metrics import mse

    mu = np.array([[1.0, 2.0], [0.0, -1.0], [3.0, 3.0]])
    y = np.array([[1.0], [1.0], [2.0]])
    # residuals: (0, 1), (-1, -2), (1, 1): squares sum to 0 + 1 + 1 + 4 + 1 + 1 = 8 over 6 entries
    got = mse(mu, y)
    assert np.ndim(got) == 0 and got == 8.0 / 6.0


def test_metrics_numpy_and_torch_agree():
    from bark_amd.utils import metrics

    rng = np.random.default_rng(1)
    mu, var, y = rng.standard_normal((9, 4)), rng.uniform(0.1, 3.0, (9, 4)), rng.standard_normal((9, 1))
    tmu, tvar, ty = (torch.from_numpy(a) for a in (mu, var, y))
    for got, want in ((metrics.gaussian_log_likelihood(tmu, tvar, ty), metrics.gaussian_log_likelihood(mu, var, y)),
                      (metrics.nlpd(tmu, tvar, ty), metrics.nlpd(mu, var, y)), (metrics.mse(tmu, ty), metrics.mse(mu, y))):
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device.type == "cpu"
        assert np.allclose(got.numpy(), want, rtol=1e-14, atol=1e-14)


def test_metrics_agree_with_the_host_reference():
    """the reference's formulas as tests/scores_ref.py writes them, on the (N, batch) layout"""
    from bark_amd.utils import metrics

    rng = np.random.default_rng(2)
    mu, var, y = rng.standard_normal((3, 11)), rng.uniform(0.1, 3.0, (3, 11)), rng.standard_normal(11)
    want = sr.scores(mu, var, y)
    assert np.allclose(metrics.nlpd(mu.T, var.T, y[:, None]), want["nlpd"], rtol=1e-13, atol=1e-13)
    assert np.allclose(metrics.mse(mu.T, y[:, None]), want["mse"].mean(), rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------- host reference ----
def test_mixture_of_identical_forests_is_the_forest():
    rng = np.random.default_rng(3)
    mu, var, y = rng.standard_normal((1, 13)), rng.uniform(0.1, 3.0, (1, 13)), rng.standard_normal(13)
    one, three = sr.scores(mu, var, y), sr.scores(np.repeat(mu, 3, 0), np.repeat(var, 3, 0), y)
    assert np.allclose(three["nlpd_mixture"], one["nlpd"][0], rtol=1e-14) and np.allclose(three["mse_mixture"], one["mse"][0], rtol=1e-14)
    assert np.allclose(one["nlpd_mixture"], one["nlpd"][0], rtol=1e-14)


@pytest.mark.parametrize("name", [n for n in sr.GPU_CASES if n != ar.SLAB_CASE.name])
def test_precheck_heldout(name):
    A = sr.precheck(name)
    print(f"{name}: A = {A:.4g}")
    assert np.isfinite(A) and A > 0


def test_precheck_heldout_slab():
    """C = 65 537 under 2-tree forests on 20 points: the variance floor holds at the case's own noise"""
    A = sr.precheck(ar.SLAB_CASE.name)
    print(f"{ar.SLAB_CASE.name}: A = {A:.4g}")
    assert np.isfinite(A) and A > 0


@pytest.mark.parametrize("name", sr.LOO_CASES + ("brute",))
def test_precheck_loo(name):
    AG = sr.loo_precheck(name)
    print(f"{name}: A G = {AG:.4g}")
    assert np.isfinite(AG) and AG > 0


def test_brute_force_loo_equals_the_inverse_based():
    """N = 24 refits on 23 points against the diagonal and the solve of one inverse; both are oracle posteriors, so they agree
    to the posterior bar (and in fact far closer)"""
    mu, var, _ = sr.loo_moments("brute")
    mu_b, var_b = sr.loo_brute()
    assert mu.shape == (sr.BRUTE_B, sr.BRUTE_N)
    print(f"brute vs inverse: mu {np.abs(mu - mu_b).max():.3g}, var {np.abs(var - var_b).max():.3g}")
    assert np.allclose(mu_b, mu, rtol=ar.RTOL, atol=ar.ATOL) and np.allclose(var_b, var, rtol=ar.RTOL, atol=ar.ATOL)
    y = sr.brute_inputs().y.reshape(-1)
    a, b = sr.scores(mu, var, y), sr.scores(mu_b, var_b, y)
    tol = sr.amplification(mu, var, y)
    for k in sr.KEYS:
        assert np.allclose(a[k], b[k], rtol=ar.RTOL * tol, atol=ar.ATOL * tol), k


# ------------------------------------------------------------------------------------------ the entry points ----
def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bark_hip.h")).read()
    for sym in ("bark_predictive_scores_workspace_bytes", "bark_predictive_scores_hip"):
        assert re.search(rf"\b{sym}\s*\(", header), sym
    assert re.search(r"#define BARK_SCORE_HELDOUT 0\b", header) and re.search(r"#define BARK_SCORE_LOO 1\b", header)
    from bark_amd import _lib

    assert (_lib.SCORE_HELDOUT, _lib.SCORE_LOO) == (0, 1)
    assert "bark_predictive_scores_hip" in _lib.SIGNATURES


def test_workspace_query_is_host_code():
    from bark_amd import _lib

    lib = _lib.lib()
    scan = lib.bark_acquisition_scan_workspace_bytes(64, 140, 50, 3, 1101)
    got = lib.bark_predictive_scores_workspace_bytes(64, 140, 50, 3, 1101)
    # the scan's areas plus (Bc + 1) x tiles x 2 doubles of tile partials, in 256-byte steps
    assert got == scan + -(-(4 * 5 * 2 * 8) // 256) * 256
    for bad in ((0, 140, 50, 3, 5), (64, 0, 50, 3, 5), (64, 140, 0, 3, 5), (64, 140, 50, 0, 5), (64, 140, 50, 3, 0)):
        assert lib.bark_predictive_scores_workspace_bytes(*bad) == 0


def test_argument_checks_come_before_any_device_use(monkeypatch):
    from bark_amd import _lib, synthetic
    from bark_amd.tree_kernels import loo_scores, predictive_scores

    def no_device(*a, **k):
        raise AssertionError("device touched before the argument checks")

    monkeypatch.setattr(_lib, "to_device", no_device)
    monkeypatch.setattr(_lib, "torch_device", no_device)
    inp = ar.make_inputs("m2_r65")
    y = sr.targets("m2_r65")
    with pytest.raises(ValueError, match="one entry per point"):
        predictive_scores(inp.model, inp.data, inp.cand, y[:-1], inp.ft)
    with pytest.raises(ValueError, match="one entry per point"):
        predictive_scores(inp.model, inp.data, inp.cand, np.zeros((len(y), 2)), inp.ft)
    with pytest.raises(ValueError, match="at least one point"):
        predictive_scores(inp.model, inp.data, inp.cand[:0], y[:0], inp.ft)
    with pytest.raises(ValueError, match="variant"):
        predictive_scores(inp.model, inp.data, inp.cand, y, inp.ft, variant="shared")
    with pytest.raises(ValueError, match="variant"):
        loo_scores(inp.model, inp.data, inp.ft, variant="shared")
    rng = np.random.default_rng(0)
    many = synthetic.full_binary_forest(65, ar.D_CONT, 1, rng, node_limit=ar.NODE_LIMIT)[None]
    with pytest.raises(ValueError, match="64 trees"):
        predictive_scores((many, inp.noise[:1], inp.scale[:1]), inp.data, inp.cand, y, inp.ft)
    with pytest.raises(ValueError, match="64 trees"):
        loo_scores((many, inp.noise[:1], inp.scale[:1]), inp.data, inp.ft)
