"""Predictive scores on the device (bark_predictive_scores_hip through `predictive_scores` / `loo_scores`) against the host
reference of tests/scores_ref.py, over the cases of tests/acq_ref.py: several tiles with a ragged tail, three chunks of forests,
one tree and one point, both sides of a code-word edge and of the LDS limit, the tree limit, and two slabs of points.

Bars (derived in scores_ref's docstring): the posterior bar of DESIGN.md section 2 times the case's amplification A of a
posterior error into a log density; times G as well for the leave-one-out moments.  The summation order is part of the
contract, so chunking and the two kernel variants are compared bit for bit.

Largest deviation measured, as a fraction of the case's bar: see DESIGN.md section 5, "Predictive scores"."""
import numpy as np
import pytest

import acq_ref as ar
import scores_ref as sr

pytestmark = pytest.mark.gpu
LDS_CASES = ("prior_n64", "prior_n257_chunks", "m1_r64", "m2_r65", "m13_lds_limit")


@pytest.fixture(scope="module")
def tk():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from bark_amd import tree_kernels

    return tree_kernels


def heldout(tk, name, **kw):
    inp = sr.inputs(name)
    kw.setdefault("chunk", inp.case.chunk)
    kw.setdefault("return_values", True)
    return tk.predictive_scores(inp.model, inp.data, inp.cand, sr.targets(name), inp.ft, **kw)


def heldout_device(tk, name, **kw):
    import torch

    inp = sr.inputs(name)
    kw.setdefault("chunk", inp.case.chunk)
    return tk.predictive_scores(inp.model, inp.data, torch.as_tensor(inp.cand, device="cuda"), sr.targets(name), inp.ft,
                                return_values=True, **kw)


def bar_used(got, want, amp):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (amp * (ar.ATOL + ar.RTOL * np.abs(want)))).max())


def check(got, want, amp, what):
    worst = 0.0
    for k in sr.KEYS:
        assert np.shape(got[k]) == np.shape(want[k]), (what, k)
        used = bar_used(got[k], want[k], amp)
        print(f"{what} {k}: fraction of the bar used {used:.3g}")
        worst = max(worst, used)
    assert worst <= 1.0, what


@pytest.mark.parametrize("name", sr.GPU_CASES)
def test_heldout_against_reference(tk, name):
    amp = sr.precheck(name)
    got = heldout(tk, name)
    case = sr.case_of(name)
    assert got["nlpd"].shape == (case.B,) and got["log_density"].shape == (case.C,) and isinstance(got["nlpd_mixture"], float)
    check(got, sr.heldout(name, np.longdouble), amp, name)


@pytest.mark.parametrize("name", ["m13_lds_limit", "m13_past_lds", "m64_r256"])
def test_case_takes_the_variant_it_claims(tk, name):
    from bark_amd.optimizer import acquisition_plan

    inp = sr.inputs(name)
    want = "lds" if name == "m13_lds_limit" else "global"
    assert acquisition_plan(tk.posterior_sample_dim(inp.F, inp.ft), inp.case.m)["variant"] == want
    if want == "global":
        with pytest.raises(ValueError, match="LDS variant"):
            heldout(tk, name, variant="lds")


def same(a, b):
    import torch

    return all(torch.equal(a[k], b[k]) for k in sr.KEYS)


@pytest.mark.parametrize("name", LDS_CASES)
def test_lds_and_global_variants_are_bit_identical(tk, name):
    a = heldout_device(tk, name, variant="lds")
    assert same(a, heldout_device(tk, name, variant="global"))
    assert same(a, heldout_device(tk, name))  # auto


@pytest.mark.parametrize("name", ["prior_n257_chunks", "prior_n64", ar.SLAB_CASE.name])
def test_chunking_is_bit_identical(tk, name):
    base = heldout_device(tk, name)
    for chunk in (1, 2, sr.case_of(name).B):
        assert same(base, heldout_device(tk, name, chunk=chunk)), chunk


@pytest.mark.parametrize("name", ["prior_n64", "m13_past_lds", "m64_r256"])
def test_agrees_with_forest_predict_and_metrics(tk, name):
    """the route the scores replace: the (B, C) posterior of the leaf-space predict, then utils.metrics"""
    from bark_amd.utils import metrics

    inp, y = sr.inputs(name), sr.targets(name)[:, None]
    amp = sr.precheck(name)
    mu, var = tk.forest_predict(inp.model, inp.data, inp.cand, inp.ft, method="leafspace")
    got = heldout(tk, name)
    mix = np.log(np.exp(metrics.gaussian_log_likelihood(mu.T, var.T, y)).mean(axis=1))
    want = {"nlpd": metrics.nlpd(mu.T, var.T, y), "mse": np.array([metrics.mse(mu[b][:, None], y) for b in range(len(mu))]),
            "nlpd_mixture": -mix.sum() / len(y), "mse_mixture": metrics.mse(mu.mean(axis=0)[:, None], y)}
    for k, w in want.items():
        used = bar_used(got[k], w, amp)
        print(f"{name} {k}: fraction of the bar used {used:.3g}")
        assert used <= 1.0, k


# ---- leave one out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.LOO_CASES)
def test_loo_against_the_inverse(tk, name):
    inp = ar.make_inputs(name)
    amp = sr.loo_precheck(name)
    got = tk.loo_scores(inp.model, inp.data, inp.ft, return_values=True, chunk=inp.case.chunk)
    check(got, sr.loo(name, np.longdouble), amp, f"loo {name}")


def test_loo_against_brute_force_refits(tk):
    inp = sr.brute_inputs()
    amp = sr.loo_precheck("brute")
    got = tk.loo_scores(inp.model, inp.data, inp.ft, return_values=True)
    mu, var = sr.loo_brute()
    check(got, sr.scores(mu, var, inp.y.reshape(-1), np.longdouble), amp, "loo brute")


def test_loo_variants_and_chunks_are_bit_identical(tk):
    import torch

    inp = ar.make_inputs("prior_n257_chunks")
    data = (torch.as_tensor(inp.X, device="cuda"), inp.y)
    base = tk.loo_scores(inp.model, data, inp.ft, return_values=True)
    for kw in (dict(chunk=1), dict(chunk=2), dict(variant="lds"), dict(variant="global")):
        assert same(base, tk.loo_scores(inp.model, data, inp.ft, return_values=True, **kw)), kw


# ---- the raw entry point ------------------------------------------------------------------------------------------
def raw(model, data, points, y_points, ft, mode, check_status=True):
    """bark_predictive_scores_hip without the Python front end's reading of info -> (status, rows (B, 2), mixture (2,), info (B,))"""
    import torch

    from bark_amd import _lib
    from bark_amd.fitting.mll import _leaf_inputs, _y_vector

    F, noise, scale = model
    q = _leaf_inputs(F, noise, scale, data[0], data[1], ft, points)
    yp = _y_vector(y_points, len(y_points))
    rows = torch.zeros((q.B, 2), dtype=torch.float64, device=q.device)
    mix = torch.zeros(2, dtype=torch.float64, device=q.device)
    info = torch.zeros(q.B, dtype=torch.int32, device=q.device)
    lib = _lib.lib()
    ws = _lib.workspace(int(lib.bark_predictive_scores_workspace_bytes(q.N, q.R, q.pf.m, q.B, q.C)))
    rc = lib.bark_predictive_scores_hip(_lib.ctx(), _lib.ptr(q.pf.packed), q.pf.info_ref, _lib.ptr(q.Xd), q.N, q.d, _lib.ptr(q.yd),
                                        _lib.ptr(q.noise_d), _lib.ptr(q.scale_d), _lib.ptr(q.cand_d), q.C, _lib.ptr(yp), mode, 0,
                                        _lib.ptr(rows), _lib.ptr(mix), None, _lib.ptr(info), _lib.ptr(ws), ws.numel(), q.B,
                                        _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, rows, mix, info


def test_entry_refuses_loo_with_other_points():
    from bark_amd import _lib

    inp, y = ar.make_inputs("m2_r65"), sr.targets("m2_r65")
    assert len(inp.cand) != len(inp.X)
    rc, rows, mix, _ = raw(inp.model, inp.data, inp.cand, y, inp.ft, _lib.SCORE_LOO)
    assert rc == _lib.BARK_ERR_ARG and b"training points" in _lib.lib().bark_last_error()
    assert not rows.any() and not mix.any()  # nothing was launched
    rc, _, _, _ = raw(inp.model, inp.data, inp.cand, y, inp.ft, 2)
    assert rc == _lib.BARK_ERR_ARG and b"mode" in _lib.lib().bark_last_error()


def test_failed_forest_is_isolated(tk):
    """One forest of three with 1e-6 + noise < 0, hence c < 0 and a leaf-space matrix that is not positive definite (the
    construction of tests/test_gpu_posterior_samples.py): LinAlgError from Python; from the raw entry NaN in its row and in the
    mixture, the other rows those of the call without it."""
    import torch

    from bark_amd import _lib

    inp, y = ar.make_inputs("prior_n64"), sr.targets("prior_n64")
    noise = inp.noise.copy()
    noise[1] = -0.5
    with pytest.raises(np.linalg.LinAlgError):
        tk.predictive_scores((inp.F, noise, inp.scale), inp.data, inp.cand, y, inp.ft)
    with pytest.raises(np.linalg.LinAlgError):
        tk.loo_scores((inp.F, noise, inp.scale), inp.data, inp.ft)
    rc, rows, mix, info = raw((inp.F, noise, inp.scale), inp.data, inp.cand, y, inp.ft, _lib.SCORE_HELDOUT)
    assert rc == 0 and info[1] != 0 and info[0] == 0 and info[2] == 0
    assert torch.isnan(rows[1]).all() and torch.isnan(mix).all()
    keep = [0, 2]
    rc2, rows2, mix2, info2 = raw((inp.F[keep], inp.noise[keep], inp.scale[keep]), inp.data, inp.cand, y, inp.ft, _lib.SCORE_HELDOUT)
    assert rc2 == 0 and not info2.any() and torch.isfinite(mix2).all()
    assert torch.equal(rows[keep], rows2)
    # a clean call afterwards
    assert np.isfinite(tk.predictive_scores(inp.model, inp.data, inp.cand, y, inp.ft)["nlpd"]).all()


def test_nan_target_propagates(tk):
    inp, y = ar.make_inputs("prior_n64"), sr.targets("prior_n64").copy()
    y[ar.TILE + 3] = np.nan
    got = heldout(tk, "prior_n64")
    bad = tk.predictive_scores(inp.model, inp.data, inp.cand, y, inp.ft, return_values=True, chunk=inp.case.chunk)
    assert np.isnan(bad["nlpd"]).all() and np.isnan(bad["mse"]).all() and np.isnan(bad["nlpd_mixture"]) and np.isnan(bad["mse_mixture"])
    ok = np.arange(len(y)) != ar.TILE + 3
    assert np.isnan(bad["log_density"][~ok]).all() and np.array_equal(bad["log_density"][ok], got["log_density"][ok])


# ---- round trips --------------------------------------------------------------------------------------------------
def test_round_trips(tk):
    import torch

    inp, y = ar.make_inputs("m2_r65"), sr.targets("m2_r65")
    got = tk.predictive_scores(inp.model, inp.data, inp.cand, y, inp.ft, return_values=True)
    assert all(isinstance(got[k], np.ndarray) and got[k].dtype == np.float64 for k in ("nlpd", "mse", "log_density", "sq_err"))
    assert isinstance(got["nlpd_mixture"], float) and isinstance(got["mse_mixture"], float)
    assert set(tk.predictive_scores(inp.model, inp.data, inp.cand, y, inp.ft)) == {"nlpd", "mse", "nlpd_mixture", "mse_mixture"}
    dev = tk.predictive_scores(inp.model, inp.data, torch.as_tensor(inp.cand, device="cuda"), torch.as_tensor(y, device="cuda"),
                               inp.ft, return_values=True)
    for k in sr.KEYS:
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda and dev[k].dtype == torch.float64
        assert np.array_equal(dev[k].cpu().numpy(), got[k])
    assert dev["nlpd"].shape == (3,) and dev["nlpd_mixture"].ndim == 0 and dev["sq_err"].shape == (5,)
    loo = tk.loo_scores(inp.model, (torch.as_tensor(inp.X, device="cuda"), inp.y), inp.ft)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in loo.values())
    loo_np = tk.loo_scores(inp.model, inp.data, inp.ft)
    assert isinstance(loo_np["nlpd"], np.ndarray) and isinstance(loo_np["mse_mixture"], float)
    assert np.array_equal(loo["nlpd"].cpu().numpy(), loo_np["nlpd"])
