"""Leaf-space MLL, posterior, explicit inverse and joint draws (bark_mll_leafspace_hip, bark_kernel_inverse_leafspace_hip,
bark_posterior_samples_hip) over the shape matrix of the R x R system, against the float64 host reference of
tests/leafspace_ref.py (pinned to the oracle's N-space route by tests/test_leafspace_reference_cpu.py).

The case table (leafspace_ref.CASES) reaches R = 50 ... 8192 leaves (2 ... 256 code words, 1 ... 64 block rows), every
layout of the R x R sweep with identity columns (plain at 1, 2, 3 and 5 block rows, split-K, pipelined), a chunk of forests
with different leaf counts, leaves that no training point reaches, every gather width of the draws (S = 1 ... 130) and
candidate counts around the gather's 64-candidate workgroups.  Each output is held to the tolerance the project's existing
tests use for it."""
import numpy as np
import pytest

import leafspace_ref as lr

pytestmark = pytest.mark.gpu

MLL_RTOL, MLL_ATOL = 1e-9, 1e-8  # the MLL tests (test_gpu_parity.py)
POST_TOL = 1e-9  # mu, var: test_posterior_against_oracle_ragged
INV_RTOL, INV_ATOL = 1e-8, 1e-9  # K_inv, K_inv_y: test_kernel_inverse_for_acquisition_builder
LOGDET_RTOL = 1e-10  # ... its logdet
DRAW_TOL = 1e-9  # test_gpu_posterior_samples.py::test_g6_mean_pinned_to_reference
CHUNK_RTOL = 1e-12  # test_many_small_matrices_and_chunk_invariance
NAMES = list(lr.CASES)


@pytest.fixture(scope="module")
def api():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import bark_amd.fitting as fit
    import bark_amd.tree_kernels as tk
    from bark_amd import _lib
    from bark_amd.fitting.mll import _run_leafspace

    class NS:
        pass

    ns = NS()
    ns.fit, ns.tk, ns.lib, ns.run_leafspace = fit, tk, _lib, _run_leafspace
    return ns


class _Prepared(dict):
    """case name -> (inputs, host reference of every output), built on first use and kept for the module"""

    def __missing__(self, name):
        inp = lr.make_inputs(lr.CASES[name])
        out = {k: [] for k in ("mll", "mu", "var", "K_inv", "K_inv_y", "logdet", "f")}
        for b in range(inp.case.B):
            ref = lr.reference(inp, b)
            mu, var = ref.posterior(inp.Zc[b])
            K_inv, K_inv_y = ref.inverse()
            vals = (ref.mll(), mu, var, K_inv, K_inv_y, ref.logdet(), ref.draws(inp.Zc[b], inp.eps[b]))
            for k, v in zip(out, vals):
                out[k].append(v)
            del ref
        self[name] = inp, {k: np.array(v) for k, v in out.items()}
        return self[name]


@pytest.fixture(scope="module")
def prepared():
    return _Prepared()


def posterior(api, inp, chunk=None):
    """(mll, mu, var) of one bark_mll_leafspace_hip call with the candidates (the sweep with identity columns)"""
    mll, mu, var = api.run_leafspace(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, api.lib.MLL_INCLUDE_SCALE,
                                     chunk=chunk or inp.case.bc, cand=inp.cand)
    return mll.cpu().numpy(), mu.cpu().numpy(), var.cpu().numpy()


def inverse(api, inp, chunk=None):
    return api.fit.batched_kernel_inverse(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, no_null=False,
                                          method="leafspace", chunk=chunk or inp.case.bc)


def draws(api, inp, cand=None, eps=None, chunk=None, reduce=None):
    eps = inp.eps if eps is None else eps
    return api.tk.posterior_samples((inp.F, inp.noise, inp.scale), (inp.X, inp.y), inp.cand if cand is None else cand, inp.ft,
                                    eps.shape[1], eps=eps, chunk=chunk or inp.case.bc, reduce=reduce)


def close(got, want, rtol, atol):
    """np.allclose, with the largest error relative to the allowed one in the message"""
    err = np.abs(got - want) / (atol + rtol * np.abs(want))
    return bool(np.all(err <= 1.0)), float(err.max())


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_shape(api, prepared, name):
    inp, _ = prepared[name]
    lr.check_shape(inp)
    assert api.tk.posterior_sample_dim(inp.F, inp.ft) == inp.R


@pytest.mark.parametrize("name", NAMES)
def test_mll(api, prepared, name):
    inp, ref = prepared[name]
    got = api.fit.batched_mll(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False,
                              method="leafspace", chunk=inp.case.bc)
    ok, err = close(got, ref["mll"], MLL_RTOL, MLL_ATOL)
    assert ok, err


@pytest.mark.parametrize("name", NAMES)
def test_posterior(api, prepared, name):
    inp, ref = prepared[name]
    mll, mu, var = posterior(api, inp)
    for key, got, rtol, atol in (("mll", mll, MLL_RTOL, MLL_ATOL), ("mu", mu, POST_TOL, POST_TOL), ("var", var, POST_TOL, POST_TOL)):
        ok, err = close(got, ref[key], rtol, atol)
        assert ok, (key, err)


@pytest.mark.parametrize("name", NAMES)
def test_inverse(api, prepared, name):
    inp, ref = prepared[name]
    K_inv, K_inv_y, logdet = inverse(api, inp)
    assert K_inv.shape == (inp.case.B, inp.case.N, inp.case.N)
    for key, got, rtol, atol in (("K_inv", K_inv, INV_RTOL, INV_ATOL), ("K_inv_y", K_inv_y, INV_RTOL, INV_ATOL),
                                 ("logdet", logdet, LOGDET_RTOL, 0.0)):
        ok, err = close(got, ref[key], rtol, atol)
        assert ok, (key, err)


@pytest.mark.parametrize("name", NAMES)
def test_draws(api, prepared, name):
    inp, ref = prepared[name]
    f = draws(api, inp)
    assert f.shape == (inp.case.B, inp.case.S, inp.case.C) and f.dtype == np.float64
    ok, err = close(f, ref["f"], DRAW_TOL, DRAW_TOL)
    assert ok, err


@pytest.mark.parametrize("C,S", [(1, 1), (1, 17), (1, 65), (65, 1), (65, 17), (65, 65)])
def test_reductions_equal_the_full_output(api, prepared, C, S):
    """max / min over the candidates, bit for bit, ties to the lowest index; 17 code words per candidate (the gather's
    second group of eight words), one candidate alone in the last gather workgroup at C = 65"""
    inp, _ = prepared["r513_splitk"]
    eps = np.random.default_rng(1000 * C + S).standard_normal((inp.case.B, S, inp.R))
    full = draws(api, inp, cand=inp.cand[:C], eps=eps)
    for red, op, arg in (("max", np.max, np.argmax), ("min", np.min, np.argmin)):
        v, i = draws(api, inp, cand=inp.cand[:C], eps=eps, reduce=red)
        assert v.shape == (inp.case.B, S) and i.dtype == np.int64
        assert np.array_equal(v, op(full, axis=-1)) and np.array_equal(i, arg(full, axis=-1)), red


@pytest.mark.parametrize("name,chunk", [("m64_r256", 1), ("prior_ragged", 2), ("r2048_pipelined", 1)])
def test_chunking(api, prepared, name, chunk):
    """Chunks of `chunk` forests (prior_ragged: B = 5, a ragged last chunk of one) against one chunk of all B: identical
    where both take the same R x R layout; otherwise within the project's chunk-invariance tolerance, rtol 1e-12, with an
    absolute floor of 1e-12 times the output's largest magnitude (entries near zero are sums of terms of that size)."""
    inp, _ = prepared[name]
    B = inp.case.B
    same = lr.rr_layout(inp.R, B) == lr.rr_layout(inp.R, chunk)
    whole = (*posterior(api, inp, chunk=B), draws(api, inp, chunk=B), *inverse(api, inp, chunk=B))
    part = (*posterior(api, inp, chunk=chunk), draws(api, inp, chunk=chunk), *inverse(api, inp, chunk=chunk))
    for k, (a, b) in enumerate(zip(whole, part)):
        if same:
            assert np.array_equal(a, b), k
        else:
            ok, err = close(b, a, CHUNK_RTOL, CHUNK_RTOL * float(np.abs(a).max()))
            assert ok, (k, err)
    if name == "r2048_pipelined":
        assert not same  # pipelined at 6 forests, split-K at 1


@pytest.mark.parametrize("m", [512, 513, 1280])
def test_inverse_up_to_the_tree_limit(api, m):
    """leaf_inverse_kernel keeps m x 64 16-bit leaf ids in LDS: 64 KiB at m = 512, more from 513 on, all 160 KiB at 1280.
    Depth-1 trees and null trees at N = 100, against the host reference."""
    inp = lr.make_inputs(lr.limit_case(m), node_limit=3)
    assert inp.m == m and inp.R == m + m // 2
    ref = lr.reference(inp, 0)
    K_inv0, K_inv_y0 = ref.inverse()
    K_inv, K_inv_y, logdet = inverse(api, inp)
    for key, got, want, rtol, atol in (("K_inv", K_inv[0], K_inv0, INV_RTOL, INV_ATOL),
                                       ("K_inv_y", K_inv_y[0], K_inv_y0, INV_RTOL, INV_ATOL),
                                       ("logdet", logdet[0], ref.logdet(), LOGDET_RTOL, 0.0)):
        ok, err = close(got, want, rtol, atol)
        assert ok, (key, err)


def test_inverse_refuses_more_trees_than_its_lds_holds(api):
    inp = lr.make_inputs(lr.limit_case(1281), node_limit=3)
    with pytest.raises(ValueError, match="at most 1280 trees"):
        inverse(api, inp)
    # the MLL alone has no such limit, and nothing is left behind
    got = api.fit.batched_mll(inp.F, inp.noise, inp.scale, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False,
                              method="leafspace")
    ok, err = close(got, np.array([lr.reference(inp, 0).mll()]), MLL_RTOL, MLL_ATOL)
    assert ok, err
