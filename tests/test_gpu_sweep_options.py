"""The optional arguments of bark_mll_batched_hip — `shift` (the no-null kernel), `cov_out`, BARK_MLL_RHS_IDENTITY, a NULL
`scale` — on every schedule of the dense sweep and in every leaf representation, against the float64 host reference of
tests/sweep_ref.py (pinned to the goldens and the oracle, and every row to its cell, by tests/test_sweep_reference_cpu.py).

K_s is formed in five places (gram.hip; form_tile, syrk_tile and panel_reduce_kernel<GEN> of chol_rows.h; the one-launch kernels
of chol_diag.h), each with its own copy of `- shift`, `* scale`, `+ jitter`.  Every row of sweep_ref.CASES passes a `shift` that
differs per forest through one of them and checks: the first, middle and last forest of every chunk against the reference; that
the shift changes the result; that a shift of zeros is a NULL shift bit for bit over the whole batch; the whole batch against
another route (the instrumented multi-launch sweep for the one-launch kernels, another chunk size for the fused sweeps);
reproducibility; and that nothing is written outside the outputs (NaN guard bands) while every element inside is.
(The fraction of each bar that a row uses is printed: run with -s to see it.)"""
import numpy as np
import pytest

import sweep_ref as sr

pytestmark = pytest.mark.gpu


def close(got, want, rtol, atol):
    got, want = np.asarray(got), np.asarray(want)
    err = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())
    return err  # fraction of the allowed error used


def check_clean(out, name):
    assert out.guards_intact(), name  # nothing behind the (B, ...) outputs was written
    assert not any(out.nan_inside().values()), (name, out.nan_inside())  # and every element inside was
    assert int(out.info[:out.B].abs().max()) == 0, (name, out.host("info"))


@pytest.mark.parametrize("name", list(sr.CASES))
def test_shift_and_outputs_on_every_schedule(name):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    case = sr.CASES[name]
    inp = sr.make_inputs(case)
    sr.check_cell(inp)
    pick = sr.compared_forests(case)
    ref, ref0 = sr.reference(inp, pick), sr.reference(inp, pick, shift=False)
    mll_bar = lambda v: sr.MLL_ATOL + sr.MLL_RTOL * np.abs(v)
    want, want0 = np.array([r["mll"] for r in ref]), np.array([r["mll"] for r in ref0])
    assert (np.abs(want - want0) > 100 * mll_bar(want)).all(), (name, want - want0)  # the shift is no no-op in this row

    got = sr.run(inp)
    check_clean(got, name)
    used = {"mll": close(got.host("mll", pick), want, sr.MLL_RTOL, sr.MLL_ATOL)}
    if case.identity:
        y = inp.y1
        K_inv, K_inv_y, diag = got.host("cov", pick), got.host("mu", pick), got.host("var", pick)
        used["K_inv"] = close(K_inv, [r["K_inv"] for r in ref], sr.INV_RTOL, sr.INV_ATOL)
        used["K_inv_y"] = close(K_inv_y, [r["K_inv_y"] for r in ref], sr.INV_RTOL, sr.INV_ATOL)
        used["diag"] = close(diag, [r["diag"] for r in ref], sr.INV_RTOL, sr.INV_ATOL)
        logdet = -2.0 * got.host("mll", pick) - K_inv_y @ y  # mll = 0.5 (-y' K_s^-1 y - log|K_s|)
        used["logdet"] = close(logdet, [r["logdet"] for r in ref], sr.LOGDET_RTOL, 0.0)
        used["resid"] = max(float(np.abs(K_inv[i] @ r["K_s"] - np.eye(case.N)).max()) for i, r in enumerate(ref)) / sr.RESID_ATOL
        # var_out and the diagonal of cov_out: two reductions of the same V = U^-T, over the whole batch
        cov_diag = torch.diagonal(got.cov[:case.B], dim1=1, dim2=2)
        used["diag_vs_cov"] = float(((got.var[:case.B] - cov_diag).abs() / cov_diag.abs()).max()) / sr.SAME_V_RTOL
    elif case.C:
        used["mu"] = close(got.host("mu", pick), [r["mu"] for r in ref], sr.POST_TOL, sr.POST_TOL)
        used["var"] = close(got.host("var", pick), [r["var"] for r in ref], sr.POST_TOL, sr.POST_TOL)
        used["cov"] = close(got.host("cov", pick), [r["cov"] for r in ref], sr.POST_TOL, sr.POST_TOL)
        # var_out = scale - colsumsq(V) and cov_out = scale - V'V: scale - diag(cov_out) is the sum var_out subtracted
        scale = torch.as_tensor(inp.scale, device=got.var.device)[:, None]
        a, b = scale - got.var[:case.B], scale - torch.diagonal(got.cov[:case.B], dim1=1, dim2=2)
        used["var_vs_cov"] = float(((a - b).abs() / b.abs()).max()) / sr.SAME_V_RTOL
    print(name, "fraction of each bar used:", {k: "%.2g" % v for k, v in used.items()})
    assert all(v <= 1.0 for v in used.values()), (name, used)

    again = sr.run(inp)
    assert got.same_bits(again), name  # fixed summation orders: the same call gives the same bits in every output

    null = sr.run(inp, shift=None)
    check_clean(null, name)
    got0 = null.host("mll", pick)
    assert close(got0, want0, sr.MLL_RTOL, sr.MLL_ATOL) <= 1.0, name
    assert (np.abs(got.host("mll", pick) - got0) > 100 * mll_bar(want)).all(), name
    zeros = sr.run(inp, shift=np.zeros(case.B))
    assert zeros.same_bits(null), name  # val - 0.0 == val in every generator, for all B forests
    del again, null, zeros

    if case.other is not None:  # all B results through the other route
        other = sr.run(inp, timing=True) if case.other == "timing" else sr.run(inp, chunk=case.other)
        check_clean(other, name)
        if case.other == "timing":
            assert other.timing.n_diag_launches >= -(-case.N // 128)  # the multi-launch sweep
        a, b = got.host("mll"), other.host("mll")
        assert np.allclose(a, b, rtol=sr.ROUTE_RTOL, atol=0.0), (name, float(np.abs(a / b - 1).max()))
        if case.n_cand and not case.identity:  # every forest's mu, var and cov (the cov_out + c0 C C offset of every chunk) at the figure
            # test_gpu_parity.py::test_many_small_matrices_and_chunk_invariance uses for the posterior at another chunk size
            for key in ("mu", "var", "cov"):
                a, b = getattr(got, key)[:case.B], getattr(other, key)[:case.B]
                assert torch.allclose(a, b, rtol=1e-10, atol=1e-11), (name, key, float((a - b).abs().max()))

    if case.null_scale:  # flags without BARK_MLL_INCLUDE_SCALE, a NULL scale, a shift: MLL only
        bare = sr.run(inp, scale=None, two_pi=True)
        check_clean(bare, name)
        want_bare = [r["mll_2pi"] for r in sr.reference(inp, pick, scale=False)]
        assert close(bare.host("mll", pick), want_bare, sr.MLL_RTOL, sr.MLL_ATOL) <= 1.0, name
        assert bare.same_bits(sr.run(inp, scale=None, two_pi=True)), name
