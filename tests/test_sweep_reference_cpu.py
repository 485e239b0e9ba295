"""The host reference of the dense sweep's options (tests/sweep_ref.py) against the goldens and the oracle, its own LU route
against a float64 Cholesky route at a tenth of every tolerance the GPU test applies (so that tests/test_gpu_sweep_options.py
measures the kernels and not the reference), and the case table against the plan query: every row reaches the cell it names,
every cell has a row, and every forest of a `shift` comparison has between 1 and m - 1 null trees.  No GPU.
(The fraction of each bar that the LU | Cholesky difference uses is printed per shape: run with -s to see it.)"""
import os
import re

import numpy as np
import pytest

import sweep_ref as sr
from conftest import load_golden
from oracle import oracle as orc

RAW = orc.nodes_from_raw
NAMES = list(sr.CASES)


class _Inputs(dict):
    """case name -> inputs, built on first use and kept for the module (sampling 288 prior forests takes seconds)"""

    def __missing__(self, name):
        self[name] = sr.make_inputs(sr.CASES[name])
        return self[name]


INPUTS = _Inputs()


def test_reference_reproduces_the_goldens():
    g = load_golden("g8_batched_mll")
    F, X, y, ft = RAW(g["forest"]), g["X"], g["y"], g["feat_types"]
    ex = sr.reference_arrays(F, X, y, ft, g["noise"], None, None)
    sa = sr.reference_arrays(F, X, y, ft, g["noise"], g["scale"], None)
    assert np.allclose([o["mll_2pi"] for o in ex], g["mll_example"], rtol=1e-12)
    assert np.allclose([o["mll"] for o in sa], g["mll_sampler"], rtol=1e-12)

    g = load_golden("g6_predict")
    F = RAW(g["forest"]).reshape(-1, 50, 100)
    out = sr.reference_arrays(F, g["X"], g["y"], g["feat_types"], g["noise"].reshape(-1), g["scale"].reshape(-1), None, cand=g["cand"])
    assert np.allclose([o["mu"] for o in out], g["mu"], rtol=1e-12, atol=1e-14)
    assert np.allclose([o["var"] for o in out], g["var"], rtol=1e-12, atol=1e-14)
    assert np.allclose([o["cov"] for o in out], g["var_full"], rtol=1e-12, atol=1e-14)

    g = load_golden("g3_prior_mixed_n257")
    F, noise, scale = RAW(g["forest"]), g["noise"], g["scale"]
    shift, factor = sr.no_null_params(F)
    assert (sr.n_null(F) >= 1).all()
    out = sr.reference_arrays(F, g["X"], g["y"], g["feat_types"], noise, scale * factor, shift, identity=True)
    for b in range(3):
        # the golden's K_no_null is factor * (K - shift) as the reference rounds it; scale * factor here is one more rounding
        K_s = scale[b] * g["K_no_null"][b] + (1e-6 + noise[b]) * np.eye(257)
        assert np.allclose(out[b]["K_s"], K_s, rtol=1e-14, atol=1e-16)
        want = np.linalg.inv(K_s)
        assert np.allclose(out[b]["K_inv"], want, rtol=1e-10, atol=1e-11)
        assert np.allclose(out[b]["K_inv_y"], (want @ g["y"])[:, 0], rtol=1e-10, atol=1e-11)
        assert np.allclose(out[b]["diag"], np.diagonal(want), rtol=1e-10, atol=1e-11)
        assert np.isclose(out[b]["logdet"], np.linalg.slogdet(K_s)[1], rtol=1e-12)


def test_reference_without_shift_is_the_oracle():
    inp = sr.make_inputs(sr.Case("seeded", "candidates", 150, 3, 20, 40, None, "prior", "mixed", ()))
    model = (inp.F, inp.noise, inp.scale)
    out = sr.reference(inp, range(3), shift=False)
    want = orc.batched_mll(*model, inp.X, inp.y, inp.ft, include_scale=True, include_2pi=False)
    assert np.allclose([o["mll"] for o in out], want, rtol=1e-13)
    mu, var = orc.forest_predict(model, (inp.X, inp.y), inp.cand, inp.ft)
    _, cov = orc.forest_predict(model, (inp.X, inp.y), inp.cand, inp.ft, diag=False)
    assert np.allclose([o["mu"] for o in out], mu, rtol=1e-12, atol=1e-14)
    assert np.allclose([o["var"] for o in out], var, rtol=1e-12, atol=1e-14)
    assert np.allclose([o["cov"] for o in out], cov, rtol=1e-12, atol=1e-14)
    bare = sr.reference(inp, range(3), shift=False, scale=False)
    want = orc.batched_mll(inp.F, inp.noise, None, inp.X, inp.y, inp.ft, include_scale=False, include_2pi=True)
    assert np.allclose([o["mll_2pi"] for o in bare], want, rtol=1e-13)
    # the steps are applied in the header's order: shift, then scale, then the jitter
    K = orc.forest_gram_matrix(inp.F[1], inp.X, inp.X, inp.ft)
    K_s = sr.reference(inp, [1])[0]["K_s"]
    assert np.array_equal(K_s, inp.scale[1] * (K - inp.shift[1]) + np.diag(np.full(150, 1e-6 + inp.noise[1])))


def test_every_cell_has_a_row():
    assert {c.cell for c in sr.CASES.values()} == set(sr.CELLS)
    kinds = {(c.cell, c.kind) for c in sr.CASES.values()}
    for cell in ("one_block", "two_block", "multi_block", "plain_fused", "pipelined_fused", "splitk", "candidates", "identity"):
        assert (cell, "prior") in kinds and ((cell, "bytes7") in kinds or (cell, "bytes8") in kinds), cell
    assert {c.n_cand for c in sr.CASES.values() if c.cell == "candidates"} >= {1, 127, 128, 129, 300}
    assert {c.null_scale for c in sr.CASES.values()} == {"", "one-launch", "fused row kernels", "gram.hip"}
    assert all(c.C == 0 for c in sr.CASES.values() if c.null_scale)
    la = sr.CASES["lookahead_n769_b50"]
    assert (la.N, la.B) == sr.smallest_lookahead_shape(m=la.m)
    # panel_reduce_kernel<GEN>: a fused row whose plan has split-K steps
    assert any(c.plan[2] == 1 and c.split for c in sr.CASES.values())


def test_ragged_tail_restates_the_source():
    """sweep_ref.ragged_tail reads the constants chol.hip's ragged_tail reads; and in a fused plain chunk (MLL only, at most 7 block
    rows: from 8 on such chunks are pipelined or paired) a split tail always starts at tile 0 — whole rounds of 512 workgroups in
    front of a tail of at most 192 would need 5 tiles at a chunk of 128, i.e. step 2, whose split of 2 is below the minimum of 3.
    With the short last chunks of the table's ragged rows the split itself is reached (check_cell asserts it per row).
    Only the constants are compared with the source: the rule itself (the j < 2 cut, the minimum split of 3, the tile-boundary
    condition) is restated by hand in sweep_ref.ragged_tail and must be kept in step with chol.hip's ragged_tail by hand."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "bark_amd", "csrc", "chol.hip")).read()
    assert int(re.search(r"constexpr int SPLITK_SLOTS = (\d+);", src).group(1)) == sr.SPLITK_SLOTS
    assert int(re.search(r"#define BARK_TAIL_MAX_WGS (\d+)", src).group(1)) == sr.TAIL_MAX_WGS
    assert int(re.search(r"#define BARK_SPLITK_MAX (\d+)", src).group(1)) == sr.SPLITK_MAX
    assert int(re.search(r"#define BARK_PIPE_MIN_NRB (\d+)", src).group(1)) == 8
    split = [(nrb, bc, st) for nrb in range(3, 8) for bc in range(1, 1025) for st in sr.ragged_steps(nrb, nrb, bc)]
    assert split and all(tail == 0 and s >= 3 and j >= 3 for _, _, (j, tail, s) in split)
    assert sr.ragged_steps(7, 7, 40) == [(3, 0, 3), (4, 0, 4), (5, 0, 5)] and sr.ragged_steps(6, 6, 10) == [(3, 0, 3), (4, 0, 4)]
    assert sr.ragged_steps(6, 6, 288) == sr.ragged_steps(6, 6, 192) == sr.ragged_steps(6, 6, 96) == []


@pytest.mark.parametrize("name", NAMES)
def test_row_reaches_its_cell(name):
    inp = INPUTS[name]
    d = sr.check_cell(inp)
    pick = sr.compared_forests(inp.case)
    assert len(pick) <= 3 * d["n_chunks"] and pick[0] == 0 and pick[-1] == inp.case.B - 1
    print(name, d["schedule"], d["last_schedule"], "words", inp.leaf_words, "null trees", sorted(set(sr.n_null(inp.F).tolist())))


WORST = {}


@pytest.mark.parametrize("name", [n for n in NAMES if sr.CASES[n].N <= 1100])
def test_lu_route_against_cholesky_route(name):
    """One forest per shape: the two float64 routes differ by less than a tenth of each output's tolerance."""
    inp = INPUTS[name]
    b = inp.case.B // 2
    lu, ch = sr.reference(inp, [b])[0], sr.reference(inp, [b], route="cholesky")[0]
    bars = {"mll": (sr.MLL_RTOL, sr.MLL_ATOL), "mll_2pi": (sr.MLL_RTOL, sr.MLL_ATOL), "logdet": (sr.LOGDET_RTOL, 0.0),
            "mu": (sr.POST_TOL, sr.POST_TOL), "var": (sr.POST_TOL, sr.POST_TOL), "cov": (sr.POST_TOL, sr.POST_TOL),
            "K_inv": (sr.INV_RTOL, sr.INV_ATOL), "K_inv_y": (sr.INV_RTOL, sr.INV_ATOL), "diag": (sr.INV_RTOL, sr.INV_ATOL)}
    used = {}
    for key, (rtol, atol) in bars.items():
        if key in lu:
            used[key] = float((np.abs(ch[key] - lu[key]) / (atol + rtol * np.abs(lu[key]))).max())
    if inp.case.identity:
        used["resid"] = float(np.abs(lu["K_inv"] @ lu["K_s"] - np.eye(inp.case.N)).max() / sr.RESID_ATOL)
    for k, v in used.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(name, {k: "%.2g" % v for k, v in used.items()}, "worst so far", {k: "%.2g" % v for k, v in WORST.items()})
    assert all(v < 0.1 for v in used.values()), used
    if inp.case.null_scale:
        lu, ch = sr.reference(inp, [b], scale=False)[0], sr.reference(inp, [b], scale=False, route="cholesky")[0]
        assert abs(ch["mll_2pi"] - lu["mll_2pi"]) < 0.1 * (sr.MLL_ATOL + sr.MLL_RTOL * abs(lu["mll_2pi"]))


@pytest.mark.parametrize("name", [n for n in NAMES if sr.CASES[n].N <= 1100])
def test_shift_changes_the_reference(name):
    """A test in which the shift is a no-op proves nothing: on the reference, the MLL with `shift` differs from the MLL without by
    more than 100 times the MLL bar (one forest of every shape up to N = 1100 here: LU solves beyond that take seconds each; the GPU
    test asserts it on its own references for every compared forest of every shape)."""
    case = sr.CASES[name]
    inp = INPUTS[name]
    b = case.B - 1
    with_shift, without = sr.reference(inp, [b])[0]["mll"], sr.reference(inp, [b], shift=False)[0]["mll"]
    assert abs(with_shift - without) > 100 * (sr.MLL_ATOL + sr.MLL_RTOL * abs(with_shift)), (with_shift, without)
