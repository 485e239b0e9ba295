"""Host-side checks of the acquisition scan: the public names exist, the plan and workspace queries of
bark_acquisition_scan_hip answer without a GPU, the product path refuses to run without one, the host reference of
tests/acq_ref.py reproduces the reference's own golden posterior (g6), and every case of the GPU test is fit for an exact
index comparison (acq_ref.precheck)."""
import ctypes

import numpy as np
import pytest

import acq_ref as ar
from bark_amd import _lib

from conftest import load_golden


def test_public_names_import():
    from bark_amd import optimizer
    from bark_amd.optimizer.acquisition import acquisition_plan, acquisition_scan, propose_from_candidates

    assert optimizer.acquisition_scan is acquisition_scan and optimizer.propose_from_candidates is propose_from_candidates
    assert callable(acquisition_plan)
    assert (_lib.ACQ_LCB_MEAN, _lib.ACQ_LCB_MIXTURE) == (0, 1)


def test_workspace_query_grows_as_expected():
    q = _lib.lib().bark_acquisition_scan_workspace_bytes
    base = q(512, 146, 50, 4, 1000)
    assert base > 0
    assert q(512, 146, 50, 8, 1000) > base  # more forests per chunk
    assert q(512, 300, 50, 4, 1000) > base  # more leaves
    assert q(512, 146, 50, 4, 0) == 0 and q(512, 146, 50, 0, 1000) == 0 and q(0, 146, 50, 4, 1000) == 0
    # per candidate: three running sums (24 bytes) and the code words of the candidates in flight, which stop growing
    # at one slab of candidates: no (B, C) array
    step = q(512, 146, 50, 4, 2_000_000) - q(512, 146, 50, 4, 1_000_000)
    assert 24 * 1_000_000 <= step <= 25 * 1_000_000
    assert q(512, 146, 50, 256, 1_000_000) - q(512, 146, 50, 256, 500_000) <= 25 * 500_000


def plan(R, m, variant=0):
    v, n = ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = _lib.lib().bark_acquisition_plan(R, m, variant, ctypes.byref(v), ctypes.byref(n))
    return rc, v.value, n.value


def test_plan_chooses_lds_for_prior_forests_and_global_past_the_limit():
    rc, v, lds = plan(146, 50)
    assert (rc, v) == (0, 1)
    assert lds == 8 * (146 * 147 // 2 + 146) + 2 * 50 * ar.TILE  # triangle + w + the tile's leaf lists
    limit = ar.lds_limit(50)  # from the query, not a constant
    assert 146 < limit < 8192
    rc, v, fits = plan(limit, 50)
    assert (rc, v) == (0, 1)
    rc, v, past = plan(limit + 1, 50)
    assert (rc, v) == (0, 2) and past == 2 * 50 * ar.TILE  # the lists only
    assert plan(limit + 1, 50, 2)[:2] == (0, 2) and plan(146, 50, 2)[:2] == (0, 2)  # global may always be forced
    rc, v, need = plan(limit + 1, 50, 1)
    assert rc == _lib.BARK_ERR_ARG and v == 0 and need > fits
    assert b"LDS variant" in _lib.lib().bark_last_error()
    assert ar.lds_limit(13) > limit > ar.lds_limit(64)  # the leaf lists share the LDS
    for bad in ((146, 65, 0), (146, 0, 0), (8193, 50, 0), (0, 50, 0), (146, 50, 3), (146, 50, -1)):
        assert plan(*bad)[0] == _lib.BARK_ERR_ARG, bad


def test_python_plan():
    from bark_amd.optimizer import acquisition_plan

    assert acquisition_plan(146, 50)["variant"] == "lds"
    assert acquisition_plan(ar.lds_limit(50) + 1, 50)["variant"] == "global"
    with pytest.raises(ValueError, match="LDS variant"):
        acquisition_plan(ar.lds_limit(50) + 1, 50, "lds")
    with pytest.raises(ValueError, match="unknown variant"):
        acquisition_plan(146, 50, "fast")


def test_product_path_without_gpu():
    import torch

    from bark_amd.optimizer import acquisition_scan

    inp = ar.make_inputs("m2_r65")
    # argument errors do not need a device
    with pytest.raises(ValueError, match="unknown kind"):
        acquisition_scan(inp.model, inp.data, inp.cand, inp.ft, kind="ucb")
    with pytest.raises(ValueError, match="kappa"):
        acquisition_scan(inp.model, inp.data, inp.cand, inp.ft, kappa=float("nan"))
    with pytest.raises(ValueError, match="at least one candidate"):
        acquisition_scan(inp.model, inp.data, inp.cand[:0], inp.ft)
    if torch.cuda.is_available():
        value, index = acquisition_scan(inp.model, inp.data, inp.cand, inp.ft)
        assert np.isfinite(value) and 0 <= index < len(inp.cand)
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            acquisition_scan(inp.model, inp.data, inp.cand, inp.ft)


@pytest.mark.parametrize("name", list(ar.CASES))
def test_precheck_of_the_gpu_cases(name):
    """float64 and longdouble agree on the arg-min, the best value is MARGIN below every other one and no variance is
    below VAR_FLOOR; the bushy cases reach the leaf count they claim"""
    case = ar.CASES[name]
    inp = ar.make_inputs(name)
    assert inp.F.shape[:2] == (case.B, case.m) and inp.cand.shape == (case.C, 8) and inp.X.shape == (case.N, 8)
    assert set(inp.ft) == {0, 1, 2}  # categorical, integer and continuous columns
    from bark_amd.tree_kernels import posterior_sample_dim

    R = posterior_sample_dim(inp.F, inp.ft)
    if ar.resolve_R(case) is not None:
        assert R == ar.resolve_R(case)
    got = ar.precheck(name)
    assert set(got) == set(ar.KINDS)


def test_case_table_reaches_the_edges():
    R = {n: ar.resolve_R(c) for n, c in ar.CASES.items()}
    assert R["m1_r64"] == 64 and R["m2_r65"] == 65  # both sides of a 32-bit code-word edge
    assert R["m13_past_lds"] == R["m13_lds_limit"] + 1 == ar.lds_limit(13) + 1
    assert {c.m for c in ar.CASES.values()} >= {1, 13, 50, 64}
    assert {c.N for c in ar.CASES.values()} == {64, 257}
    assert {c.C for c in ar.CASES.values()} >= {1, ar.TILE - 1, ar.TILE, ar.TILE + 1}
    assert any(c.C > 3 * ar.TILE and c.C % ar.TILE for c in ar.CASES.values())
    assert {c.B for c in ar.CASES.values()} >= {1, 3}
    assert any(c.chunk and -(-c.B // c.chunk) == 3 for c in ar.CASES.values())
    from bark_amd.optimizer import acquisition_plan

    assert acquisition_plan(128, 64)["variant"] == "lds" and acquisition_plan(256, 64)["variant"] == "global"


def test_g6_pin():
    """The reference's own posterior at 33 candidates (golden g6): both acquisitions have their minimum at candidate 26"""
    g = load_golden("g6_predict")
    for kind, gap in (("lcb_mean", 0.119), ("lcb_mixture", 0.285)):
        for dtype in (np.float64, np.longdouble):
            v = ar.acquisition(g["mu"], g["var"], 1.96, kind, dtype)
            assert int(np.argmin(v)) == 26, kind
            assert abs(float(np.sort(v)[1] - v[26]) - gap) < 5e-4, (kind, float(np.sort(v)[1] - v[26]))
    mu_y, var_y = g["mix_mu"], g["mix_var"]  # the reference's mixture moments give the same vector
    v = ar.acquisition(g["mu"], g["var"], 1.96, "lcb_mixture")
    assert np.allclose(v, mu_y - 1.96 * np.sqrt(var_y), rtol=1e-12, atol=1e-12)
