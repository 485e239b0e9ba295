"""Host side of the acquisition scan's target kinds (EI, PI, MES; no GPU): the prechecks that make the cases of
tests/test_gpu_acquisition_targets.py fit for an exact index test, the limits of the formulas in tests/acq_targets_ref.py,
the refusals of the Python front end that come before anything needs a device, and the plan of the other kinds."""
import math

import numpy as np
import pytest

import acq_pending_ref as apr
import acq_ref as ar
import acq_targets_ref as tr


@pytest.mark.parametrize("kind", tr.KINDS)
def test_prechecks_hold_for_the_chosen_cases(kind):
    """variance floor, a gap of MARGIN between best and runner-up, float64 within 1 % of the bar of mpmath"""
    names = tr.survivors(kind)
    print(f"{kind}: {len(names)} of {len(ar.CASES)} cases survive")
    assert "m1_r64" in names and len(names) >= tr.MIN_SURVIVORS
    assert names == tr.CASES[kind]  # the GPU tests run this list
    for name in names:
        v, bar, i = tr.precheck(name, kind)
        assert v.shape == bar.shape == (ar.CASES[name].C,) and i == int(np.argmin(v))


def test_targets_are_low_quantiles_of_the_reference_posterior():
    for name, case in ar.CASES.items():
        mu, _ = ar.posterior(name)
        t = tr.targets_of(name)
        assert t.shape == (case.B, tr.S_OF[name]) and tr.S_OF[name] in (1, 5)
        assert (t >= mu.min(axis=1, keepdims=True)).all() and (t <= np.median(mu, axis=1, keepdims=True)).all()
        assert (np.diff(t, axis=1) >= 0).all()


def test_pending_and_greedy_cases_are_fit():
    """the conditioned EI case and every pick of the greedy EI batch: a relative gap of MARGIN to the runner-up and a bar
    below half of it"""
    _, skip, v, bar, i = tr.pending_reference()
    gap = apr.gap_of(v, skip)[1]
    assert gap >= apr.MARGIN and float(bar.max()) < gap / 2 and i not in skip
    assert int(np.argmin(v)) in skip  # the skipped candidate would have won
    assert len(apr.pending_of(tr.PENDING_CASE)) == 2
    _, picks, vecs, bars = tr.greedy_ei()
    assert len(set(picks.tolist())) == tr.GREEDY_Q == len(picks)
    for k, (vec, b) in enumerate(zip(vecs, bars)):
        at, gap = apr.gap_of(vec, picks[:k])
        assert at == picks[k] and gap >= apr.MARGIN and float(b.max()) < gap / 2


def test_ei_limits():
    """S = 1: sd large -> sd phi(0) + (t - mu) / 2; t far above mu -> t - mu; t far below -> 0; sd == 0 -> max(t - mu, 0)"""
    mu = 0.3
    g = float(tr.utility(mu, 1e8, 1.0, "ei"))
    assert math.isclose(g, 1e8 / math.sqrt(2 * math.pi) + 0.5 * (1.0 - mu), rel_tol=1e-12)
    assert math.isclose(float(tr.utility(mu, 0.5, 1e6, "ei")), 1e6 - mu, rel_tol=1e-15)
    assert float(tr.utility(mu, 0.5, -1e6, "ei")) == 0.0
    assert float(tr.utility(mu, 0.5, -15.0, "ei")) > 0.0  # the tail is not flushed
    assert float(tr.utility(mu, 0.0, 1.0, "ei")) == 1.0 - mu and float(tr.utility(mu, 0.0, -1.0, "ei")) == 0.0
    # the acquisition is the negated mean: one forest, one target
    acq = tr.acquisition(np.array([[mu]]), np.array([[0.25]]), np.array([[1.0]]), "ei")
    assert acq.shape == (1,) and acq[0] == -float(tr.utility(mu, 0.5, 1.0, "ei"))


def test_pi_and_mes_limits():
    assert float(tr.utility(0.0, 1.0, 0.0, "pi")) == 0.5
    assert float(tr.utility(0.0, 0.0, 1.0, "pi")) == 1.0 and float(tr.utility(0.0, 0.0, -1.0, "pi")) == 0.0
    assert float(tr.utility(0.0, 1.0, 40.0, "pi")) == 1.0 and 0.0 < float(tr.utility(0.0, 1.0, -30.0, "pi")) < 1e-190
    # gam = 0: log(sd E) - log(E sd / 2) = log 2; t far above mu: no information (the truncation does not bind)
    assert math.isclose(float(tr.utility(0.3, 0.5, 0.3, "mes")), math.log(2.0), rel_tol=1e-12)
    assert abs(float(tr.utility(0.3, 0.5, 30.0, "mes"))) < 1e-12
    assert float(tr.utility(0.3, 0.0, 1.0, "mes")) == -np.inf  # sd == 0: never wins
    # S targets repeated: the same value up to the rounding of the mean
    mu, var = ar.posterior("m2_r65")
    t1 = tr.targets_of("m2_r65", 1)
    for kind in tr.KINDS:
        a, b = tr.acquisition(mu, var, t1, kind), tr.acquisition(mu, var, np.repeat(t1, 5, axis=1), kind)
        assert np.allclose(a, b, rtol=1e-14, atol=0.0)


def test_nan_target_gives_nan():
    for kind in tr.KINDS:
        assert np.isnan(tr.acquisition(np.zeros((2, 3)), np.ones((2, 3)), np.array([[0.1], [np.nan]]), kind)).all()


def test_python_refusals_need_no_gpu():
    from bark_amd.optimizer import acquisition_scan, propose_batch_from_candidates, propose_from_candidates

    inp = ar.make_inputs("m2_r65")
    args = (inp.model, inp.data, inp.cand, inp.ft)
    B = inp.case.B
    with pytest.raises(ValueError, match="needs targets"):
        acquisition_scan(*args, kind="mes")
    with pytest.raises(ValueError, match="needs targets"):
        propose_from_candidates(*args, kind="mes")
    with pytest.raises(ValueError, match="targets per forest"):
        acquisition_scan(*args, kind="ei", targets=np.zeros((B, 1025)))
    with pytest.raises(ValueError, match="targets per forest"):
        acquisition_scan(*args, kind="pi", targets=np.zeros((B, 0)))
    for bad in (np.zeros(B + 1), np.zeros((B + 1, 2)), np.zeros((1, B)), np.zeros((B, 2, 2))):
        with pytest.raises(ValueError, match="one row per forest"):
            acquisition_scan(*args, kind="mes", targets=bad)
        with pytest.raises(ValueError, match="one row per forest"):
            propose_batch_from_candidates(*args, q=2, kind="ei", targets=bad)
    with pytest.raises(ValueError, match="unknown kind"):
        acquisition_scan(*args, kind="ucb", targets=0.0)
    with pytest.raises(ValueError, match="kappa"):
        acquisition_scan(*args, kind="ei", targets=0.0, kappa=float("nan"))


def test_torch_targets_are_checked_like_numpy_ones():
    import torch

    from bark_amd.optimizer import acquisition_scan

    inp = ar.make_inputs("m2_r65")
    args = (inp.model, inp.data, inp.cand, inp.ft)
    with pytest.raises(ValueError, match="one row per forest"):
        acquisition_scan(*args, kind="ei", targets=torch.zeros(inp.case.B + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="targets per forest"):
        acquisition_scan(*args, kind="ei", targets=torch.zeros((inp.case.B, 1025), dtype=torch.float64))


# bark_acquisition_plan before the target kinds existed (R, m) -> (variant, dynamic LDS bytes): the table of R (R + 1) / 2 + R
# doubles and m x 256 16-bit ids where it fits the 160 KiB of a CU, the ids alone otherwise.  The target kinds add nothing.
PLAN = [(1, 1, "lds", 528), (64, 1, "lds", 17_664), (65, 2, "lds", 18_704), (140, 50, "lds", 105_680),
        (128, 64, "lds", 99_840), (256, 64, "global", 32_768), (8192, 64, "global", 32_768), (190, 1, "lds", 147_192),
        (201, 1, "global", 512)]


@pytest.mark.parametrize("R,m,variant,nbytes", PLAN)
def test_plan_of_the_existing_kinds_is_unchanged(R, m, variant, nbytes):
    from bark_amd.optimizer import acquisition_plan

    assert acquisition_plan(R, m) == {"variant": variant, "lds_bytes": nbytes}
    tri = (R * (R + 1) // 2 + R) * 8 + m * 512
    assert (variant == "lds") == (tri <= 160 * 1024) and nbytes == (tri if variant == "lds" else m * 512)


def test_lds_limit_at_13_trees_is_where_it_was():
    assert ar.lds_limit(13) == 196  # (196 * 197 / 2 + 196) * 8 + 13 * 512 = 162 672 <= 163 840 < 164 256 at R = 197
