"""Host-side checks of the acquisition scan conditioned on pending points: for every case of the GPU test
(tests/test_gpu_acquisition_pending.py) the leaf-space downdate (a) in longdouble agrees with the oracle's dense route (b)
within 1 % of the posterior bar, the winner is separated from the best value that differs from it by a relative gap of at
least 1e-6 in float64 and in longdouble (so the device has to return identical indices) at every pick of every greedy
case, and w is unchanged by the conditioning; the refusals of the Python layer that need no device.

Smallest gap found over all cases, kinds and picks: 1.76e-3 (greedy_q8_n257, lcb_mean, pick 7); the seeds of
acq_pending_ref.CASES and the noise of acq_ref.make_inputs (0.1 ... 0.3) were kept because every gap clears 1e-6 by three
orders of magnitude."""
import numpy as np
import pytest

import acq_pending_ref as pr
import acq_ref as ar
from bark_amd import _lib


def within(got, want, fraction=1.0):
    return float((np.abs(got - want) / (fraction * (pr.ATOL + pr.RTOL * np.abs(want)))).max())


def check_vectors(inp, pending, kappa, skip=(), cand=None):
    """(a) in both precisions against (b) for both kinds; -> {kind: (index, gap)} with the smaller of the two gaps"""
    mu_b, var_b = pr.dense(inp, pending, cand)
    mu64, var64, _ = pr.leafspace(inp, pending, cand)
    muld, varld, _ = pr.leafspace(inp, pending, cand, np.longdouble)
    assert var_b.min() >= ar.VAR_FLOOR / 10, float(var_b.min())  # pending points collapse the variance near them, not to zero
    out = {}
    for kind in pr.KINDS:
        vb = ar.acquisition(mu_b, var_b, kappa, kind)
        v64 = ar.acquisition(mu64, var64, kappa, kind)
        vld = ar.acquisition(muld, varld, kappa, kind, np.longdouble)
        used = within(vld.astype(np.float64), vb, pr.AGREE)
        assert used <= 1.0, (kind, used)
        i64, g64 = pr.gap_of(v64, skip)
        ild, gld = pr.gap_of(vld.astype(np.float64), skip)
        ib, gb = pr.gap_of(vb, skip)
        assert i64 == ild == ib, (kind, i64, ild, ib)
        assert min(g64, gld, gb) >= pr.MARGIN, (kind, g64, gld, gb)
        out[kind] = (ib, min(g64, gld, gb))
    return out


@pytest.mark.parametrize("name", pr.CONDITIONING + pr.AWKWARD + ["pair_ab", "pair_ba"])
def test_conditioning_cases(name):
    case = pr.CASES[name]
    inp = ar.make_inputs(case.base)
    got = check_vectors(inp, pr.pending_of(name), case.base.kappa)
    for kind in pr.KINDS:
        print(f"{name} {kind}: gap {got[kind][1]:.3g}")
        assert got[kind][0] == pr.conditioned(name)[kind][1]


@pytest.mark.parametrize("name", pr.GREEDY)
def test_greedy_cases(name):
    """every pick of the reference loop: the same three checks on the scan that pick is the arg-min of"""
    case = pr.CASES[name]
    inp = ar.make_inputs(case.base)
    for kind in pr.KINDS:
        picks, _, pends = pr.greedy(name, kind)
        assert len(set(picks.tolist())) == case.q
        for k in range(case.q):
            got = check_vectors(inp, pends[k], case.base.kappa, skip=picks[:k].tolist())
            print(f"{name} {kind} pick {k}: index {got[kind][0]} gap {got[kind][1]:.3g}")
            assert got[kind][0] == picks[k]


def test_slab_case():
    """C = 70 000 under two-tree forests: many candidates share all their leaves, so the winner is tied with exact copies
    (the lowest index wins) and separated from every other value.  (a) over all candidates, (b) on the strided subset."""
    case = pr.SLAB
    inp = ar.make_inputs(case.base)
    pend = pr.pending_of(case)
    mu64, var64, _ = pr.leafspace(inp, pend)
    muld, varld, _ = pr.leafspace(inp, pend, dtype=np.longdouble)
    sub = inp.cand[::pr.SLAB_STRIDE]
    mu_b, var_b = pr.dense(inp, pend, sub)
    for kind in pr.KINDS:
        v64 = ar.acquisition(mu64, var64, case.base.kappa, kind)
        vld = ar.acquisition(muld, varld, case.base.kappa, kind, np.longdouble).astype(np.float64)
        vb = ar.acquisition(mu_b, var_b, case.base.kappa, kind)
        assert within(vld[::pr.SLAB_STRIDE], vb, pr.AGREE) <= 1.0
        (i64, g64), (ild, gld) = pr.gap_of(v64), pr.gap_of(vld)
        print(f"{case.name} {kind}: index {i64} gap {min(g64, gld):.3g}")
        assert i64 == ild and min(g64, gld) >= pr.MARGIN


@pytest.mark.parametrize("name", ["n20_m1_p1", "n64_m13_p2", "same_point_twice", "unreached_leaves"])
def test_w_is_unchanged_by_the_believer(name):
    """w' = w + t (y* - c z'w) / (1 + c q) with y* = c z'w: the innovation is zero.  Numerically: w recomputed from the
    system augmented by the pending points, each observed at the posterior mean, equals w."""
    inp = ar.make_inputs(pr.CASES[name].base)
    for dtype, tol in ((np.float64, 1e-10), (np.longdouble, 1e-13)):
        for w, w_aug in pr.leafspace(inp, pr.pending_of(name), dtype=dtype)[2]:
            assert np.abs(w_aug - w).max() <= tol * max(1.0, float(np.abs(w).max())), name


def test_conditioning_only_lowers_the_variance():
    inp = ar.make_inputs(pr.CASES["p64"].base)
    _, v0 = pr.dense(inp, None)
    mu1, v1 = pr.dense(inp, pr.pending_of("p64"))
    assert (v1 <= v0 + 1e-12).all() and (v1 < v0 - 1e-6).any()
    assert np.array_equal(mu1, pr.dense(inp, None)[0])  # the mean is the one given the real data


def test_case_table_reaches_the_edges():
    from bark_amd.tree_kernels import posterior_sample_dim

    R = {n: posterior_sample_dim(ar.make_inputs(c.base).F, ar.make_inputs(c.base).ft) for n, c in pr.CASES.items()}
    assert R["n20_m1_p1"] == 8 and R["n64_m13_p2"] == 100
    assert R["n257_prior_p5"] % 64 and R["n257_prior_p5"] % 32  # neither a wave nor a code word
    assert [len(pr.pending_of(n)) for n in pr.CONDITIONING] == [1, 2, 5] and len(pr.pending_of("p64")) == 64
    assert {c.base.N for c in pr.CASES.values()} == {20, 64, 257} and all(c.base.B == 3 and c.base.C == 300 for c in pr.CASES.values())
    p = pr.pending_of("same_point_twice")
    assert np.array_equal(p[0], p[1])
    inp = ar.make_inputs(pr.CASES["unreached_leaves"].base)
    assert pr.unreached_count(inp, pr.pending_of("unreached_leaves"))[0] >= 3
    p = pr.pending_of("candidate_and_training_point")
    assert np.array_equal(p[0], inp.cand[7]) and np.array_equal(p[1], inp.X[3])
    assert np.array_equal(pr.pending_of("pair_ab"), pr.pending_of("pair_ba")[::-1])
    assert pr.SLAB.base.C > (1 << 16) and [pr.CASES[n].q for n in pr.GREEDY] == [4, 8]
    assert all(ar.make_inputs(c.base).noise.min() >= 1e-2 for c in list(pr.CASES.values()) + [pr.SLAB])


def test_public_names_and_prototypes():
    from bark_amd import optimizer
    from bark_amd.optimizer.acquisition import propose_batch_from_candidates

    assert optimizer.propose_batch_from_candidates is propose_batch_from_candidates
    assert "bark_acquisition_scan_pending_hip" in _lib.SIGNATURES
    q = _lib.lib().bark_acquisition_scan_pending_workspace_bytes
    base = _lib.lib().bark_acquisition_scan_workspace_bytes(257, 146, 50, 3, 300)
    assert q(257, 146, 50, 3, 300, 0) == base  # without pending points: the scan's own workspace
    assert q(257, 146, 50, 3, 300, 1) == q(257, 146, 50, 3, 300, 64) == base + 3 * 5 * 128 * 4  # (Bc, W, 128) code words
    assert q(257, 146, 50, 3, 300, 65) == 0 and q(257, 146, 50, 3, 300, -1) == 0


def test_python_refusals_without_a_device():
    from bark_amd.optimizer import acquisition_scan, propose_batch_from_candidates

    inp = ar.make_inputs(pr.CASES["n64_m13_p2"].base)
    args = (inp.model, inp.data, inp.cand, inp.ft)
    for q in (0, -1, 301):
        with pytest.raises(ValueError, match="q must lie"):
            propose_batch_from_candidates(*args, q)
    with pytest.raises(ValueError, match="exceed 64"):
        propose_batch_from_candidates(*args, 66)
    with pytest.raises(ValueError, match="exceed 64"):
        propose_batch_from_candidates(*args, 2, pending=pr.pending_of("p64"))
    with pytest.raises(TypeError):
        propose_batch_from_candidates(*args, 2, fantasies="mean")
    with pytest.raises(TypeError):
        acquisition_scan(*args, pendng=pr.pending_of("p64"))
    with pytest.raises(ValueError, match="unknown kind"):
        acquisition_scan(*args, kind="ucb", pending=pr.pending_of("p64"))
