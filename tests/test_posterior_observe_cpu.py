"""Host-side checks of conditioning on points with values (tests/observe_ref.py): for every case of the GPU test
(tests/test_gpu_posterior_observe.py) the sequential leaf-space update agrees with the oracle's dense route on the augmented
data — float64 within the posterior bar, longdouble within 1 % of it — the log predictive equals the oracle's MLL
difference, values equal to the posterior mean reproduce the believer, the fantasy normals are named by (seed, forest,
draw) alone, and the constant-liar greedy loop picks what a loop over the dense oracle picks.  No GPU."""
import numpy as np
import pytest

import acq_pending_ref as pr
import acq_ref as ar
import observe_ref as ob
from bark_amd import _lib
from bark_amd.fitting import _philox


def used(got, want, fraction=1.0):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (fraction * (ob.ATOL + ob.RTOL * np.abs(want)))).max())


def value_sets(name):
    """the deterministic values of a case: the generator's y; for one case also the constant liar and a (B, P) array"""
    vals = ob.values_of(name)
    out = [("y", vals)]
    if name == "n64_m13_p2":
        B = ob.case_of(name).base.B
        out += [("liar", ob.LIAR), ("per_forest", vals[None, :] + 0.5 * np.arange(B)[:, None])]
    return out


@pytest.mark.parametrize("name", ob.NAMES)
def test_sequential_update_against_the_dense_oracle(name):
    inp, pts = ar.make_inputs(ob.case_of(name).base), ob.points_of(name)
    for label, vals in value_sets(name):
        mu_d, var_d = ob.dense(inp, pts, vals)
        r64, rld = ob.sequential(inp, pts, vals), ob.sequential(inp, pts, vals, dtype=np.longdouble)
        figures = {k: (used(r64[k], d), used(rld[k].astype(np.float64), d, ob.AGREE)) for k, d in (("mu", mu_d), ("var", var_d))}
        print(f"{name} {label}: fraction of the bar used (float64, longdouble / 1 %) {figures}")
        assert all(max(f) <= 1.0 for f in figures.values()), (name, label, figures)
        assert not np.allclose(r64["mu"], pr.leafspace(inp, pts)[0], rtol=1e-6, atol=1e-6)  # the values matter


@pytest.mark.parametrize("name", ob.NAMES)
def test_log_predictive_is_the_mll_difference(name):
    inp, pts = ar.make_inputs(ob.case_of(name).base), ob.points_of(name)
    for label, vals in value_sets(name):
        got = ob.sequential(inp, pts, vals)["logpred"]
        want, by_def = ob.mll_difference(inp, pts, vals), ob.logpred_dense(inp, pts, vals)
        print(f"{name} {label}: bar used against the MLL difference {used(got, want):.3g}, against the definition {used(got, by_def):.3g}")
        assert used(got, want) <= 1.0 and used(got, by_def) <= 1.0
        assert used(ob.sequential(inp, pts, vals, dtype=np.longdouble)["logpred"].astype(np.float64), by_def) <= 1.0


@pytest.mark.parametrize("name", ["n20_m1_p1", "n64_m13_p2", "same_point_twice", "unreached_leaves"])
def test_values_at_the_mean_are_the_believer(name):
    """eps = 0 is y* = mu: w does not move and M^-1 is the believer's"""
    inp, pts = ar.make_inputs(ob.case_of(name).base), ob.points_of(name)
    B, P = inp.F.shape[0], len(pts)
    res = ob.sequential(inp, pts, eps=np.zeros((B, P)))
    believer = pr.leafspace(inp, pts)
    for b, f in enumerate(res["forests"]):
        assert np.array_equal(f.w, believer[2][b][0])
    assert np.array_equal(res["var"], believer[1]) and np.array_equal(res["mu"], believer[0])
    # the values it used are the predictive means, point by point
    again = ob.sequential(inp, pts, res["values"])
    assert used(again["mu"], res["mu"]) <= 1.0 and np.array_equal(again["var"], res["var"])


def test_sampled_fantasies_are_the_values_they_return():
    name = "n64_m13_p2"
    inp, pts = ar.make_inputs(ob.case_of(name).base), ob.points_of(name)
    eps = np.random.default_rng(3).standard_normal((inp.F.shape[0], len(pts)))
    drawn = ob.sequential(inp, pts, eps=eps)
    given = ob.sequential(inp, pts, drawn["values"])
    assert used(given["mu"], drawn["mu"]) <= 1.0 and np.array_equal(given["var"], drawn["var"])
    assert np.abs(drawn["values"] - ob.sequential(inp, pts, eps=0 * eps)["values"]).min() > 1e-3


def test_fantasy_normals():
    alone = _philox.fantasy_normals(7, [2], [5], 9)
    among = _philox.fantasy_normals(7, [0, 2, 1, 2], [5, 5, 0, 6], 12)
    assert alone.shape == (1, 9) and among.shape == (4, 12)
    assert np.array_equal(among[1, :9], alone[0])  # the row of (seed, forest, draw), whatever else is asked for
    assert not np.array_equal(among[1], among[3]) and not np.array_equal(among[0], among[1])
    assert not np.array_equal(alone, _philox.path_normals(7, [2], [5], 9))  # the other key
    assert not np.array_equal(alone, _philox.fantasy_normals(8, [2], [5], 9))
    big = _philox.fantasy_normals(1, np.arange(64), 0, 64)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1.0) < 0.05


@pytest.mark.parametrize("name", ob.GREEDY)
def test_constant_liar_greedy_loop(name):
    case = pr.CASES[name]
    inp, pend = ar.make_inputs(case.base), pr.pending_of(name)
    checked = 0
    for kind in pr.KINDS:
        want, gap_d = ob.greedy_dense(inp, pend, case.q, kind, case.base.kappa, ob.LIAR)
        got, gap = ob.greedy(inp, pend, case.q, kind, case.base.kappa, ob.LIAR)
        print(f"{name} {kind}: picks {want.tolist()} gap {min(gap, gap_d):.3g}")
        assert len(set(want.tolist())) == case.q
        if min(gap, gap_d) >= ob.MARGIN:
            checked += 1
            assert np.array_equal(got, want), (name, kind)
    assert checked, "no kind of this case has a winner's margin"


def test_case_table():
    from bark_amd.tree_kernels import posterior_sample_dim

    for name in ob.NAMES:
        case = ob.case_of(name)
        assert ob.values_of(name).shape == (len(ob.points_of(name)),) and np.isfinite(ob.values_of(name)).all()
    wide, ragged = ar.make_inputs(ob.WIDE_BASE), ar.make_inputs(ob.CHUNK_BASE)
    assert posterior_sample_dim(wide.F, wide.ft) == 1100 > 1024 and wide.F.shape[0] == 2 and len(ob.points_of("leaves1100_p3")) == 3
    assert ragged.F.shape[0] == 5 and ob.CHUNK_BASE.chunk == 2
    assert case.base is ob.CHUNK_BASE


def test_prototypes_and_refusals_without_a_device():
    from bark_amd.optimizer import propose_batch_from_candidates
    from bark_amd.tree_kernels import LeafPosterior

    assert {"bark_leaf_posterior_observe_hip", "bark_leaf_posterior_observe_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    q, cond = lib.bark_leaf_posterior_observe_workspace_bytes, lib.bark_leaf_posterior_condition_workspace_bytes
    assert q(146, 50, 3, 5) == cond(146, 50, 3, 5) == 3 * 5 * 128 * 4 and q(146, 50, 3, 0) == 0
    assert q(146, 50, 3, 65) == 0 and q(146, 50, 3, -1) == 0 and q(8193, 50, 3, 1) == 0 and q(146, 65, 3, 1) == 0
    assert (_lib.OBSERVE_VALUES, _lib.OBSERVE_SAMPLE) == (0, 1)
    for name in ("observe", "observe_", "fantasise", "log_predictive"):
        assert callable(getattr(LeafPosterior, name))
    inp = ar.make_inputs(pr.CASES["n64_m13_p2"].base)
    args = (inp.model, inp.data, inp.cand, inp.ft, 2)
    for fantasy in (0.0, "sample"):
        with pytest.raises(ValueError, match="fit_posterior"):
            propose_batch_from_candidates(*args, fantasy=fantasy)
    with pytest.raises(ValueError, match="unknown fantasy"):
        propose_batch_from_candidates(*args, fantasy="liar")
    with pytest.raises(ValueError, match="finite"):
        propose_batch_from_candidates(*args, fantasy=float("nan"))
